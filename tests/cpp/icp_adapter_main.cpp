// Compiles the mrslam::IterativeClosestPoint adapter against the PCL mock and (on a GPU box) runs the call sequence of
// GlobalManager::performLoopClosure (Mapping/src/global_manager/src/global_manager.cpp:890-906) and the PCL_ICP branch of
// select_registration_method (:2427-2434), both with the one-type-name change INTEGRATION.md section 2 describes.  Test scaffolding.
#include "mock_pcl.hpp"
#include <mrslam/icp.hpp>

#include <cmath>
#include <cstdio>
#include <random>
#include <string>

typedef pcl::PointXYZI PointTI;
typedef pcl::PointCloud<PointTI> PointCloudI;
typedef PointCloudI::Ptr PointCloudIPtr;

static double icp_iters_ = 50;   // launch/global_manager.launch:53

// :2427-2434
static pcl::Registration<PointTI, PointTI>::Ptr select_pcl_icp()
{
    mrslam::IterativeClosestPoint<PointTI, PointTI>::Ptr icp(new mrslam::IterativeClosestPoint<PointTI, PointTI>());
    icp->setTransformationEpsilon(1e-3);
    icp->setMaximumIterations((int)icp_iters_);
    icp->setMaxCorrespondenceDistance(100.0);
    icp->setEuclideanFitnessEpsilon(1e-3);
    return icp;
}

static bool same(const Eigen::Matrix4f& m, const double* f)
{
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c)
            if (m(r, c) != (float)f[4 * r + c]) return false;
    return true;
}

int main()
{
    PointCloudIPtr queryKeyframe(new PointCloudI), databaseKeyframe(new PointCloudI);
    std::mt19937 rng(1);
    std::uniform_real_distribution<float> u(-20.f, 20.f);
    std::normal_distribution<float> nz(0.f, 0.01f);
    const float yaw = 0.02f, tx = 0.3f, ty = -0.2f;
    std::vector<float> src, tgt;
    for (int i = 0; i < 6000; ++i) {  // three orthogonal noisy planes
        pcl::PointXYZI p{};
        const float a = u(rng), b = u(rng);
        if (i % 3 == 0) { p.x = a; p.y = b; p.z = nz(rng); }
        else if (i % 3 == 1) { p.x = a; p.y = 20.f + nz(rng); p.z = std::fabs(b) * 0.3f; }
        else { p.x = -20.f + nz(rng); p.y = a; p.z = std::fabs(b) * 0.3f; }
        queryKeyframe->points.push_back(p);
        pcl::PointXYZI q = p;
        q.x = std::cos(yaw) * p.x - std::sin(yaw) * p.y + tx + nz(rng);
        q.y = std::sin(yaw) * p.x + std::cos(yaw) * p.y + ty + nz(rng);
        databaseKeyframe->points.push_back(q);
        src.insert(src.end(), {p.x, p.y, p.z});
        tgt.insert(tgt.end(), {q.x, q.y, q.z});
    }
    bool all_ok = true;

    // the C ABI called directly with the :890 settings: what the adapter must reproduce
    mrs_icp_params prm;
    mrs_icp_default_params(&prm);
    prm.max_correspondence_distance = 2.0; prm.max_iterations = (int)icp_iters_; prm.transformation_epsilon = 1e-3; prm.euclidean_fitness_epsilon = 1e-3;
    mrs_gicp_batch* h = nullptr;
    const int64_t offs[2] = {0, 6000};
    double direct[16];
    int32_t dconv = 0, dits = 0, dstate = 0;
    if (mrs_gicp_batch_create(fast_gicp::detail::shared_ctx(0), 1, &h) != MRS_OK || mrs_gicp_batch_set_clouds_host(h, 0, src.data(), 3, offs) != MRS_OK ||
        mrs_gicp_batch_set_clouds_host(h, 1, tgt.data(), 3, offs) != MRS_OK ||
        mrs_gicp_batch_align_icp(h, &prm, nullptr, direct, &dconv, &dits, &dstate, nullptr) != MRS_OK) {
        std::printf("direct call failed: %s\n", mrs_last_error());
        return 1;
    }
    mrs_gicp_batch_destroy(h);

    {   // :890-906, through a pcl::Registration::Ptr as ICPCheck holds its registration
        mrslam::IterativeClosestPoint<PointTI, PointTI>::Ptr derived(new mrslam::IterativeClosestPoint<PointTI, PointTI>());
        pcl::Registration<PointTI, PointTI>::Ptr icp = derived;
        icp->setInputSource(queryKeyframe);
        icp->setInputTarget(databaseKeyframe);
        icp->setMaxCorrespondenceDistance(2.0);
        icp->setMaximumIterations((int)icp_iters_);
        icp->setTransformationEpsilon(1e-3);
        derived->setEuclideanFitnessEpsilon(1e-3);
        PointCloudIPtr unused_result(new PointCloudI);
        icp->align(*unused_result);
        const bool conv = icp->hasConverged();
        const double host_fit = icp->getFitnessScore();              // PCL's host score (the mock's brute force)
        const double gpu_fit = derived->getFitnessScore();
        const Eigen::Matrix4f finalResult = icp->getFinalTransformation();
        // the same cloud objects again: nothing is uploaded, the alignment repeats bit for bit
        icp->setInputSource(queryKeyframe);
        icp->setInputTarget(databaseKeyframe);
        PointCloudIPtr again(new PointCloudI);
        icp->align(*again);
        const bool ok = conv && (int)conv == dconv && same(finalResult, direct) && same(icp->getFinalTransformation(), direct) &&
                        derived->getConvergenceState() == dstate && std::fabs(gpu_fit - host_fit) < 1e-5 &&
                        unused_result->points.size() == queryKeyframe->points.size() && std::fabs(finalResult(0, 3) - tx) < 0.05 &&
                        std::fabs(finalResult(1, 3) - ty) < 0.05;
        std::printf("performLoopClosure converged=%d state=%d iterations=%d tx=%.4f ty=%.4f yaw=%.5f fitness(pcl host)=%.6f fitness(gpu)=%.6f %s\n", (int)conv,
                    derived->getConvergenceState(), dits, finalResult(0, 3), finalResult(1, 3), std::atan2(finalResult(1, 0), finalResult(0, 0)),
                    host_fit, gpu_fit, ok ? "ok" : "FAILED");
        all_ok = all_ok && ok;
    }
    {   // :2427-2434 + ICPCheck's use of the returned pointer (:2016-2021, :2058-2071)
        auto icp = select_pcl_icp();
        icp->setInputSource(queryKeyframe);
        icp->setInputTarget(databaseKeyframe);
        PointCloudIPtr unused_result(new PointCloudI);
        Eigen::Matrix4f guess = Eigen::Matrix4f::Identity();
        guess(0, 3) = 0.25f; guess(1, 3) = -0.15f;
        icp->align(*unused_result, guess);
        const Eigen::Matrix4f finalResult = icp->getFinalTransformation();
        // these settings stop after two loose iterations (|t|^2 <= 1e-3): accepted by ICPCheck's fitness bound (:2058), within a decimetre
        const bool ok = icp->hasConverged() && icp->getFitnessScore(1.0) < 0.3 && std::fabs(finalResult(0, 3) - tx) < 0.1 &&
                        std::fabs(finalResult(1, 3) - ty) < 0.1;
        std::printf("PCL_ICP converged=%d tx=%.4f ty=%.4f %s\n", (int)icp->hasConverged(), finalResult(0, 3), finalResult(1, 3), ok ? "ok" : "FAILED");
        all_ok = all_ok && ok;
    }
    return all_ok ? 0 : 1;
}
