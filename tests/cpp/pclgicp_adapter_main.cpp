// Compiles the mrslam::GeneralizedIterativeClosestPoint adapter against the PCL mock and (on a GPU box) runs the PCL_GICP branch of
// GlobalManager::select_registration_method (Mapping/src/global_manager/src/global_manager.cpp:2419-2426) followed by ICPCheck's use of the
// returned pointer (:2018-2021, :2058-2071), with the one-type-name change INTEGRATION.md section 2 describes.  Test scaffolding.
#include "mock_pcl.hpp"
#include <mrslam/gicp.hpp>

#include <cmath>
#include <cstdio>
#include <random>
#include <string>

typedef pcl::PointXYZI PointTI;
typedef pcl::PointCloud<PointTI> PointCloudI;
typedef PointCloudI::Ptr PointCloudIPtr;

static double icp_iters_ = 50;   // launch/global_manager.launch:53

// :2419-2426
static pcl::Registration<PointTI, PointTI>::Ptr select_pcl_gicp()
{
    mrslam::GeneralizedIterativeClosestPoint<PointTI, PointTI>::Ptr gicp(new mrslam::GeneralizedIterativeClosestPoint<PointTI, PointTI>());
    gicp->setTransformationEpsilon(1e-3);
    gicp->setMaximumIterations((int)icp_iters_);
    gicp->setMaxCorrespondenceDistance(100.0);
    gicp->setEuclideanFitnessEpsilon(1e-3);
    return gicp;
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

    // the C ABI called directly with the :2422-2425 settings: what the adapter must reproduce
    mrs_pclgicp_params prm;
    mrs_pclgicp_default_params(&prm);
    prm.max_correspondence_distance = 100.0; prm.max_iterations = (int)icp_iters_; prm.transformation_epsilon = 1e-3;
    mrs_gicp_batch* h = nullptr;
    const int64_t offs[2] = {0, 6000};
    double direct[16];
    int32_t dconv = 0, dits = 0, dstate = 0;
    if (mrs_gicp_batch_create(fast_gicp::detail::shared_ctx(0), 1, &h) != MRS_OK || mrs_gicp_batch_set_clouds_host(h, 0, src.data(), 3, offs) != MRS_OK ||
        mrs_gicp_batch_set_clouds_host(h, 1, tgt.data(), 3, offs) != MRS_OK ||
        mrs_gicp_batch_align_pcl(h, &prm, nullptr, direct, &dconv, &dits, &dstate, nullptr) != MRS_OK) {
        std::printf("direct call failed: %s\n", mrs_last_error());
        return 1;
    }
    mrs_gicp_batch_destroy(h);

    {   // :2419-2426 + ICPCheck's use of the returned pointer (:2018-2021, :2058-2071), through a pcl::Registration::Ptr
        pcl::Registration<PointTI, PointTI>::Ptr reg = select_pcl_gicp();
        reg->setInputSource(queryKeyframe);
        reg->setInputTarget(databaseKeyframe);
        PointCloudIPtr unused_result(new PointCloudI);
        reg->align(*unused_result);
        const bool conv = reg->hasConverged();
        const double host_fit = reg->getFitnessScore(1.0);             // PCL's host score (the mock's brute force), ICPCheck's range
        const Eigen::Matrix4f finalResult = reg->getFinalTransformation();
        // the same cloud objects again: nothing is uploaded, the alignment repeats bit for bit
        reg->setInputSource(queryKeyframe);
        reg->setInputTarget(databaseKeyframe);
        PointCloudIPtr again(new PointCloudI);
        reg->align(*again);
        const bool ok = conv && (int)conv == dconv && same(finalResult, direct) && same(reg->getFinalTransformation(), direct) && host_fit < 0.3 &&
                        unused_result->points.size() == queryKeyframe->points.size() && std::fabs(finalResult(0, 3) - tx) < 0.01 &&
                        std::fabs(finalResult(1, 3) - ty) < 0.01 && std::fabs(std::atan2(finalResult(1, 0), finalResult(0, 0)) - yaw) < 1e-3;
        std::printf("PCL_GICP converged=%d state=%d iterations=%d tx=%.4f ty=%.4f yaw=%.5f fitness(pcl host)=%.6f %s\n", (int)conv, dstate, dits,
                    finalResult(0, 3), finalResult(1, 3), std::atan2(finalResult(1, 0), finalResult(0, 0)), host_fit, ok ? "ok" : "FAILED");
        all_ok = all_ok && ok;
    }
    {   // on the derived type: PCL's own setters, the GPU fitness score, a guess
        mrslam::GeneralizedIterativeClosestPoint<PointTI, PointTI> gicp;
        gicp.setTransformationEpsilon(1e-3);
        gicp.setMaximumIterations((int)icp_iters_);
        gicp.setMaxCorrespondenceDistance(100.0);
        gicp.setEuclideanFitnessEpsilon(1e-3);
        gicp.setRotationEpsilon(2e-3);
        gicp.setCorrespondenceRandomness(20);
        gicp.setMaximumOptimizerIterations(20);
        gicp.setInputSource(queryKeyframe);
        gicp.setInputTarget(databaseKeyframe);
        PointCloudIPtr unused_result(new PointCloudI);
        gicp.align(*unused_result);
        pcl::Registration<PointTI, PointTI>& base = gicp;
        const double host_fit = base.getFitnessScore(), gpu_fit = gicp.getFitnessScore();
        const bool same_as_direct = same(gicp.getFinalTransformation(), direct) && gicp.getConvergenceState() == dstate;
        Eigen::Matrix4f guess = Eigen::Matrix4f::Identity();
        guess(0, 3) = 0.25f; guess(1, 3) = -0.15f;
        gicp.align(*unused_result, guess);
        const Eigen::Matrix4f finalResult = gicp.getFinalTransformation();
        const bool ok = same_as_direct && gicp.hasConverged() && std::fabs(gpu_fit - host_fit) < 1e-5 && gicp.getEuclideanFitnessEpsilon() == 1e-3 &&
                        gicp.getCorrespondenceRandomness() == 20 && std::fabs(finalResult(0, 3) - tx) < 0.01 && std::fabs(finalResult(1, 3) - ty) < 0.01;
        std::printf("derived converged=%d tx=%.4f ty=%.4f fitness(pcl host)=%.6f fitness(gpu)=%.6f %s\n", (int)gicp.hasConverged(), finalResult(0, 3),
                    finalResult(1, 3), host_fit, gpu_fit, ok ? "ok" : "FAILED");
        all_ok = all_ok && ok;
    }
    return all_ok ? 0 : 1;
}
