// Compiles mrslam::addNormal and the mrslam::IterativeClosestPointWithNormals adapter against the PCL mock and (on a GPU box) runs, on a pair
// of clouds read from a file, the call sequence the Mapping workspace's addNormal helper exists for (global_manager.cpp:2679-2693):
// normals of the target, then point-to-plane ICP with the :890-906 settings -- once on a target type that carries its normals
// (PointXYZINormal), once on plain PointXYZI, where the adapter computes them.  Results go to a file for tests/test_icp_normals_adapter.py,
// which compares them with the Python path.  Test scaffolding.
#include "mock_pcl_normals.hpp"
#include <mrslam/icp_normals.hpp>

#include <cmath>
#include <cstdio>

typedef pcl::PointXYZI PointTI;
typedef pcl::PointXYZINormal PointTIN;      // typedefs.h:64-68

template <class Icp>
static void settings_890(Icp& icp)
{
    icp.setMaxCorrespondenceDistance(2.0);
    icp.setMaximumIterations(50);
    icp.setTransformationEpsilon(1e-3);
    icp.setEuclideanFitnessEpsilon(1e-3);
}

// IN: int32 n_src, n_tgt, then n_src + n_tgt points of 3 floats.  OUT: n_tgt x 4 floats (addNormal's fields), then per run (given, computed)
// 16 floats (row-major final transformation) and 3 floats (converged, iterations, state).
int main(int argc, char** argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 2; }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    int32_t n[2];
    if (std::fread(n, sizeof(int32_t), 2, f) != 2) return 3;
    std::vector<float> xyz(3 * (size_t)(n[0] + n[1]));
    if (std::fread(xyz.data(), sizeof(float), xyz.size(), f) != xyz.size()) return 3;
    std::fclose(f);
    pcl::PointCloud<PointTI>::Ptr src(new pcl::PointCloud<PointTI>), tgt(new pcl::PointCloud<PointTI>);
    for (int i = 0; i < n[0] + n[1]; ++i) {
        PointTI p{};
        p.x = xyz[3 * (size_t)i]; p.y = xyz[3 * (size_t)i + 1]; p.z = xyz[3 * (size_t)i + 2]; p.intensity = (float)i;
        (i < n[0] ? src : tgt)->points.push_back(p);
    }
    std::vector<float> out;
    bool all_ok = true;

    pcl::PointCloud<PointTIN>::Ptr tgtWithNormals(new pcl::PointCloud<PointTIN>);
    mrslam::addNormal(tgt, tgtWithNormals);
    bool fields = tgtWithNormals->points.size() == tgt->points.size();
    for (size_t i = 0; fields && i < tgt->points.size(); ++i) {
        const PointTIN& q = tgtWithNormals->points[i];
        const PointTI& p = tgt->points[i];
        fields = q.x == p.x && q.y == p.y && q.z == p.z && q.intensity == p.intensity;
        out.insert(out.end(), {q.normal_x, q.normal_y, q.normal_z, q.curvature});
    }
    std::printf("addNormal points=%zu %s\n", tgtWithNormals->points.size(), fields ? "ok" : "FAILED");
    all_ok = all_ok && fields;

    auto record = [&](const Eigen::Matrix4f& T, bool conv, int its, int state) {
        for (int r = 0; r < 4; ++r)
            for (int c = 0; c < 4; ++c) out.push_back(T(r, c));
        out.insert(out.end(), {conv ? 1.f : 0.f, (float)its, (float)state});
    };
    {   // the target carries its normals; driven through a pcl::Registration::Ptr
        typedef mrslam::IterativeClosestPointWithNormals<PointTI, PointTIN> Icp;
        Icp::Ptr derived(new Icp());
        pcl::Registration<PointTI, PointTIN>::Ptr icp = derived;
        settings_890(*derived);
        icp->setInputSource(src);
        icp->setInputTarget(tgtWithNormals);
        pcl::PointCloud<PointTI> aligned;
        icp->align(aligned);
        const Eigen::Matrix4f T = icp->getFinalTransformation();
        const double host_fit = icp->getFitnessScore(), gpu_fit = derived->getFitnessScore();
        icp->setInputSource(src);                        // the same cloud objects again: nothing is uploaded, the alignment repeats bit for bit
        icp->setInputTarget(tgtWithNormals);
        pcl::PointCloud<PointTI> again;
        icp->align(again);
        bool same = true;
        for (int i = 0; i < 16; ++i) same = same && T.m[i] == icp->getFinalTransformation().m[i];
        const bool ok = icp->hasConverged() && same && aligned.points.size() == src->points.size() && std::fabs(gpu_fit - host_fit) < 1e-5;
        std::printf("given normals converged=%d state=%d fitness(pcl host)=%.6f fitness(gpu)=%.6f %s\n", (int)icp->hasConverged(),
                    derived->getConvergenceState(), host_fit, gpu_fit, ok ? "ok" : "FAILED");
        record(T, icp->hasConverged(), 0, derived->getConvergenceState());
        all_ok = all_ok && ok;
    }
    {   // a target without normal fields: the adapter computes them (k = 15)
        mrslam::IterativeClosestPointWithNormals<PointTI, PointTI> icp;
        settings_890(icp);
        icp.setInputSource(src);
        icp.setInputTarget(tgt);
        pcl::PointCloud<PointTI> aligned;
        icp.align(aligned);
        std::printf("computed normals converged=%d state=%d\n", (int)icp.hasConverged(), icp.getConvergenceState());
        record(icp.getFinalTransformation(), icp.hasConverged(), 0, icp.getConvergenceState());
        all_ok = all_ok && icp.hasConverged();
    }
    f = std::fopen(argv[2], "wb");
    if (!f) return 4;
    const bool written = std::fwrite(out.data(), sizeof(float), out.size(), f) == out.size();
    std::fclose(f);
    return all_ok && written ? 0 : 1;
}
