// Drives the noise, kernel and Levenberg-Marquardt methods of mrslam::PoseGraph (include/mrslam/posegraph.hpp) on a scene written by
// tests/test_posegraph_robust_adapter.py:
//   in : int32 nr, L, kernel | double k | int32 chain_lengths [nr] | double odom [poses - nr][16] | double oC [poses - nr][36] |
//        int32 i [L] | j [L] | double Z [L][16] | double lC [L][36]
//   out: double solves, accepted, converged, max_delta, cost_initial, cost_final, separators, lambda | poses [poses][16] | w [L] | r2 [L] |
//        double iterations, converged of the weighted Gauss-Newton call without the kernel | its poses [poses][16]
#include <cstdio>
#include <vector>

#include "mrslam/posegraph.hpp"

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    int32_t hdr[3];
    double k = 0.0;
    if (!f || std::fread(hdr, sizeof(int32_t), 3, f) != 3 || std::fread(&k, sizeof(double), 1, f) != 1) return 2;
    const int nr = hdr[0], L = hdr[1], kernel = hdr[2];
    std::vector<int32_t> lengths(nr), li(L), lj(L);
    bool ok = std::fread(lengths.data(), 4, nr, f) == (size_t)nr;
    int poses = 0;
    for (int c = 0; ok && c < nr; ++c) poses += lengths[c];
    const size_t n_odo = ok ? (size_t)(poses - nr) : 0;
    std::vector<double> odom(16 * n_odo), oC(36 * n_odo), Z(16 * (size_t)L), lC(36 * (size_t)L);
    ok = ok && std::fread(odom.data(), 8, odom.size(), f) == odom.size() && std::fread(oC.data(), 8, oC.size(), f) == oC.size();
    ok = ok && std::fread(li.data(), 4, L, f) == (size_t)L && std::fread(lj.data(), 4, L, f) == (size_t)L;
    ok = ok && std::fread(Z.data(), 8, Z.size(), f) == Z.size() && std::fread(lC.data(), 8, lC.size(), f) == lC.size();
    std::fclose(f);
    if (!ok) return 2;
    try {
        mrslam::PoseGraph graph(lengths);
        graph.setOdometry(odom.data(), (int)n_odo);
        graph.setOdometryNoise(oC.data(), (int)n_odo);
        graph.addLoops(li.data(), lj.data(), Z.data(), lC.data(), L);
        graph.setLoopKernel(kernel, k);
        try {                                                    // a kernel needs the step control
            graph.optimize();
            std::printf("FAILED optimize ran with a kernel set\n");
            return 1;
        } catch (const std::runtime_error& e) {
            std::printf("refused: %s\n", e.what());
        }
        const mrslam::PoseGraph::ResultLM r = graph.optimizeLM();
        const mrslam::PoseGraph::LoopState s = graph.loopState();
        std::printf("poses=%d loops=%d solves=%d accepted=%d converged=%d\n", graph.poses(), graph.loops(), r.solves, r.accepted, (int)r.converged);
        graph.setLoopKernel(MRS_PGO_KERNEL_NONE);
        const mrslam::PoseGraph::Result gn = graph.optimize(1e-9, 3);
        const double head[8] = {(double)r.solves, (double)r.accepted, r.converged ? 1.0 : 0.0, r.max_delta, r.cost_initial, r.cost_final,
                                (double)r.separators, r.lambda};
        const double tail[2] = {(double)gn.iterations, gn.converged ? 1.0 : 0.0};
        FILE* o = std::fopen(argv[2], "wb");
        if (!o) return 2;
        std::fwrite(head, sizeof(double), 8, o);
        std::fwrite(r.poses.data(), sizeof(double), r.poses.size(), o);
        std::fwrite(s.weight.data(), sizeof(double), s.weight.size(), o);
        std::fwrite(s.r2.data(), sizeof(double), s.r2.size(), o);
        std::fwrite(tail, sizeof(double), 2, o);
        std::fwrite(gn.poses.data(), sizeof(double), gn.poses.size(), o);
        std::fclose(o);
        try {                                                    // a refusal is an exception with the C ABI's text, and changes nothing
            std::vector<double> bad(lC.begin(), lC.begin() + 36);
            bad[0] = bad[7] = bad[14] = 0.0;
            graph.addLoops(li.data(), lj.data(), Z.data(), bad.data(), 1);
            std::printf("FAILED a covariance without a rotation variance was accepted\n");
            return 1;
        } catch (const std::runtime_error& e) {
            std::printf("refused: %s\n", e.what());
        }
        if (graph.loops() != L) {
            std::printf("FAILED the refused loop changed the count\n");
            return 1;
        }
        graph.setOdometryNoise(nullptr, 0);
    } catch (const std::exception& e) {
        std::printf("FAILED %s\n", e.what());
        return 1;
    }
    return 0;
}
