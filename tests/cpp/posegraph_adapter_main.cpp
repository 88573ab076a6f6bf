// Drives mrslam::PoseGraph (include/mrslam/posegraph.hpp) on a scene written by tests/test_posegraph_adapter.py:
//   in : int32 nr, L | int32 chain_lengths [nr] | double odom [poses - nr][16] | int32 i [L] | j [L] | double Z [L][16]
//   out: double iterations, converged, max_delta, error_initial, error_final, separators | double initial [poses][16] | poses [poses][16]
#include <cstdio>
#include <vector>

#include "mrslam/posegraph.hpp"

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    int32_t hdr[2];
    if (!f || std::fread(hdr, sizeof(int32_t), 2, f) != 2) return 2;
    const int nr = hdr[0], L = hdr[1];
    std::vector<int32_t> lengths(nr), li(L), lj(L);
    bool ok = std::fread(lengths.data(), 4, nr, f) == (size_t)nr;
    int poses = 0;
    for (int c = 0; ok && c < nr; ++c) poses += lengths[c];
    std::vector<double> odom(16 * (size_t)(ok ? poses - nr : 0)), Z(16 * (size_t)L);
    ok = ok && std::fread(odom.data(), 8, odom.size(), f) == odom.size();
    ok = ok && std::fread(li.data(), 4, L, f) == (size_t)L && std::fread(lj.data(), 4, L, f) == (size_t)L;
    ok = ok && std::fread(Z.data(), 8, Z.size(), f) == Z.size();
    std::fclose(f);
    if (!ok) return 2;
    try {
        mrslam::PoseGraph graph(lengths);
        graph.setOdometry(odom.data(), poses - nr);
        graph.addLoops(li.data(), lj.data(), Z.data(), L);
        const std::vector<double> initial = graph.initialize();
        const mrslam::PoseGraph::Result r = graph.optimize();
        std::printf("poses=%d loops=%d iterations=%d converged=%d separators=%d\n", graph.poses(), graph.loops(), r.iterations, (int)r.converged,
                    r.separators);
        const double head[6] = {(double)r.iterations, r.converged ? 1.0 : 0.0, r.max_delta, r.error_initial, r.error_final, (double)r.separators};
        FILE* o = std::fopen(argv[2], "wb");
        if (!o) return 2;
        std::fwrite(head, sizeof(double), 6, o);
        std::fwrite(initial.data(), sizeof(double), initial.size(), o);
        std::fwrite(r.poses.data(), sizeof(double), r.poses.size(), o);
        std::fclose(o);
        try {                                                    // a refusal is an exception with the C ABI's text, and changes nothing
            const int32_t same = 3;
            graph.addLoops(&same, &same, Z.data(), 1);
            std::printf("FAILED a loop from a pose to itself was accepted\n");
            return 1;
        } catch (const std::runtime_error& e) {
            std::printf("refused: %s\n", e.what());
        }
        if (graph.loops() != L) {
            std::printf("FAILED the refused loop changed the count\n");
            return 1;
        }
    } catch (const std::exception& e) {
        std::printf("FAILED %s\n", e.what());
        return 1;
    }
    return 0;
}
