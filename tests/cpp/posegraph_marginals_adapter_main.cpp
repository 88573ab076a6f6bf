// Drives mrslam::PoseGraph::markPoses / marginals / jointMarginals (include/mrslam/posegraph.hpp) on a scene written by
// tests/test_posegraph_marginals_adapter.py:
//   in : int32 nr, L, n_marks | int32 chain_lengths [nr] | double odom [poses - nr][16] | int32 i [L] | j [L] | double Z [L][16] |
//        int32 marks [n_marks]
//   out: double separators, order, bytes | marginals of all poses [poses][36], chordal | of the marked poses [n_marks][36], Pose3 |
//        joint marginals of the loops [L][144], chordal | of the marked poses pairwise (a < b) [..][144], Pose3
#include <cstdio>
#include <vector>

#include "mrslam/posegraph.hpp"

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    int32_t hdr[3];
    if (!f || std::fread(hdr, sizeof(int32_t), 3, f) != 3) return 2;
    const int nr = hdr[0], L = hdr[1], n_marks = hdr[2];
    std::vector<int32_t> lengths(nr), li(L), lj(L), marks(n_marks);
    bool ok = std::fread(lengths.data(), 4, nr, f) == (size_t)nr;
    int poses = 0;
    for (int c = 0; ok && c < nr; ++c) poses += lengths[c];
    std::vector<double> odom(16 * (size_t)(ok ? poses - nr : 0)), Z(16 * (size_t)L);
    ok = ok && std::fread(odom.data(), 8, odom.size(), f) == odom.size();
    ok = ok && std::fread(li.data(), 4, L, f) == (size_t)L && std::fread(lj.data(), 4, L, f) == (size_t)L;
    ok = ok && std::fread(Z.data(), 8, Z.size(), f) == Z.size();
    ok = ok && std::fread(marks.data(), 4, n_marks, f) == (size_t)n_marks;
    std::fclose(f);
    if (!ok) return 2;
    try {
        mrslam::PoseGraph graph(lengths);
        graph.setOdometry(odom.data(), poses - nr);
        graph.addLoops(li.data(), lj.data(), Z.data(), L);
        try {                                                    // a refusal is an exception with the C ABI's text
            graph.marginals();
            std::printf("FAILED marginals without a result were answered\n");
            return 1;
        } catch (const std::runtime_error& e) {
            std::printf("refused: %s\n", e.what());
        }
        graph.markPoses(marks);
        const mrslam::PoseGraph::Result r = graph.optimize();
        const mrslam::PoseGraph::MarginalInfo info = graph.computeMarginals();
        std::vector<double> out = {(double)info.separators, (double)info.order, (double)info.bytes};
        std::printf("poses=%d loops=%d iterations=%d separators=%lld order=%lld\n", graph.poses(), graph.loops(), r.iterations, info.separators,
                    info.order);
        const auto put = [&](const std::vector<double>& v) { out.insert(out.end(), v.begin(), v.end()); };
        put(graph.marginals());
        put(graph.marginals(marks, MRS_PGO_FRAME_POSE3));
        put(graph.jointMarginals(li, lj));
        std::vector<int32_t> a, b;
        for (int u = 0; u < n_marks; ++u)
            for (int v = u + 1; v < n_marks; ++v) {
                a.push_back(marks[u]);
                b.push_back(marks[v]);
            }
        put(graph.jointMarginals(a, b, MRS_PGO_FRAME_POSE3));
        try {
            graph.jointMarginals({marks[0]}, {marks[0]});
            std::printf("FAILED a joint marginal of a pose with itself was answered\n");
            return 1;
        } catch (const std::runtime_error& e) {
            std::printf("refused: %s\n", e.what());
        }
        FILE* o = std::fopen(argv[2], "wb");
        if (!o) return 2;
        std::fwrite(out.data(), sizeof(double), out.size(), o);
        std::fclose(o);
    } catch (const std::exception& e) {
        std::printf("FAILED %s\n", e.what());
        return 1;
    }
    return 0;
}
