// Drives mrslam::PoseGraph::setSolver / solverStats (include/mrslam/posegraph.hpp) on a scene written by
// tests/test_posegraph_sparse_adapter.py:
//   in : int32 nr, L, dense_limit | int32 chain_lengths [nr] | double odom [poses - nr][16] | int32 i [L] | j [L] | double Z [L][16]
//   out: double iterations, converged, max_delta, error_initial, error_final, separators | the 8 solver stats of stage 1 | of stage 2 |
//        of stage 2 after the return to the dense solver | double poses [poses][16] under the sparse solver | under the dense solver
#include <cstdio>
#include <vector>

#include "mrslam/posegraph.hpp"

static void put(std::vector<double>& out, const mrslam::PoseGraph::SolverStats& s)
{
    for (long long v : {s.separators, s.eliminated, s.core, s.levels, s.blocks, s.updates, s.max_degree, (long long)s.solver}) out.push_back((double)v);
}

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    int32_t hdr[3];
    if (!f || std::fread(hdr, sizeof(int32_t), 3, f) != 3) return 2;
    const int nr = hdr[0], L = hdr[1], dense_limit = hdr[2];
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
        graph.setSolver(MRS_PGO_SOLVER_SPARSE, dense_limit);
        const mrslam::PoseGraph::Result r = graph.optimize();
        std::vector<double> out = {(double)r.iterations, r.converged ? 1.0 : 0.0, r.max_delta, r.error_initial, r.error_final, (double)r.separators};
        put(out, graph.solverStats(1));
        put(out, graph.solverStats());
        std::printf("poses=%d loops=%d iterations=%d converged=%d eliminated=%lld core=%lld\n", graph.poses(), graph.loops(), r.iterations,
                    (int)r.converged, graph.solverStats().eliminated, graph.solverStats().core);
        try {                                                    // a refusal is an exception with the C ABI's text, and changes nothing
            graph.setSolver(MRS_PGO_SOLVER_SPARSE, MRS_PGO_MAX_SEPARATORS + 1);
            std::printf("FAILED a dense limit past MRS_PGO_MAX_SEPARATORS was accepted\n");
            return 1;
        } catch (const std::runtime_error& e) {
            std::printf("refused: %s\n", e.what());
        }
        if (graph.solverStats().core != dense_limit) {
            std::printf("FAILED the refused setting changed the solver\n");
            return 1;
        }
        graph.setSolver(MRS_PGO_SOLVER_DENSE);
        put(out, graph.solverStats());
        const mrslam::PoseGraph::Result d = graph.optimize();
        out.insert(out.end(), r.poses.begin(), r.poses.end());
        out.insert(out.end(), d.poses.begin(), d.poses.end());
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
