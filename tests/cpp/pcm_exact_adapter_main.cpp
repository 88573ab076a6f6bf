// Drives mrslam::PairwiseConsistency::solveExact (include/mrslam/pcm.hpp) on a scene written by tests/test_pcm_exact_adapter.py:
//   in : int32 na, nb, L, p in percent | double XA [na][16] | XB [nb][16] | int32 ia [L] | kb [L] | double Z [L][16]
//   out: int32 size, proof, heuristic size, rounds | int32 members [size]
#include <cstdio>
#include <vector>

#include "mrslam/pcm.hpp"

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    int32_t hdr[4];
    if (!f || std::fread(hdr, sizeof(int32_t), 4, f) != 4) return 2;
    const int na = hdr[0], nb = hdr[1], L = hdr[2];
    std::vector<double> XA(16 * na), XB(16 * nb), Z(16 * L);
    std::vector<int32_t> ia(L), kb(L);
    bool ok = std::fread(XA.data(), 8, XA.size(), f) == XA.size() && std::fread(XB.data(), 8, XB.size(), f) == XB.size();
    ok = ok && std::fread(ia.data(), 4, L, f) == (size_t)L && std::fread(kb.data(), 4, L, f) == (size_t)L;
    ok = ok && std::fread(Z.data(), 8, Z.size(), f) == Z.size();
    std::fclose(f);
    if (!ok) return 2;
    try {
        mrslam::PairwiseConsistency pcm(L, hdr[3] / 100.0);
        pcm.setTrajectories(XA.data(), na, XB.data(), nb);
        pcm.addLoops(ia.data(), kb.data(), Z.data(), L);
        const std::vector<int> heuristic = pcm.solve();
        const int rounds = pcm.rounds();
        const std::vector<int> members = pcm.solveExact();
        if (pcm.solve() != heuristic || pcm.rounds() != rounds) throw std::runtime_error("solve() changed after solveExact()");
        const int32_t head[4] = {(int32_t)members.size(), pcm.proof(), (int32_t)heuristic.size(), rounds};
        std::printf("loops=%d exact=%d proof=%d nodes=%lld heuristic=%d\n", pcm.size(), head[0], head[1], (long long)pcm.nodes(), head[2]);
        FILE* o = std::fopen(argv[2], "wb");
        if (!o) return 2;
        std::fwrite(head, sizeof(int32_t), 4, o);
        std::fwrite(members.data(), sizeof(int), members.size(), o);
        std::fclose(o);
    } catch (const std::exception& e) {
        std::printf("FAILED %s\n", e.what());
        return 1;
    }
    return 0;
}
