// Drives mrslam::PairwiseConsistency (include/mrslam/pcm.hpp) with covariances on a scene written by tests/test_pcm_cov_adapter.py:
//   in : int32 na, nb, L | double XA [na][16] | XB [nb][16] | QA [na - 1][36] | QB [nb - 1][36] | int32 ia [L] | kb [L] | double Z [L][16] |
//        C [L][36]
//   out: int32 size, rounds | int32 members [size]
#include <cstdio>
#include <vector>

#include "mrslam/pcm.hpp"

template <class T>
static bool rd(FILE* f, std::vector<T>& v) { return v.empty() || std::fread(v.data(), sizeof(T), v.size(), f) == v.size(); }

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    int32_t hdr[3];
    if (!f || std::fread(hdr, sizeof(int32_t), 3, f) != 3) return 2;
    const int na = hdr[0], nb = hdr[1], L = hdr[2];
    std::vector<double> XA(16 * na), XB(16 * nb), QA(36 * (na - 1)), QB(36 * (nb - 1)), Z(16 * L), C(36 * L);
    std::vector<int32_t> ia(L), kb(L);
    const bool ok = rd(f, XA) && rd(f, XB) && rd(f, QA) && rd(f, QB) && rd(f, ia) && rd(f, kb) && rd(f, Z) && rd(f, C);
    std::fclose(f);
    if (!ok) return 2;
    try {
        using mrslam::PairwiseConsistency;
        PairwiseConsistency pcm(L, PairwiseConsistency::Threshold{PairwiseConsistency::chiSquaredUpper(0.99)});
        pcm.setTrajectories(XA.data(), na, XB.data(), nb);
        pcm.setCovariances(MRS_PCM_COV_SPAN, QA.data(), QB.data(), nullptr);
        pcm.addLoops(ia.data(), kb.data(), Z.data(), C.data(), L);
        const std::vector<int> members = pcm.solve();
        const int32_t head[2] = {(int32_t)members.size(), pcm.rounds()};
        std::printf("loops=%d clique=%d rounds=%d\n", pcm.size(), head[0], head[1]);
        FILE* o = std::fopen(argv[2], "wb");
        if (!o) return 2;
        std::fwrite(head, sizeof(int32_t), 2, o);
        std::fwrite(members.data(), sizeof(int), members.size(), o);
        std::fclose(o);
    } catch (const std::exception& e) {
        std::printf("FAILED %s\n", e.what());
        return 1;
    }
    return 0;
}
