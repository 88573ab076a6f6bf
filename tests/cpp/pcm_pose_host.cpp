// pcm_pose.hpp, the text the pairwise-consistency kernels compile, built for the host (tests/test_pcm_cpu.py).
//   logmap IN OUT : IN = int32 n | double poses [n][16]                                   -> OUT = double xi [n][6]
//   dist   IN OUT : IN = int32 na, nb, L | XA [na][16] | XB [nb][16] | int32 ia [L] | kb [L] | double Z [L][16]
//                                                                                           -> OUT = double d [L][L], evaluated as k_pcm_rows does
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "pcm_pose.hpp"

template <class T>
static bool rd(FILE* f, std::vector<T>& v) { return v.empty() || std::fread(v.data(), sizeof(T), v.size(), f) == v.size(); }

int main(int argc, char** argv)
{
    if (argc != 4) return 2;
    FILE* f = std::fopen(argv[2], "rb");
    if (!f) return 2;
    std::vector<double> out;
    if (!std::strcmp(argv[1], "logmap")) {
        int32_t n = 0;
        if (std::fread(&n, 4, 1, f) != 1) return 2;
        std::vector<double> T(16 * (size_t)n);
        if (!rd(f, T)) return 2;
        out.resize(6 * (size_t)n);
        for (int i = 0; i < n; ++i) {
            double p[mrs::pcm::kPose];
            mrs::pcm::pose_from_4x4(&T[16 * (size_t)i], p);
            mrs::pcm::pose_logmap(p, &out[6 * (size_t)i]);
        }
    } else {
        int32_t h[3];
        if (std::fread(h, 4, 3, f) != 3) return 2;
        const int na = h[0], nb = h[1], L = h[2];
        std::vector<double> XA(16 * (size_t)na), XB(16 * (size_t)nb), Z(16 * (size_t)L), rec((size_t)mrs::pcm::kRecord * L);
        std::vector<int32_t> ia(L), kb(L);
        if (!(rd(f, XA) && rd(f, XB) && rd(f, ia) && rd(f, kb) && rd(f, Z))) return 2;
        for (int u = 0; u < L; ++u)
            mrs::pcm::loop_record(&XA[16 * (size_t)ia[u]], &Z[16 * (size_t)u], &XB[16 * (size_t)kb[u]], &rec[(size_t)mrs::pcm::kRecord * u]);
        out.assign((size_t)L * L, 0.0);
        for (int u = 0; u < L; ++u)
            for (int v = 0; v < L; ++v)
                if (u != v) {
                    const int a = u < v ? u : v, b = u < v ? v : u;
                    out[(size_t)u * L + v] = mrs::pcm::pair_distance(&rec[(size_t)mrs::pcm::kRecord * a], &rec[(size_t)mrs::pcm::kRecord * b]);
                }
    }
    std::fclose(f);
    FILE* o = std::fopen(argv[3], "wb");
    if (!o) return 2;
    std::fwrite(out.data(), sizeof(double), out.size(), o);
    std::fclose(o);
    return 0;
}
