// posegraph_marginal.hpp, the text posegraph.hip compiles for its backward segment walk, built for the host
// (tests/test_posegraph_marginals_cpu.py).  Per problem the segments are eliminated as k_pgo_eliminate eliminates them (pivot factor L, the
// fill towards the left separator A, the block towards the next pose W) and then walked backwards with marginal_step from the blocks of a
// given inverse at the bounding poses.
//   in : per problem int32 N, nseg | double Hpp [N][36] = H(p, p) | double Hpn [N][36] = H(p, p + 1) | per segment int32 first, length,
//        left, right (1 where the bounding pose exists and is not held, else 0) and double S_ll, S_rl, S_rr [3][36] (zeros without it)
//   out: per problem double Spp [N][36] | double Spn [N][36] (S_{p, p + 1}); zeros where no segment writes
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "posegraph_marginal.hpp"

namespace {

constexpr int B = 6, BB = 36;

bool cholesky(double* D)
{
    for (int j = 0; j < B; ++j) {
        double d = D[j * B + j];
        for (int k = 0; k < j; ++k) d -= D[j * B + k] * D[j * B + k];
        if (!(d > 0.0) || !std::isfinite(d)) return false;
        d = std::sqrt(d);
        D[j * B + j] = d;
        for (int i = j + 1; i < B; ++i) {
            double s = D[i * B + j];
            for (int k = 0; k < j; ++k) s -= D[i * B + k] * D[j * B + k];
            D[i * B + j] = s / d;
        }
    }
    return true;
}

// M <- L^-1 M
void lower_solve(const double* L, double* M)
{
    for (int c = 0; c < B; ++c)
        for (int i = 0; i < B; ++i) {
            double s = M[i * B + c];
            for (int k = 0; k < i; ++k) s -= L[i * B + k] * M[k * B + c];
            M[i * B + c] = s / L[i * B + i];
        }
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    FILE* o = std::fopen(argv[2], "wb");
    if (!f || !o) return 2;
    int32_t hdr[2];
    while (std::fread(hdr, sizeof(int32_t), 2, f) == 2) {
        const int N = hdr[0], nseg = hdr[1];
        std::vector<double> Hpp((size_t)N * BB), Hpn((size_t)N * BB), Spp((size_t)N * BB, 0.0), Spn((size_t)N * BB, 0.0);
        if (std::fread(Hpp.data(), 8, Hpp.size(), f) != Hpp.size() || std::fread(Hpn.data(), 8, Hpn.size(), f) != Hpn.size()) return 2;
        for (int s = 0; s < nseg; ++s) {
            int32_t seg[4];
            double Sll[BB], Snl[BB], Snn[BB];
            if (std::fread(seg, 4, 4, f) != 4 || std::fread(Sll, 8, BB, f) != BB || std::fread(Snl, 8, BB, f) != BB ||
                std::fread(Snn, 8, BB, f) != BB)
                return 2;
            const int first = seg[0], m = seg[1];
            const bool left = seg[2] != 0, right = seg[3] != 0;
            if (first < (left ? 1 : 0) || m < 1 || first + m + (right ? 1 : 0) > N) return 2;
            std::vector<double> Lk((size_t)m * BB), Ak((size_t)m * BB), Wk((size_t)m * BB);
            double Ct[BB], cD[BB] = {0.0}, D[BB], W[BB], A[BB];
            for (int r = 0; r < B; ++r)                          // H(first, left) = H(left, first)^T
                for (int c = 0; c < B; ++c) Ct[r * B + c] = left ? Hpn[(size_t)(first - 1) * BB + c * B + r] : 0.0;
            for (int k = 0; k < m; ++k) {
                const int p = first + k;
                const bool has_next = k + 1 < m || right;
                for (int e = 0; e < BB; ++e) {
                    D[e] = Hpp[(size_t)p * BB + e] - cD[e];
                    W[e] = has_next ? Hpn[(size_t)p * BB + e] : 0.0;
                    A[e] = Ct[e];
                }
                if (!cholesky(D)) {
                    std::printf("FAILED the pivot block of pose %d is not positive definite\n", p);
                    return 1;
                }
                lower_solve(D, W);
                lower_solve(D, A);
                for (int a = 0; a < B; ++a)
                    for (int b = 0; b < B; ++b) {
                        double ww = 0.0, wa = 0.0;
                        for (int i = 0; i < B; ++i) {
                            ww += W[i * B + a] * W[i * B + b];
                            wa += W[i * B + a] * A[i * B + b];
                        }
                        cD[a * B + b] = ww;
                        Ct[a * B + b] = -wa;
                    }
                for (int e = 0; e < BB; ++e) {
                    Lk[(size_t)k * BB + e] = D[e];
                    Ak[(size_t)k * BB + e] = A[e];
                    Wk[(size_t)k * BB + e] = W[e];
                }
            }
            double pl[BB], pn[BB], pp[BB];
            for (int k = m - 1; k >= 0; --k) {
                const int p = first + k;
                mrs::pgo::marginal_step<B>(&Lk[(size_t)k * BB], &Ak[(size_t)k * BB], &Wk[(size_t)k * BB], Sll, Snl, Snn, pl, pn, pp);
                const bool has_next = k + 1 < m || right;
                for (int e = 0; e < BB; ++e) {
                    Spp[(size_t)p * BB + e] = pp[e];
                    Spn[(size_t)p * BB + e] = has_next ? pn[e] : 0.0;
                    Snl[e] = pl[e];
                    Snn[e] = pp[e];
                }
            }
            if (left)
                for (int r = 0; r < B; ++r)
                    for (int c = 0; c < B; ++c) Spn[(size_t)(first - 1) * BB + r * B + c] = Snl[c * B + r];
        }
        std::fwrite(Spp.data(), 8, Spp.size(), o);
        std::fwrite(Spn.data(), 8, Spn.size(), o);
    }
    std::fclose(f);
    std::fclose(o);
    return 0;
}
