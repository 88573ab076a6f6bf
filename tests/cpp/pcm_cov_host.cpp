// pcm_cov.hpp, the text the covariance kernels of pairwise consistency compile, built for the host (tests/test_pcm_cov_cpu.py).
//   pairs IN OUT : IN = int32 mode, na, nb, L | double XA [na][16] | XB [nb][16] | QA [na - 1][36] | QB [nb - 1][36] | first [36] |
//                       int32 ia [L] | kb [L] | double Z [L][16] | C [L][36]
//                  -> OUT = for every pair u < v in row-major order: double xi [6] | Sigma_E [36] | d2, evaluated as k_pcm_rows_cov does
//                     from records and prefix tables built as mrs_pcm_set_covariances and k_pcm_records_cov build them
//   pd IN OUT    : IN = int32 n | double m [n][36] -> OUT = double [n], 1 where the lower triangle is finite and positive definite
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "pcm_cov.hpp"

namespace P = mrs::pcm;

template <class T>
static bool rd(FILE* f, std::vector<T>& v) { return v.empty() || std::fread(v.data(), sizeof(T), v.size(), f) == v.size(); }

static std::vector<double> syms(const std::vector<double>& dense)
{
    std::vector<double> s(dense.size() / 36 * P::kSym);
    for (size_t e = 0; e < dense.size() / 36; ++e) P::sym_from_lower(&dense[36 * e], &s[P::kSym * e]);
    return s;
}

int main(int argc, char** argv)
{
    if (argc != 4) return 2;
    FILE* f = std::fopen(argv[2], "rb");
    if (!f) return 2;
    std::vector<double> out;
    if (!std::strcmp(argv[1], "pd")) {
        int32_t n = 0;
        if (std::fread(&n, 4, 1, f) != 1) return 2;
        std::vector<double> m(36 * (size_t)n);
        if (!rd(f, m)) return 2;
        const std::vector<double> s = syms(m);
        for (int e = 0; e < n; ++e) out.push_back(P::sym_is_pd(&s[(size_t)P::kSym * e]) ? 1.0 : 0.0);
    } else {
        int32_t h[4];
        if (std::fread(h, 4, 4, f) != 4) return 2;
        const int mode = h[0], na = h[1], nb = h[2], L = h[3];
        std::vector<double> XA(16 * (size_t)na), XB(16 * (size_t)nb), QA(36 * (size_t)(na - 1)), QB(36 * (size_t)(nb - 1)), first(36),
            Z(16 * (size_t)L), C(36 * (size_t)L);
        std::vector<int32_t> ia(L), kb(L);
        if (!(rd(f, XA) && rd(f, XB) && rd(f, QA) && rd(f, QB) && rd(f, first) && rd(f, ia) && rd(f, kb) && rd(f, Z) && rd(f, C))) return 2;
        const std::vector<double> qa = syms(QA), qb = syms(QB), fs = syms(first), cs = syms(C);
        double fa[P::kSym], fb[P::kSym], x0[P::kPose];
        P::pose_from_4x4(XA.data(), x0);
        P::adj_conj(x0, fs.data(), fa);
        P::pose_from_4x4(XB.data(), x0);
        P::adj_conj(x0, fs.data(), fb);
        const bool ref = mode == P::kCovReference;
        std::vector<double> WA((size_t)P::kSym * na), WB((size_t)P::kSym * nb), rec((size_t)P::kCovRecord * L);
        P::prefix_table(XA.data(), na, qa.data(), ref ? fa : nullptr, WA.data());
        P::prefix_table(XB.data(), nb, qb.data(), ref ? fb : nullptr, WB.data());
        for (int u = 0; u < L; ++u)
            P::loop_record_cov(&XA[16 * (size_t)ia[u]], &Z[16 * (size_t)u], &XB[16 * (size_t)kb[u]], &cs[(size_t)P::kSym * u], ia[u], kb[u],
                               &rec[(size_t)P::kCovRecord * u]);
        for (int u = 0; u < L; ++u)
            for (int v = u + 1; v < L; ++v) {
                double xi[6], sigma[36];
                const double d2 = P::pair_mahalanobis2_full(&rec[(size_t)P::kCovRecord * u], &rec[(size_t)P::kCovRecord * v], WA.data(), WB.data(),
                                                            mode, xi, sigma);
                const double plain = P::pair_mahalanobis2(&rec[(size_t)P::kCovRecord * u], &rec[(size_t)P::kCovRecord * v], WA.data(), WB.data(), mode);
                if (std::memcmp(&d2, &plain, sizeof(double)) != 0) return 3;        // one arithmetic behind both entry points
                out.insert(out.end(), xi, xi + 6);
                out.insert(out.end(), sigma, sigma + 36);
                out.push_back(d2);
            }
    }
    std::fclose(f);
    FILE* o = std::fopen(argv[3], "wb");
    if (!o) return 2;
    std::fwrite(out.data(), sizeof(double), out.size(), o);
    std::fclose(o);
    return 0;
}
