// The weighted and robust part of posegraph_factor.hpp, the text the pose-graph kernels compile, built for the host
// (tests/test_posegraph_robust_cpu.py).
//   weighted IN OUT : IN = int32 n | double Ti [n][16] | Tj [n][16] | Z [n][16] | C [n][36] | Tk [n][16] (the pose whose rotation is Rhat)
//                       -> OUT = per factor wr, Lt [10] | e^T L e [1] | e [12] | Hi^T L Hi [36] | Hi^T L Hj [36] | -Hi^T L e [6] | -Hj^T L e [6]
//   kernel   IN OUT : IN = int32 n | double kernel [n] | k [n] | r2 [n]  ->  OUT = per entry w, rho
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "posegraph_factor.hpp"

namespace P = mrs::pgo;

template <class T>
static bool rd(FILE* f, std::vector<T>& v) { return v.empty() || std::fread(v.data(), sizeof(T), v.size(), f) == v.size(); }

int main(int argc, char** argv)
{
    if (argc != 4) return 2;
    FILE* f = std::fopen(argv[2], "rb");
    if (!f) return 2;
    int32_t n = 0;
    if (std::fread(&n, 4, 1, f) != 1 || n < 0) return 2;
    std::vector<double> out;
    if (!std::strcmp(argv[1], "weighted")) {
        constexpr int kOut = 10 + 1 + 12 + 36 + 36 + 6 + 6;
        std::vector<double> Ti(16 * (size_t)n), Tj(16 * (size_t)n), Z(16 * (size_t)n), C(36 * (size_t)n), Tk(16 * (size_t)n);
        if (!(rd(f, Ti) && rd(f, Tj) && rd(f, Z) && rd(f, C) && rd(f, Tk))) return 2;
        out.resize((size_t)kOut * n);
        for (int k = 0; k < n; ++k) {
            double a[P::kPose], b[P::kPose], z[P::kPose], t[P::kPose], terms[10];
            P::pose_from_4x4(&Ti[16 * (size_t)k], a);
            P::pose_from_4x4(&Tj[16 * (size_t)k], b);
            P::pose_from_4x4(&Z[16 * (size_t)k], z);
            P::pose_from_4x4(&Tk[16 * (size_t)k], t);
            double* o = &out[(size_t)kOut * k];
            P::covariance_terms(&C[36 * (size_t)k], terms);
            o[0] = terms[0];
            P::translation_information(t, terms + 1, o + 1);
            P::factor_normal_weighted(a, b, z, o[0], o + 1, o + 11, o + 23, o + 59, o + 95, o + 101);
            o[10] = P::factor_sq_weighted(o + 11, o[0], o + 1);
        }
    } else if (!std::strcmp(argv[1], "kernel")) {
        std::vector<double> kind((size_t)n), k((size_t)n), r2((size_t)n);
        if (!(rd(f, kind) && rd(f, k) && rd(f, r2))) return 2;
        out.resize(2 * (size_t)n);
        for (int u = 0; u < n; ++u) {
            out[2 * (size_t)u] = P::kernel_weight((int)kind[u], k[u], r2[u]);
            out[2 * (size_t)u + 1] = P::kernel_cost((int)kind[u], k[u], r2[u]);
        }
    } else {
        return 2;
    }
    std::fclose(f);
    FILE* o = std::fopen(argv[3], "wb");
    if (!o) return 2;
    std::fwrite(out.data(), sizeof(double), out.size(), o);
    std::fclose(o);
    return 0;
}
