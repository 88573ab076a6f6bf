// posegraph_factor.hpp, the text the pose-graph kernels compile, built for the host (tests/test_posegraph_cpu.py).
//   factor IN OUT : IN = int32 n | double Ti [n][16] | Tj [n][16] | Z [n][16]
//                     -> OUT = per factor e [12] | Hi^T Hi [36] | Hi^T Hj [36] | -Hi^T e [6] | -Hj^T e [6] | 0.5 |e|^2 [1] | diag Hj^T Hj [6]
//   pose   IN OUT : IN = int32 n | double T [n][16] | delta [n][6] | X [n][9]
//                     -> OUT = per pose retract(T, delta) [12] | closest_rotation(X) [9]
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
    if (!std::strcmp(argv[1], "factor")) {
        constexpr int kOut = 12 + 36 + 36 + 6 + 6 + 1 + 6;
        std::vector<double> Ti(16 * (size_t)n), Tj(16 * (size_t)n), Z(16 * (size_t)n);
        if (!(rd(f, Ti) && rd(f, Tj) && rd(f, Z))) return 2;
        out.resize((size_t)kOut * n);
        for (int k = 0; k < n; ++k) {
            double a[P::kPose], b[P::kPose], z[P::kPose];
            P::pose_from_4x4(&Ti[16 * (size_t)k], a);
            P::pose_from_4x4(&Tj[16 * (size_t)k], b);
            P::pose_from_4x4(&Z[16 * (size_t)k], z);
            double* o = &out[(size_t)kOut * k];
            P::factor_normal(a, b, z, o, o + 12, o + 48, o + 84, o + 90);
            o[96] = P::factor_half_sq(o);
            for (int d = 0; d < 6; ++d) o[97 + d] = P::hjj_diagonal(d);
        }
    } else if (!std::strcmp(argv[1], "pose")) {
        std::vector<double> T(16 * (size_t)n), D(6 * (size_t)n), X(9 * (size_t)n);
        if (!(rd(f, T) && rd(f, D) && rd(f, X))) return 2;
        out.resize((size_t)21 * n);
        for (int k = 0; k < n; ++k) {
            double t[P::kPose];
            P::pose_from_4x4(&T[16 * (size_t)k], t);
            P::retract(t, &D[6 * (size_t)k], &out[(size_t)21 * k]);
            P::closest_rotation(&X[9 * (size_t)k], &out[(size_t)21 * k + 12]);
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
