// posegraph_factor.hpp -- the per-factor and per-pose arithmetic of the pose-graph optimiser (posegraph.hip), for the
// device and, compiled by g++, for the CPU tests (tests/cpp/posegraph_factor_host.cpp).
//
// A pose is 12 doubles, the row-major 3x4 [R | t].  The error and the Jacobians are BetweenChordalFactor::evaluateError
// (include/distributed_mapper/between_chordal_factor.h:97-144), the retraction is retractPose3Global (evaluation_utils.cpp:89-99) with
// Rodrigues' Exp standing for gtsam's Rot3::retract.  Everything is fp64; the caller compiles without contraction.
#pragma once
#include <cmath>

#include "eig3.hpp"

#if defined(__HIPCC__)
#define MRS_PGO_HD __host__ __device__ inline
#else
#define MRS_PGO_HD inline
#endif

namespace mrs {
namespace pgo {

constexpr int kPose = 12;                // doubles per pose
constexpr int kErr = 12;                 // rows of a factor's error
constexpr double kSmallAngle = 1e-4;     // below it Exp takes sin(t)/t and (1 - cos t)/t^2 from their series

// rows 0..2 of a row-major 4x4
MRS_PGO_HD void pose_from_4x4(const double* m, double* p)
{
    for (int i = 0; i < kPose; ++i) p[i] = m[i];
}

// E [9] = Exp(w) = I + a W + b W^2
MRS_PGO_HD void exp_so3(const double* w, double* E)
{
    const double x = w[0], y = w[1], z = w[2];
    const double t2 = (x * x + y * y) + z * z, t = sqrt(t2);
    double a, b;
    if (t < kSmallAngle) {
        a = 1.0 - t2 / 6.0;
        b = 0.5 - t2 / 24.0;
    } else {
        a = sin(t) / t;
        b = (1.0 - cos(t)) / t2;
    }
    // W^2 = w w^T - t2 I
    E[0] = 1.0 + b * (x * x - t2); E[1] = -a * z + b * (x * y);     E[2] = a * y + b * (x * z);
    E[3] = a * z + b * (x * y);    E[4] = 1.0 + b * (y * y - t2);   E[5] = -a * x + b * (y * z);
    E[6] = -a * y + b * (x * z);   E[7] = a * x + b * (y * z);      E[8] = 1.0 + b * (z * z - t2);
}

// out = [R Exp(d[0:3]) | t + d[3:6]] (out may alias T)
MRS_PGO_HD void retract(const double* T, const double* d, double* out)
{
    double E[9], R[9];
    exp_so3(d, E);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) R[3 * r + c] = (T[4 * r] * E[c] + T[4 * r + 1] * E[3 + c]) + T[4 * r + 2] * E[6 + c];
    for (int r = 0; r < 3; ++r) {
        const double t = T[4 * r + 3] + d[3 + r];
        out[4 * r] = R[3 * r]; out[4 * r + 1] = R[3 * r + 1]; out[4 * r + 2] = R[3 * r + 2];
        out[4 * r + 3] = t;
    }
}

// RiRij [9] = Ri Rij and e [12]: the columns of Ri Rij - Rj, then tj - ti - Ri tij
MRS_PGO_HD void factor_error(const double* Ti, const double* Tj, const double* Z, double* RiRij, double* e)
{
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) RiRij[3 * r + c] = (Ti[4 * r] * Z[c] + Ti[4 * r + 1] * Z[4 + c]) + Ti[4 * r + 2] * Z[8 + c];
    for (int c = 0; c < 3; ++c)
        for (int r = 0; r < 3; ++r) e[3 * c + r] = RiRij[3 * r + c] - Tj[4 * r + c];
    for (int r = 0; r < 3; ++r)
        e[9 + r] = (Tj[4 * r + 3] - Ti[4 * r + 3]) - ((Ti[4 * r] * Z[3] + Ti[4 * r + 1] * Z[7]) + Ti[4 * r + 2] * Z[11]);
}

// 0.5 |e|^2, summed in the order of e
MRS_PGO_HD double factor_half_sq(const double* e)
{
    double s = 0.0;
    for (int k = 0; k < kErr; ++k) s += e[k] * e[k];
    return 0.5 * s;
}

// the 12 x 3 rotation columns of Hi and Hj (row-major [12][3]); the translation columns are constant: rows 9..11 hold -I in Hi, +I in Hj
MRS_PGO_HD void factor_jacobians(const double* Ti, const double* Tj, const double* Z, const double* RiRij, double* Ai, double* Aj)
{
    // S_k = skewSymmetric(-e_k): (M S_k)[r][c] for a 3x3 M is M[r][c1] * sign, written out per k
    //   S1 = [0 0 0; 0 0 1; 0 -1 0], S2 = [0 0 -1; 0 0 0; 1 0 0], S3 = [0 1 0; -1 0 0; 0 0 0]
    for (int k = 0; k < 3; ++k) {
        const int u = (k + 1) % 3, v = (k + 2) % 3;          // S_k has +1 at (u, v) and -1 at (v, u)
        for (int r = 0; r < 3; ++r) {
            // (RiRij S_k)[r][.]: column v takes +RiRij[r][u], column u takes -RiRij[r][v]; then times Rij^T
            const double mv = RiRij[3 * r + u], mu = -RiRij[3 * r + v];
            for (int c = 0; c < 3; ++c) Ai[3 * (3 * k + r) + c] = mu * Z[4 * c + u] + mv * Z[4 * c + v];
            // -(Rj S_k)[r][.]
            Aj[3 * (3 * k + r) + u] = Tj[4 * r + v];
            Aj[3 * (3 * k + r) + v] = -Tj[4 * r + u];
            Aj[3 * (3 * k + r) + k] = 0.0;
        }
    }
    // Ri skew(tij)
    const double tx = Z[3], ty = Z[7], tz = Z[11];
    for (int r = 0; r < 3; ++r) {
        const double a = Ti[4 * r], b = Ti[4 * r + 1], c = Ti[4 * r + 2];
        Ai[3 * (9 + r)] = b * tz - c * ty;
        Ai[3 * (9 + r) + 1] = c * tx - a * tz;
        Ai[3 * (9 + r) + 2] = a * ty - b * tx;
        Aj[3 * (9 + r)] = 0.0; Aj[3 * (9 + r) + 1] = 0.0; Aj[3 * (9 + r) + 2] = 0.0;
    }
}

// Hj^T Hj = diag(2, 2, 2, 1, 1, 1) whenever Rj is a rotation
MRS_PGO_HD double hjj_diagonal(int k) { return k < 3 ? 2.0 : 1.0; }

// the normal-equation blocks of one factor: e [12], Hii = Hi^T Hi [36], Hij = Hi^T Hj [36] (rows of pose i, columns of pose j),
// gi = -Hi^T e [6], gj = -Hj^T e [6]
MRS_PGO_HD void factor_normal(const double* Ti, const double* Tj, const double* Z, double* e, double* Hii, double* Hij, double* gi, double* gj)
{
    double RiRij[9], Ai[36], Aj[36];
    factor_error(Ti, Tj, Z, RiRij, e);
    factor_jacobians(Ti, Tj, Z, RiRij, Ai, Aj);
    for (int a = 0; a < 3; ++a) {
        for (int b = 0; b < 3; ++b) {
            double sii = 0.0, sij = 0.0;
            for (int k = 0; k < 12; ++k) sii += Ai[3 * k + a] * Ai[3 * k + b];
            for (int k = 0; k < 9; ++k) sij += Ai[3 * k + a] * Aj[3 * k + b];
            Hii[6 * a + b] = sii;
            Hij[6 * a + b] = sij;
            // rotation rows against the translation columns: Hi's are -I in rows 9..11, Hj's are +I
            Hii[6 * a + 3 + b] = -Ai[3 * (9 + b) + a];
            Hii[6 * (3 + b) + a] = -Ai[3 * (9 + b) + a];
            Hij[6 * a + 3 + b] = Ai[3 * (9 + b) + a];
            Hij[6 * (3 + a) + b] = 0.0;
            Hii[6 * (3 + a) + 3 + b] = a == b ? 1.0 : 0.0;
            Hij[6 * (3 + a) + 3 + b] = a == b ? -1.0 : 0.0;
        }
        double si = 0.0, sj = 0.0;
        for (int k = 0; k < 12; ++k) si += Ai[3 * k + a] * e[k];
        for (int k = 0; k < 9; ++k) sj += Aj[3 * k + a] * e[k];
        gi[a] = -si;
        gj[a] = -sj;
        gi[3 + a] = e[9 + a];
        gj[3 + a] = -e[9 + a];
    }
}

// ------------------------------------------------------------------ per-factor noise and robust kernels
//
// A factor's information is wr on the nine rotation rows and the symmetric 3 x 3 Lt on the translation rows: what
// evaluation_utils::convertToChordalNoise (evaluation_utils.cpp:333-366) makes of a Pose3 covariance C, wr = 1 / max(C00, C11, C22) and
// Lt = Rhat (C[3:6, 3:6] + 0.01 I)^-1 Rhat^T.  The unit model is wr = 1, Lt = I.

constexpr double kTranslationFloor = 0.01;                       // evaluation_utils.cpp:361
enum Kernel : int { kKernelNone = 0, kKernelHuber = 1, kKernelCauchy = 2, kKernelGemanMcClure = 3 };

// o [10] = 1 / max(C00, C11, C22) and P = C[3:6, 3:6] + 0.01 I of the covariance C [36]: the part of the conversion that needs no pose
MRS_PGO_HD void covariance_terms(const double* C, double* o)
{
    const double m = C[0] > C[7] ? C[0] : C[7];
    o[0] = 1.0 / (m > C[14] ? m : C[14]);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) o[1 + 3 * r + c] = C[6 * (3 + r) + 3 + c] + (r == c ? kTranslationFloor : 0.0);
}

// Lt [9] = Rhat P^-1 Rhat^T for the positive definite P [9] (row-major, by cofactors) and the rotation block of the pose Tk [12]
MRS_PGO_HD void translation_information(const double* Tk, const double* P, double* Lt)
{
    double M[9], RM[9];
    M[0] = P[4] * P[8] - P[5] * P[7]; M[1] = P[2] * P[7] - P[1] * P[8]; M[2] = P[1] * P[5] - P[2] * P[4];
    M[3] = P[5] * P[6] - P[3] * P[8]; M[4] = P[0] * P[8] - P[2] * P[6]; M[5] = P[2] * P[3] - P[0] * P[5];
    M[6] = P[3] * P[7] - P[4] * P[6]; M[7] = P[1] * P[6] - P[0] * P[7]; M[8] = P[0] * P[4] - P[1] * P[3];
    const double det = (P[0] * M[0] + P[1] * M[3]) + P[2] * M[6];
    for (int k = 0; k < 9; ++k) M[k] /= det;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) RM[3 * r + c] = (Tk[4 * r] * M[c] + Tk[4 * r + 1] * M[3 + c]) + Tk[4 * r + 2] * M[6 + c];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c <= r; ++c) {
            const double v = (RM[3 * r] * Tk[4 * c] + RM[3 * r + 1] * Tk[4 * c + 1]) + RM[3 * r + 2] * Tk[4 * c + 2];
            Lt[3 * r + c] = v;
            Lt[3 * c + r] = v;
        }
}

// e^T Lambda e
MRS_PGO_HD double factor_sq_weighted(const double* e, double wr, const double* Lt)
{
    double s = 0.0, q = 0.0;
    for (int k = 0; k < 9; ++k) s += e[k] * e[k];
    for (int a = 0; a < 3; ++a) q += e[9 + a] * ((Lt[3 * a] * e[9] + Lt[3 * a + 1] * e[10]) + Lt[3 * a + 2] * e[11]);
    return wr * s + q;
}

// the weight w(r) of a robust kernel with parameter k at the squared residual r2 = e^T Lambda e: rho'(r) = w(r) r
MRS_PGO_HD double kernel_weight(int kernel, double k, double r2)
{
    if (kernel == kKernelHuber) {
        const double r = sqrt(r2);
        return r <= k ? 1.0 : k / r;
    }
    if (kernel == kKernelCauchy) return (k * k) / (k * k + r2);
    if (kernel == kKernelGemanMcClure) {
        const double s = (k * k) / (k * k + r2);
        return s * s;
    }
    return 1.0;
}

// its cost rho(r); 0.5 r2 without a kernel
MRS_PGO_HD double kernel_cost(int kernel, double k, double r2)
{
    if (kernel == kKernelHuber) {
        const double r = sqrt(r2);
        return r <= k ? 0.5 * r2 : k * (r - 0.5 * k);
    }
    if (kernel == kKernelCauchy) return 0.5 * (k * k) * log1p(r2 / (k * k));
    if (kernel == kKernelGemanMcClure) return 0.5 * (k * k) * r2 / (k * k + r2);
    return 0.5 * r2;
}

// factor_normal under the information (wr, Lt): Hii = Hi^T L Hi, Hij = Hi^T L Hj, gi = -Hi^T L e, gj = -Hj^T L e; e is not scaled.
// Hj^T L Hj is block diagonal, wr hjj_diagonal(k) for the rotation and Lt for the translation, whenever Rj is a rotation.
MRS_PGO_HD void factor_normal_weighted(const double* Ti, const double* Tj, const double* Z, double wr, const double* Lt, double* e, double* Hii,
                                       double* Hij, double* gi, double* gj)
{
    double RiRij[9], Ai[36], Aj[36], LK[9], Le[3];
    factor_error(Ti, Tj, Z, RiRij, e);
    factor_jacobians(Ti, Tj, Z, RiRij, Ai, Aj);
    const double* K = Ai + 27;                                   // rows 9..11 of Hi's rotation columns: Ri skew(tij)
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) LK[3 * r + c] = (Lt[3 * r] * K[c] + Lt[3 * r + 1] * K[3 + c]) + Lt[3 * r + 2] * K[6 + c];
        Le[r] = (Lt[3 * r] * e[9] + Lt[3 * r + 1] * e[10]) + Lt[3 * r + 2] * e[11];
    }
    for (int a = 0; a < 3; ++a) {
        for (int b = 0; b < 3; ++b) {
            double sii = 0.0, sij = 0.0, kk = 0.0;
            for (int k = 0; k < 9; ++k) sii += Ai[3 * k + a] * Ai[3 * k + b];
            for (int k = 0; k < 9; ++k) sij += Ai[3 * k + a] * Aj[3 * k + b];
            for (int r = 0; r < 3; ++r) kk += K[3 * r + a] * LK[3 * r + b];
            Hii[6 * a + b] = wr * sii + kk;
            Hij[6 * a + b] = wr * sij;
            // rotation rows against the translation columns: -K^T Lt in Hii, +K^T Lt in Hij (Lt is symmetric)
            Hii[6 * a + 3 + b] = -LK[3 * b + a];
            Hii[6 * (3 + b) + a] = -LK[3 * b + a];
            Hij[6 * a + 3 + b] = LK[3 * b + a];
            Hij[6 * (3 + a) + b] = 0.0;
            Hii[6 * (3 + a) + 3 + b] = Lt[3 * a + b];
            Hij[6 * (3 + a) + 3 + b] = -Lt[3 * a + b];
        }
        double si = 0.0, sj = 0.0, sk = 0.0;
        for (int k = 0; k < 9; ++k) si += Ai[3 * k + a] * e[k];
        for (int k = 0; k < 9; ++k) sj += Aj[3 * k + a] * e[k];
        for (int r = 0; r < 3; ++r) sk += K[3 * r + a] * Le[r];
        gi[a] = -(wr * si + sk);
        gj[a] = -(wr * sj);
        gi[3 + a] = Le[a];
        gj[3 + a] = -Le[a];
    }
}

// the rotation closest to X [9] (row-major) in the Frobenius norm, U diag(1, 1, det(U V^T)) V^T of X = U S V^T, as
// X V diag(1/s1, 1/s2, d/s3) V^T from the eigenpairs of X^T X (s3 the smallest singular value, d = sign det X).  X must have full rank.
MRS_PGO_HD void closest_rotation(const double* X, double* R)
{
    double G[9], w[3], v[9];
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) G[3 * a + b] = (X[a] * X[b] + X[3 + a] * X[3 + b]) + X[6 + a] * X[6 + b];
    sym3_eigvecs_desc(G, w, v);
    const double det = X[0] * (X[4] * X[8] - X[5] * X[7]) - X[1] * (X[3] * X[8] - X[5] * X[6]) + X[2] * (X[3] * X[7] - X[4] * X[6]);
    double P[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int k = 0; k < 3; ++k) {
        const double s = (k == 2 && det < 0.0 ? -1.0 : 1.0) / sqrt(w[k]);
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) P[3 * a + b] += s * v[3 * k + a] * v[3 * k + b];
    }
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) R[3 * r + c] = (X[3 * r] * P[c] + X[3 * r + 1] * P[3 + c]) + X[3 * r + 2] * P[6 + c];
}

}  // namespace pgo
}  // namespace mrs
