// pcm_cov.hpp -- pairwise consistency under covariances (pcm.hip), for the device and, compiled by g++, for the CPU tests.
//
// The Mahalanobis distance of the cycle pose of two loops under the covariance propagated around the cycle (computeConsistencyError,
// pairwise_consistency.cpp:99-128, with gtsam's Jacobians of compose / between restated from upstream GTSAM 4.0).  Tangent order is gtsam's
// Pose3 order, rotation then translation, and Ad(T) = [[R, 0], [[t]x R, R]].  Every covariance is moved to the world frame through its own
// pose, so that a trajectory contributes a difference (or a sum) of two per-pose prefixes W and a pair costs two conjugations by an adjoint,
// one Logmap and one 6x6 Cholesky solve.
//
// A symmetric 6x6 is 21 doubles in 3x3 blocks: A (rotation, 6: 00 01 02 11 12 22) | B (rotation x translation, 9, row-major) | D (translation,
// 6).  Only those 21 are ever computed, so a result is symmetric by construction.  Everything is fp64; the caller compiles without contraction.
#pragma once
#include <cstddef>

#include "pcm_pose.hpp"

#if defined(__HIPCC__)
#define MRS_PCM_UNROLL _Pragma("unroll")
#else
#define MRS_PCM_UNROLL
#endif

namespace mrs {
namespace pcm {

constexpr int kSym = 21;                              // doubles per symmetric 6x6
constexpr int kCovRecord = kRecord + kSym + 3;        // P | B | CZ = Ad(B) C Ad(B)^T | i | k | one of padding: 48 doubles
constexpr int kRecCZ = kRecord, kRecI = kRecord + kSym, kRecK = kRecI + 1;
constexpr int kCovNone = 0, kCovSpan = 1, kCovReference = 2;
constexpr double kFixedRot = 0.0001, kFixedTrans = 0.01;      // FIXED_COVARIANCE (graph_types.h:79-85): its diagonal

MRS_PCM_HD int sym3_at(int r, int c) { return r <= c ? (r == 0 ? c : r + c + 1) : (c == 0 ? r : r + c + 1); }       // 00 01 02 11 12 22

// entry (i, j) of the 21-double storage
MRS_PCM_HD double sym_get(const double* s, int i, int j)
{
    if (i > j) { const int t = i; i = j; j = t; }
    if (j < 3) return s[sym3_at(i, j)];
    if (i < 3) return s[6 + 3 * i + (j - 3)];
    return s[15 + sym3_at(i - 3, j - 3)];
}

// from the lower triangle of a row-major 6x6, and back to a full one
MRS_PCM_HD void sym_from_lower(const double* m, double* s)
{
    MRS_PCM_UNROLL
    for (int r = 0; r < 3; ++r) {
        MRS_PCM_UNROLL
        for (int c = 0; c < 3; ++c) {
            if (r <= c) {
                s[sym3_at(r, c)] = m[6 * c + r];
                s[15 + sym3_at(r, c)] = m[6 * (3 + c) + 3 + r];
            }
            s[6 + 3 * r + c] = m[6 * (3 + c) + r];
        }
    }
}

MRS_PCM_HD void sym_to_dense(const double* s, double* m)
{
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) m[6 * i + j] = sym_get(s, i, j);
}

MRS_PCM_HD void sym_fixed(double* s)
{
    for (int e = 0; e < kSym; ++e) s[e] = 0.0;
    s[0] = s[3] = s[5] = kFixedRot;
    s[15] = s[18] = s[20] = kFixedTrans;
}

// out = R x R^T for the rotation R of pose p and a full row-major 3x3 x (out must not alias x)
MRS_PCM_HD void rot_conj(const double* p, const double* x, double* out)
{
    double rx[9];
    MRS_PCM_UNROLL
    for (int r = 0; r < 3; ++r) {
        MRS_PCM_UNROLL
        for (int c = 0; c < 3; ++c) rx[3 * r + c] = (p[4 * r] * x[c] + p[4 * r + 1] * x[3 + c]) + p[4 * r + 2] * x[6 + c];
    }
    MRS_PCM_UNROLL
    for (int r = 0; r < 3; ++r) {
        MRS_PCM_UNROLL
        for (int c = 0; c < 3; ++c) out[3 * r + c] = (rx[3 * r] * p[4 * c] + rx[3 * r + 1] * p[4 * c + 1]) + rx[3 * r + 2] * p[4 * c + 2];
    }
}

// R s R^T of a packed symmetric 3x3 -> packed
MRS_PCM_HD void rot_conj_sym(const double* p, const double* s, double* out)
{
    const double x[9] = {s[0], s[1], s[2], s[1], s[3], s[4], s[2], s[4], s[5]};
    double f[9];
    rot_conj(p, x, f);
    out[0] = f[0]; out[1] = f[1]; out[2] = f[2]; out[3] = f[4]; out[4] = f[5]; out[5] = f[8];
}

// out = [t]x x: every column c of out is t x (column c of x)
MRS_PCM_HD void cross_cols(double t0, double t1, double t2, const double* x, double* out)
{
    MRS_PCM_UNROLL
    for (int c = 0; c < 3; ++c) {
        out[c] = t1 * x[6 + c] - t2 * x[3 + c];
        out[3 + c] = t2 * x[c] - t0 * x[6 + c];
        out[6 + c] = t0 * x[3 + c] - t1 * x[c];
    }
}

// out = Ad(p) s Ad(p)^T.  With A' = R A R^T, B' = R B R^T, D' = R D R^T and K = [t]x:
//   A_out = A',  B_out = (K A')^T + B',  D_out = K B_out + (K B')^T + D'  (its upper triangle)
MRS_PCM_HD void adj_conj(const double* p, const double* s, double* out)
{
    const double t0 = p[3], t1 = p[7], t2 = p[11];
    double a[6], b[9], d[6], ka[9], kb[9], kn[9];
    rot_conj_sym(p, s, a);
    rot_conj(p, s + 6, b);
    rot_conj_sym(p, s + 15, d);
    const double af[9] = {a[0], a[1], a[2], a[1], a[3], a[4], a[2], a[4], a[5]};
    cross_cols(t0, t1, t2, af, ka);
    cross_cols(t0, t1, t2, b, kb);
    MRS_PCM_UNROLL
    for (int e = 0; e < 6; ++e) out[e] = a[e];
    MRS_PCM_UNROLL
    for (int r = 0; r < 3; ++r) {
        MRS_PCM_UNROLL
        for (int c = 0; c < 3; ++c) out[6 + 3 * r + c] = ka[3 * c + r] + b[3 * r + c];
    }
    cross_cols(t0, t1, t2, out + 6, kn);
    out[15] = (kn[0] + kb[0]) + d[0];
    out[16] = (kn[1] + kb[3]) + d[1];
    out[17] = (kn[2] + kb[6]) + d[2];
    out[18] = (kn[4] + kb[4]) + d[3];
    out[19] = (kn[5] + kb[7]) + d[4];
    out[20] = (kn[8] + kb[8]) + d[5];
}

// y = Ad(p) x: [R w, t x (R w) + R v]
MRS_PCM_HD void adj_apply(const double* p, const double* x, double* y)
{
    double rw[3], rv[3];
    MRS_PCM_UNROLL
    for (int r = 0; r < 3; ++r) {
        rw[r] = (p[4 * r] * x[0] + p[4 * r + 1] * x[1]) + p[4 * r + 2] * x[2];
        rv[r] = (p[4 * r] * x[3] + p[4 * r + 1] * x[4]) + p[4 * r + 2] * x[5];
    }
    y[0] = rw[0]; y[1] = rw[1]; y[2] = rw[2];
    y[3] = (p[7] * rw[2] - p[11] * rw[1]) + rv[0];
    y[4] = (p[11] * rw[0] - p[3] * rw[2]) + rv[1];
    y[5] = (p[3] * rw[1] - p[7] * rw[0]) + rv[2];
}

// y^T S^-1 y through the Cholesky factor of S; NaN when a pivot is not positive and finite or the result is not finite
MRS_PCM_HD double chol_norm2(const double* s, const double* y)
{
    const double kMax = 1.7976931348623157e308, kNaN = __builtin_nan("");
    double l[kSym], z[6];                             // l (i, j), i >= j, at i (i + 1) / 2 + j
    bool ok = true;
    double d2 = 0.0;
    MRS_PCM_UNROLL
    for (int j = 0; j < 6; ++j) {
        double d = sym_get(s, j, j);
        MRS_PCM_UNROLL
        for (int k = 0; k < j; ++k) d -= l[j * (j + 1) / 2 + k] * l[j * (j + 1) / 2 + k];
        ok = ok && d > 0.0 && d <= kMax;
        const double r = sqrt(d);
        l[j * (j + 1) / 2 + j] = r;
        MRS_PCM_UNROLL
        for (int i = j + 1; i < 6; ++i) {
            double e = sym_get(s, i, j);
            MRS_PCM_UNROLL
            for (int k = 0; k < j; ++k) e -= l[i * (i + 1) / 2 + k] * l[j * (j + 1) / 2 + k];
            l[i * (i + 1) / 2 + j] = e / r;
        }
        double w = y[j];
        MRS_PCM_UNROLL
        for (int k = 0; k < j; ++k) w -= l[j * (j + 1) / 2 + k] * z[k];
        z[j] = w / r;
        d2 += z[j] * z[j];
    }
    return ok && d2 <= kMax ? d2 : kNaN;              // a NaN fails the comparison too
}

// true if the symmetric matrix has a Cholesky factor with positive finite pivots and no entry that is not finite
MRS_PCM_HD bool sym_is_pd(const double* s)
{
    const double zero[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int e = 0; e < kSym; ++e)
        if (!(fabs(s[e]) <= 1.7976931348623157e308)) return false;
    const double d2 = chol_norm2(s, zero);
    return d2 == d2;
}

// the record of loop (i, k, Z, C): P = XA_i Z XB_k^-1, B = XB_k, CZ = Ad(B) C Ad(B)^T, and the two pose numbers
MRS_PCM_HD void loop_record_cov(const double* XA_i, const double* Z, const double* XB_k, const double* C, int i, int k, double* rec)
{
    loop_record(XA_i, Z, XB_k, rec);
    adj_conj(rec + kPose, C, rec + kRecCZ);
    rec[kRecI] = (double)i;
    rec[kRecK] = (double)k;
    rec[kRecK + 1] = 0.0;
}

// Loops u < v from their records and the prefix tables WA [na][21], WB [nb][21] (SPAN: W_n = sum_{m<n} Ad(X_m+1) Q_m Ad(X_m+1)^T; REFERENCE:
// that plus Ad(X_0) first Ad(X_0)^T) -> xi = Logmap(E), M with Sigma_E = Ad(B_u^-1) M Ad(B_u^-1)^T, and y = Ad(B_u) xi:
//   M = ((Ad(P_v^-1) dA Ad(P_v^-1)^T + CZ_v) + dB) + Ad(P_v^-1 P_u) CZ_u Ad(P_v^-1 P_u)^T
// with dA = +-(WA_j - WA_i), the sign that makes it positive semidefinite (REFERENCE: WA_j + WA_i), and dB likewise from l = k_v to k = k_u.
MRS_PCM_HD void pair_cov(const double* rec_u, const double* rec_v, const double* WA, const double* WB, int mode, double* xi, double* M, double* y)
{
    const int i = (int)rec_u[kRecI], k = (int)rec_u[kRecK], j = (int)rec_v[kRecI], l = (int)rec_v[kRecK];
    const bool ref = mode == kCovReference;
    const double aj = ref || j >= i ? 1.0 : -1.0, ai = ref ? 1.0 : -aj;
    const double bk = ref || k >= l ? 1.0 : -1.0, bl = ref ? 1.0 : -bk;
    double pinv[kPose], g[kPose], delta[kSym], t[kSym];
    pose_inv(rec_v, pinv);
    MRS_PCM_UNROLL
    for (int e = 0; e < kSym; ++e) delta[e] = aj * WA[(size_t)j * kSym + e] + ai * WA[(size_t)i * kSym + e];
    adj_conj(pinv, delta, M);
    MRS_PCM_UNROLL
    for (int e = 0; e < kSym; ++e)
        M[e] = (M[e] + rec_v[kRecCZ + e]) + (bk * WB[(size_t)k * kSym + e] + bl * WB[(size_t)l * kSym + e]);
    pose_mul(pinv, rec_u, g);                         // P_v^-1 P_u
    adj_conj(g, rec_u + kRecCZ, t);
    MRS_PCM_UNROLL
    for (int e = 0; e < kSym; ++e) M[e] += t[e];
    // the cycle pose exactly as pair_distance takes it
    double uinv[kPose], m[kPose], binv[kPose], mb[kPose], e[kPose];
    pose_inv(rec_u, uinv);
    pose_mul(uinv, rec_v, m);
    pose_inv(rec_u + kPose, binv);
    pose_mul(m, rec_u + kPose, mb);
    pose_mul(binv, mb, e);
    pose_logmap(e, xi);
    adj_apply(rec_u + kPose, xi, y);
}

// the squared Mahalanobis distance of loops u < v; NaN when it is not finite or Sigma_E has no Cholesky factor
MRS_PCM_HD double pair_mahalanobis2(const double* rec_u, const double* rec_v, const double* WA, const double* WB, int mode)
{
    double xi[6], M[kSym], y[6];
    pair_cov(rec_u, rec_v, WA, WB, mode, xi, M, y);
    return chol_norm2(M, y);
}

// the same with xi and Sigma_E [6][6] written out (mrs_pcm_get_pair, tests)
MRS_PCM_HD double pair_mahalanobis2_full(const double* rec_u, const double* rec_v, const double* WA, const double* WB, int mode, double* xi,
                                         double* sigma)
{
    double M[kSym], y[6], binv[kPose], se[kSym];
    pair_cov(rec_u, rec_v, WA, WB, mode, xi, M, y);
    pose_inv(rec_u + kPose, binv);
    adj_conj(binv, M, se);
    sym_to_dense(se, sigma);
    return chol_norm2(M, y);
}

// one step of the world-frame prefix: W_next = W + Ad(X_next) Q Ad(X_next)^T (X_next: 12 doubles)
MRS_PCM_HD void prefix_step(const double* X_next, const double* Q, const double* W, double* W_next)
{
    double t[kSym];
    adj_conj(X_next, Q, t);
    for (int e = 0; e < kSym; ++e) W_next[e] = W[e] + t[e];
}

// the prefixes of a trajectory X [n] (row-major 4x4 each) with step covariances Q [n - 1][21]: W_0 = base (nullptr: zero), in sequence
MRS_PCM_HD void prefix_table(const double* X, int n, const double* Q, const double* base, double* W)
{
    for (int e = 0; e < kSym; ++e) W[e] = base ? base[e] : 0.0;
    for (int m = 0; m + 1 < n; ++m) {
        double x[kPose];
        pose_from_4x4(X + (size_t)(m + 1) * 16, x);
        prefix_step(x, Q + (size_t)m * kSym, W + (size_t)m * kSym, W + (size_t)(m + 1) * kSym);
    }
}

}  // namespace pcm
}  // namespace mrs
