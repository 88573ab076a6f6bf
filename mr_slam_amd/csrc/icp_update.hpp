// icp_update.hpp -- the per-pair tail of point-to-point ICP in fp64: the rigid fit of
// pcl::registration::TransformationEstimationSVD (Umeyama without scale) from the 17 correspondence sums, and the stopping rules of
// pcl::registration::DefaultConvergenceCriteria with max_iterations_similar_transforms = 0.  PCL is not part of the reference tree: the
// definition in DESIGN.md 4.13 is the contract, tests/golden/icp_restate.py restates it in NumPy, parity with PCL itself is unpinned.
//
// The rotation: H = sum (a - abar)(b - bbar)^T = U S V^T, R = V diag(1, 1, det(V U^T)) U^T maximises tr(R H).  A one-sided (Hestenes)
// Jacobi on the matrix scaled to unit largest entry rotates the COLUMNS of H until they are orthogonal: H V = [s_i u_i].  Only the two
// dominant columns are used,
//      R = v1 u1^T + v2 u2^T + (v1 x v2)(u1 x u2)^T,
// which is V diag(1, 1, det(V U^T)) U^T whatever the signs of the third singular vectors are (v3 = det(V) v1 x v2, u3 = det(U) u1 x u2), so
// a reflection (det(V U^T) < 0) and a planar cloud (s3 = 0, u3 undefined) need no special case and det R = +1 by construction.  u2 is
// re-orthogonalised against u1 (twice); a collinear cloud (s2 <= 1e-13 s1: the loss in tr(R H) is below 2 s2) takes any unit vector orthogonal
// to u1 -- every proper rotation that maps the line onto the line attains the minimum; H = 0 gives the identity.
// Compiled for the device by hipcc and for the host by g++ (tests/cpp/icp_update_host.cpp, tests/test_icp_cpu.py checks this very text
// against LAPACK's SVD).
#pragma once
#include <cfloat>
#include <cmath>

#include "eig3.hpp"

namespace mrs {

// pcl::registration::DefaultConvergenceCriteria::ConvergenceState
enum IcpState {
    ICP_NOT_CONVERGED = 0,
    ICP_ITERATIONS = 1,
    ICP_TRANSFORM = 2,
    ICP_ABS_MSE = 3,
    ICP_REL_MSE = 4,
    ICP_NO_CORRESPONDENCES = 5
};

constexpr int kIcpTerms = 17;   // n, sum a (3), sum b (3), sum a b^T (9, row-major: a_r b_c), sum |b - a|^2

struct IcpCriteria {
    double trans_eps;   // compared with the SQUARED translation of the increment, as PCL does
    double rot_thr;     // cosine of the increment's angle that counts as "no rotation"
    double fit_eps;     // relative change of the mean squared error
    int max_iter;
    int force_iters;    // > 0: exactly this many iterations, no stopping rule
};

// PCL: rotation threshold = rotation_epsilon if set, else 1 - transformation_epsilon
MRS_HD double icp_rotation_threshold(double rotation_epsilon, double transformation_epsilon)
{
    return rotation_epsilon > 0.0 ? rotation_epsilon : 1.0 - transformation_epsilon;
}

MRS_HD void icp_identity3(double* R)
{
    for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0) ? 1.0 : 0.0;
}

// R (row-major 3x3, proper rotation) that maximises tr(R H); H row-major 3x3, any rank, any scale
MRS_HD void icp_rotation(const double* H, double* R)
{
    double m = 0.0;
    for (int i = 0; i < 9; ++i) m = eig3_max(m, fabs(H[i]));
    if (!(m > 0.0) || !(m <= DBL_MAX)) { icp_identity3(R); return; }      // zero matrix, NaN or inf
    double A[9], V[9];
    for (int i = 0; i < 9; ++i) { A[i] = H[i] / m; V[i] = (i % 4 == 0) ? 1.0 : 0.0; }
    for (int sweep = 0; sweep < 30; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                const double alpha = A[p] * A[p] + A[3 + p] * A[3 + p] + A[6 + p] * A[6 + p];
                const double beta = A[q] * A[q] + A[3 + q] * A[3 + q] + A[6 + q] * A[6 + q];
                const double gamma = A[p] * A[q] + A[3 + p] * A[3 + q] + A[6 + p] * A[6 + q];
                if (gamma == 0.0 || fabs(gamma) <= DBL_EPSILON * sqrt(alpha * beta)) continue;
                const double zeta = (beta - alpha) / (2.0 * gamma);
                const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));   // zeta^2 = inf: t = 0
                const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
                if (s == 0.0) continue;
                rotated = true;
                for (int r = 0; r < 3; ++r) {
                    const double ap = A[3 * r + p], aq = A[3 * r + q];
                    A[3 * r + p] = c * ap - s * aq;
                    A[3 * r + q] = s * ap + c * aq;
                    const double vp = V[3 * r + p], vq = V[3 * r + q];
                    V[3 * r + p] = c * vp - s * vq;
                    V[3 * r + q] = s * vp + c * vq;
                }
            }
        if (!rotated) break;
    }
    // the two longest columns of H V
    double nrm[3];
    for (int c = 0; c < 3; ++c) nrm[c] = sqrt(A[c] * A[c] + A[3 + c] * A[3 + c] + A[6 + c] * A[6 + c]);
    int i1 = 0;
    if (nrm[1] > nrm[i1]) i1 = 1;
    if (nrm[2] > nrm[i1]) i1 = 2;
    int i2 = i1 == 0 ? 1 : 0;
    for (int c = 0; c < 3; ++c)
        if (c != i1 && nrm[c] > nrm[i2]) i2 = c;
    if (!(nrm[i1] > 0.0)) { icp_identity3(R); return; }
    double u1[3], u2[3], u3[3], v1[3], v2[3], v3[3];
    for (int r = 0; r < 3; ++r) {
        u1[r] = A[3 * r + i1] / nrm[i1];
        u2[r] = A[3 * r + i2];
        v1[r] = V[3 * r + i1];
        v2[r] = V[3 * r + i2];
    }
    for (int pass = 0; pass < 2; ++pass) {
        const double d = u2[0] * u1[0] + u2[1] * u1[1] + u2[2] * u1[2];
        for (int r = 0; r < 3; ++r) u2[r] -= d * u1[r];
    }
    double n2 = sqrt(u2[0] * u2[0] + u2[1] * u2[1] + u2[2] * u2[2]);
    if (!(n2 > 1e-13 * nrm[i1])) {       // collinear: the unit axis least aligned with u1, made orthogonal to it
        int k = 0;
        if (fabs(u1[1]) < fabs(u1[k])) k = 1;
        if (fabs(u1[2]) < fabs(u1[k])) k = 2;
        for (int r = 0; r < 3; ++r) u2[r] = (r == k ? 1.0 : 0.0) - u1[k] * u1[r];
        for (int pass = 0; pass < 2; ++pass) {
            const double d = u2[0] * u1[0] + u2[1] * u1[1] + u2[2] * u1[2];
            for (int r = 0; r < 3; ++r) u2[r] -= d * u1[r];
        }
        n2 = sqrt(u2[0] * u2[0] + u2[1] * u2[1] + u2[2] * u2[2]);
    }
    for (int r = 0; r < 3; ++r) u2[r] /= n2;
    eig3_cross(u1, u2, u3);
    eig3_cross(v1, v2, v3);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) R[3 * r + c] = v1[r] * u1[c] + v2[r] * u2[c] + v3[r] * u3[c];
}

// Step 4: the increment D = [R t; 0 1] (row-major 4x4) from the 17 sums (s[0] >= 1).  Returns the mean squared error of the correspondences
// BEFORE the increment (what the convergence criteria compare).
MRS_HD double icp_rigid_fit(const double* s, double* D)
{
    const double n = s[0];
    const double abar[3] = {s[1] / n, s[2] / n, s[3] / n}, bbar[3] = {s[4] / n, s[5] / n, s[6] / n};
    double H[9], R[9];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) H[3 * r + c] = s[7 + 3 * r + c] - n * abar[r] * bbar[c];
    icp_rotation(H, R);
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) D[4 * r + c] = R[3 * r + c];
        D[4 * r + 3] = bbar[r] - (R[3 * r] * abar[0] + R[3 * r + 1] * abar[1] + R[3 * r + 2] * abar[2]);
    }
    D[12] = D[13] = D[14] = 0.0;
    D[15] = 1.0;
    return s[16] / n;
}

// Step 6 after iteration `it` (counted from 1) with increment D and this iteration's mean squared error; prev_mse starts at DBL_MAX and is
// updated when the pair goes on.  Returns the state that ends the pair, or ICP_NOT_CONVERGED.  The order of the tests is PCL's.
MRS_HD int icp_converged(const IcpCriteria& c, int it, const double* D, double mse, double& prev_mse)
{
    if (c.force_iters > 0) return ICP_NOT_CONVERGED;       // the caller stops at the forced count
    if (it >= c.max_iter) return ICP_ITERATIONS;
    const double cos_angle = 0.5 * (D[0] + D[5] + D[10] - 1.0);
    const double t2 = D[3] * D[3] + D[7] * D[7] + D[11] * D[11];
    if (cos_angle >= c.rot_thr && t2 <= c.trans_eps) return ICP_TRANSFORM;
    const double d = fabs(mse - prev_mse);
    if (d < 1e-12) return ICP_ABS_MSE;
    if (d / prev_mse < c.fit_eps) return ICP_REL_MSE;
    prev_mse = mse;
    return ICP_NOT_CONVERGED;
}

}  // namespace mrs
