// pclgicp_bfgs.hpp -- the per-pair tail of PCL-style GICP in fp64: the objective of
// pcl::GeneralizedIterativeClosestPoint with the Mahalanobis matrices frozen, as an exact quadratic form in the 12 entries of (R, t) whose
// coefficients are 74 sums over the correspondences; a BFGS over (t, roll, pitch, yaw) on those sums; the pose update and PCL's stopping rule.
// PCL is not part of the reference tree: the definition in DESIGN.md 4.15 is the contract, tests/golden/pclgicp_restate.py restates it in
// NumPy, parity with PCL itself is unpinned (the line search in particular is the one defined there, not GSL's vector_bfgs2).
//
// With p = A_i - c, q = B_j - c (c: the pivot) and r_a the a-th COLUMN of R,
//      n f = sum_ab r_a^T Q_ab r_b + 2 sum_a t^T P_a r_a + t^T S t - 2 sum_a r_a^T w_a - 2 t^T v + k
// with S = sum M, v = sum M q, k = sum q^T M q, P_a = sum p_a M, w_a = sum p_a M q, Q_ab = sum p_a p_b M, and t the translation of the
// pivot-centred pose (t~ = t + R c - c).  Layout of the sums (symmetric 3x3 as xx xy xz yy yz zz):
//      [0] n   [1,7) S   [7,10) v   [10] k   [11,29) P_a (a major)   [29,38) w_a (a major)   [38,74) Q_ab ((a,b) = xx xy xz yy yz zz)
// Every loop has constant bounds and every array a constant index after unrolling: the device build keeps all of it in registers.
// Compiled for the device by hipcc and for the host by g++ (tests/cpp/pclgicp_bfgs_host.cpp, tests/test_pclgicp_cpu.py).
#pragma once
#include <cfloat>
#include <cmath>

#include "eig3.hpp"

#if defined(__HIPCC__)
#define MRS_UNROLL _Pragma("unroll")
#else
#define MRS_UNROLL
#endif

namespace mrs {

constexpr int kPclTerms = 74;

// state codes: the ICP numbering (icp_update.hpp), of which GICP uses 0, 1, 2 and 5
enum PclGicpState { PCL_NOT_CONVERGED = 0, PCL_ITERATIONS = 1, PCL_TRANSFORM = 2, PCL_NO_CORRESPONDENCES = 5 };
// how the inner minimisation ended
enum PclInnerEnd { PCL_END_GRADIENT = 0, PCL_END_LIMIT = 1, PCL_END_NO_PROGRESS = 2 };

struct PclGicpCriteria {
    double rot_eps;      // rotation_epsilon: scale of the rotation entries of the pose change
    double trans_eps;    // transformation_epsilon: scale of its translation entries
    double grad_tol;     // gradient_tolerance of the inner minimisation
    int max_iter;
    int max_inner;
    int force_iters;     // > 0: exactly this many outer iterations, no stopping rule
    int pad;
};

constexpr int pcl_sym6(int r, int c) { return r <= c ? 3 * r - (r * (r - 1)) / 2 + (c - r) : 3 * c - (c * (c - 1)) / 2 + (r - c); }

// u = M v for a symmetric 3x3 stored as 6
MRS_HD void pcl_symv(const double* m6, const double* v, double* u)
{
MRS_UNROLL
    for (int i = 0; i < 3; ++i) u[i] = m6[pcl_sym6(i, 0)] * v[0] + m6[pcl_sym6(i, 1)] * v[1] + m6[pcl_sym6(i, 2)] * v[2];
}

// R = Rz(x[5]) Ry(x[4]) Rx(x[3]) (row-major) and, when dR is not null, its three partial derivatives dR[9 k + .] by angle k
MRS_HD void pcl_rotation(const double* x, double* R, double* dR)
{
    const double cf = cos(x[3]), sf = sin(x[3]), ct = cos(x[4]), st = sin(x[4]), cp = cos(x[5]), sp = sin(x[5]);
    R[0] = cp * ct; R[1] = cp * st * sf - sp * cf; R[2] = cp * st * cf + sp * sf;
    R[3] = sp * ct; R[4] = sp * st * sf + cp * cf; R[5] = sp * st * cf - cp * sf;
    R[6] = -st;     R[7] = ct * sf;                R[8] = ct * cf;
    if (!dR) return;
    dR[0] = 0.0; dR[1] = cp * st * cf + sp * sf; dR[2] = -cp * st * sf + sp * cf;
    dR[3] = 0.0; dR[4] = sp * st * cf - cp * sf; dR[5] = -sp * st * sf - cp * cf;
    dR[6] = 0.0; dR[7] = ct * cf;                dR[8] = -ct * sf;
    dR[9] = -cp * st;  dR[10] = cp * ct * sf; dR[11] = cp * ct * cf;
    dR[12] = -sp * st; dR[13] = sp * ct * sf; dR[14] = sp * ct * cf;
    dR[15] = -ct;      dR[16] = -st * sf;     dR[17] = -st * cf;
    dR[18] = -sp * ct; dR[19] = -sp * st * sf - cp * cf; dR[20] = -sp * st * cf + cp * sf;
    dR[21] = cp * ct;  dR[22] = cp * st * sf - sp * cf;  dR[23] = cp * st * cf + sp * sf;
    dR[24] = 0.0;      dR[25] = 0.0;                     dR[26] = 0.0;
}

// f(x) from the 74 sums; g (6, may be null): its exact gradient
MRS_HD double pcl_objective(const double* s, const double* x, double* g)
{
    double R[9], dR[27];
    pcl_rotation(x, R, g ? dR : nullptr);
    const double n = s[0];
    const double t[3] = {x[0], x[1], x[2]};
    double col[3][3];       // col[a] = r_a
MRS_UNROLL
    for (int a = 0; a < 3; ++a)
MRS_UNROLL
        for (int i = 0; i < 3; ++i) col[a][i] = R[3 * i + a];
    double St[3], Bt[3] = {0.0, 0.0, 0.0};
    pcl_symv(s + 1, t, St);
    double val = t[0] * (St[0] - 2.0 * s[7]) + t[1] * (St[1] - 2.0 * s[8]) + t[2] * (St[2] - 2.0 * s[9]) + s[10];
    double gr[3][3];        // n/2 times the gradient by r_a
MRS_UNROLL
    for (int a = 0; a < 3; ++a) {
        double A[3] = {0.0, 0.0, 0.0}, u[3], Ca[3];
MRS_UNROLL
        for (int b = 0; b < 3; ++b) {
            pcl_symv(s + 38 + 6 * pcl_sym6(a, b), col[b], u);
            A[0] += u[0]; A[1] += u[1]; A[2] += u[2];
        }
        pcl_symv(s + 11 + 6 * a, t, Ca);
        pcl_symv(s + 11 + 6 * a, col[a], u);
        Bt[0] += u[0]; Bt[1] += u[1]; Bt[2] += u[2];
        const double* w = s + 29 + 3 * a;
MRS_UNROLL
        for (int i = 0; i < 3; ++i) {
            val += col[a][i] * (A[i] + 2.0 * Ca[i] - 2.0 * w[i]);
            gr[a][i] = A[i] + Ca[i] - w[i];
        }
    }
    if (g) {
        const double k2 = 2.0 / n;
MRS_UNROLL
        for (int i = 0; i < 3; ++i) g[i] = k2 * (St[i] + Bt[i] - s[7 + i]);
MRS_UNROLL
        for (int k = 0; k < 3; ++k) {
            double d = 0.0;
MRS_UNROLL
            for (int a = 0; a < 3; ++a)
MRS_UNROLL
                for (int i = 0; i < 3; ++i) d += gr[a][i] * dR[9 * k + 3 * i + a];
            g[3 + k] = k2 * d;
        }
    }
    return val / n;
}

MRS_HD double pcl_dot6(const double* a, const double* b)
{
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3] + a[4] * b[4] + a[5] * b[5];
}

// x (6) from the pose X (row-major 4x4) and the pivot c: t~ = t + R c - c, roll / pitch / yaw of R = Rz Ry Rx
MRS_HD void pcl_params_from_pose(const double* X, const double* c, double* x)
{
MRS_UNROLL
    for (int r = 0; r < 3; ++r) x[r] = X[4 * r + 3] + (X[4 * r] * c[0] + X[4 * r + 1] * c[1] + X[4 * r + 2] * c[2]) - c[r];
    x[3] = atan2(X[9], X[10]);
    const double m = -X[8];
    x[4] = asin(m > 1.0 ? 1.0 : (m < -1.0 ? -1.0 : m));
    x[5] = atan2(X[4], X[0]);
}

// the pose of x: rotation R(x), translation t~ - R c + c
MRS_HD void pcl_pose_from_params(const double* x, const double* c, double* X)
{
    double R[9];
    pcl_rotation(x, R, nullptr);
MRS_UNROLL
    for (int r = 0; r < 3; ++r) {
        X[4 * r] = R[3 * r]; X[4 * r + 1] = R[3 * r + 1]; X[4 * r + 2] = R[3 * r + 2];
        X[4 * r + 3] = x[r] - (R[3 * r] * c[0] + R[3 * r + 1] * c[1] + R[3 * r + 2] * c[2]) + c[r];
    }
    X[12] = X[13] = X[14] = 0.0;
    X[15] = 1.0;
}

// Step 5: minimises f over x (in place) from the 74 sums.  Returns how it ended; *iterations: the iterations counted.
// One loop whose every pass evaluates f and its gradient once, at ONE call site (the first evaluation, then the line-search trials): two
// inlined copies of the objective with the sums hoisted into registers do not fit the register file of the device build.
MRS_HD int pcl_bfgs(const double* s, double grad_tol, int max_inner, double* x, int* iterations)
{
    double H[36], g[6], d[6], xn[6], gn[6];
MRS_UNROLL
    for (int i = 0; i < 36; ++i) H[i] = (i % 7 == 0) ? 1.0 : 0.0;
MRS_UNROLL
    for (int i = 0; i < 6; ++i) { xn[i] = x[i]; g[i] = d[i] = 0.0; }
    double f = 0.0, alpha = 1.0, gd = 0.0;
    bool scaled = false;
    int k = 0, trial = -1, end = PCL_END_LIMIT;      // trial -1: the evaluation at the start
    for (;;) {
        __asm__ volatile("" ::: "memory");          // the sums are read where they are used, not kept in 148 registers across the loop
        const double fn = pcl_objective(s, xn, gn);
        if (trial >= 0) {
            if (!(fn <= f + 0.01 * alpha * gd)) {   // Armijo test failed: halve, at most 30 trials
                alpha *= 0.5;
                if (++trial >= 30) { ++k; end = PCL_END_NO_PROGRESS; break; }
MRS_UNROLL
                for (int i = 0; i < 6; ++i) xn[i] = x[i] + alpha * d[i];
                continue;
            }
            ++k;
            double sv[6], yv[6], Hy[6];
MRS_UNROLL
            for (int i = 0; i < 6; ++i) { sv[i] = xn[i] - x[i]; yv[i] = gn[i] - g[i]; }
            const double sy = pcl_dot6(sv, yv), yy = pcl_dot6(yv, yv);
            if (sy > 1e-12 * sqrt(pcl_dot6(sv, sv)) * sqrt(yy)) {
                if (!scaled) {
                    scaled = true;
MRS_UNROLL
                    for (int i = 0; i < 36; ++i) H[i] = (i % 7 == 0) ? sy / yy : 0.0;
                }
                // (I - rho s y^T) H (I - rho y s^T) + rho s s^T = H - rho (s (Hy)^T + (Hy) s^T) + (rho^2 y^T H y + rho) s s^T
                const double rho = 1.0 / sy;
MRS_UNROLL
                for (int i = 0; i < 6; ++i) Hy[i] = pcl_dot6(H + 6 * i, yv);
                const double q = rho * rho * pcl_dot6(yv, Hy) + rho;
MRS_UNROLL
                for (int i = 0; i < 6; ++i)
MRS_UNROLL
                    for (int j = 0; j < 6; ++j) H[6 * i + j] += -rho * (sv[i] * Hy[j] + Hy[i] * sv[j]) + q * sv[i] * sv[j];
            }
        }
        // x, f, g move to the evaluated point; the next iteration starts
MRS_UNROLL
        for (int i = 0; i < 6; ++i) { x[i] = xn[i]; g[i] = gn[i]; }
        f = fn;
        if (k >= max_inner) { end = PCL_END_LIMIT; break; }
        const double gnorm = sqrt(pcl_dot6(g, g));
        if (gnorm < grad_tol) { end = PCL_END_GRADIENT; break; }
MRS_UNROLL
        for (int i = 0; i < 6; ++i) d[i] = -pcl_dot6(H + 6 * i, g);
        gd = pcl_dot6(g, d);
        if (!(gd < 0.0)) {
MRS_UNROLL
            for (int i = 0; i < 36; ++i) H[i] = (i % 7 == 0) ? 1.0 : 0.0;
MRS_UNROLL
            for (int i = 0; i < 6; ++i) d[i] = -g[i];
            gd = -pcl_dot6(g, g);
        }
        alpha = (k == 0 && 0.01 / gnorm < 1.0) ? 0.01 / gnorm : 1.0;
        trial = 0;
MRS_UNROLL
        for (int i = 0; i < 6; ++i) xn[i] = x[i] + alpha * d[i];
    }
    *iterations = k;
    return end;
}

// Steps 5-7 for one pair: X (row-major 4x4, in: the pose of this iteration, out: the next), the largest scaled entry-wise change in *delta.
MRS_HD int pcl_gicp_iterate(const double* s, const double* c, const PclGicpCriteria& crit, double* X, double* delta, int* inner_iterations)
{
    double x[6], Xn[16];
    pcl_params_from_pose(X, c, x);
    const int end = pcl_bfgs(s, crit.grad_tol, crit.max_inner, x, inner_iterations);
    pcl_pose_from_params(x, c, Xn);
    double dl = 0.0;
MRS_UNROLL
    for (int r = 0; r < 3; ++r)
MRS_UNROLL
        for (int cc = 0; cc < 4; ++cc) dl = eig3_max(dl, fabs(Xn[4 * r + cc] - X[4 * r + cc]) / (cc < 3 ? crit.rot_eps : crit.trans_eps));
MRS_UNROLL
    for (int i = 0; i < 16; ++i) X[i] = Xn[i];
    *delta = dl;
    return end;
}

// Step 7 after outer iteration `it` (counted from 1): the state that ends the pair, or PCL_NOT_CONVERGED (forced runs: the caller stops them)
MRS_HD int pcl_gicp_converged(const PclGicpCriteria& crit, int it, double delta)
{
    if (crit.force_iters > 0) return PCL_NOT_CONVERGED;
    if (it >= crit.max_iter) return PCL_ITERATIONS;
    if (delta < 1.0) return PCL_TRANSFORM;
    return PCL_NOT_CONVERGED;
}

}  // namespace mrs
