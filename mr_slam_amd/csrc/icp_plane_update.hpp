// icp_plane_update.hpp -- the per-pair fit of point-to-plane ICP in fp64: the linear least squares
// of pcl::registration::TransformationEstimationPointToPlaneLLS from the 29 correspondence sums.  The stopping rules are those of
// point-to-point ICP (icp_update.hpp: icp_converged), unchanged.  PCL is not part of the reference tree: the definition in DESIGN.md 4.16 is
// the contract, tests/golden/icp_plane_restate.py restates it in NumPy, parity with PCL itself is unpinned.
//
// With a_i = [s_i x n_j, n_j] (6) and r_i = n_j . (d_j - s_i) the increment x = (alpha, beta, gamma, tx, ty, tz) minimises sum (a_i . x - r_i)^2:
// M x = g with M = sum a a^T, g = sum a r.  M's rotational and translational blocks differ by the square of the clouds' extent, so the system is
// solved in the scaled form  Mt = S M S,  S = diag(M_ii^-1/2)  (unit diagonal, entries in [-1, 1]) by a Cholesky factorisation whose pivots
// say how much of each unknown the correspondences determine: a pivot <= kIcpPlanePivot, or a diagonal entry <= 0, is a rank-deficient
// system (a target whose normals are all parallel leaves three unknowns free) and ends the pair as ICP_DEGENERATE -- PCL inverts regardless.
// Compiled for the device by hipcc and for the host by g++ (tests/cpp/icp_plane_update_host.cpp, tests/test_icp_plane_cpu.py checks this
// very text against LAPACK).
#pragma once
#include "icp_update.hpp"

namespace mrs {

constexpr int ICP_DEGENERATE = 6;     // after pcl's ConvergenceState 0 .. 5 (IcpState): the 6 x 6 system has no unique solution

// n, the upper triangle of sum a a^T (21, row-major: 00 01 .. 05 11 12 ..), sum a r (6), sum |d - s|^2
constexpr int kIcpPlaneTerms = 29;
constexpr double kIcpPlanePivot = 1e-10;

// x[6] from the sums; false when the system is rank-deficient (x is then untouched)
MRS_HD bool icp_plane_solve(const double* s, double* x)
{
    double M[6][6], sc[6];
    {
        int t = 1;
        for (int r = 0; r < 6; ++r)
            for (int c = r; c < 6; ++c) M[r][c] = M[c][r] = s[t++];
    }
    for (int i = 0; i < 6; ++i) {
        if (!(M[i][i] > 0.0) || !(M[i][i] <= DBL_MAX)) return false;       // zero, negative, NaN or inf
        sc[i] = 1.0 / sqrt(M[i][i]);
    }
    double L[6][6];
    for (int j = 0; j < 6; ++j) {
        double d = M[j][j] * sc[j] * sc[j];
        for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
        if (!(d > kIcpPlanePivot)) return false;
        L[j][j] = sqrt(d);
        for (int i = j + 1; i < 6; ++i) {
            double v = M[i][j] * sc[i] * sc[j];
            for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k];
            L[i][j] = v / L[j][j];
        }
    }
    double y[6];
    for (int i = 0; i < 6; ++i) {                       // L y = S g
        double v = s[22 + i] * sc[i];
        for (int k = 0; k < i; ++k) v -= L[i][k] * y[k];
        y[i] = v / L[i][i];
    }
    for (int i = 5; i >= 0; --i) {                      // L^T z = y, x = S z
        double v = y[i];
        for (int k = i + 1; k < 6; ++k) v -= L[k][i] * y[k];
        y[i] = v / L[i][i];
    }
    for (int i = 0; i < 6; ++i) x[i] = y[i] * sc[i];
    return true;
}

// pcl's constructTransformationMatrix: D = [Rz(gamma) Ry(beta) Rx(alpha), t; 0 1] (row-major 4x4) with full sines and cosines
MRS_HD void icp_plane_delta(const double* x, double* D)
{
    const double ca = cos(x[0]), sa = sin(x[0]), cb = cos(x[1]), sb = sin(x[1]), cg = cos(x[2]), sg = sin(x[2]);
    D[0] = cg * cb;  D[1] = -sg * ca + cg * sb * sa;  D[2] = sg * sa + cg * sb * ca;   D[3] = x[3];
    D[4] = sg * cb;  D[5] = cg * ca + sg * sb * sa;   D[6] = -cg * sa + sg * sb * ca;  D[7] = x[4];
    D[8] = -sb;      D[9] = cb * sa;                  D[10] = cb * ca;                 D[11] = x[5];
    D[12] = D[13] = D[14] = 0.0;
    D[15] = 1.0;
}

// Step 4: the increment from the 29 sums (s[0] >= 1); false (D = identity) when the system is rank-deficient.  mse: the point-to-point mean
// squared error of the correspondences BEFORE the increment (what the convergence criteria compare, as in PCL).
MRS_HD bool icp_plane_fit(const double* s, double* D, double* mse)
{
    *mse = s[28] / s[0];
    double x[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const bool ok = icp_plane_solve(s, x);
    icp_plane_delta(x, D);
    return ok;
}

}  // namespace mrs
