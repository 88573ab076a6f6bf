// posegraph_marginal.hpp -- the per-pose arithmetic of the pose-graph optimiser's marginal covariances (posegraph.hip, k_pgo_marginal_walk
// and k_pgo_marginal_gather), for the device and, compiled by g++, for the CPU tests
// (tests/cpp/posegraph_marginal_host.cpp).
//
// Selected inversion (Takahashi) read off the segment walk's factor.  Pose p of a segment was eliminated with the pivot factor L_p and the
// two blocks below it, A_p = L_p^-1 H(p, l)-with-fill towards the left separator l and W_p = L_p^-1 H(p, n) towards the next pose n
// (k_pgo_eliminate).  With G_l = L_p^-T A_p and G_n = L_p^-T W_p the rows of the inverse on that pattern are
//   S_pl = -G_l S_ll - G_n S_nl,   S_pn = -G_l S_ln - G_n S_nn,   S_pp = L_p^-T L_p^-1 - S_pl G_l^T - S_pn G_n^T,
// taken from the last pose of the segment to the first.  Blocks are B x B, row-major; every sum has a fixed order; the caller compiles
// without contraction.
#pragma once

#if defined(__HIPCC__)
#define MRS_PGM_HD __host__ __device__ inline
#define MRS_PGM_UNROLL _Pragma("unroll")
#else
#define MRS_PGM_HD inline
#define MRS_PGM_UNROLL
#endif

namespace mrs {
namespace pgo {

// M [B][B] <- L^-T M for a lower L, column by column
template <int B>
MRS_PGM_HD void marginal_upper_solve(const double* L, double* M)
{
    MRS_PGM_UNROLL
    for (int c = 0; c < B; ++c) {
        MRS_PGM_UNROLL
        for (int i = B - 1; i >= 0; --i) {
            double s = M[i * B + c];
            MRS_PGM_UNROLL
            for (int k = i + 1; k < B; ++k) s -= L[k * B + i] * M[k * B + c];
            M[i * B + c] = s / L[i * B + i];
        }
    }
}

// X <- 0.5 (X + X^T): symmetric to the bit
template <int B>
MRS_PGM_HD void marginal_symmetrize(double* X)
{
    MRS_PGM_UNROLL
    for (int r = 0; r < B; ++r) {
        MRS_PGM_UNROLL
        for (int c = 0; c < r; ++c) {
            const double v = 0.5 * (X[r * B + c] + X[c * B + r]);
            X[r * B + c] = v;
            X[c * B + r] = v;
        }
    }
}

// One step of the walk.  In: L, A, W of pose p as k_pgo_eliminate left them (A and W are overwritten by G_l and G_n), S_ll, S_nl (rows of
// the next pose, columns of the left separator) and S_nn.  Out: S_pl, S_pn (rows of p, columns of the next pose) and the symmetric S_pp.
// A bounding pose that is missing or held enters as zero blocks.
template <int B>
MRS_PGM_HD void marginal_step(const double* L, double* A, double* W, const double* Sll, const double* Snl, const double* Snn, double* Spl,
                              double* Spn, double* Spp)
{
    marginal_upper_solve<B>(L, A);
    marginal_upper_solve<B>(L, W);
    MRS_PGM_UNROLL
    for (int r = 0; r < B; ++r) {
        MRS_PGM_UNROLL
        for (int c = 0; c < B; ++c) {
            double pl = 0.0, pn = 0.0;
            MRS_PGM_UNROLL
            for (int k = 0; k < B; ++k) {
                pl -= A[r * B + k] * Sll[k * B + c];
                pn -= A[r * B + k] * Snl[c * B + k];             // S_ln = S_nl^T
            }
            MRS_PGM_UNROLL
            for (int k = 0; k < B; ++k) {
                pl -= W[r * B + k] * Snl[k * B + c];
                pn -= W[r * B + k] * Snn[k * B + c];
            }
            Spl[r * B + c] = pl;
            Spn[r * B + c] = pn;
        }
    }
    // Spp <- L^-1 (rows of the identity through the forward substitution), then L^-T L^-1 in place of it
    double Li[B * B];
    MRS_PGM_UNROLL
    for (int c = 0; c < B; ++c) {
        MRS_PGM_UNROLL
        for (int i = 0; i < B; ++i) {
            double s = i == c ? 1.0 : 0.0;
            MRS_PGM_UNROLL
            for (int k = 0; k < i; ++k) s -= L[i * B + k] * Li[k * B + c];
            Li[i * B + c] = i < c ? 0.0 : s / L[i * B + i];
        }
    }
    MRS_PGM_UNROLL
    for (int r = 0; r < B; ++r) {
        MRS_PGM_UNROLL
        for (int c = 0; c < B; ++c) {
            double s = 0.0;
            MRS_PGM_UNROLL
            for (int k = 0; k < B; ++k) s += Li[k * B + r] * Li[k * B + c];
            MRS_PGM_UNROLL
            for (int k = 0; k < B; ++k) s -= Spl[r * B + k] * A[c * B + k];
            MRS_PGM_UNROLL
            for (int k = 0; k < B; ++k) s -= Spn[r * B + k] * W[c * B + k];
            Spp[r * B + c] = s;
        }
    }
    marginal_symmetrize<B>(Spp);
}

// the block S_ij [6][6] of the optimiser's tangent (rotation, translation in the world frame) -> Pose3 local coordinates to first order:
// M_i S_ij M_j^T with M = blockdiag(I, R^T); Ti, Tj are poses of 12 doubles, the row-major [R | t]
MRS_PGM_HD void marginal_to_pose3(const double* Ti, const double* Tj, double* S)
{
    double X[36];
    MRS_PGM_UNROLL
    for (int r = 0; r < 6; ++r) {
        MRS_PGM_UNROLL
        for (int c = 0; c < 6; ++c) {
            double s = S[r * 6 + c];
            if (r >= 3) s = (Ti[r - 3] * S[18 + c] + Ti[4 + r - 3] * S[24 + c]) + Ti[8 + r - 3] * S[30 + c];
            X[r * 6 + c] = s;
        }
    }
    MRS_PGM_UNROLL
    for (int r = 0; r < 6; ++r) {
        MRS_PGM_UNROLL
        for (int c = 0; c < 6; ++c) {
            double s = X[r * 6 + c];
            if (c >= 3) s = (X[r * 6 + 3] * Tj[c - 3] + X[r * 6 + 4] * Tj[4 + c - 3]) + X[r * 6 + 5] * Tj[8 + c - 3];
            S[r * 6 + c] = s;
        }
    }
}

}  // namespace pgo
}  // namespace mrs
