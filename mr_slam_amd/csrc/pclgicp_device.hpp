// pclgicp_device.hpp -- device code of the batched PCL-style GICP: pcl::GeneralizedIterativeClosestPoint
// as the PCL_GICP branch of GlobalManager::select_registration_method configures it (global_manager.cpp:2419-2426).  Included by gicp.hip after
// gicp_device.hpp: correspondences (nn_pass), covariances (the unit normals of k_cov_from_knn), handle, clouds and LmState are GICP's own; this
// file adds PCL's optimiser.  With the Mahalanobis matrices frozen per outer iteration the objective is an exact quadratic form in (R, t):
//   k_pclgicp_sums   : its 74 fp64 coefficients, per workgroup (the point -> lane -> workgroup mapping and the software pipeline of k_linearize);
//   k_pclgicp_update : per pair, the workgroup partials in fixed order, then the whole inner BFGS, the pose update and PCL's stopping rule
//                      (pclgicp_bfgs.hpp) on one lane, and the counters of the host's tick loop (as k_lm_update counts them).
// A pair is always in phase 0 while it is active (every iteration searches).  LmState fields with another meaning here:
//   inner  the state code (mrs::PclGicpState),   trials  the iterations of the last inner minimisation,   failed  how it ended (mrs::PclInnerEnd),
//   y0     the last outer delta,   delta  the last pose increment X_new X^-1 (what pair_motion reads: the searches' schedule works unchanged).
// The partial buffer has one row more per pair than there are workgroups: row max_blocks holds the pair's 74 totals of the last iteration
// (zeros below 4 correspondences).
#pragma once
#include "pclgicp_bfgs.hpp"

namespace {

using mrs::kPclTerms;

struct PclGicpParams {
    mrs::PclGicpCriteria crit;
    float motion_switch;     // GicpParams::motion_switch
    int pad;
};

// Step 4's pivot: the float32 midpoint of the target cloud's exact bounding box (k_cloud_bbox), per axis
__device__ __forceinline__ void pcl_pivot(const int* __restrict__ tgt_bbox, int pair, double (&c)[3])
{
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float m = 0.5f * (ordered_to_float(tgt_bbox[6 * pair + a]) + ordered_to_float(tgt_bbox[6 * pair + 3 + a]));
        c[a] = (m - m == 0.0f) ? (double)m : 0.0;       // an empty cloud's box is (+max, -max)
    }
}

// Steps 3 and 4.  grid = (blocks, pairs), one source point per lane and round, kPts rounds per block of 1024 points:
// partial[pair][block][74], terms [T0, T1) of them (one launch: 0, 74).  Per correspondence: 16 B own point + 4 B index + 16 B gathered point
// + 2 x 24 B normals = 84 B, as k_linearize.  The index travels two points ahead, points and normals one ahead of the arithmetic.
template <int T0, int T1>
__global__ __launch_bounds__(kNNThreads) void k_pclgicp_sums(
    const float4* __restrict__ src_all, const int64_t* __restrict__ src_offs, const double* __restrict__ src_cov,
    const float4* __restrict__ tgt_all, const int64_t* __restrict__ tgt_offs, const double* __restrict__ tgt_cov,
    const int* __restrict__ tgt_bbox, const LmState* __restrict__ st, const int* __restrict__ corr, double* __restrict__ partial, int max_blocks)
{
    constexpr int NT = T1 - T0;
    __shared__ double red[kNNThreads / 64][NT];
    const int pair = blockIdx.y;
    const LmState& S = st[pair];
    if (!S.active) return;
    const int64_t so = src_offs[pair], to = tgt_offs[pair];
    const int n = (int)(src_offs[pair + 1] - so);
    const float4* src = src_all + so;
    const float4* tgt = tgt_all + to;
    double* pout = partial + ((size_t)pair * (max_blocks + 1) + blockIdx.x) * kPclTerms;
    double TL[9], piv[3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) TL[3 * r + c] = S.x[4 * r + c];
    pcl_pivot(tgt_bbox, pair, piv);
    double acc[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) acc[i] = 0.0;
    // term `idx` of the layout (a compile-time constant after unrolling): kept if this instantiation owns it
    auto add = [&](int idx, double v) { if (idx >= T0 && idx < T1) acc[idx - T0] += v; };
    const int per_block = kNNThreads * kPts;  // same point -> block mapping as the scan and k_linearize (fixed summation order)
    for (int base = blockIdx.x * per_block; base < n; base += gridDim.x * per_block) {
        auto idx_of = [&](int p) { const int i = base + p * kNNThreads + (int)threadIdx.x; return (p < kPts && i < n) ? corr[so + i] : -1; };
        int j_cur = idx_of(0), j_nx = idx_of(1);
        float4 a_nx = make_float4(0.f, 0.f, 0.f, 0.f), b_nx = a_nx;
        double na_nx[3] = {0.0, 0.0, 0.0}, nb_nx[3] = {0.0, 0.0, 0.0};
        auto fetch_normals = [&](int i_next, int j_next) {
            const double* pa = src_cov + kCovDoubles * (size_t)(so + i_next);
            const double* pb = tgt_cov + kCovDoubles * (size_t)(to + j_next);
            na_nx[0] = pa[0]; na_nx[1] = pa[1]; na_nx[2] = pa[2];
            nb_nx[0] = pb[0]; nb_nx[1] = pb[1]; nb_nx[2] = pb[2];
        };
        if (j_cur >= 0) {
            a_nx = src[base + threadIdx.x]; b_nx = tgt[j_cur];
            fetch_normals(base + (int)threadIdx.x, j_cur);
        }
#pragma unroll 1
        for (int p = 0; p < kPts; ++p) {
            const int i = base + p * kNNThreads + threadIdx.x;
            const int j = j_cur;
            const float4 a = a_nx, bb = b_nx;
            const double na[3] = {na_nx[0], na_nx[1], na_nx[2]}, nbv[3] = {nb_nx[0], nb_nx[1], nb_nx[2]};
            j_cur = j_nx;
            j_nx = idx_of(p + 2);
            if (j_cur >= 0) {
                a_nx = src[i + kNNThreads]; b_nx = tgt[j_cur];
                fetch_normals(i + kNNThreads, j_cur);
            }
            if (j < 0) continue;
            // step 3: M = (C_B + R0 C_A R0^T)^-1 with k_linearize's expressions
            double ca[6], cb[6];
            cov6_from_normal(na, ca);
            cov6_from_normal(nbv, cb);
            const double CA[9] = {ca[0], ca[1], ca[2], ca[1], ca[3], ca[4], ca[2], ca[4], ca[5]};
            double RC[9], RCR[9], M[9];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    RC[3 * r + c] = TL[3 * r] * CA[c] + TL[3 * r + 1] * CA[3 + c] + TL[3 * r + 2] * CA[6 + c];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    RCR[3 * r + c] = RC[3 * r] * TL[3 * c] + RC[3 * r + 1] * TL[3 * c + 1] + RC[3 * r + 2] * TL[3 * c + 2];
            RCR[0] += cb[0]; RCR[1] += cb[1]; RCR[2] += cb[2];
            RCR[3] += cb[1]; RCR[4] += cb[3]; RCR[5] += cb[4];
            RCR[6] += cb[2]; RCR[7] += cb[4]; RCR[8] += cb[5];
            if (!inv3_sym(RCR, M)) continue;
            // step 4
            const double M6[6] = {M[0], M[1], M[2], M[4], M[5], M[8]};
            const double pp[3] = {(double)a.x - piv[0], (double)a.y - piv[1], (double)a.z - piv[2]};
            const double q[3] = {(double)bb.x - piv[0], (double)bb.y - piv[1], (double)bb.z - piv[2]};
            double Mq[3];
            mrs::pcl_symv(M6, q, Mq);
            add(0, 1.0);
#pragma unroll
            for (int k = 0; k < 6; ++k) add(1 + k, M6[k]);
#pragma unroll
            for (int k = 0; k < 3; ++k) add(7 + k, Mq[k]);
            add(10, q[0] * Mq[0] + q[1] * Mq[1] + q[2] * Mq[2]);
#pragma unroll
            for (int aa = 0; aa < 3; ++aa) {
#pragma unroll
                for (int k = 0; k < 6; ++k) add(11 + 6 * aa + k, pp[aa] * M6[k]);
#pragma unroll
                for (int k = 0; k < 3; ++k) add(29 + 3 * aa + k, pp[aa] * Mq[k]);
#pragma unroll
                for (int b = aa; b < 3; ++b) {
                    const double pab = pp[aa] * pp[b];
#pragma unroll
                    for (int k = 0; k < 6; ++k) add(38 + 6 * mrs::pcl_sym6(aa, b) + k, pab * M6[k]);
                }
            }
        }
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        const double v = wave_sum_d(acc[i]);
        if (lane == 0) red[wave][i] = v;
    }
    __syncthreads();
    if (threadIdx.x < NT) {
        double v = 0;
        for (int w = 0; w < kNNThreads / 64; ++w) v += red[w][threadIdx.x];
        pout[T0 + threadIdx.x] = v;
    }
}

// Steps 2 and 5-7; grid = pairs.  n_next as in k_lm_update: [0] pairs that iterate again, [2] those of [0] whose increment moved them farther
// than motion_switch, [3] set when the tick carried a search.
__global__ __launch_bounds__(kLmThreads) void k_pclgicp_update(LmState* __restrict__ st, double* __restrict__ partial, const int* __restrict__ nblocks,
                                                              int max_blocks, const int* __restrict__ tgt_bbox, PclGicpParams prm,
                                                              int* __restrict__ n_next)
{
    const int pair = blockIdx.x;
    LmState& S = st[pair];
    if (!S.active) return;
    __shared__ double sum[kPclTerms];
    double* const rows = partial + (size_t)pair * (max_blocks + 1) * kPclTerms;
    {   // fixed-order final sum of the workgroup partials: lane l adds blocks l, l + 64, ... in ascending order, then one wave butterfly per term
        const int nb = nblocks[pair];
        const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
        for (int t = wave; t < kPclTerms; t += kLmThreads / 64) {
            double v = 0;
            for (int b = lane; b < nb; b += 64) v += rows[(size_t)b * kPclTerms + t];
            v = wave_sum_d(v);
            if (lane == 0) sum[t] = v;
        }
    }
    __syncthreads();
    // the totals' row: zeros for a pair with too few correspondences (step 2)
    if (threadIdx.x < kPclTerms) rows[(size_t)max_blocks * kPclTerms + threadIdx.x] = sum[0] < 4.0 ? 0.0 : sum[threadIdx.x];
    if (threadIdx.x != 0) return;
    n_next[3] = 1;
    if (sum[0] < 4.0) {      // step 2: the pose stays as it is
        for (int i = 0; i < 16; ++i) S.delta[i] = (i % 5 == 0) ? 1.0 : 0.0;
        S.inner = mrs::PCL_NO_CORRESPONDENCES;
        S.trials = 0; S.failed = 0;
        S.converged = 0; S.active = 0; S.phase = 2;
        return;
    }
    double piv[3], X[16], D[16], dl;
    pcl_pivot(tgt_bbox, pair, piv);
#pragma unroll
    for (int i = 0; i < 16; ++i) X[i] = S.x[i];
    int inner_its = 0;
    const int end = mrs::pcl_gicp_iterate(sum, piv, prm.crit, X, &dl, &inner_its);
    // the increment X_new X^-1 (X is rigid: its inverse rotation is the transpose)
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) D[4 * r + c] = X[4 * r] * S.x[4 * c] + X[4 * r + 1] * S.x[4 * c + 1] + X[4 * r + 2] * S.x[4 * c + 2];
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) D[4 * r + 3] = X[4 * r + 3] - (D[4 * r] * S.x[3] + D[4 * r + 1] * S.x[7] + D[4 * r + 2] * S.x[11]);
    D[12] = D[13] = D[14] = 0.0; D[15] = 1.0;
#pragma unroll
    for (int i = 0; i < 16; ++i) { S.x[i] = S.xi[i] = X[i]; S.delta[i] = D[i]; }
    ++S.outer;
    S.y0 = dl; S.trials = inner_its; S.failed = end;
    const int state = mrs::pcl_gicp_converged(prm.crit, S.outer, dl);
    const bool forced_out = prm.crit.force_iters > 0 && S.outer >= prm.crit.force_iters;
    if (state != mrs::PCL_NOT_CONVERGED || forced_out) {
        S.inner = state;
        S.converged = state != mrs::PCL_NOT_CONVERGED ? 1 : 0;
        S.active = 0; S.phase = 2;
        return;
    }
    atomicAdd(&n_next[0], 1);
    if (pair_motion(S) > prm.motion_switch) atomicAdd(&n_next[2], 1);
}

}  // namespace
