// icp_device.hpp -- device code of the batched point-to-point ICP: pcl::IterativeClosestPoint as the
// Mapping node configures it at global_manager.cpp:890-906 (its own loop-closing thread) and :2427-2434 (PCL_ICP of
// select_registration_method).  Included by gicp.hip after gicp_device.hpp: the correspondences are those of the GICP searches, unchanged
// (nn_pass: k_nn_scan, k_nn_certify, k_nn_scan_g), on the same handle, clouds and LmState; this file adds the estimator.
//   k_icp_sums   : the 17 fp64 sums of one iteration, per workgroup (the point -> lane -> workgroup mapping of k_linearize);
//   k_icp_update : per pair, the workgroup partials in fixed order, then the rigid fit, the pose update and PCL's stopping rules
//                  (icp_update.hpp), and the counters of the host's tick loop (as k_lm_update counts them).
// An ICP pair is always in phase 0 while it is active (every iteration searches).  LmState fields with another meaning here:
//   y0    the mean squared error of the previous iteration (DBL_MAX before the first),
//   inner the convergence state (mrs::IcpState),
//   H     [0, 17) the sums of the last iteration,
//   delta the last increment (what pair_motion reads: the searches' schedule works unchanged).
#pragma once
#include "icp_update.hpp"

namespace {

using mrs::kIcpTerms;

struct IcpParams {
    mrs::IcpCriteria crit;
    float motion_switch;     // GicpParams::motion_switch
    int pad;
};

// Step 3.  grid = (blocks, pairs), one source point per lane and round, kPts rounds per block of 1024 points: partial[pair][block][17].
// Streams the lane's float4 source point (16 B) and its correspondence (4 B) and gathers the target float4 (16 B): 36 B per point.  The
// index travels two points ahead and the two points one ahead of the arithmetic, as in k_linearize.
__global__ __launch_bounds__(kNNThreads) void k_icp_sums(const float4* __restrict__ src_all, const int64_t* __restrict__ src_offs,
                                                         const float4* __restrict__ tgt_all, const int64_t* __restrict__ tgt_offs,
                                                         const LmState* __restrict__ st, const int* __restrict__ corr,
                                                         double* __restrict__ partial, int max_blocks)
{
    __shared__ double red[kNNThreads / 64][kIcpTerms];
    const int pair = blockIdx.y;
    const LmState& S = st[pair];
    if (!S.active) return;
    const int64_t so = src_offs[pair], to = tgt_offs[pair];
    const int n = (int)(src_offs[pair + 1] - so);
    const float4* src = src_all + so;
    const float4* tgt = tgt_all + to;
    double* pout = partial + ((size_t)pair * max_blocks + blockIdx.x) * kIcpTerms;
    double T[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) T[i] = S.x[i];
    double acc[kIcpTerms];
#pragma unroll
    for (int i = 0; i < kIcpTerms; ++i) acc[i] = 0.0;
    const int per_block = kNNThreads * kPts;  // same point -> block mapping as the scan and k_linearize (fixed summation order)
    for (int base = blockIdx.x * per_block; base < n; base += gridDim.x * per_block) {
        auto idx_of = [&](int p) { const int i = base + p * kNNThreads + (int)threadIdx.x; return (p < kPts && i < n) ? corr[so + i] : -1; };
        int j_cur = idx_of(0), j_nx = idx_of(1);
        float4 a_nx = make_float4(0.f, 0.f, 0.f, 0.f), b_nx = a_nx;
        if (j_cur >= 0) { a_nx = src[base + threadIdx.x]; b_nx = tgt[j_cur]; }
#pragma unroll 1
        for (int p = 0; p < kPts; ++p) {
            const int i = base + p * kNNThreads + threadIdx.x;
            const int j = j_cur;
            const float4 af = a_nx, bf = b_nx;
            j_cur = j_nx;
            j_nx = idx_of(p + 2);
            if (j_cur >= 0) { a_nx = src[i + kNNThreads]; b_nx = tgt[j_cur]; }
            if (j < 0) continue;
            double a[3];
#pragma unroll
            for (int r = 0; r < 3; ++r)
                a[r] = T[4 * r] * (double)af.x + T[4 * r + 1] * (double)af.y + T[4 * r + 2] * (double)af.z + T[4 * r + 3];
            const double b[3] = {(double)bf.x, (double)bf.y, (double)bf.z};
            const double e0 = b[0] - a[0], e1 = b[1] - a[1], e2 = b[2] - a[2];
            acc[0] += 1.0;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                acc[1 + r] += a[r];
                acc[4 + r] += b[r];
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[7 + 3 * r + c] += a[r] * b[c];
            }
            acc[16] += e0 * e0 + e1 * e1 + e2 * e2;
        }
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int i = 0; i < kIcpTerms; ++i) {
        const double v = wave_sum_d(acc[i]);
        if (lane == 0) red[wave][i] = v;
    }
    __syncthreads();
    if (threadIdx.x < kIcpTerms) {
        double v = 0;
        for (int w = 0; w < kNNThreads / 64; ++w) v += red[w][threadIdx.x];
        pout[threadIdx.x] = v;
    }
}

// Steps 2 and 4-6; grid = pairs.  n_next as in k_lm_update: [0] pairs that iterate again, [2] those of [0] whose increment moved them farther
// than motion_switch, [3] set when the tick carried a search.
__global__ __launch_bounds__(kLmThreads) void k_icp_update(LmState* __restrict__ st, const double* __restrict__ partial,
                                                          const int* __restrict__ nblocks, int max_blocks, IcpParams prm, int* __restrict__ n_next)
{
    const int pair = blockIdx.x;
    LmState& S = st[pair];
    if (!S.active) return;
    __shared__ double sum[kIcpTerms];
    {   // fixed-order final sum of the workgroup partials: lane l adds blocks l, l + 64, ... in ascending order, then one wave butterfly per term
        const double* p = partial + (size_t)pair * max_blocks * kIcpTerms;
        const int nb = nblocks[pair];
        const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
        for (int t = wave; t < kIcpTerms; t += kLmThreads / 64) {
            double v = 0;
            for (int b = lane; b < nb; b += 64) v += p[(size_t)b * kIcpTerms + t];
            v = wave_sum_d(v);
            if (lane == 0) sum[t] = v;
        }
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    n_next[3] = 1;
    for (int i = 0; i < kIcpTerms; ++i) S.H[i] = sum[i];
    if (sum[0] < 3.0) {      // step 2: the pose stays as it is
        for (int i = 0; i < 16; ++i) S.delta[i] = (i % 5 == 0) ? 1.0 : 0.0;
        S.inner = mrs::ICP_NO_CORRESPONDENCES;
        S.converged = 0; S.active = 0; S.phase = 2;
        return;
    }
    double D[16], X[16];
    const double mse = mrs::icp_rigid_fit(sum, D);
    mul4d(D, S.x, X);
    for (int i = 0; i < 16; ++i) { S.x[i] = S.xi[i] = X[i]; S.delta[i] = D[i]; }
    ++S.outer;
    const int state = mrs::icp_converged(prm.crit, S.outer, D, mse, S.y0);
    const bool forced_out = prm.crit.force_iters > 0 && S.outer >= prm.crit.force_iters;
    if (state != mrs::ICP_NOT_CONVERGED || forced_out) {
        S.inner = state;
        S.converged = state != mrs::ICP_NOT_CONVERGED ? 1 : 0;
        S.active = 0; S.phase = 2;
        return;
    }
    atomicAdd(&n_next[0], 1);
    if (pair_motion(S) > prm.motion_switch) atomicAdd(&n_next[2], 1);
}

}  // namespace
