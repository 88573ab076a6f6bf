// icp_plane_device.hpp -- device code of the batched point-to-plane ICP: pcl::NormalEstimation
// with setKSearch as GlobalManager::addNormal drives it (global_manager.cpp:2679-2693) and pcl::IterativeClosestPointWithNormals, the
// class that helper feeds.  Included by gicp.hip after icp_device.hpp: the correspondences are those of the GICP searches (nn_pass), the
// neighbour lists those of the covariance front end (k_knn_cov / k_knn_select), on the same handle, clouds and LmState; this file adds
//   k_normals_from_knn : contract A, one float4 (unit normal, curvature) per point in sorted space;
//   k_normals_scatter  : normals the caller already has, from input order into sorted space;
//   k_icp_plane_sums   : the 29 fp64 sums of one iteration, per workgroup (the point -> lane -> workgroup mapping of k_icp_sums);
//   k_icp_plane_update : k_icp_update with the linear least-squares fit of icp_plane_update.hpp.
// LmState as in icp_device.hpp, with H [0, 29) the sums of the last iteration and inner possibly mrs::ICP_DEGENERATE.
#pragma once
#include "icp_plane_update.hpp"

namespace {

using mrs::kIcpPlaneTerms;

// Contract A, steps 2-7.  One point per lane; knn = the selection's output (knn_at), read in the chunked, prefetched pattern of
// k_cov_from_knn (neighbour_moments: no k-sized register array).  The second moments are taken about the query point in one pass and
// re-centred on the neighbour mean, as for the GICP covariances.
__global__ __launch_bounds__(256) void k_normals_from_knn(const float4* __restrict__ pts_all, const int64_t* __restrict__ offs, int k,
                                                         const int* __restrict__ knn, double vx, double vy, double vz,
                                                         float4* __restrict__ nrm_all)
{
    const int c = blockIdx.y;
    const int64_t o = offs[c];
    const int n = (int)(offs[c + 1] - o);
    const float4* pts = pts_all + o;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int* nb = knn + knn_at(o, c, i, k, 0);       // slot s at nb[64 s]: one row per wave and slot
        const float4 q = pts[i];
        double cv[9];
        float unused[32];
        const int cnt = neighbour_moments<32, false>(pts, nb, k, i, q, cv, unused);
        for (int a = 0; a < 9; ++a) cv[a] /= cnt;
        double nrm[3], w[3];
        mrs::smallest_eigvec(cv, nrm);
        mrs::sym3_eigvals(cv, w);                           // descending
        const double toward = nrm[0] * (vx - (double)q.x) + nrm[1] * (vy - (double)q.y) + nrm[2] * (vz - (double)q.z);
        const double sgn = toward < 0.0 ? -1.0 : 1.0;
        const double tr = w[0] + w[1] + w[2];
        float4 out = make_float4((float)(sgn * nrm[0]), (float)(sgn * nrm[1]), (float)(sgn * nrm[2]), tr > 0.0 ? (float)(w[2] / tr) : 0.0f);
        if (cnt < 3) out.x = out.y = out.z = out.w = __builtin_nanf("");   // pcl::computePointNormal refuses fewer than three neighbours
        nrm_all[o + i] = out;
    }
}

// in: [total][stride] floats in the caller's INPUT order, (nx, ny, nz) first and the curvature fourth when stride >= 4 -> sorted space
__global__ __launch_bounds__(256) void k_normals_scatter(const float4* __restrict__ pts_all, const int64_t* __restrict__ offs,
                                                        const float* __restrict__ in, int stride, float4* __restrict__ nrm_all)
{
    const int c = blockIdx.y;
    const int64_t o = offs[c];
    const int n = (int)(offs[c + 1] - o);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float* p = in + (size_t)(o + __float_as_int(pts_all[o + i].w)) * stride;
        nrm_all[o + i] = make_float4(p[0], p[1], p[2], stride >= 4 ? p[3] : 0.0f);
    }
}

// Step 3.  grid = (blocks, pairs), one source point per lane and round, kPts rounds per block of 1024 points: partial[pair][block][29].
// Streams the lane's float4 source point (16 B) and its correspondence (4 B) and gathers the target float4 (16 B) and its normal (16 B):
// 52 B per point.  The index travels two points ahead and the three float4 one ahead of the arithmetic, as in k_icp_sums.
__global__ __launch_bounds__(kNNThreads) void k_icp_plane_sums(const float4* __restrict__ src_all, const int64_t* __restrict__ src_offs,
                                                               const float4* __restrict__ tgt_all, const float4* __restrict__ nrm_all,
                                                               const int64_t* __restrict__ tgt_offs, const LmState* __restrict__ st,
                                                               const int* __restrict__ corr, double* __restrict__ partial, int max_blocks)
{
    __shared__ double red[kNNThreads / 64][kIcpPlaneTerms];
    const int pair = blockIdx.y;
    const LmState& S = st[pair];
    if (!S.active) return;
    const int64_t so = src_offs[pair], to = tgt_offs[pair];
    const int n = (int)(src_offs[pair + 1] - so);
    const float4* src = src_all + so;
    const float4* tgt = tgt_all + to;
    const float4* nrm = nrm_all + to;
    double* pout = partial + ((size_t)pair * max_blocks + blockIdx.x) * kIcpPlaneTerms;
    double T[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) T[i] = S.x[i];
    double acc[kIcpPlaneTerms];
#pragma unroll
    for (int i = 0; i < kIcpPlaneTerms; ++i) acc[i] = 0.0;
    const int per_block = kNNThreads * kPts;  // same point -> block mapping as the scan and k_icp_sums (fixed summation order)
    for (int base = blockIdx.x * per_block; base < n; base += gridDim.x * per_block) {
        auto idx_of = [&](int p) { const int i = base + p * kNNThreads + (int)threadIdx.x; return (p < kPts && i < n) ? corr[so + i] : -1; };
        int j_cur = idx_of(0), j_nx = idx_of(1);
        float4 a_nx = make_float4(0.f, 0.f, 0.f, 0.f), b_nx = a_nx, n_nx = a_nx;
        if (j_cur >= 0) { a_nx = src[base + threadIdx.x]; b_nx = tgt[j_cur]; n_nx = nrm[j_cur]; }
#pragma unroll 1
        for (int p = 0; p < kPts; ++p) {
            const int i = base + p * kNNThreads + threadIdx.x;
            const int j = j_cur;
            const float4 af = a_nx, bf = b_nx, nf = n_nx;
            j_cur = j_nx;
            j_nx = idx_of(p + 2);
            if (j_cur >= 0) { a_nx = src[i + kNNThreads]; b_nx = tgt[j_cur]; n_nx = nrm[j_cur]; }
            if (j < 0 || !(fabsf(nf.x) <= FLT_MAX && fabsf(nf.y) <= FLT_MAX && fabsf(nf.z) <= FLT_MAX)) continue;   // step 2: no finite normal
            double s[3];
#pragma unroll
            for (int r = 0; r < 3; ++r)
                s[r] = T[4 * r] * (double)af.x + T[4 * r + 1] * (double)af.y + T[4 * r + 2] * (double)af.z + T[4 * r + 3];
            const double nn[3] = {(double)nf.x, (double)nf.y, (double)nf.z};
            const double e0 = (double)bf.x - s[0], e1 = (double)bf.y - s[1], e2 = (double)bf.z - s[2];
            const double a[6] = {s[1] * nn[2] - s[2] * nn[1], s[2] * nn[0] - s[0] * nn[2], s[0] * nn[1] - s[1] * nn[0], nn[0], nn[1], nn[2]};
            const double res = nn[0] * e0 + nn[1] * e1 + nn[2] * e2;
            acc[0] += 1.0;
#pragma unroll
            for (int r = 0; r < 6; ++r)
#pragma unroll
                for (int c = r; c < 6; ++c) acc[1 + 6 * r - r * (r - 1) / 2 + (c - r)] += a[r] * a[c];     // upper triangle, row-major
#pragma unroll
            for (int r = 0; r < 6; ++r) acc[22 + r] += a[r] * res;
            acc[28] += e0 * e0 + e1 * e1 + e2 * e2;
        }
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int i = 0; i < kIcpPlaneTerms; ++i) {
        const double v = wave_sum_d(acc[i]);
        if (lane == 0) red[wave][i] = v;
    }
    __syncthreads();
    if (threadIdx.x < kIcpPlaneTerms) {
        double v = 0;
        for (int w = 0; w < kNNThreads / 64; ++w) v += red[w][threadIdx.x];
        pout[threadIdx.x] = v;
    }
}

// Steps 2 and 4-6; grid = pairs.  n_next as in k_icp_update.
__global__ __launch_bounds__(kLmThreads) void k_icp_plane_update(LmState* __restrict__ st, const double* __restrict__ partial,
                                                                const int* __restrict__ nblocks, int max_blocks, IcpParams prm,
                                                                int* __restrict__ n_next)
{
    const int pair = blockIdx.x;
    LmState& S = st[pair];
    if (!S.active) return;
    __shared__ double sum[kIcpPlaneTerms];
    {   // fixed-order final sum of the workgroup partials, as in k_icp_update
        const double* p = partial + (size_t)pair * max_blocks * kIcpPlaneTerms;
        const int nb = nblocks[pair];
        const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
        for (int t = wave; t < kIcpPlaneTerms; t += kLmThreads / 64) {
            double v = 0;
            for (int b = lane; b < nb; b += 64) v += p[(size_t)b * kIcpPlaneTerms + t];
            v = wave_sum_d(v);
            if (lane == 0) sum[t] = v;
        }
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    n_next[3] = 1;
    for (int i = 0; i < kIcpPlaneTerms; ++i) S.H[i] = sum[i];
    double D[16], X[16], mse = 0.0;
    const bool few = sum[0] < 3.0;
    if (few || !mrs::icp_plane_fit(sum, D, &mse)) {      // step 2, or a rank-deficient system: the pose stays as it is
        for (int i = 0; i < 16; ++i) S.delta[i] = (i % 5 == 0) ? 1.0 : 0.0;
        S.inner = few ? (int)mrs::ICP_NO_CORRESPONDENCES : mrs::ICP_DEGENERATE;
        S.converged = 0; S.active = 0; S.phase = 2;
        return;
    }
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
