// scancontext.hip -- Scan Context on the device: keys, sector-key pre-alignment, windowed column-cosine distance (C ABI mrs_sc_*, and the
// kernels behind the MRS_LOOPDB_SC loop database of loopdb.hip).
//
// What it replaces: RING_ros/pr_methods/ScanContext.py (make_ringkey / make_sectorkey :13-31, distance_sc :34-69,
// fast_align_with_sectorkey :86-101, dist_direct_sc :105-126, dist_align_sc :128-142) and the candidate step of RING_ros/main_SC.py:153-172
// (`KDTree(ring keys).query(k=1)` + `dist_align_sc(SC_candidate, SC_current, 0.1)`).  The descriptor is the node's, main_SC.py:57-69: the
// CARTESIAN max-z BEV of voxelocc (120 x 120), axis -2 called "ring", axis -1 "sector"; a "sector shift" is a roll along the y bins.
//
// Layout of a packed descriptor ("entry"): kHdr floats of header -- sector keys [0, 128), column L2 norms [128, 256) -- then the descriptor
// itself, row-major [R][S] as the reference holds it.  Ring keys live in a separate dense [n][R] array (what the nearest-key sweep streams).
//
// Alignment kernel: one workgroup per (fixed F, rolled Q) pair at a time, persistent over the pairs.  Q (the rolled operand: the query of
// the database, which is the same for every pair) sits in LDS; thread (j, h) holds rows [h*RH, h*RH + RH) of F's column j in registers and,
// for every shift t of the window, takes the partial dot product with Q's column (j - t) mod S from LDS.  Per entry byte fetched from HBM
// the kernel reads wlen bytes of LDS (13 at search_ratio 0.1).  The two halves meet in LDS; one wave per shift sums the column cosines.
#include "common.hpp"

#include <algorithm>
#include <atomic>
#include <cfloat>
#include <climits>
#include <cmath>

namespace {

constexpr int kHdr = 256, kMaxDim = 128, kThreads = 256, kChunk = 16, kMaxWin = 2 * kMaxDim;
constexpr int kNearThreads = 256, kMergeThreads = 1024, kMergePer = 16, kMaxK = 64;

// ---- keys + packing ---------------------------------------------------------------------------------------------------------------
// one workgroup per descriptor: the header (sector keys = column means, column norms) and, where asked, a copy into the entry; ring keys =
// row means.  Means are summed in fp64 and rounded once (np.mean of the float32 rows / columns); norms are np.linalg.norm's float32 sqrt(x.x).
__global__ __launch_bounds__(kThreads) void k_sc_pack(const float* __restrict__ sc, int R, int S, float* __restrict__ ent, size_t ent_stride,
                                                      float* __restrict__ ring, float* __restrict__ sector)
{
    const int b = blockIdx.x, t = threadIdx.x;
    const float* src = sc + (size_t)b * R * S;
    float* dst = ent ? ent + (size_t)b * ent_stride : nullptr;
    if (dst)
        for (int i = t; i < R * S; i += kThreads) dst[kHdr + i] = src[i];
    if (t < S) {                                     // column t: lanes read consecutive floats of a row
        double sum = 0.0;
        float sq = 0.0f;
        for (int r = 0; r < R; ++r) {
            const float v = src[(size_t)r * S + t];
            sum += (double)v;
            sq = __builtin_fmaf(v, v, sq);
        }
        const float key = (float)(sum / R);
        if (dst) { dst[t] = key; dst[kMaxDim + t] = sqrtf(sq); }
        if (sector) sector[(size_t)b * S + t] = key;
    }
    if (ring) {                                      // rows: one wave per row, fixed butterfly (deterministic)
        const int lane = t & 63, wave = t >> 6;
        for (int r = wave; r < R; r += kThreads / 64) {
            double s = 0.0;
            for (int c = lane; c < S; c += 64) s += (double)src[(size_t)r * S + c];
            for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
            if (lane == 0) ring[(size_t)b * R + r] = (float)(s / S);
        }
    }
}

// ---- nearest ring keys ------------------------------------------------------------------------------------------------------------
// (squared distance, index), lexicographic: ties go to the lower index
__device__ __forceinline__ bool key_less(double a, int ia, double b, int ib) { return a < b || (a == b && ia < ib); }

// stage 1: a workgroup scores `chunk` consecutive entries (fp64 squared distance of the float32 keys: sklearn's metric) and writes the
// ones whose rank within the chunk is < k to cand[block][rank].  Padding past n carries +inf and indices n + e (unique, never chosen first).
__global__ __launch_bounds__(kNearThreads) void k_sc_near_chunk(const float* __restrict__ q, const float* __restrict__ keys, int n, int R,
                                                                int chunk, int k, double* __restrict__ cd, int* __restrict__ ci)
{
    extern __shared__ double sh_near[];
    double* sd = sh_near;                                      // [chunk]
    int* si = reinterpret_cast<int*>(sd + chunk);              // [chunk]
    __shared__ float qs[kMaxDim];
    const int t = threadIdx.x;
    if (t < R) qs[t] = q[t];
    __syncthreads();
    const int base = blockIdx.x * chunk;
    for (int e = t; e < chunk; e += kNearThreads) {
        const int i = base + e;
        double acc = INFINITY;
        if (i < n) {
            const float* row = keys + (size_t)i * R;
            acc = 0.0;
            for (int r = 0; r < R; ++r) {
                const double d = (double)row[r] - (double)qs[r];
                acc = __builtin_fma(d, d, acc);
            }
        }
        sd[e] = acc;
        si[e] = i;
    }
    __syncthreads();
    for (int e = t; e < chunk; e += kNearThreads) {
        const double me = sd[e];
        const int mi = si[e];
        int rank = 0;
        for (int f = 0; f < chunk; ++f) rank += key_less(sd[f], si[f], me, mi) ? 1 : 0;
        if (rank < k) { cd[(size_t)blockIdx.x * k + rank] = me; ci[(size_t)blockIdx.x * k + rank] = mi; }
    }
}

// stage 2: one workgroup, the m = blocks * k candidates in registers (at most kMergePer per thread), k rounds of "smallest key above the
// previous one".  Out: index (-1 past n) and squared distance, ascending.
__global__ __launch_bounds__(kMergeThreads) void k_sc_near_merge(const double* __restrict__ cd, const int* __restrict__ ci, int m, int n, int k,
                                                                 int* __restrict__ out_idx, double* __restrict__ out_d2)
{
    __shared__ double wd[kMergeThreads / 64];
    __shared__ int wi[kMergeThreads / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    double d[kMergePer];
    int id[kMergePer];
#pragma unroll
    for (int u = 0; u < kMergePer; ++u) {
        const int c = t + u * kMergeThreads;
        d[u] = c < m ? cd[c] : INFINITY;
        id[u] = c < m ? ci[c] : INT_MAX;
    }
    double pd = -1.0;
    int pi = -1;
    for (int round = 0; round < k; ++round) {
        double bd = INFINITY;
        int bi = INT_MAX;
#pragma unroll
        for (int u = 0; u < kMergePer; ++u)
            if (key_less(pd, pi, d[u], id[u]) && key_less(d[u], id[u], bd, bi)) { bd = d[u]; bi = id[u]; }
        for (int o = 32; o > 0; o >>= 1) {
            const double od = __shfl_xor(bd, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (key_less(od, oi, bd, bi)) { bd = od; bi = oi; }
        }
        if (lane == 0) { wd[wave] = bd; wi[wave] = bi; }
        __syncthreads();
        bd = wd[0]; bi = wi[0];
        for (int w = 1; w < kMergeThreads / 64; ++w)
            if (key_less(wd[w], wi[w], bd, bi)) { bd = wd[w]; bi = wi[w]; }
        if (t == 0) { out_idx[round] = bi < n ? bi : -1; out_d2[round] = bd; }
        pd = bd; pi = bi;
        __syncthreads();
    }
}

// ---- sector-key pre-alignment (fast_align_with_sectorkey) on its own -------------------------------------------------------------------
// pairs of key vectors [len]; shift s scores ||k1 - roll(k2, s)|| in fp64 over s = 0 .. len-1, first minimum
__global__ __launch_bounds__(kMaxDim) void k_sc_key_align(const float* __restrict__ k1, const float* __restrict__ k2, int len,
                                                          double* __restrict__ out_norm, int* __restrict__ out_shift)
{
    __shared__ float a[kMaxDim], b[kMaxDim];
    __shared__ double wd[2];
    __shared__ int wi[2];
    const int p = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (t < len) { a[t] = k1[(size_t)p * len + t]; b[t] = k2[(size_t)p * len + t]; }
    __syncthreads();
    double nrm = INFINITY;
    int s = INT_MAX;
    if (t < len) {
        double acc = 0.0;
        for (int j = 0; j < len; ++j) {
            int c = j - t;
            if (c < 0) c += len;
            const double d = (double)a[j] - (double)b[c];
            acc = __builtin_fma(d, d, acc);
        }
        nrm = sqrt(acc);
        s = t;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const double od = __shfl_xor(nrm, o, 64);
        const int oi = __shfl_xor(s, o, 64);
        if (key_less(od, oi, nrm, s)) { nrm = od; s = oi; }
    }
    if (lane == 0) { wd[wave] = nrm; wi[wave] = s; }
    __syncthreads();
    if (t == 0) {
        if (key_less(wd[1], wi[1], wd[0], wi[0])) { wd[0] = wd[1]; wi[0] = wi[1]; }
        out_norm[p] = wd[0];
        out_shift[p] = wi[0];
    }
}

// ---- windowed column-cosine distance ------------------------------------------------------------------------------------------------
enum { kModeAlign = 0, kModeDistance = 1, kModeDirect = 2 };

// RHF: rows per half fixed at compile time (60: the 120 x 120 database), 0: runtime (R <= 128).  Pairs p < npairs: F = entry list[p] (or p),
// Q = Q + p * q_stride (q_stride 0: one Q for every pair, loaded once per workgroup).
//   kModeAlign   : dist_align_sc(F, Q): s* from the sector keys, then dist_direct_sc(F, roll(Q, t)) over the window, first minimum -> (dist, t)
//   kModeDistance: distance_sc(Q, F): sim(t) = mean cosine of (roll(Q, t), F), t = 1 .. S, first maximum -> (1 - max, t)
//   kModeDirect  : dist_direct_sc(F, Q) (the window {0})
template <int RHF>
__global__ __launch_bounds__(kThreads) void k_sc_align(const float* __restrict__ F, size_t f_stride, const int* __restrict__ list, int npairs,
                                                       const float* __restrict__ Q, size_t q_stride, int R, int S, int mode, int radius,
                                                       float* __restrict__ out_dist, int* __restrict__ out_shift)
{
    constexpr int RHM = RHF > 0 ? RHF : kMaxDim / 2;
    extern __shared__ float sh_align[];
    float* Qd = sh_align;                      // [R][S]
    float* part = sh_align + R * S;            // [kChunk][2][S]
    __shared__ float Qsk[kMaxDim], Qn[kMaxDim], Fsk[kMaxDim], Fn[kMaxDim], sums[kMaxWin];
    __shared__ int cnts[kMaxWin];
    __shared__ double wd[kThreads / 64];
    __shared__ int wi[kThreads / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int j = t % S, h = t / S;
    const bool active = t < 2 * S;
    const int rh = RHF > 0 ? RHF : (R + 1) / 2;
    const int r0 = h * rh;
    const int rows = RHF > 0 ? RHF : (h == 0 ? rh : R - rh);
    bool loaded = false;
    for (int p = blockIdx.x; p < npairs; p += gridDim.x) {
        const int e = list ? list[p] : p;
        const float* Fe = F + (size_t)e * f_stride;
        if (q_stride != 0 || !loaded) {
            const float* Qp = Q + (size_t)p * q_stride;
            for (int i = t; i < R * S; i += kThreads) Qd[i] = Qp[kHdr + i];
            if (t < S) { Qsk[t] = Qp[t]; Qn[t] = Qp[kMaxDim + t]; }
            loaded = true;
        }
        float f[RHM];
#pragma unroll
        for (int k = 0; k < RHM; ++k) f[k] = (active && k < rows) ? Fe[kHdr + (size_t)(r0 + k) * S + j] : 0.0f;
        if (t < S) { Fsk[t] = Fe[t]; Fn[t] = Fe[kMaxDim + t]; }
        __syncthreads();
        int lo, wlen;
        if (mode == kModeAlign) {
            // fast_align_with_sectorkey(sk(F), sk(Q)): ||sk1 - roll(sk2, s)|| in fp64, s = 0 .. S-1, first minimum (strict <)
            double nrm = INFINITY;
            int s = INT_MAX;
            if (t < S) {
                double acc = 0.0;
                for (int jj = 0; jj < S; ++jj) {
                    int c = jj - t;
                    if (c < 0) c += S;
                    const double d = (double)Fsk[jj] - (double)Qsk[c];
                    acc = __builtin_fma(d, d, acc);
                }
                nrm = sqrt(acc);
                s = t;
            }
            for (int o = 32; o > 0; o >>= 1) {
                const double od = __shfl_xor(nrm, o, 64);
                const int oi = __shfl_xor(s, o, 64);
                if (key_less(od, oi, nrm, s)) { nrm = od; s = oi; }
            }
            if (lane == 0) { wd[wave] = nrm; wi[wave] = s; }
            __syncthreads();
            double bn = wd[0];
            int bs = wi[0];
            for (int w = 1; w < kThreads / 64; ++w)
                if (key_less(wd[w], wi[w], bn, bs)) { bn = wd[w]; bs = wi[w]; }
            lo = max(-S, bs - radius);
            wlen = min(S, bs + radius + 1) - lo;
        } else if (mode == kModeDistance) {
            lo = 1; wlen = S;
        } else {
            lo = 0; wlen = 1;
        }
        for (int c0 = 0; c0 < wlen; c0 += kChunk) {
            const int nt = min(kChunk, wlen - c0);
            if (active) {
                for (int tt = 0; tt < nt; ++tt) {
                    int c = j - (lo + c0 + tt);          // roll(Q, shift)[:, j] = Q[:, (j - shift) mod S]; shift in [-S, S)
                    if (c < 0) c += S;
                    if (c >= S) c -= S;
                    const float* qc = Qd + r0 * S + c;
                    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
#pragma unroll
                    for (int k = 0; k < RHM; k += 4) {
                        if (RHF > 0 || k < rows) a0 = __builtin_fmaf(f[k], qc[k * S], a0);
                        if (k + 1 < RHM && (RHF > 0 || k + 1 < rows)) a1 = __builtin_fmaf(f[k + 1], qc[(k + 1) * S], a1);
                        if (k + 2 < RHM && (RHF > 0 || k + 2 < rows)) a2 = __builtin_fmaf(f[k + 2], qc[(k + 2) * S], a2);
                        if (k + 3 < RHM && (RHF > 0 || k + 3 < rows)) a3 = __builtin_fmaf(f[k + 3], qc[(k + 3) * S], a3);
                    }
                    part[(tt * 2 + h) * S + j] = (a0 + a1) + (a2 + a3);
                }
            }
            __syncthreads();
            // one wave per shift: cosine of every column where both norms are > 0, summed with a fixed butterfly
            for (int tt = wave; tt < nt; tt += kThreads / 64) {
                const int sh = lo + c0 + tt;
                float v = 0.0f;
                int cnt = 0;
                for (int jj = lane; jj < S; jj += 64) {
                    int c = jj - sh;
                    if (c < 0) c += S;
                    if (c >= S) c -= S;
                    const float nf = Fn[jj], nq = Qn[c];
                    if (nf > 0.0f && nq > 0.0f) {
                        const float dot = part[(tt * 2) * S + jj] + part[(tt * 2 + 1) * S + jj];
                        v += dot / (nf * nq);
                        ++cnt;
                    }
                }
                for (int o = 32; o > 0; o >>= 1) {
                    v += __shfl_xor(v, o, 64);
                    cnt += __shfl_xor(cnt, o, 64);
                }
                if (lane == 0) { sums[c0 + tt] = v; cnts[c0 + tt] = cnt; }
            }
            __syncthreads();
        }
        if (t == 0) {
            if (mode == kModeDistance) {                 // sim = mean cosine (0 without columns), np.argmax: first maximum
                float best = cnts[0] > 0 ? sums[0] / (float)cnts[0] : 0.0f;
                int bi = 0;
                for (int i = 1; i < wlen; ++i) {
                    const float sim = cnts[i] > 0 ? sums[i] / (float)cnts[i] : 0.0f;
                    if (sim > best) { best = sim; bi = i; }
                }
                out_dist[p] = 1.0f - best;
                out_shift[p] = lo + bi;
            } else {                                     // dist = 1 - mean cosine (1 without columns), first minimum (strict <)
                float best = 1e8f;
                int bi = 0;
                for (int i = 0; i < wlen; ++i) {
                    const float d = cnts[i] > 0 ? 1.0f - sums[i] / (float)cnts[i] : 1.0f;
                    if (d < best) { best = d; bi = i; }
                }
                out_dist[p] = best;
                if (out_shift) out_shift[p] = lo + bi;
            }
        }
        __syncthreads();                                 // Fsk / Fn / sums / cnts are rewritten by the next pair
    }
}

size_t align_lds(int R, int S) { return ((size_t)R * S + (size_t)kChunk * 2 * S) * sizeof(float); }

// the 64 KiB default is exceeded at R = S = 120: the attribute is set once per device and instantiation
template <int RHF>
int align_attr(int device, size_t lds)
{
    static std::atomic<int> done[64];
    if (device < 0 || device >= 64) return MRS_ERR_ARG;
    if (done[device].load(std::memory_order_acquire) >= (int)lds) return MRS_OK;
    MRS_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_sc_align<RHF>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)(sizeof(float) * ((size_t)kMaxDim * kMaxDim + (size_t)kChunk * 2 * kMaxDim))));
    done[device].store(INT_MAX, std::memory_order_release);
    return MRS_OK;
}

int pairs_geometry(int R, int S)
{
    if (R < 1 || S < 1) { mrs::set_error("bad argument: num_ring / num_sector must be >= 1"); return MRS_ERR_ARG; }
    if (R > kMaxDim || S > kMaxDim) { mrs::set_error("Scan Context geometry %d x %d exceeds %d x %d", R, S, kMaxDim, kMaxDim); return MRS_ERR_UNSUPPORTED; }
    return MRS_OK;
}

}  // namespace

namespace mrs {

size_t sc_entry_floats(int R, int S) { return ((size_t)kHdr + (size_t)R * S + 3) & ~(size_t)3; }

int sc_pack(const float* d_sc, int n, int R, int S, float* d_entries, size_t entry_stride, float* d_ring, float* d_sector, hipStream_t s)
{
    if (n <= 0) return MRS_OK;
    hipLaunchKernelGGL(k_sc_pack, dim3(n), dim3(kThreads), 0, s, d_sc, R, S, d_entries, entry_stride, d_ring, d_sector);
    MRS_HIP_TRY(hipGetLastError());
    return MRS_OK;
}

int sc_search_radius(double search_ratio, int S)
{
    // round(0.5 * search_ratio * num_sector) (Python's round: half to even); the window is clipped to [-S, S) anyway
    const double r = std::nearbyint(0.5 * search_ratio * (double)S);
    return (int)std::min(std::max(r, 0.0), 2.0 * S);
}

int sc_align(mrs_ctx* ctx, const float* d_F, size_t f_stride, const int* d_list, int npairs, const float* d_Q, size_t q_stride, int R, int S,
             int mode, int radius, float* d_dist, int* d_shift, hipStream_t s)
{
    if (npairs <= 0) return MRS_OK;
    const size_t lds = align_lds(R, S);
    const int cu = ctx->num_cu > 0 ? ctx->num_cu : 256;
    const int blocks = std::max(1, std::min(npairs, (q_stride ? 8 : 2) * cu));
    if (R == 120) {
        int st = align_attr<60>(ctx->device, lds);
        if (st != MRS_OK) return st;
        hipLaunchKernelGGL(k_sc_align<60>, dim3(blocks), dim3(kThreads), lds, s, d_F, f_stride, d_list, npairs, d_Q, q_stride, R, S, mode, radius,
                           d_dist, d_shift);
    } else {
        int st = align_attr<0>(ctx->device, lds);
        if (st != MRS_OK) return st;
        hipLaunchKernelGGL(k_sc_align<0>, dim3(blocks), dim3(kThreads), lds, s, d_F, f_stride, d_list, npairs, d_Q, q_stride, R, S, mode, radius,
                           d_dist, d_shift);
    }
    MRS_HIP_TRY(hipGetLastError());
    return MRS_OK;
}

int sc_nearest(const float* d_q, const float* d_keys, int n, int R, int k, int* d_idx, double* d_d2, hipStream_t s)
{
    if (n <= 0) return MRS_OK;
    if (k < 1 || k > kMaxK || R < 1 || R > kMaxDim) { set_error("bad argument: k in 1..%d, R in 1..%d", kMaxK, kMaxDim); return MRS_ERR_ARG; }
    // chunk per workgroup: the smallest that keeps blocks * k candidates within what the merge holds in registers
    int chunk = kNearThreads;
    while ((size_t)((n + chunk - 1) / chunk) * k > (size_t)kMergeThreads * kMergePer && chunk < 16 * kNearThreads) chunk *= 2;
    const int blocks = (n + chunk - 1) / chunk;
    const size_t m = (size_t)blocks * k;
    if (m > (size_t)kMergeThreads * kMergePer) { set_error("%d entries x k = %d exceed the nearest-key merge", n, k); return MRS_ERR_UNSUPPORTED; }
    Scratch cand;
    int st = cand.alloc(m * (sizeof(double) + sizeof(int)), s);
    if (st != MRS_OK) return st;
    double* cd = cand.as<double>();
    int* ci = reinterpret_cast<int*>(cd + m);
    hipLaunchKernelGGL(k_sc_near_chunk, dim3(blocks), dim3(kNearThreads), (size_t)chunk * (sizeof(double) + sizeof(int)), s, d_q, d_keys, n, R, chunk,
                       k, cd, ci);
    MRS_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_sc_near_merge, dim3(1), dim3(kMergeThreads), 0, s, cd, ci, (int)m, n, k, d_idx, d_d2);
    MRS_HIP_TRY(hipGetLastError());
    return MRS_OK;
}

}  // namespace mrs

extern "C" {

int mrs_sc_keys(mrs_ctx* ctx, const float* d_sc, int32_t n, int32_t num_ring, int32_t num_sector, float* d_ring_key, float* d_sector_key,
                mrs_stream stream)
{
    MRS_REQUIRE(ctx && d_sc && (d_ring_key || d_sector_key), "null pointer");
    MRS_REQUIRE(n >= 0, "n >= 0");
    int st = pairs_geometry(num_ring, num_sector);
    if (st != MRS_OK) return st;
    MRS_HIP_TRY(hipSetDevice(ctx->device));
    return mrs::sc_pack(d_sc, n, num_ring, num_sector, nullptr, 0, d_ring_key, d_sector_key, (hipStream_t)stream);
}

int mrs_sc_key_align_pairs(mrs_ctx* ctx, const float* d_key1, const float* d_key2, int32_t n_pairs, int32_t len, double* d_norm, int32_t* d_shift,
                           mrs_stream stream)
{
    MRS_REQUIRE(ctx && d_key1 && d_key2 && d_norm && d_shift, "null pointer");
    MRS_REQUIRE(n_pairs >= 0, "n_pairs >= 0");
    int st = pairs_geometry(len, len);
    if (st != MRS_OK) return st;
    if (n_pairs == 0) return MRS_OK;
    MRS_HIP_TRY(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_sc_key_align, dim3(n_pairs), dim3(kMaxDim), 0, (hipStream_t)stream, d_key1, d_key2, len, d_norm, d_shift);
    MRS_HIP_TRY(hipGetLastError());
    return MRS_OK;
}

namespace {
// pack both sides of n pairs into scratch entries, then one alignment launch; `swap`: F = sc2, Q = sc1 (distance_sc rolls its FIRST argument)
int pairs_common(mrs_ctx* ctx, const float* d_sc1, const float* d_sc2, int n, int R, int S, int mode, int radius, bool swap, float* d_dist,
                 int* d_shift, hipStream_t s)
{
    MRS_REQUIRE(ctx && d_sc1 && d_sc2 && d_dist && (d_shift || mode == kModeDirect), "null pointer");
    MRS_REQUIRE(n >= 0, "n_pairs >= 0");
    int st = pairs_geometry(R, S);
    if (st != MRS_OK) return st;
    if (n == 0) return MRS_OK;
    MRS_HIP_TRY(hipSetDevice(ctx->device));
    const size_t ef = mrs::sc_entry_floats(R, S);
    mrs::Scratch buf;
    if ((st = buf.alloc((size_t)2 * n * ef * sizeof(float), s)) != MRS_OK) return st;
    float* e1 = buf.as<float>();
    float* e2 = e1 + (size_t)n * ef;
    if ((st = mrs::sc_pack(d_sc1, n, R, S, e1, ef, nullptr, nullptr, s)) != MRS_OK) return st;
    if ((st = mrs::sc_pack(d_sc2, n, R, S, e2, ef, nullptr, nullptr, s)) != MRS_OK) return st;
    return mrs::sc_align(ctx, swap ? e2 : e1, ef, nullptr, n, swap ? e1 : e2, ef, R, S, mode, radius, d_dist, d_shift, s);
}
}  // namespace

int mrs_sc_dist_direct_pairs(mrs_ctx* ctx, const float* d_sc1, const float* d_sc2, int32_t n_pairs, int32_t num_ring, int32_t num_sector,
                             float* d_dist, mrs_stream stream)
{
    return pairs_common(ctx, d_sc1, d_sc2, n_pairs, num_ring, num_sector, kModeDirect, 0, false, d_dist, nullptr, (hipStream_t)stream);
}

int mrs_sc_dist_align_pairs(mrs_ctx* ctx, const float* d_sc1, const float* d_sc2, int32_t n_pairs, int32_t num_ring, int32_t num_sector,
                            double search_ratio, float* d_dist, int32_t* d_shift, mrs_stream stream)
{
    MRS_REQUIRE(std::isfinite(search_ratio) && search_ratio >= 0.0, "search_ratio >= 0");
    return pairs_common(ctx, d_sc1, d_sc2, n_pairs, num_ring, num_sector, kModeAlign, mrs::sc_search_radius(search_ratio, num_sector), false,
                        d_dist, d_shift, (hipStream_t)stream);
}

int mrs_sc_distance_pairs(mrs_ctx* ctx, const float* d_sc1, const float* d_sc2, int32_t n_pairs, int32_t num_ring, int32_t num_sector, float* d_dist,
                          int32_t* d_yaw, mrs_stream stream)
{
    return pairs_common(ctx, d_sc1, d_sc2, n_pairs, num_ring, num_sector, kModeDistance, 0, true, d_dist, d_yaw, (hipStream_t)stream);
}

}  // extern "C"
