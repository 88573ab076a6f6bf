// fasthist.hip -- the range histogram ("Fast Histogram") descriptor of a batch of raw 3-D clouds (C ABI mrs_fh_*).
//
// What it replaces: RING_ros/pr_methods/FastHistogram.py:10-63 -- calculateRange (a Python loop over the points for the largest range),
// then statisticsOnRange: one distanceJudge call per point with a loop over all b buckets inside, then the division by the point count.
// 0.49 s per 20 000-point scan there, linear in the point count.  Here, per call and for the whole batch:
//   tiles  : k_fh_tile_base and k_fh_tile_cloud turn the offsets into the tile tables (first tile of each cloud, cloud of each tile; a tile
//            = MRS_FH_TILE_POINTS points of ONE cloud), so that a long scan spreads over many workgroups, a workgroup never straddles two
//            clouds and finds its span with one load; nothing is uploaded per call;
//   range  : k_fh_range, a workgroup per tile; a thread issues the loads of its 8 points together.  d = sqrt((x x + y y) + z z) in fp64; a
//            non-negative double orders like its bit pattern, so the per-wave / per-workgroup maximum of the patterns and ONE 64-bit
//            integer atomicMax per workgroup give the exact maximum whatever the launch shape.  Points whose range is not finite are
//            skipped;
//   bins   : k_fh_bin, a workgroup per tile.  fh_bucket (fasthist_bucket.hpp) settles a quotient guess against the exact edges fl(i w).
//            Consecutive lanes hold consecutive points, and a lidar ring puts long runs of them into one bucket: a run of equal buckets
//            inside a wave is added once, by its first lane, into the wave's own LDS sub-histogram (integer LDS adds); the four
//            sub-histograms are summed and flushed with at most one global integer add per bucket per workgroup;
//   finish : k_fh_finish writes hist = counts / n, counts, M and the unbound count.
// Everything is integer or a correctly rounded fp64 operation on one point (no contraction: -ffp-contract=off), so a cloud gives the same
// bits alone, in any batch and from run to run.
#include "common.hpp"
#include "fasthist_bucket.hpp"

#include <algorithm>

namespace {

constexpr int kTile = MRS_FH_TILE_POINTS;
constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kPer = kTile / kThreads;                       // points per thread: their loads are issued together
static_assert(kTile % kThreads == 0, "a tile is a whole number of points per thread");
constexpr int kMaxBins = MRS_FH_MAX_BINS;
static_assert(kMaxBins <= kThreads, "the flush of k_fh_bin takes one thread per bucket");

// tile_base[c] = number of tiles of the clouds before c; tile_base[batch] = all tiles.  One workgroup: each thread sums a contiguous
// chunk of clouds, the chunk sums are scanned in LDS, then each thread writes its chunk.
__global__ __launch_bounds__(kThreads) void k_fh_tile_base(const int64_t* __restrict__ offs, int batch, int* __restrict__ tile_base)
{
    __shared__ int part[kThreads];
    const int t = threadIdx.x;
    const int per = (batch + kThreads - 1) / kThreads;
    const int c0 = min(t * per, batch), c1 = min(c0 + per, batch);
    int s = 0;
    for (int c = c0; c < c1; ++c) s += (int)((offs[c + 1] - offs[c] + kTile - 1) / kTile);
    part[t] = s;
    __syncthreads();
    int before = 0;
    for (int k = 0; k < t; ++k) before += part[k];
    for (int c = c0; c < c1; ++c) {
        tile_base[c] = before;
        before += (int)((offs[c + 1] - offs[c] + kTile - 1) / kTile);
    }
    if (t == kThreads - 1) tile_base[batch] = before;
}

// tile_cloud[tile] = the cloud a tile belongs to: a workgroup per cloud fills in the cloud's tiles (a cloud without points has none), so that
// a workgroup of the passes below finds its cloud with one load
__global__ __launch_bounds__(kThreads) void k_fh_tile_cloud(const int* __restrict__ tile_base, int* __restrict__ tile_cloud)
{
    const int c = blockIdx.x;
    const int t0 = tile_base[c], t1 = tile_base[c + 1];
    for (int j = t0 + threadIdx.x; j < t1; j += kThreads) tile_cloud[j] = c;
}

// first point and point count (1 .. kTile) of this workgroup's tile
__device__ __forceinline__ void tile_span(const int64_t* __restrict__ offs, const int* __restrict__ tile_base, const int* __restrict__ tile_cloud,
                                          int& c, int64_t& first, int& m)
{
    const int tile = blockIdx.x;
    c = tile_cloud[tile];
    const int64_t o0 = offs[c], n = offs[c + 1] - o0, i0 = (int64_t)(tile - tile_base[c]) * kTile;
    first = o0 + i0;
    m = (int)(n - i0 < kTile ? n - i0 : kTile);
}

// This thread's kPer points of the tile: point k * kThreads + t of the tile in slot k.  All loads are issued before any is used.  A slot
// past the end of the tile reads the tile's last point instead (in bounds, no branch); the kernels mask it by index where it matters.
template <class T>
struct TilePoints {
    T x[kPer], y[kPer], z[kPer];
    __device__ __forceinline__ void load(const T* __restrict__ pts, int stride, int64_t first, int m)
    {
#pragma unroll
        for (int k = 0; k < kPer; ++k) {
            const int i = min(k * kThreads + (int)threadIdx.x, m - 1);
            const T* q = pts + (size_t)(first + i) * stride;
            x[k] = q[0]; y[k] = q[1]; z[k] = q[2];
        }
    }
    __device__ __forceinline__ double range(int k) const
    {
        const double a = (double)x[k], b = (double)y[k], c = (double)z[k];
        return sqrt((a * a + b * b) + c * c);
    }
};

// range_bits [batch], zeroed by the caller: the bit pattern of the largest finite range of each cloud
template <class T>
__global__ __launch_bounds__(kThreads) void k_fh_range(const T* __restrict__ pts, int stride, const int64_t* __restrict__ offs,
                                                       const int* __restrict__ tile_base, const int* __restrict__ tile_cloud,
                                                       unsigned long long* __restrict__ range_bits)
{
    __shared__ unsigned long long wmax[kWaves];
    int c, m;
    int64_t first;
    tile_span(offs, tile_base, tile_cloud, c, first, m);
    const int t = threadIdx.x;
    TilePoints<T> p;
    p.load(pts, stride, first, m);
    unsigned long long best = 0ull;
#pragma unroll
    for (int k = 0; k < kPer; ++k) {                           // a slot past the end holds a copy of the last point: harmless for a maximum
        const double d = p.range(k);
        const unsigned long long bits = (unsigned long long)__double_as_longlong(d);
        if (d < INFINITY && bits > best) best = bits;          // NaN and +inf fail the comparison; d is never negative
    }
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(best, o, 64);
        best = other > best ? other : best;
    }
    if ((t & 63) == 0) wmax[t >> 6] = best;
    __syncthreads();
    if (t == 0) {
        for (int k = 1; k < kWaves; ++k) best = wmax[k] > best ? wmax[k] : best;
        if (best) atomicMax(range_bits + c, best);
    }
}

// counts int32 [batch][bins] and unbound int32 [batch], zeroed by the caller
template <class T>
__global__ __launch_bounds__(kThreads) void k_fh_bin(const T* __restrict__ pts, int stride, const int64_t* __restrict__ offs,
                                                     const int* __restrict__ tile_base, const int* __restrict__ tile_cloud, int bins,
                                                     const unsigned long long* __restrict__ range_bits, int* __restrict__ counts,
                                                     int* __restrict__ unbound)
{
    __shared__ int sub[kWaves * kMaxBins];
    __shared__ int sub_unbound;
    int c, m;
    int64_t first;
    tile_span(offs, tile_base, tile_cloud, c, first, m);
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    TilePoints<T> p;
    p.load(pts, stride, first, m);
    for (int i = t; i < kWaves * bins; i += kThreads) sub[i] = 0;
    if (t == 0) sub_unbound = 0;
    const double M = __longlong_as_double((long long)range_bits[c]);
    const double w = mrs::fh_width(M, bins), inv_w = 1.0 / w;
    __syncthreads();
    int* mine = sub + wave * bins;
    int nu = 0;
#pragma unroll
    for (int k = 0; k < kPer; ++k) {                            // every lane takes every turn: the shuffles below see whole waves
        int bucket = -1;
        if (k * kThreads + t < m) {
            int u;
            bucket = mrs::fh_bucket(p.range(k), M, w, inv_w, bins, &u);
            nu += u;
        }
        // a run of equal buckets in consecutive lanes is added by its first lane
        const int prev = __shfl_up(bucket, 1, 64);
        const bool head = lane == 0 || prev != bucket;
        const unsigned long long heads = __ballot(head);
        if (head && bucket >= 0) {
            const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);      // heads past this lane
            const int run = above ? __ffsll((long long)above) : 64 - lane;
            atomicAdd(mine + bucket, run);
        }
    }
    for (int o = 32; o > 0; o >>= 1) nu += __shfl_xor(nu, o, 64);
    if (lane == 0 && nu) atomicAdd(&sub_unbound, nu);
    __syncthreads();
    if (t < bins) {
        int v = 0;
#pragma unroll
        for (int k = 0; k < kWaves; ++k) v += sub[k * bins + t];
        if (v) atomicAdd(counts + (size_t)c * bins + t, v);
    }
    if (t == 0 && sub_unbound) atomicAdd(unbound + c, sub_unbound);
}

// one thread per (cloud, bucket): hist = counts / n in fp64 (zeros for an empty cloud); the outputs past d_hist are optional
__global__ void k_fh_finish(const int64_t* __restrict__ offs, int batch, int bins, const int* __restrict__ counts,
                            const unsigned long long* __restrict__ range_bits, const int* __restrict__ unbound, double* __restrict__ d_hist,
                            int32_t* __restrict__ d_counts, double* __restrict__ d_range, int32_t* __restrict__ d_unbound)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (int64_t)batch * bins) return;
    const int c = (int)(e / bins), i = (int)(e - (int64_t)c * bins);
    const int64_t n = offs[c + 1] - offs[c];
    const int v = counts[e];
    d_hist[e] = n > 0 ? (double)v / (double)n : 0.0;
    if (d_counts) d_counts[e] = v;
    if (i == 0) {
        if (d_range) d_range[c] = __longlong_as_double((long long)range_bits[c]);
        if (d_unbound) d_unbound[c] = unbound[c];
    }
}

template <class T>
int fh_impl(const T* p, int stride, const int64_t* d_offs, int64_t all_tiles, int batch, int bins, double* d_hist, int32_t* d_counts,
            double* d_range, int32_t* d_unbound, hipStream_t s)
{
    // one zeroed block: range bits [batch] (8 bytes each) | counts [batch][bins] | unbound [batch]; then the tile tables: first tile of
    // each cloud [batch + 1] | cloud of each tile [all_tiles]
    const size_t b_range = (size_t)batch * sizeof(unsigned long long), b_counts = (size_t)batch * bins * sizeof(int), b_unb = (size_t)batch * sizeof(int);
    mrs::Scratch acc, table;
    int st = acc.alloc(b_range + b_counts + b_unb, s);
    if (st != MRS_OK) return st;
    if ((st = table.alloc((size_t)(batch + 1 + all_tiles) * sizeof(int), s)) != MRS_OK) return st;
    int* tile_base = table.as<int>();
    int* tile_cloud = tile_base + batch + 1;
    unsigned long long* range_bits = acc.as<unsigned long long>();
    int* counts = reinterpret_cast<int*>(acc.as<char>() + b_range);
    int* unbound = counts + (size_t)batch * bins;
    MRS_HIP_TRY(hipMemsetAsync(acc.p, 0, b_range + b_counts + b_unb, s));
    hipLaunchKernelGGL(k_fh_tile_base, dim3(1), dim3(kThreads), 0, s, d_offs, batch, tile_base);
    if (all_tiles > 0) {
        hipLaunchKernelGGL(k_fh_tile_cloud, dim3(batch), dim3(kThreads), 0, s, tile_base, tile_cloud);
        hipLaunchKernelGGL(k_fh_range<T>, dim3((unsigned)all_tiles), dim3(kThreads), 0, s, p, stride, d_offs, tile_base, tile_cloud, range_bits);
        hipLaunchKernelGGL(k_fh_bin<T>, dim3((unsigned)all_tiles), dim3(kThreads), 0, s, p, stride, d_offs, tile_base, tile_cloud, bins, range_bits,
                           counts, unbound);
    }
    const int64_t elems = (int64_t)batch * bins;
    hipLaunchKernelGGL(k_fh_finish, dim3((unsigned)((elems + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, d_offs, batch, bins, counts, range_bits,
                       unbound, d_hist, d_counts, d_range, d_unbound);
    MRS_HIP_TRY(hipGetLastError());
    return MRS_OK;
}

}  // namespace

extern "C" {

int mrs_fh_batch(mrs_ctx* ctx, const void* d_points, int32_t is_double, int32_t stride, const int64_t* d_offsets, const int64_t* h_offsets,
                 int32_t batch, int32_t bins, double* d_hist, int32_t* d_counts, double* d_range, int32_t* d_unbound, mrs_stream stream)
{
    MRS_REQUIRE(ctx && d_offsets && h_offsets && d_hist, "null pointer");
    MRS_REQUIRE(batch > 0 && batch <= mrs::kMaxGridY && stride >= 3, "batch must be within [1, 65535] and stride >= 3");
    MRS_REQUIRE(bins >= 1 && bins <= kMaxBins, "bins in 1..256");
    int64_t longest = 0, tiles = 0;
    for (int b = 0; b < batch; ++b) {
        MRS_REQUIRE(h_offsets[b + 1] >= h_offsets[b], "offsets must be non-decreasing");
        const int64_t n = h_offsets[b + 1] - h_offsets[b];
        longest = std::max(longest, n);
        tiles += (n + kTile - 1) / kTile;
    }
    MRS_REQUIRE(h_offsets[0] >= 0 && longest < (1ll << 31), "fewer than 2^31 points per cloud");
    MRS_REQUIRE(tiles < (1ll << 31), "fewer than 2^31 tiles per call");
    MRS_REQUIRE(d_points || longest == 0, "null pointer");
    MRS_HIP_TRY(hipSetDevice(ctx->device));
    return is_double ? fh_impl<double>((const double*)d_points, stride, d_offsets, tiles, batch, bins, d_hist, d_counts, d_range, d_unbound,
                                       (hipStream_t)stream)
                     : fh_impl<float>((const float*)d_points, stride, d_offsets, tiles, batch, bins, d_hist, d_counts, d_range, d_unbound,
                                      (hipStream_t)stream);
}

int mrs_fh_host(mrs_ctx* ctx, const void* h_points, int32_t is_double, int32_t stride, int32_t n, int32_t bins, double* h_hist, int32_t* h_counts,
                double* h_range, int32_t* h_unbound)
{
    MRS_REQUIRE(ctx && h_hist && (h_points || n == 0), "null pointer");
    MRS_REQUIRE(n >= 0 && stride >= 3, "n must not be negative and stride >= 3");
    MRS_REQUIRE(bins >= 1 && bins <= kMaxBins, "bins in 1..256");
    if (n == 0) {                                                   // zeros, no device work
        memset(h_hist, 0, (size_t)bins * sizeof(double));
        if (h_counts) memset(h_counts, 0, (size_t)bins * sizeof(int32_t));
        if (h_range) *h_range = 0.0;
        if (h_unbound) *h_unbound = 0;
        return MRS_OK;
    }
    MRS_HIP_TRY(hipSetDevice(ctx->device));
    const size_t in_bytes = (size_t)n * stride * (is_double ? 8 : 4);
    // out: hist [bins] doubles | range [1] double | counts [bins] ints | unbound [1] int
    const size_t b_hist = (size_t)bins * sizeof(double), b_counts = (size_t)bins * sizeof(int32_t);
    mrs::Scratch in, out, offs;
    int st = in.alloc(in_bytes, nullptr);
    if (st != MRS_OK) return st;
    if ((st = out.alloc(b_hist + sizeof(double) + b_counts + sizeof(int32_t), nullptr)) != MRS_OK) return st;
    if ((st = offs.alloc(2 * sizeof(int64_t), nullptr)) != MRS_OK) return st;
    double* d_hist = out.as<double>();
    double* d_range = d_hist + bins;
    int32_t* d_counts = reinterpret_cast<int32_t*>(d_range + 1);
    int32_t* d_unbound = d_counts + bins;
    const int64_t h_offs[2] = {0, n};
    MRS_HIP_TRY(hipMemcpy(in.p, h_points, in_bytes, hipMemcpyHostToDevice));
    MRS_HIP_TRY(hipMemcpy(offs.p, h_offs, sizeof(h_offs), hipMemcpyHostToDevice));
    st = mrs_fh_batch(ctx, in.p, is_double, stride, offs.as<int64_t>(), h_offs, 1, bins, d_hist, d_counts, d_range, d_unbound, nullptr);
    if (st != MRS_OK) return st;
    MRS_HIP_TRY(hipMemcpy(h_hist, d_hist, b_hist, hipMemcpyDeviceToHost));
    if (h_counts) MRS_HIP_TRY(hipMemcpy(h_counts, d_counts, b_counts, hipMemcpyDeviceToHost));
    if (h_range) MRS_HIP_TRY(hipMemcpy(h_range, d_range, sizeof(double), hipMemcpyDeviceToHost));
    if (h_unbound) MRS_HIP_TRY(hipMemcpy(h_unbound, d_unbound, sizeof(int32_t), hipMemcpyDeviceToHost));
    return MRS_OK;
}

}  // extern "C"
