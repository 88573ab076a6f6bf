// submap.hip -- device-resident keyframe store and batched GICP submap assembly (C ABI mrs_keyframes_*, mrs_submap_*).
//
// What it replaces: GlobalManager::mergeNearestKeyframes (Mapping/src/global_manager/src/global_manager.cpp:1894-1939), called twice per loop
// candidate by ICPCheck (:1968-1969): concatenate the 2 * submap_size + 1 keyframes around the loop keyframe, each moved into the loop
// keyframe's frame, pcl::PassThrough on x and y, pcl::VoxelGrid with leaf icp_filter_size -- on the host, per candidate, on whole clouds.
// Here every keyframe is uploaded ONCE into a growable arena of float4 (x, y, z, intensity); a batch of submaps is one chain of launches:
//   k_cells  : every segment point transformed and cropped, per-submap minimum / maximum voxel cell (reduced in the wave and in LDS, one
//              global atomic per workgroup and component);
//   k_grid   : per submap, the grid divisions and key multipliers (63-bit check);
//   k_keys   : the transform recomputed (deterministic float32 arithmetic, no fused multiply-add: 16 B per point not stored) -> 64-bit voxel key,
//              dropped points get the largest key;
//   segmented radix sort of (key, input position) per submap (stable: equal keys keep input order), run heads, prefix sum;
//   k_means  : one voxel per thread, its points summed in sorted (= input) order in float64, rounded to float32 once.
// The order of every sum is fixed by the sort, so two runs give the same bits; there are no floating-point atomics.  One host
// synchronisation per call, at the end, brings the n_submaps + 1 output offsets (and the overflow flag) home.
#include "submap_device.hpp"

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <memory>

namespace {

using namespace mrs::kfdev;

constexpr int kThreads = 256, kPerThread = 4, kTile = kThreads * kPerThread;      // points of one workgroup of k_cells / k_keys
constexpr unsigned long long kDropped = ~0ull;                                  // key of a point the pass-through dropped (valid keys < 2^63)

struct Segment {          // one keyframe of one submap, as the kernels see it
    long long arena;      // first point in the arena
    long long base;       // first position in the concatenated input of this call
    int count;            // points
    int submap;
    float T[12];          // rows 0..2 of the relative transform
};

struct Tile {
    int seg;
    int start;            // first point of the tile inside the segment
};

struct Grid {             // per submap, written by k_grid
    long long mn[3];
    long long mul_y, mul_z;
    int kept;             // 0: no point survived the pass-through
    int pad;
};

// ---- append: any input form -> float4 (x, y, z, intensity) -----------------------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(256) void k_to_float4(const T* __restrict__ src, int stride, int icol, long long n, float4* __restrict__ dst)
{
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const T* r = src + i * stride;
        dst[i] = make_float4((float)r[0], (float)r[1], (float)r[2], icol >= 0 ? (float)r[icol] : 0.0f);
    }
}

// ---- pass 1: per-submap cell bounds -----------------------------------------------------------------------------------------------------
// bounds: [n_submaps][6] ordered bits of min x, y, z (initialised to 0xffffffff) and max x, y, z (initialised to 0)
__global__ __launch_bounds__(kThreads) void k_cells(const float4* __restrict__ arena, const Segment* __restrict__ segs, const Tile* __restrict__ tiles,
                                                    float crop, float inv, unsigned* __restrict__ bounds)
{
    __shared__ Segment sg;
    __shared__ unsigned red[kThreads / 64][6];
    const Tile t = tiles[blockIdx.x];
    if (threadIdx.x < sizeof(Segment) / 4) reinterpret_cast<int*>(&sg)[threadIdx.x] = reinterpret_cast<const int*>(segs + t.seg)[threadIdx.x];
    __syncthreads();
    const float4* src = arena + sg.arena;
    unsigned lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < kPerThread; ++j) {
        const int i = t.start + j * kThreads + threadIdx.x;
        if (i < sg.count) {
            float x, y, z;
            if (move_and_crop(src[i], sg.T, crop, x, y, z)) {
                const unsigned c[3] = {order_bits(cell_of(x, inv)), order_bits(cell_of(y, inv)), order_bits(cell_of(z, inv))};
#pragma unroll
                for (int a = 0; a < 3; ++a) { lo[a] = min(lo[a], c[a]); hi[a] = max(hi[a], c[a]); }
            }
        }
    }
    wave_minmax3(lo, hi);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0)
        for (int a = 0; a < 3; ++a) { red[wave][a] = lo[a]; red[wave][3 + a] = hi[a]; }
    __syncthreads();
    if (threadIdx.x < 6) {                       // one global atomic per workgroup and component, none when the tile kept nothing
        const int a = threadIdx.x;
        unsigned v = red[0][a];
        for (int w = 1; w < kThreads / 64; ++w) v = a < 3 ? min(v, red[w][a]) : max(v, red[w][a]);
        unsigned* dst = bounds + (size_t)sg.submap * 6 + a;
        if (a < 3) { if (v != 0xffffffffu) atomicMin(dst, v); }
        else if (v != 0u) atomicMax(dst, v);
    }
}

// ---- per submap: minimum cell, key multipliers, 63-bit check ------------------------------------------------------------------------------
__global__ void k_grid(const unsigned* __restrict__ bounds, int n_submaps, Grid* __restrict__ grids, int* __restrict__ overflow)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n_submaps) return;
    Grid g = {};
    const unsigned* bb = bounds + (size_t)b * 6;
    if (bb[0] <= bb[3]) {                        // something was kept (all three components are set together)
        g.kept = 1;
        int bits;
        const bool ok = grid_from_bounds(bb, g.mn, g.mul_y, g.mul_z, bits);
        if (!ok) { g.kept = 0; atomicOr(overflow, 1); }
    }
    grids[b] = g;
}

// ---- pass 2: voxel keys ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_keys(const float4* __restrict__ arena, const Segment* __restrict__ segs, const Tile* __restrict__ tiles,
                                                   const Grid* __restrict__ grids, float crop, float inv, unsigned long long* __restrict__ keys,
                                                   int* __restrict__ vals)
{
    __shared__ Segment sg;
    __shared__ Grid gr;
    const Tile t = tiles[blockIdx.x];
    if (threadIdx.x < sizeof(Segment) / 4) reinterpret_cast<int*>(&sg)[threadIdx.x] = reinterpret_cast<const int*>(segs + t.seg)[threadIdx.x];
    __syncthreads();
    if (threadIdx.x < sizeof(Grid) / 4) reinterpret_cast<int*>(&gr)[threadIdx.x] = reinterpret_cast<const int*>(grids + sg.submap)[threadIdx.x];
    __syncthreads();
    const float4* src = arena + sg.arena;
#pragma unroll
    for (int j = 0; j < kPerThread; ++j) {
        const int i = t.start + j * kThreads + threadIdx.x;
        if (i < sg.count) {
            float x, y, z;
            unsigned long long key = kDropped;
            if (move_and_crop(src[i], sg.T, crop, x, y, z) && gr.kept) {
                key = voxel_key(x, y, z, inv, gr.mn[0], gr.mn[1], gr.mn[2], gr.mul_y, gr.mul_z);
            }
            const long long pos = sg.base + i;
            keys[pos] = key;
            vals[pos] = (int)pos;
        }
    }
}

// ---- run heads of the sorted keys -------------------------------------------------------------------------------------------------------------
// sub_base [n_submaps + 1]: first input position of every submap.  The tiles partition the positions, and a tile lies inside one submap.
__global__ __launch_bounds__(kThreads) void k_heads(const unsigned long long* __restrict__ keys, const Segment* __restrict__ segs,
                                                    const Tile* __restrict__ tiles, const int* __restrict__ sub_base, int* __restrict__ head)
{
    const Tile t = tiles[blockIdx.x];
    const Segment* sg = segs + t.seg;
    const int count = sg->count;
    const long long base = sg->base, first = sub_base[sg->submap];
#pragma unroll
    for (int j = 0; j < kPerThread; ++j) {
        const int i = t.start + j * kThreads + threadIdx.x;
        if (i < count) {
            const long long pos = base + i;
            const unsigned long long k = keys[pos];
            head[pos] = (k != kDropped && (pos == first || keys[pos - 1] != k)) ? 1 : 0;
        }
    }
}

// segment of input position `pos` (seg_base ascending, n_seg >= 1)
__device__ __forceinline__ int segment_of(const Segment* __restrict__ segs, int n_seg, long long pos)
{
    int lo = 0, hi = n_seg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (segs[mid].base <= pos) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// ---- one voxel per thread: ordered float64 sums of the recomputed points, one rounding to float32 -----------------------------------------------
__global__ __launch_bounds__(kThreads) void k_means(const float4* __restrict__ arena, const Segment* __restrict__ segs, int n_seg,
                                                    const unsigned long long* __restrict__ keys, const int* __restrict__ vals,
                                                    const int* __restrict__ head, const int* __restrict__ slot, long long n_in, float crop,
                                                    float4* __restrict__ out)
{
    for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < n_in; p += (long long)gridDim.x * blockDim.x) {
        if (!head[p]) continue;
        const unsigned long long k = keys[p];
        int s = segment_of(segs, n_seg, vals[p]);
        const int submap = segs[s].submap;
        double sx = 0.0, sy = 0.0, sz = 0.0, si = 0.0;
        long long m = 0;
        for (long long q = p; q < n_in && keys[q] == k; ++q) {
            const long long pos = vals[q];
            // equal keys keep input order, so the positions of a run ascend: the segment only ever moves forward
            if (pos < segs[s].base) s = segment_of(segs, n_seg, pos);
            while (s + 1 < n_seg && segs[s + 1].base <= pos) ++s;
            if (segs[s].submap != submap) break;               // the same key in the next submap
            const float4 pt = arena[segs[s].arena + (pos - segs[s].base)];
            float x, y, z;
            (void)move_and_crop(pt, segs[s].T, crop, x, y, z);
            sx += (double)x; sy += (double)y; sz += (double)z; si += (double)pt.w;
            ++m;
        }
        out[slot[p]] = mean_of(sx, sy, sz, si, (double)m);
    }
}

// offsets [n_submaps + 1] (int64) from the prefix sum of the run heads, then the overflow flag as one more int64
__global__ void k_offsets(const int* __restrict__ head, const int* __restrict__ slot, const int* __restrict__ sub_base, int n_submaps,
                          const int* __restrict__ overflow, long long* __restrict__ out)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b > n_submaps + 1) return;
    if (b == n_submaps + 1) { out[b] = *overflow; return; }
    const int n_in = sub_base[n_submaps];
    const int pos = sub_base[b];
    out[b] = pos < n_in ? slot[pos] : slot[n_in - 1] + head[n_in - 1];
}

// inverse(centre) * near, float32, term by term (every product and sum rounded once, in this order)
void relative_transform(const float* Pc, const float* Pk, float* T)
{
    for (int i = 0; i < 3; ++i) {
        const float r0 = Pc[0 * 4 + i], r1 = Pc[1 * 4 + i], r2 = Pc[2 * 4 + i];       // row i of Rc^T
        const float ti = -((r0 * Pc[3] + r1 * Pc[7]) + r2 * Pc[11]);
        for (int j = 0; j < 3; ++j) T[4 * i + j] = (r0 * Pk[j] + r1 * Pk[4 + j]) + r2 * Pk[8 + j];
        T[4 * i + 3] = ((r0 * Pk[3] + r1 * Pk[7]) + r2 * Pk[11]) + ti;
    }
    T[12] = T[13] = T[14] = 0.0f; T[15] = 1.0f;
}

// the whole assembly; lock held, device current
int assemble_locked(mrs_keyframes* kf, int n_submaps, int n_seg, const int32_t* seg_submap, const int32_t* seg_keyframe, const float* seg_T,
                    float crop, float leaf, float* d_out, long long capacity, int64_t* h_offsets, hipStream_t user)
{
    MRS_REQUIRE(std::isfinite(leaf) && leaf > 0.0f, "the leaf size must be positive and finite");
    MRS_REQUIRE(std::isfinite(crop) && crop >= 0.0f, "the crop must be non-negative and finite");
    const int n_kf = (int)kf->offsets.size() - 1;
    std::vector<Segment> segs;
    std::vector<Tile> tiles;
    std::vector<int> sub_base(n_submaps + 1, 0);
    long long n_in = 0;
    int prev = 0;
    for (int i = 0; i < n_seg; ++i) {
        const int b = seg_submap[i], k = seg_keyframe[i];
        MRS_REQUIRE(b >= prev && b < n_submaps, "segments must be grouped by submap, in ascending submap order");
        MRS_REQUIRE(k >= 0 && k < n_kf, "keyframe id out of range");
        for (int j = 0; j < 12; ++j) MRS_REQUIRE(std::isfinite(seg_T[16 * i + j]), "a segment transform is not finite");
        const long long cnt = kf->offsets[k + 1] - kf->offsets[k];
        for (int bb = prev + 1; bb <= b; ++bb) sub_base[bb] = (int)n_in;
        prev = b;
        if (cnt == 0) continue;
        MRS_REQUIRE(n_in + cnt < 0x7fffffffll, "more than 2^31 - 1 segment points in one call: split the batch");
        Segment s;
        s.arena = kf->offsets[k]; s.base = n_in; s.count = (int)cnt; s.submap = b;
        memcpy(s.T, seg_T + 16 * i, 12 * sizeof(float));
        for (long long st = 0; st < cnt; st += kTile) tiles.push_back(Tile{(int)segs.size(), (int)st});
        segs.push_back(s);
        n_in += cnt;
    }
    for (int bb = prev + 1; bb <= n_submaps; ++bb) sub_base[bb] = (int)n_in;
    MRS_REQUIRE(capacity >= n_in, "capacity below the sum of the segments' point counts");
    if (n_in == 0) {
        for (int b = 0; b <= n_submaps; ++b) h_offsets[b] = 0;
        return MRS_OK;
    }
    MRS_REQUIRE(d_out != nullptr, "null pointer");
    const int n_tiles = (int)tiles.size(), ns = (int)segs.size();
    const float inv = 1.0f / leaf;

    // one scratch block, carved: tables (segments | tiles | submap bases | cell bounds | overflow flag: built on the host, one copy) | grids |
    // keys x 2 | values x 2 | heads | slots | offsets | sort / scan workspace
    const size_t b_segs = round256(ns * sizeof(Segment)), b_tiles = round256(n_tiles * sizeof(Tile)), b_sub = round256((n_submaps + 1) * sizeof(int));
    const size_t b_bounds = round256((size_t)n_submaps * 6 * sizeof(unsigned));
    const size_t b_tables = b_segs + b_tiles + b_sub + b_bounds + 256;
    const size_t b_grids = round256((size_t)n_submaps * sizeof(Grid));
    const size_t b_keys = round256((size_t)n_in * 8), b_vals = round256((size_t)n_in * 4), b_offs = round256((size_t)(n_submaps + 2) * 8);
    size_t b_sort = 0, b_scan = 0;
    unsigned long long* nk = nullptr;
    int* ni = nullptr;
    MRS_HIP_TRY(hipcub::DeviceSegmentedRadixSort::SortPairs(nullptr, b_sort, nk, nk, ni, ni, (int)n_in, n_submaps, ni, ni, 0, 64, kf->s));
    MRS_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, b_scan, ni, ni, (int)n_in, kf->s));
    const size_t b_tmp = round256(std::max(b_sort, b_scan));
    mrs::Scratch work;
    int st = work.alloc(b_tables + b_grids + 2 * b_keys + 4 * b_vals + b_offs + b_tmp, kf->s);
    if (st != MRS_OK) return st;
    char* w = work.as<char>();
    Segment* d_segs = reinterpret_cast<Segment*>(w);
    Tile* d_tiles = reinterpret_cast<Tile*>(w + b_segs);
    int* d_sub = reinterpret_cast<int*>(w + b_segs + b_tiles);
    unsigned* d_bounds = reinterpret_cast<unsigned*>(w + b_segs + b_tiles + b_sub);
    int* d_overflow = reinterpret_cast<int*>(w + b_segs + b_tiles + b_sub + b_bounds);
    w += b_tables;
    Grid* d_grids = reinterpret_cast<Grid*>(w); w += b_grids;
    unsigned long long* d_keys = reinterpret_cast<unsigned long long*>(w); w += b_keys;
    unsigned long long* d_keys_s = reinterpret_cast<unsigned long long*>(w); w += b_keys;
    int* d_vals = reinterpret_cast<int*>(w); w += b_vals;
    int* d_vals_s = reinterpret_cast<int*>(w); w += b_vals;
    int* d_head = reinterpret_cast<int*>(w); w += b_vals;
    int* d_slot = reinterpret_cast<int*>(w); w += b_vals;
    long long* d_offs = reinterpret_cast<long long*>(w); w += b_offs;
    void* d_tmp = w;

    if ((st = stage_reserve(kf, std::max(b_tables, b_offs))) != MRS_OK) return st;
    char* h = kf->h_stage.get();
    memset(h, 0, b_tables);
    memcpy(h, segs.data(), ns * sizeof(Segment));
    memcpy(h + b_segs, tiles.data(), n_tiles * sizeof(Tile));
    memcpy(h + b_segs + b_tiles, sub_base.data(), (n_submaps + 1) * sizeof(int));
    unsigned* hb = reinterpret_cast<unsigned*>(h + b_segs + b_tiles + b_sub);
    for (int b = 0; b < n_submaps; ++b) hb[6 * b] = hb[6 * b + 1] = hb[6 * b + 2] = 0xffffffffu;      // minima; the maxima and the flag start at 0
    MRS_TRY(kf->s.join_in(user));        // d_out may still be in use on the caller's stream
    MRS_HIP_TRY(hipMemcpyAsync(d_segs, h, b_tables, hipMemcpyHostToDevice, kf->s));
    // development aid (MRS_DEV=1 MRS_SUBMAP_TIMING=1, tools/bench_submap.py): events between the steps, one line on stderr per call
    mrs::StageMarks marks(mrs::dev_env("MRS_SUBMAP_TIMING") != nullptr, kf->s);
    const float4* arena = kf->arena.get();
    marks.mark(0);
    hipLaunchKernelGGL(k_cells, dim3(n_tiles), dim3(kThreads), 0, kf->s, arena, d_segs, d_tiles, crop, inv, d_bounds);
    hipLaunchKernelGGL(k_grid, dim3((n_submaps + 63) / 64), dim3(64), 0, kf->s, d_bounds, n_submaps, d_grids, d_overflow);
    marks.mark(1);
    hipLaunchKernelGGL(k_keys, dim3(n_tiles), dim3(kThreads), 0, kf->s, arena, d_segs, d_tiles, d_grids, crop, inv, d_keys, d_vals);
    marks.mark(2);
    MRS_HIP_TRY(hipcub::DeviceSegmentedRadixSort::SortPairs(d_tmp, b_sort, d_keys, d_keys_s, d_vals, d_vals_s, (int)n_in, n_submaps, d_sub, d_sub + 1,
                                                            0, 64, kf->s));
    marks.mark(3);
    hipLaunchKernelGGL(k_heads, dim3(n_tiles), dim3(kThreads), 0, kf->s, d_keys_s, d_segs, d_tiles, d_sub, d_head);
    MRS_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(d_tmp, b_scan, d_head, d_slot, (int)n_in, kf->s));
    marks.mark(4);
    const int mean_blocks = (int)std::min<long long>((n_in + kThreads - 1) / kThreads, 8192);
    hipLaunchKernelGGL(k_means, dim3(mean_blocks), dim3(kThreads), 0, kf->s, arena, d_segs, ns, d_keys_s, d_vals_s, d_head, d_slot, n_in, crop,
                       reinterpret_cast<float4*>(d_out));
    hipLaunchKernelGGL(k_offsets, dim3((n_submaps + 2 + 63) / 64), dim3(64), 0, kf->s, d_head, d_slot, d_sub, n_submaps, d_overflow, d_offs);
    marks.mark(5);
    MRS_HIP_TRY(hipGetLastError());
    MRS_HIP_TRY(hipMemcpyAsync(h, d_offs, (size_t)(n_submaps + 2) * 8, hipMemcpyDeviceToHost, kf->s));
    MRS_HIP_TRY(hipStreamSynchronize(kf->s));                   // the one synchronisation of the call
    if (marks)
        fprintf(stderr, "[mrslam] submap steps ms: cells+grid %.4f keys %.4f sort %.4f heads+scan %.4f means+offsets %.4f points %lld\n", marks.ms(0),
                marks.ms(1), marks.ms(2), marks.ms(3), marks.ms(4), n_in);
    const long long* ho = reinterpret_cast<const long long*>(h);
    if (ho[n_submaps + 1]) {
        mrs::set_error("a submap's voxel grid needs keys of more than 63 bits (leaf %g): choose a larger leaf", (double)leaf);
        return MRS_ERR_ARG;
    }
    for (int b = 0; b <= n_submaps; ++b) h_offsets[b] = ho[b];
    return MRS_OK;
}

}  // namespace

extern "C" {

int mrs_keyframes_create(mrs_ctx* ctx, int64_t capacity_hint_points, mrs_keyframes** out)
{
    MRS_REQUIRE(ctx && out, "null pointer");
    *out = nullptr;
    MRS_REQUIRE(capacity_hint_points >= 0 && capacity_hint_points <= kMaxArenaPoints, "capacity hint negative or above 2^34 points");
    MRS_HIP_TRY(hipSetDevice(ctx->device));
    std::unique_ptr<mrs_keyframes> kf(new mrs_keyframes());      // an early return deletes it: every member frees itself
    kf->ctx = ctx;
    MRS_TRY(kf->s.create());
    MRS_TRY(arena_reserve(kf.get(), std::max<long long>(capacity_hint_points, 1)));      // nobody else can hold the handle yet: no lock
    *out = kf.release();
    return MRS_OK;
}

int mrs_keyframes_destroy(mrs_keyframes* kf)
{
    if (!kf) return MRS_OK;
    (void)hipSetDevice(kf->ctx->device);
    delete kf;
    return MRS_OK;
}

int mrs_keyframes_size(mrs_keyframes* kf, int32_t* out_n, int64_t* out_points)
{
    MRS_REQUIRE(kf && out_n, "null pointer");
    std::lock_guard<std::mutex> lk(kf->mu);
    *out_n = (int32_t)kf->offsets.size() - 1;
    if (out_points) *out_points = kf->offsets.back();
    return MRS_OK;
}

int mrs_keyframes_append(mrs_keyframes* kf, const void* points, int32_t on_device, int32_t is_double, int32_t stride, int32_t intensity_col,
                         int64_t n, const float* h_pose16, int32_t* out_id, mrs_stream stream)
{
    MRS_REQUIRE(kf && h_pose16 && out_id, "null pointer");
    MRS_REQUIRE(n >= 0 && n < 0x7fffffffll, "point count out of range");
    MRS_REQUIRE(points || n == 0, "null pointer");
    MRS_REQUIRE(stride == 3 || stride == 4 || stride == 8, "stride must be 3, 4 or 8");
    MRS_REQUIRE(intensity_col < stride && (intensity_col < 0 || intensity_col >= 3), "the intensity column must be -1 (none) or in [3, stride)");
    MRS_REQUIRE(rigid_finite(h_pose16), "the pose is not finite");
    MRS_HIP_TRY(hipSetDevice(kf->ctx->device));
    std::lock_guard<std::mutex> lk(kf->mu);
    const long long used = kf->offsets.back();
    int st = arena_reserve(kf, used + n);
    if (st != MRS_OK) return st;
    float4* dst = kf->arena.get() + used;
    if (n > 0) {
        const size_t elem = is_double ? 8 : 4, bytes = (size_t)n * stride * elem;
        const bool as_is = !is_double && stride == 4 && intensity_col == 3;                  // already float4 (x, y, z, intensity): one copy
        const void* src = points;
        mrs::Scratch raw;
        if (on_device) {
            MRS_TRY(kf->s.join_in((hipStream_t)stream));
            if (as_is) MRS_HIP_TRY(hipMemcpyAsync(dst, points, bytes, hipMemcpyDeviceToDevice, kf->s));
        } else {
            if ((st = stage_reserve(kf, bytes)) != MRS_OK) return st;
            memcpy(kf->h_stage.get(), points, bytes);
            void* to = dst;
            if (!as_is) {
                if ((st = raw.alloc(bytes, kf->s)) != MRS_OK) return st;
                to = raw.p;
            }
            MRS_HIP_TRY(hipMemcpyAsync(to, kf->h_stage.get(), bytes, hipMemcpyHostToDevice, kf->s));
            src = to;
        }
        if (!as_is) {
            const int blocks = (int)std::min<long long>((n + 255) / 256, 4096);
            if (is_double) hipLaunchKernelGGL(k_to_float4<double>, dim3(blocks), dim3(256), 0, kf->s, static_cast<const double*>(src), stride, intensity_col, (long long)n, dst);
            else hipLaunchKernelGGL(k_to_float4<float>, dim3(blocks), dim3(256), 0, kf->s, static_cast<const float*>(src), stride, intensity_col, (long long)n, dst);
            MRS_HIP_TRY(hipGetLastError());
        }
        if (on_device) {          // the caller may overwrite its buffer once ITS stream has passed this point
            MRS_TRY(kf->s.release_to((hipStream_t)stream));
        } else {
            MRS_HIP_TRY(hipStreamSynchronize(kf->s));       // the staging buffer and the caller's memory are free again
        }
    }
    *out_id = (int32_t)kf->offsets.size() - 1;
    kf->offsets.push_back(used + n);
    kf->poses.insert(kf->poses.end(), h_pose16, h_pose16 + 16);
    return MRS_OK;
}

int mrs_keyframes_set_pose(mrs_keyframes* kf, int32_t id, const float* h_pose16)
{
    MRS_REQUIRE(kf && h_pose16, "null pointer");
    MRS_REQUIRE(rigid_finite(h_pose16), "the pose is not finite");
    std::lock_guard<std::mutex> lk(kf->mu);
    MRS_REQUIRE(id >= 0 && id < (int)kf->offsets.size() - 1, "keyframe id out of range");
    memcpy(kf->poses.data() + 16 * (size_t)id, h_pose16, 16 * sizeof(float));
    return MRS_OK;
}

int mrs_keyframes_get_pose(mrs_keyframes* kf, int32_t id, float* h_pose16, int64_t* out_points)
{
    MRS_REQUIRE(kf && h_pose16, "null pointer");
    std::lock_guard<std::mutex> lk(kf->mu);
    MRS_REQUIRE(id >= 0 && id < (int)kf->offsets.size() - 1, "keyframe id out of range");
    memcpy(h_pose16, kf->poses.data() + 16 * (size_t)id, 16 * sizeof(float));
    if (out_points) *out_points = kf->offsets[id + 1] - kf->offsets[id];
    return MRS_OK;
}

int mrs_submap_assemble(mrs_keyframes* kf, int32_t n_submaps, int32_t n_segments, const int32_t* h_seg_submap, const int32_t* h_seg_keyframe,
                        const float* h_seg_T16, float crop, float leaf, float* d_out, int64_t capacity_points, int64_t* h_offsets, mrs_stream stream)
{
    MRS_REQUIRE(kf && h_offsets, "null pointer");
    MRS_REQUIRE(n_submaps >= 0 && n_segments >= 0 && capacity_points >= 0, "negative count");
    MRS_REQUIRE(n_segments == 0 || (h_seg_submap && h_seg_keyframe && h_seg_T16), "null pointer");
    MRS_HIP_TRY(hipSetDevice(kf->ctx->device));
    std::lock_guard<std::mutex> lk(kf->mu);
    return assemble_locked(kf, n_submaps, n_segments, h_seg_submap, h_seg_keyframe, h_seg_T16, crop, leaf, d_out, capacity_points, h_offsets,
                           (hipStream_t)stream);
}

int mrs_submap_merge_nearest(mrs_keyframes* kf, int32_t n_submaps, const int32_t* h_loop_ids, int32_t submap_size, float crop, float leaf,
                             float* d_out, int64_t capacity_points, int64_t* h_offsets, mrs_stream stream)
{
    MRS_REQUIRE(kf && h_offsets, "null pointer");
    MRS_REQUIRE(n_submaps >= 0 && capacity_points >= 0, "negative count");
    MRS_REQUIRE(n_submaps == 0 || h_loop_ids, "null pointer");
    MRS_REQUIRE(submap_size >= 0 && submap_size <= (1 << 20), "submap_size out of range");
    MRS_HIP_TRY(hipSetDevice(kf->ctx->device));
    std::lock_guard<std::mutex> lk(kf->mu);
    const int n_kf = (int)kf->offsets.size() - 1;
    std::vector<int32_t> seg_submap, seg_keyframe;
    std::vector<float> seg_T;
    for (int b = 0; b < n_submaps; ++b) {
        const int c = h_loop_ids[b];
        MRS_REQUIRE(c >= 0 && c < n_kf, "loop keyframe id out of range");
        // global_manager.cpp:1904-1911: keyNear = loop_id + i, i = -submap_size .. submap_size; `keyNear <= 0` skipped like the reference does
        // (keyframe 0 is never merged); the reference lets keyNear == size() through and reads past the vector -- dropped here
        const int lo = std::max(c - submap_size, 1), hi = std::min(c + submap_size, n_kf - 1);
        for (int k = lo; k <= hi; ++k) {
            seg_submap.push_back(b);
            seg_keyframe.push_back(k);
            seg_T.resize(seg_T.size() + 16);
            relative_transform(kf->poses.data() + 16 * (size_t)c, kf->poses.data() + 16 * (size_t)k, seg_T.data() + seg_T.size() - 16);
        }
    }
    return assemble_locked(kf, n_submaps, (int)seg_submap.size(), seg_submap.data(), seg_keyframe.data(), seg_T.data(), crop, leaf, d_out,
                           capacity_points, h_offsets, (hipStream_t)stream);
}

}  // extern "C"
