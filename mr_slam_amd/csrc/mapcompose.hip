// mapcompose.hip -- the merged multi-robot point-cloud map composed on the GPU from the robots' keyframe stores (C ABI mrs_map_compose;
// SURVEY.md 8(a) row G8).
//
// What it replaces: GlobalManager::composeGlobalMap (Mapping/src/global_manager/src/global_manager.cpp:2090-2210) and savingGlobalMap
// (:143-170): every robot's keyframes moved by their optimised poses, concatenated (after the map composed so far, in the incremental
// branch), pcl::VoxelGrid over the whole thing -- on the host, on one thread.  Here ONE voxel grid covers the whole call:
//   k_mc_bounds : every point transformed, minimum / maximum voxel cell and the number of kept points (wave shuffles, LDS, one global
//                 atomic per workgroup and component); a segment reads its own store's arena through a table of base pointers, the
//                 previous map is one more source read as it is;
//   k_mc_grid   : minimum cell, key multipliers, 63-bit check, the number of key BITS the grid needs -> host (synchronisation 1 of 2);
//   k_mc_keys   : transform recomputed -> 64-bit key; a dropped point gets bit `bits` alone, so it sorts after every valid key;
//   device-wide stable radix sort of (key, input position) over the bits that matter;
//   k_mc_heads + inclusive prefix sum: the output slot of every sorted position;
//   k_mc_means  : one workgroup per 1024 consecutive SORTED positions: segment lookup in LDS, parallel gathers, segmented scan by key (thread,
//                 wave shuffles, LDS);
//                 runs inside the tile are written, runs across a tile edge leave partial sums in a per-tile table;
//   k_mc_stitch : the partial sums of a run added in tile order, the run written.
// All sums are float64 in an order fixed by the sorted order alone: the same bits from call to call, no floating-point atomics.
#include "submap_device.hpp"

#include <hipcub/hipcub.hpp>

#include <cmath>
#include <cstdlib>
#include <functional>

namespace {

using namespace mrs::kfdev;

constexpr int kThreads = 256, kPerThread = 4, kTile = kThreads * kPerThread, kWaves = kThreads / 64;
constexpr int kLdsSegments = 1024;       // k_mc_means keeps the segment lookup of a call with at most this many segments in LDS (12 KiB)
constexpr int kBoundsBlocks = 1024;      // workgroups of k_mc_bounds at most: 4 per compute unit, 7 atomics each on the same words

struct MapSegment {       // one keyframe (or the previous map) as the kernels see it
    long long first;      // first point in its source
    long long base;       // first position in the concatenated input of this call
    int count;            // points
    int source;           // row of the table of source pointers: a store's arena, or the previous map
    int raw;              // 1: the previous map, taken as it is
    int pad;
    float T[12];          // rows 0..2 of the transform
};

struct Tile {
    int seg;
    int start;            // first point of the tile inside the segment
};

struct Info {             // initial state from the host, results back to the host at the first synchronisation
    unsigned bounds[6];   // ordered bits of the minimum cell (initialised to 0xffffffff) and the maximum cell (0)
    unsigned kept;        // points that were not dropped
    int overflow;
    int bits;             // valid keys are < 2^bits
    int pad;
    long long mn[3];
    long long mul_y, mul_z;
};

struct Acc {              // partial sum of a run
    double x, y, z, w;
    int n;
};

struct Carry {            // per tile of k_mc_means
    Acc lead;             // the positions before the tile's first run head (the end of a run that began in an earlier tile)
    Acc trail;            // from the tile's last run head to its end, when that run goes on in the next tile
    int trail_slot;
    int flags;            // 1: the tile holds a run head; 2: trail is set
};
static_assert(sizeof(MapSegment) == 80 && sizeof(Acc) == 40 && sizeof(Carry) == 88, "DESIGN.md section 4.12 quotes these sizes");

__device__ __forceinline__ Acc acc_zero() { return Acc{0.0, 0.0, 0.0, 0.0, 0}; }
__device__ __forceinline__ Acc acc_add(const Acc& a, const Acc& b) { return Acc{a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w, a.n + b.n}; }      // earlier + later
__device__ __forceinline__ Acc acc_up(const Acc& a, int o)
{
    return Acc{__shfl_up(a.x, o, 64), __shfl_up(a.y, o, 64), __shfl_up(a.z, o, 64), __shfl_up(a.w, o, 64), __shfl_up(a.n, o, 64)};
}
__device__ __forceinline__ float4 acc_mean(const Acc& a)
{
    return mean_of(a.x, a.y, a.z, a.w, (double)a.n);
}

// a segment's point moved (section 4.11's arithmetic; the previous map is not moved) and whether it is kept: x', y', z' finite
__device__ __forceinline__ bool moved(const float4 p, const MapSegment& sg, float& x, float& y, float& z)
{
    if (sg.raw) {
        x = p.x; y = p.y; z = p.z;
        return finite3(x, y, z);
    }
    return move_and_crop(p, sg.T, kFltMax, x, y, z);
}

// ---- pass 1: cell bounds of the whole call, kept points -------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_mc_bounds(const float4* const* __restrict__ sources, const MapSegment* __restrict__ segs,
                                                        const Tile* __restrict__ tiles, int n_tiles, float inv, Info* __restrict__ info)
{
    __shared__ MapSegment sg;
    __shared__ unsigned red[kWaves][7];
    unsigned lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u}, kept = 0;
    // a workgroup walks several tiles before it touches the seven global words: every workgroup of the call updates the SAME words
    for (int tb = blockIdx.x; tb < n_tiles; tb += gridDim.x) {
        const Tile t = tiles[tb];
        __syncthreads();                         // the previous tile's segment is not read any more
        if (threadIdx.x < sizeof(MapSegment) / 4) reinterpret_cast<int*>(&sg)[threadIdx.x] = reinterpret_cast<const int*>(segs + t.seg)[threadIdx.x];
        __syncthreads();
        const float4* src = sources[sg.source] + sg.first;
#pragma unroll
        for (int j = 0; j < kPerThread; ++j) {
            const int i = t.start + j * kThreads + threadIdx.x;
            if (i < sg.count) {
                float x, y, z;
                if (moved(src[i], sg, x, y, z)) {
                    const unsigned c[3] = {order_bits(cell_of(x, inv)), order_bits(cell_of(y, inv)), order_bits(cell_of(z, inv))};
#pragma unroll
                    for (int a = 0; a < 3; ++a) { lo[a] = min(lo[a], c[a]); hi[a] = max(hi[a], c[a]); }
                    ++kept;
                }
            }
        }
    }
    wave_minmax3(lo, hi);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) kept += (unsigned)__shfl_xor((int)kept, o, 64);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        for (int a = 0; a < 3; ++a) { red[wave][a] = lo[a]; red[wave][3 + a] = hi[a]; }
        red[wave][6] = kept;
    }
    __syncthreads();
    if (threadIdx.x < 7) {                       // one global atomic per workgroup and component, none when the tile kept nothing
        const int a = threadIdx.x;
        unsigned v = red[0][a];
        for (int w = 1; w < kWaves; ++w) v = a < 3 ? min(v, red[w][a]) : a < 6 ? max(v, red[w][a]) : v + red[w][a];
        if (a < 3) { if (v != 0xffffffffu) atomicMin(&info->bounds[a], v); }
        else if (a < 6) { if (v != 0u) atomicMax(&info->bounds[a], v); }
        else if (v != 0u) atomicAdd(&info->kept, v);
    }
}

// ---- the grid: minimum cell, key multipliers, 63-bit check, key width ----------------------------------------------------------------------
__global__ void k_mc_grid(Info* __restrict__ info)
{
    if (blockIdx.x != 0 || threadIdx.x != 0 || info->kept == 0) return;
    if (!grid_from_bounds(info->bounds, info->mn, info->mul_y, info->mul_z, info->bits)) info->overflow = 1;
}

// ---- pass 2: voxel keys ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_mc_keys(const float4* const* __restrict__ sources, const MapSegment* __restrict__ segs,
                                                      const Tile* __restrict__ tiles, const Info* __restrict__ info, float inv,
                                                      unsigned long long* __restrict__ keys, int* __restrict__ vals)
{
    __shared__ MapSegment sg;
    const Tile t = tiles[blockIdx.x];
    if (threadIdx.x < sizeof(MapSegment) / 4) reinterpret_cast<int*>(&sg)[threadIdx.x] = reinterpret_cast<const int*>(segs + t.seg)[threadIdx.x];
    __syncthreads();
    const long long mx = info->mn[0], my = info->mn[1], mz = info->mn[2], mul_y = info->mul_y, mul_z = info->mul_z;
    const unsigned long long dropped = 1ull << info->bits;       // above every valid key, inside the bits + 1 that are sorted then
    const float4* src = sources[sg.source] + sg.first;
#pragma unroll
    for (int j = 0; j < kPerThread; ++j) {
        const int i = t.start + j * kThreads + threadIdx.x;
        if (i < sg.count) {
            float x, y, z;
            unsigned long long key = dropped;
            if (moved(src[i], sg, x, y, z)) {
                key = voxel_key(x, y, z, inv, mx, my, mz, mul_y, mul_z);
            }
            const long long pos = sg.base + i;
            keys[pos] = key;
            vals[pos] = (int)pos;
        }
    }
}

// ---- run heads of the sorted valid keys -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_mc_heads(const unsigned long long* __restrict__ keys, int n_valid, int* __restrict__ head)
{
    for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < n_valid; p += (long long)gridDim.x * blockDim.x)
        head[p] = (p == 0 || keys[p - 1] != keys[p]) ? 1 : 0;
}

// segment of input position `pos`: the last one whose base is <= pos (bases ascending, bases[0] == 0, n_seg >= 1)
template <class Bases>
__device__ __forceinline__ int segment_of(Bases bases, int n_seg, int pos)
{
    int lo = 0, hi = n_seg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (bases[mid] <= pos) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// ---- means, cooperatively: segmented scan by key over a tile of sorted positions --------------------------------------------------------------
// rank[p] = run heads in [0, p] (inclusive prefix sum), so rank[p] - 1 is the output slot of the run position p belongs to.  Thread t owns the
// positions tile + 4 t .. tile + 4 t + 3.  The scan element is (a run head was seen, sum since that head or since the tile's start).
// The segment lookup is two compact tables, bases[s] = first input position of segment s and origin[s] = the address input position 0 would
// have if the segment's source went on to the left, so that input position pos lies at origin[s][pos].  With at most kLdsSegments segments
// the workgroup copies both to LDS first, and what is left of the chain in global memory is position -> point; otherwise they stay in
// global memory.
__global__ __launch_bounds__(kThreads) void k_mc_means(const int* __restrict__ bases, const float4* const* __restrict__ origin,
                                                       const MapSegment* __restrict__ segs, int n_seg,
                                                       const unsigned long long* __restrict__ keys, const int* __restrict__ vals,
                                                       const int* __restrict__ rank, int n_valid, float4* __restrict__ out,
                                                       Carry* __restrict__ carry)
{
    __shared__ Acc w_sum[kWaves];
    __shared__ int w_seen[kWaves];
    __shared__ int s_bases[kLdsSegments];
    __shared__ const float4* s_origin[kLdsSegments];
    const bool in_lds = n_seg <= kLdsSegments;                   // the same for every thread of the call
    if (in_lds)
        for (int i = threadIdx.x; i < n_seg; i += kThreads) { s_bases[i] = bases[i]; s_origin[i] = origin[i]; }
    const long long p0 = (long long)blockIdx.x * kTile + (long long)threadIdx.x * kPerThread;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    Acc v[kPerThread];
    bool valid[kPerThread], head[kPerThread], tail[kPerThread];
    unsigned long long k[kPerThread + 2] = {};
#pragma unroll
    for (int i = 0; i < kPerThread + 2; ++i) {
        const long long p = p0 - 1 + i;
        if (p >= 0 && p < n_valid) k[i] = keys[p];
    }
    int pos[kPerThread], sgi[kPerThread];
    const float4* from[kPerThread];
#pragma unroll
    for (int i = 0; i < kPerThread; ++i) {
        const long long p = p0 + i;
        valid[i] = p < n_valid;
        head[i] = valid[i] && (p == 0 || k[i] != k[i + 1]);
        tail[i] = valid[i] && (p + 1 >= n_valid || k[i + 2] != k[i + 1]);
        pos[i] = valid[i] ? vals[p] : 0;
    }
    __syncthreads();                                             // the tables are in LDS
    if (in_lds) {
#pragma unroll
        for (int i = 0; i < kPerThread; ++i) { sgi[i] = segment_of(s_bases, n_seg, pos[i]); from[i] = s_origin[sgi[i]]; }
    } else {
#pragma unroll
        for (int i = 0; i < kPerThread; ++i) { sgi[i] = segment_of(bases, n_seg, pos[i]); from[i] = origin[sgi[i]]; }
    }
    // the four gathers of the thread, issued together
    float4 pt[kPerThread];
#pragma unroll
    for (int i = 0; i < kPerThread; ++i) pt[i] = valid[i] ? from[i][pos[i]] : make_float4(0.f, 0.f, 0.f, 0.f);
    Acc agg = acc_zero();
    int seen = 0;
#pragma unroll
    for (int i = 0; i < kPerThread; ++i) {
        v[i] = acc_zero();
        if (valid[i]) {
            float x, y, z;
            (void)moved(pt[i], segs[sgi[i]], x, y, z);
            v[i] = Acc{(double)x, (double)y, (double)z, (double)pt[i].w, 1};
            if (head[i]) { agg = v[i]; seen = 1; }
            else agg = acc_add(agg, v[i]);
        }
    }
    // inclusive segmented scan of the threads' elements across the wave: fixed shape
    Acc inc = agg;
    int f = seen;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const Acc up = acc_up(inc, o);
        const int uf = __shfl_up(f, o, 64);
        if (lane >= o) {
            if (!f) inc = acc_add(up, inc);
            f |= uf;
        }
    }
    Acc ex = acc_up(inc, 1);
    int ef = __shfl_up(f, 1, 64);
    if (lane == 0) { ex = acc_zero(); ef = 0; }
    if (lane == 63) { w_sum[wave] = inc; w_seen[wave] = f; }
    __syncthreads();
    Acc run = acc_zero();
    int run_seen = 0;
    for (int w = 0; w < wave; ++w) {             // the waves before this one, in order
        if (w_seen[w]) { run = w_sum[w]; run_seen = 1; }
        else run = acc_add(run, w_sum[w]);
    }
    if (ef) run = ex; else run = acc_add(run, ex);
    run_seen |= ef;
    // the thread's own positions again, now with what came before them in the tile
    Carry* c = carry + blockIdx.x;
    if (threadIdx.x == 0 && head[0]) c->lead = acc_zero();
#pragma unroll
    for (int i = 0; i < kPerThread; ++i) {
        if (!valid[i]) continue;
        const long long p = p0 + i;
        if (head[i]) { run = v[i]; run_seen = 1; }
        else run = acc_add(run, v[i]);
        const bool last = (threadIdx.x == kThreads - 1 && i == kPerThread - 1) || p + 1 >= n_valid;       // last position of the tile
        if (tail[i]) {
            if (run_seen) out[rank[p] - 1] = acc_mean(run);      // the run began in this tile
            else c->lead = run;                                  // it began earlier
        } else if (last) {                                       // the run goes on in the next tile
            if (run_seen) { c->trail = run; c->trail_slot = rank[p] - 1; }
            else c->lead = run;                                  // the whole tile is the middle of one run
        }
        if (last) c->flags = (run_seen ? 1 : 0) | ((!tail[i] && run_seen) ? 2 : 0);
    }
}

// ---- a run that crosses tile edges: its parts added in tile order ----------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_mc_stitch(const Carry* __restrict__ carry, int n_tiles, float4* __restrict__ out)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_tiles || !(carry[t].flags & 2)) return;
    Acc sum = carry[t].trail;
    for (int u = t + 1; u < n_tiles; ++u) {
        sum = acc_add(sum, carry[u].lead);
        if (carry[u].flags & 1) break;           // the run ended before that tile's first head
    }
    out[carry[t].trail_slot] = acc_mean(sum);
}

}  // namespace

extern "C" {

int mrs_map_compose(int32_t n_stores, mrs_keyframes* const* stores, int32_t n_segments, const int32_t* h_seg_store, const int32_t* h_seg_keyframe,
                    const float* h_seg_T16, const float* d_prev, int64_t n_prev, float leaf, float* d_out, int64_t capacity_points,
                    int64_t* out_points, mrs_stream stream)
{
    MRS_REQUIRE(stores && out_points, "null pointer");
    MRS_REQUIRE(n_stores >= 1 && n_stores <= MRS_MAP_MAX_STORES, "the number of stores must be 1 .. MRS_MAP_MAX_STORES");
    MRS_REQUIRE(n_segments >= 0 && n_prev >= 0 && capacity_points >= 0, "negative count");
    MRS_REQUIRE(n_segments == 0 || (h_seg_store && h_seg_keyframe && h_seg_T16), "null pointer");
    MRS_REQUIRE(n_prev == 0 || d_prev, "null pointer");
    MRS_REQUIRE(std::isfinite(leaf) && leaf > 0.0f, "the leaf size must be positive and finite");
    for (int i = 0; i < n_stores; ++i) {
        MRS_REQUIRE(stores[i] != nullptr, "null pointer");
        MRS_REQUIRE(stores[i]->ctx->device == stores[0]->ctx->device, "the stores live on different devices");
    }
    mrs_keyframes* kf = stores[0];               // the call runs on the first store's stream and uses its staging buffer
    MRS_HIP_TRY(hipSetDevice(kf->ctx->device));
    // every distinct store locked once, in address order: two concurrent calls cannot wait for each other
    std::vector<mrs_keyframes*> uniq(stores, stores + n_stores);
    std::sort(uniq.begin(), uniq.end(), std::less<mrs_keyframes*>());
    uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
    std::vector<std::unique_lock<std::mutex>> locks;
    locks.reserve(uniq.size());
    for (mrs_keyframes* u : uniq) locks.emplace_back(u->mu);

    std::vector<MapSegment> segs;
    std::vector<Tile> tiles;
    long long n_in = 0;
    auto push = [&](const MapSegment& s) {
        for (long long st = 0; st < s.count; st += kTile) tiles.push_back(Tile{(int)segs.size(), (int)st});
        segs.push_back(s);
        n_in += s.count;
    };
    MRS_REQUIRE(n_prev <= 0x7fffffffll, "more than 2^31 - 1 input points in one call");
    if (n_prev > 0) {
        MapSegment s = {};
        s.count = (int)n_prev; s.source = n_stores; s.raw = 1;
        push(s);
    }
    for (int i = 0; i < n_segments; ++i) {
        const int r = h_seg_store[i], k = h_seg_keyframe[i];
        MRS_REQUIRE(r >= 0 && r < n_stores, "store index out of range");
        MRS_REQUIRE(k >= 0 && k < (int)stores[r]->offsets.size() - 1, "keyframe id out of range");
        for (int j = 0; j < 16; ++j) MRS_REQUIRE(std::isfinite(h_seg_T16[16 * i + j]), "a segment transform is not finite");
        const long long cnt = stores[r]->offsets[k + 1] - stores[r]->offsets[k];
        if (cnt == 0) continue;
        MRS_REQUIRE(n_in + cnt <= 0x7fffffffll, "more than 2^31 - 1 input points in one call");
        MapSegment s = {};
        s.first = stores[r]->offsets[k]; s.base = n_in; s.count = (int)cnt; s.source = r;
        memcpy(s.T, h_seg_T16 + 16 * i, 12 * sizeof(float));
        push(s);
    }
    MRS_REQUIRE(capacity_points >= n_in, "capacity below the previous map's points plus the segments' point counts");
    if (n_in == 0) { *out_points = 0; return MRS_OK; }
    MRS_REQUIRE(d_out != nullptr, "null pointer");
    if (n_prev > 0) {
        const uintptr_t a = (uintptr_t)d_prev, a_end = a + (size_t)n_prev * 16, b = (uintptr_t)d_out, b_end = b + (size_t)capacity_points * 16;
        MRS_REQUIRE(a_end <= b || b_end <= a, "the previous map overlaps the output");
    }
    const int n_tiles = (int)tiles.size(), ns = (int)segs.size();
    const float inv = 1.0f / leaf;
    hipStream_t s = kf->s;

    // tables, built on the host, one copy: info (bounds in their initial state) | source pointers | segments | tiles | segment bases | origins
    const size_t b_info = round256(sizeof(Info)), b_src = round256((size_t)(n_stores + 1) * sizeof(void*)), b_segs = round256(ns * sizeof(MapSegment)),
                 b_tiles = round256(n_tiles * sizeof(Tile)), b_bases = round256(ns * sizeof(int)), b_origin = round256(ns * sizeof(void*)),
                 b_tables = b_info + b_src + b_segs + b_tiles + b_bases + b_origin;
    mrs::Scratch tables;
    int st = tables.alloc(b_tables, s);
    if (st != MRS_OK) return st;
    if ((st = stage_reserve(kf, b_tables)) != MRS_OK) return st;
    char* h = kf->h_stage.get();
    memset(h, 0, b_tables);
    Info* hi = reinterpret_cast<Info*>(h);
    hi->bounds[0] = hi->bounds[1] = hi->bounds[2] = 0xffffffffu;
    const float4** hs = reinterpret_cast<const float4**>(h + b_info);
    for (int i = 0; i < n_stores; ++i) hs[i] = stores[i]->arena.get();
    hs[n_stores] = reinterpret_cast<const float4*>(d_prev);
    memcpy(h + b_info + b_src, segs.data(), ns * sizeof(MapSegment));
    memcpy(h + b_info + b_src + b_segs, tiles.data(), n_tiles * sizeof(Tile));
    int* hb = reinterpret_cast<int*>(h + b_info + b_src + b_segs + b_tiles);
    uintptr_t* ho = reinterpret_cast<uintptr_t*>(h + b_info + b_src + b_segs + b_tiles + b_bases);
    for (int i = 0; i < ns; ++i) {               // input position pos of segment i is the point (first - base) + pos of its source
        hb[i] = (int)segs[i].base;
        ho[i] = (uintptr_t)hs[segs[i].source] + (uintptr_t)((segs[i].first - segs[i].base) * (long long)sizeof(float4));
    }
    char* w = tables.as<char>();
    Info* d_info = reinterpret_cast<Info*>(w);
    const float4* const* d_src = reinterpret_cast<const float4* const*>(w + b_info);
    const MapSegment* d_segs = reinterpret_cast<const MapSegment*>(w + b_info + b_src);
    const Tile* d_tiles = reinterpret_cast<const Tile*>(w + b_info + b_src + b_segs);
    const int* d_bases = reinterpret_cast<const int*>(w + b_info + b_src + b_segs + b_tiles);
    const float4* const* d_origin = reinterpret_cast<const float4* const*>(w + b_info + b_src + b_segs + b_tiles + b_bases);

    // appends may still be in flight on the other stores' streams; d_prev and d_out belong to the caller's stream
    for (mrs_keyframes* u : uniq)
        if (u != kf) MRS_TRY(u->s.release_to(s));      // the other store's own ev_out
    MRS_TRY(kf->s.join_in((hipStream_t)stream));
    MRS_HIP_TRY(hipMemcpyAsync(w, h, b_tables, hipMemcpyHostToDevice, s));
    // development aid (MRS_DEV=1 MRS_MAP_TIMING=1, tools/bench_globalmap.py): events between the steps, one line on stderr per call
    mrs::StageMarks marks(mrs::dev_env("MRS_MAP_TIMING") != nullptr, s);
    marks.mark(0);
    hipLaunchKernelGGL(k_mc_bounds, dim3(std::min(n_tiles, kBoundsBlocks)), dim3(kThreads), 0, s, d_src, d_segs, d_tiles, n_tiles, inv, d_info);
    hipLaunchKernelGGL(k_mc_grid, dim3(1), dim3(64), 0, s, d_info);
    MRS_HIP_TRY(hipGetLastError());
    MRS_HIP_TRY(hipMemcpyAsync(h, d_info, sizeof(Info), hipMemcpyDeviceToHost, s));
    marks.mark(1);
    MRS_HIP_TRY(hipStreamSynchronize(s));                        // synchronisation 1 of 2: the key width decides how much is sorted
    const Info info = *hi;
    if (info.overflow) {
        mrs::set_error("the map's voxel grid needs keys of more than 63 bits (leaf %g): choose a larger leaf", (double)leaf);
        return MRS_ERR_ARG;
    }
    const int n_valid = (int)info.kept;
    if (n_valid == 0) { *out_points = 0; return MRS_OK; }
    const int end_bit = n_valid < n_in ? info.bits + 1 : info.bits;      // the dropped points carry bit `bits`

    // keys x 2 | values x 2 | carry table | sort / scan workspace.  The run heads and their prefix sum reuse the halves of the two
    // double buffers the sort left unused.
    const int n_mean_tiles = (n_valid + kTile - 1) / kTile;
    const size_t b_keys = round256((size_t)n_in * 8), b_vals = round256((size_t)n_in * 4), b_carry = round256((size_t)n_mean_tiles * sizeof(Carry));
    size_t b_sort = 0, b_scan = 0;
    {
        hipcub::DoubleBuffer<unsigned long long> nk(nullptr, nullptr);
        hipcub::DoubleBuffer<int> nv(nullptr, nullptr);
        int* ni = nullptr;
        MRS_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, b_sort, nk, nv, (int)n_in, 0, end_bit, s));
        MRS_HIP_TRY(hipcub::DeviceScan::InclusiveSum(nullptr, b_scan, ni, ni, n_valid, s));
    }
    const size_t b_tmp = round256(std::max(b_sort, b_scan));
    mrs::Scratch work;
    if ((st = work.alloc(2 * b_keys + 2 * b_vals + b_carry + b_tmp, s)) != MRS_OK) return st;
    w = work.as<char>();
    unsigned long long* d_keys0 = reinterpret_cast<unsigned long long*>(w); w += b_keys;
    unsigned long long* d_keys1 = reinterpret_cast<unsigned long long*>(w); w += b_keys;
    int* d_vals0 = reinterpret_cast<int*>(w); w += b_vals;
    int* d_vals1 = reinterpret_cast<int*>(w); w += b_vals;
    Carry* d_carry = reinterpret_cast<Carry*>(w); w += b_carry;
    void* d_tmp = w;

    marks.mark(2);
    hipLaunchKernelGGL(k_mc_keys, dim3(n_tiles), dim3(kThreads), 0, s, d_src, d_segs, d_tiles, d_info, inv, d_keys0, d_vals0);
    marks.mark(3);
    hipcub::DoubleBuffer<unsigned long long> keys(d_keys0, d_keys1);
    hipcub::DoubleBuffer<int> vals(d_vals0, d_vals1);
    MRS_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(d_tmp, b_sort, keys, vals, (int)n_in, 0, end_bit, s));
    marks.mark(4);
    const unsigned long long* d_sorted = keys.Current();
    const int* d_pos = vals.Current();
    int* d_head = vals.Alternate();
    int* d_rank = reinterpret_cast<int*>(keys.Alternate());
    const int blocks = (int)std::min<long long>(((long long)n_valid + kThreads - 1) / kThreads, 8192);
    hipLaunchKernelGGL(k_mc_heads, dim3(blocks), dim3(kThreads), 0, s, d_sorted, n_valid, d_head);
    MRS_HIP_TRY(hipcub::DeviceScan::InclusiveSum(d_tmp, b_scan, d_head, d_rank, n_valid, s));
    marks.mark(5);
    hipLaunchKernelGGL(k_mc_means, dim3(n_mean_tiles), dim3(kThreads), 0, s, d_bases, d_origin, d_segs, ns, d_sorted, d_pos, d_rank, n_valid,
                       reinterpret_cast<float4*>(d_out), d_carry);
    hipLaunchKernelGGL(k_mc_stitch, dim3((n_mean_tiles + kThreads - 1) / kThreads), dim3(kThreads), 0, s, d_carry, n_mean_tiles,
                       reinterpret_cast<float4*>(d_out));
    marks.mark(6);
    MRS_HIP_TRY(hipGetLastError());
    MRS_HIP_TRY(hipMemcpyAsync(h, d_rank + (n_valid - 1), sizeof(int), hipMemcpyDeviceToHost, s));
    MRS_HIP_TRY(hipStreamSynchronize(s));                        // synchronisation 2 of 2: the number of voxels
    if (marks)                                                   // events 1 and 2 bracket the first synchronisation: not a step
        fprintf(stderr, "[mrslam] map steps ms: bounds+grid %.4f keys %.4f sort %.4f heads+scan %.4f means+stitch %.4f points %lld bits %d\n",
                marks.ms(0), marks.ms(2), marks.ms(3), marks.ms(4), marks.ms(5), n_in, end_bit);
    *out_points = *reinterpret_cast<const int*>(h);
    return MRS_OK;
}

}  // extern "C"
