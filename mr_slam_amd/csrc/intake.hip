// intake.hip -- raw keyframe clouds filtered on the GPU and registered in the keyframe store (C ABI mrs_keyframes_ingest,
// mrs_keyframes_get_points).
//
// What it replaces: the front of GlobalManager::mapUpdate (Mapping/src/global_manager/src/global_manager.cpp:1684-1709, :1735, :1797):
// pcl::fromROSMsg, an exact pcl::VoxelGrid with leaf submap_voxel_leaf_size_, pcl::PassThrough on z, the intensity set to robotid * 30,
// keyframes.emplace_back -- on the host, on one thread, for every keyframe of every robot.  Here a call takes the messages' point blobs as
// they are (point_step and the byte offsets of x, y, z, intensity: what a sensor_msgs/PointCloud2 describes) and runs ONE chain of launches
// for all its clouds:
//   k_in_bounds : every point decoded from the strided blob (16-byte loads when point_step is 16, 4-byte loads otherwise), per-cloud minimum /
//                 maximum voxel cell and number of finite points (wave shuffles, LDS, one global atomic per workgroup and component);
//   k_in_grid   : per cloud, the minimum cell, the key multipliers, the 63-bit check, the key width -> host (synchronisation 1 of 2);
//   k_in_keys   : (cloud, 64-bit voxel key) packed into one word, the cloud above the widest grid's bits; a dropped point sorts after all;
//   device-wide stable radix sort of (word, input position) over the bits in use: one cloud of 10^5 points is spread over the whole device;
//   k_in_heads + running maximum: the first sorted position of the voxel every sorted position belongs to;
//   k_in_chunks : a voxel's points in sorted (= input) order are cut into chunks of 32; every chunk but a voxel's first is summed by a thread
//                 of its own, in float64, left to right;
//   k_in_means  : one voxel per thread: its first chunk summed left to right, the other chunks' sums added in order, one division, one
//                 rounding to float32, the z test on the float32 mean, the tag;
//   inclusive prefix sum of the verdicts, k_in_scatter: the survivors written, in order, straight to the arena's tail; k_in_counts: the
//                 survivors of every cloud -> host (synchronisation 2 of 2).
// The shape of a voxel's sum depends on its own points in input order alone, so a cloud's bits depend neither on the run nor on the clouds it
// shares a call with, and a voxel of N points costs one thread 32 + N / 32 dependent additions, not N.
// No floating-point atomics.
#include "submap_device.hpp"

#include <hipcub/hipcub.hpp>

#include <cmath>
#include <cstdlib>

namespace {

using namespace mrs::kfdev;

constexpr int kThreads = 256, kPerThread = 4, kTile = kThreads * kPerThread, kWaves = kThreads / 64;
constexpr int kChunk = 32;      // points of a voxel summed left to right before the chunks' sums are added; even

struct Layout {           // of one point in the blob, in 4-byte words
    int words;            // point_step / 4
    int x, y, z;
    int w;                // the intensity, or -1 for none
};

struct Tile {
    int cloud;
    int start;            // first point of the tile inside the cloud
};

struct CloudInfo {        // initial state from the host, results back to the host at the first synchronisation
    unsigned bounds[6];   // ordered bits of the minimum cell (initialised to 0xffffffff) and the maximum cell (0)
    unsigned kept;        // points with finite x, y, z
    int bits;             // valid keys are < 2^bits
    long long mn[3];
    long long mul_y, mul_z;
    int overflow;
    int pad;
};
struct Acc {              // float64 sums of a chunk
    double x, y, z, w;
};
static_assert(sizeof(CloudInfo) == 80 && sizeof(Acc) == 32, "DESIGN.md section 4.14 quotes these sizes");

__device__ __forceinline__ float pick(const float4 v, int k) { return k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w; }

// point i of the blob; kVec16: point_step is 16 and the blob is 16-byte aligned
template <bool kVec16>
__device__ __forceinline__ float4 decode(const float* __restrict__ raw, long long i, const Layout L)
{
    if (kVec16) {
        const float4 v = reinterpret_cast<const float4*>(raw)[i];
        return make_float4(pick(v, L.x), pick(v, L.y), pick(v, L.z), L.w >= 0 ? pick(v, L.w) : 0.0f);
    }
    const float* p = raw + i * L.words;
    return make_float4(p[L.x], p[L.y], p[L.z], L.w >= 0 ? p[L.w] : 0.0f);
}

// ---- pass 1: per-cloud cell bounds and kept points -------------------------------------------------------------------------------------------
// cloud_first [n_clouds + 1]: first point of every cloud in the blob.  One workgroup per tile; a tile lies inside one cloud.
template <bool kVec16>
__global__ __launch_bounds__(kThreads) void k_in_bounds(const float* __restrict__ raw, Layout L, const Tile* __restrict__ tiles,
                                                        const int* __restrict__ cloud_first, float inv, CloudInfo* __restrict__ info)
{
    __shared__ unsigned red[kWaves][7];
    const Tile t = tiles[blockIdx.x];
    const long long first = cloud_first[t.cloud];
    const int count = (int)(cloud_first[t.cloud + 1] - first);
    unsigned lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u}, kept = 0;
#pragma unroll
    for (int j = 0; j < kPerThread; ++j) {
        const int i = t.start + j * kThreads + threadIdx.x;
        if (i < count) {
            const float4 p = decode<kVec16>(raw, first + i, L);
            if (finite3(p.x, p.y, p.z)) {
                const unsigned c[3] = {order_bits(cell_of(p.x, inv)), order_bits(cell_of(p.y, inv)), order_bits(cell_of(p.z, inv))};
#pragma unroll
                for (int a = 0; a < 3; ++a) { lo[a] = min(lo[a], c[a]); hi[a] = max(hi[a], c[a]); }
                ++kept;
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
        CloudInfo* ci = info + t.cloud;
        if (a < 3) { if (v != 0xffffffffu) atomicMin(&ci->bounds[a], v); }
        else if (a < 6) { if (v != 0u) atomicMax(&ci->bounds[a], v); }
        else if (v != 0u) atomicAdd(&ci->kept, v);
    }
}

// ---- per cloud: minimum cell, key multipliers, 63-bit check, key width ---------------------------------------------------------------------------
__global__ void k_in_grid(CloudInfo* __restrict__ info, int n_clouds)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_clouds || info[c].kept == 0) return;
    CloudInfo ci = info[c];
    if (!grid_from_bounds(ci.bounds, ci.mn, ci.mul_y, ci.mul_z, ci.bits)) ci.overflow = 1;
    info[c] = ci;
}

// ---- pass 2: (cloud, voxel key) of every point -------------------------------------------------------------------------------------------------
// The cloud sits above bit `shift` (the width of the widest grid of the call); a dropped point belongs to "cloud" n_clouds, after all others.
template <bool kVec16>
__global__ __launch_bounds__(kThreads) void k_in_keys(const float* __restrict__ raw, Layout L, const Tile* __restrict__ tiles,
                                                      const int* __restrict__ cloud_first, const CloudInfo* __restrict__ info, int n_clouds,
                                                      int shift, float inv, unsigned long long* __restrict__ keys, int* __restrict__ vals)
{
    const Tile t = tiles[blockIdx.x];
    const long long first = cloud_first[t.cloud];
    const int count = (int)(cloud_first[t.cloud + 1] - first);
    const CloudInfo* ci = info + t.cloud;
    const long long mx = ci->mn[0], my = ci->mn[1], mz = ci->mn[2], mul_y = ci->mul_y, mul_z = ci->mul_z;
    const unsigned long long dropped = (unsigned long long)n_clouds << shift, high = (unsigned long long)t.cloud << shift;
#pragma unroll
    for (int j = 0; j < kPerThread; ++j) {
        const int i = t.start + j * kThreads + threadIdx.x;
        if (i < count) {
            const long long pos = first + i;
            const float4 p = decode<kVec16>(raw, pos, L);
            keys[pos] = finite3(p.x, p.y, p.z) ? (high | voxel_key(p.x, p.y, p.z, inv, mx, my, mz, mul_y, mul_z)) : dropped;
            vals[pos] = (int)pos;
        }
    }
}

// ---- run heads: start[p] = p at the first sorted position of a voxel, 0 elsewhere (its running maximum is the voxel's first position) --------
__global__ __launch_bounds__(kThreads) void k_in_heads(const unsigned long long* __restrict__ keys, int n_valid, int* __restrict__ start)
{
    for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < n_valid; p += (long long)gridDim.x * blockDim.x)
        start[p] = (p == 0 || keys[p - 1] != keys[p]) ? (int)p : 0;
}

// the sum of the points at the sorted positions [p, p + kChunk) that carry the key k, left to right; *end = the position after the last one
template <bool kVec16>
__device__ __forceinline__ Acc chunk_sum(const float* __restrict__ raw, const Layout L, const unsigned long long* __restrict__ keys,
                                         const int* __restrict__ vals, long long p, int n_valid, unsigned long long k, long long* end)
{
    Acc a = {0.0, 0.0, 0.0, 0.0};
    long long q = p;
    for (; q < p + kChunk && q < n_valid && keys[q] == k; ++q) {          // equal keys keep input order: the sum's order is the input's
        const float4 pt = decode<kVec16>(raw, vals[q], L);
        a.x += (double)pt.x; a.y += (double)pt.y; a.z += (double)pt.z; a.w += (double)pt.w;
    }
    *end = q;
    return a;
}

// ---- the chunks of the long voxels ----------------------------------------------------------------------------------------------------------------
// start[p] = first sorted position of p's voxel.  A chunk begins where p - start[p] is a multiple of kChunk.  A voxel's first chunk is left to
// k_in_means, and so is a chunk of ONE point (its sum is the point).  Every other chunk covers at least the sorted positions p and p + 1, so two
// such chunks begin at least two positions apart: slot p / 2 of `part` belongs to one chunk.
template <bool kVec16>
__global__ __launch_bounds__(kThreads) void k_in_chunks(const float* __restrict__ raw, Layout L, const unsigned long long* __restrict__ keys,
                                                        const int* __restrict__ vals, const int* __restrict__ start, int n_valid,
                                                        Acc* __restrict__ part)
{
    for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < n_valid; p += (long long)gridDim.x * blockDim.x) {
        const long long r = p - start[p];
        if (r == 0 || r % kChunk != 0) continue;
        const unsigned long long k = keys[p];
        if (p + 1 >= n_valid || keys[p + 1] != k) continue;
        long long end;
        part[p >> 1] = chunk_sum<kVec16>(raw, L, keys, vals, p, n_valid, k, &end);
    }
}

// ---- one voxel per thread: the chunks' float64 sums added in order, one rounding, the z test on the float32 mean, the tag ----------------------
// vox[p] and keep[p] are indexed by the SORTED position of the voxel's first point; keep[p] = 0 everywhere else.
template <bool kVec16>
__global__ __launch_bounds__(kThreads) void k_in_means(const float* __restrict__ raw, Layout L, const unsigned long long* __restrict__ keys,
                                                       const int* __restrict__ vals, const Acc* __restrict__ part, int n_valid, float z_lo,
                                                       float z_hi, int set_intensity, float intensity, float4* __restrict__ vox,
                                                       int* __restrict__ keep)
{
    for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < n_valid; p += (long long)gridDim.x * blockDim.x) {
        const unsigned long long k = keys[p];
        int verdict = 0;
        if (p == 0 || keys[p - 1] != k) {
            long long end;
            Acc a = chunk_sum<kVec16>(raw, L, keys, vals, p, n_valid, k, &end);
            for (long long q = p + kChunk; q < n_valid && keys[q] == k; q += kChunk) {
                if (q + 1 < n_valid && keys[q + 1] == k) {
                    const Acc c = part[q >> 1];
                    a.x += c.x; a.y += c.y; a.z += c.z; a.w += c.w;
                    end = q;                                     // where this chunk ends is found below, for the last one only
                } else {                                         // a chunk of one point
                    const float4 pt = decode<kVec16>(raw, vals[q], L);
                    a.x += (double)pt.x; a.y += (double)pt.y; a.z += (double)pt.z; a.w += (double)pt.w;
                    end = q + 1;
                }
            }
            const long long limit = end + kChunk;
            while (end < limit && end < n_valid && keys[end] == k) ++end;      // at most kChunk steps: `end` lies in the voxel's last chunk
            float4 mean = mean_of(a.x, a.y, a.z, a.w, (double)(end - p));
            verdict = (z_lo <= mean.z && mean.z <= z_hi) ? 1 : 0;
            if (set_intensity) mean.w = intensity;
            vox[p] = mean;
        }
        keep[p] = verdict;
    }
}

// ---- the survivors, in sorted order, to the arena's tail: rank = inclusive prefix sum of keep ---------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_in_scatter(const float4* __restrict__ vox, const int* __restrict__ keep, const int* __restrict__ rank,
                                                         int n_valid, float4* __restrict__ tail)
{
    for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < n_valid; p += (long long)gridDim.x * blockDim.x)
        if (keep[p]) tail[rank[p] - 1] = vox[p];
}

// out [n_clouds + 1] (int64): survivors before every cloud; sorted_first [n_clouds + 1]: first sorted position of every cloud
__global__ void k_in_counts(const int* __restrict__ rank, const int* __restrict__ sorted_first, int n_clouds, long long* __restrict__ out)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c > n_clouds) return;
    const int f = sorted_first[c];
    out[c] = f > 0 ? rank[f - 1] : 0;
}

int bit_width(unsigned v)
{
    int b = 0;
    while (v) { ++b; v >>= 1; }
    return b;
}

struct Filter {
    float leaf, z_lo, z_hi, intensity;
    int set_intensity;
};

// the whole call; lock held, device current, arguments checked
int ingest_locked(mrs_keyframes* kf, int n_clouds, const void* data, bool on_device, const int64_t* h_offsets, long long point_step, const Layout L,
                  const Filter f, const float* h_pose16s, int32_t* out_ids, int64_t* out_counts, hipStream_t user)
{
    const long long n_in = h_offsets[n_clouds], used = kf->offsets.back();
    const int first_id = (int)kf->offsets.size() - 1;
    std::vector<long long> survivors(n_clouds + 1, 0);           // before every cloud
    mrs::DeviceBuffer<float4> old_arena;                         // kept until the stream has been synchronised, when the arena grows
    hipStream_t s = kf->s;
    int st;
    if (n_in > 0) {
        std::vector<Tile> tiles;
        for (int c = 0; c < n_clouds; ++c)
            for (long long t = 0; t < h_offsets[c + 1] - h_offsets[c]; t += kTile) tiles.push_back(Tile{c, (int)t});
        const int n_tiles = (int)tiles.size();
        const float inv = 1.0f / f.leaf;
        const size_t bytes = (size_t)n_in * (size_t)point_step;

        // tables, built on the host, one copy: cloud infos (bounds in their initial state) | tiles | first point of every cloud | first sorted
        // position of every cloud (filled after the first synchronisation).  The pinned buffer holds them, then a host blob.
        const size_t b_info = round256((size_t)n_clouds * sizeof(CloudInfo)), b_tiles = round256(n_tiles * sizeof(Tile)),
                     b_first = round256((size_t)(n_clouds + 1) * sizeof(int)), b_counts = round256((size_t)(n_clouds + 1) * 8),
                     b_tables = b_info + b_tiles + 2 * b_first + b_counts;
        mrs::Scratch tables, blob;
        if ((st = tables.alloc(b_tables, s)) != MRS_OK) return st;
        if ((st = stage_reserve(kf, b_tables + (on_device ? 0 : bytes))) != MRS_OK) return st;
        char* h = kf->h_stage.get();
        memset(h, 0, b_tables);
        CloudInfo* h_info = reinterpret_cast<CloudInfo*>(h);
        for (int c = 0; c < n_clouds; ++c) h_info[c].bounds[0] = h_info[c].bounds[1] = h_info[c].bounds[2] = 0xffffffffu;
        memcpy(h + b_info, tiles.data(), n_tiles * sizeof(Tile));
        int* h_first = reinterpret_cast<int*>(h + b_info + b_tiles);
        int* h_sorted = reinterpret_cast<int*>(h + b_info + b_tiles + b_first);
        long long* h_counts = reinterpret_cast<long long*>(h + b_info + b_tiles + 2 * b_first);
        for (int c = 0; c <= n_clouds; ++c) h_first[c] = (int)h_offsets[c];
        char* w = tables.as<char>();
        CloudInfo* d_info = reinterpret_cast<CloudInfo*>(w);
        const Tile* d_tiles = reinterpret_cast<const Tile*>(w + b_info);
        const int* d_first = reinterpret_cast<const int*>(w + b_info + b_tiles);
        int* d_sorted = reinterpret_cast<int*>(w + b_info + b_tiles + b_first);
        long long* d_counts = reinterpret_cast<long long*>(w + b_info + b_tiles + 2 * b_first);

        // development aid (MRS_DEV=1 MRS_INTAKE_TIMING=1, tools/bench_intake.py): events between the steps, one line on stderr per call
        mrs::StageMarks marks(mrs::dev_env("MRS_INTAKE_TIMING") != nullptr, s);

        const float* raw = static_cast<const float*>(data);
        marks.mark(0);
        if (on_device) {
            MRS_TRY(kf->s.join_in(user));
        } else {
            if ((st = blob.alloc(bytes, s)) != MRS_OK) return st;
            memcpy(h + b_tables, data, bytes);
            MRS_HIP_TRY(hipMemcpyAsync(blob.p, h + b_tables, bytes, hipMemcpyHostToDevice, s));
            raw = blob.as<float>();
        }
        MRS_HIP_TRY(hipMemcpyAsync(w, h, b_tables, hipMemcpyHostToDevice, s));
        const bool vec16 = point_step == 16 && ((uintptr_t)raw & 15) == 0;      // chosen from the arguments
        marks.mark(1);
        if (vec16) hipLaunchKernelGGL(k_in_bounds<true>, dim3(n_tiles), dim3(kThreads), 0, s, raw, L, d_tiles, d_first, inv, d_info);
        else hipLaunchKernelGGL(k_in_bounds<false>, dim3(n_tiles), dim3(kThreads), 0, s, raw, L, d_tiles, d_first, inv, d_info);
        hipLaunchKernelGGL(k_in_grid, dim3((n_clouds + 63) / 64), dim3(64), 0, s, d_info, n_clouds);
        MRS_HIP_TRY(hipGetLastError());
        MRS_HIP_TRY(hipMemcpyAsync(h, d_info, (size_t)n_clouds * sizeof(CloudInfo), hipMemcpyDeviceToHost, s));
        marks.mark(2);
        MRS_HIP_TRY(hipStreamSynchronize(s));                    // synchronisation 1 of 2: the key widths decide how much is sorted
        long long n_valid = 0;
        int shift = 0;
        for (int c = 0; c < n_clouds; ++c) {
            if (h_info[c].overflow) {
                mrs::set_error("the voxel grid of cloud %d needs keys of more than 63 bits (leaf %g): choose a larger leaf", c, (double)f.leaf);
                return MRS_ERR_ARG;
            }
            h_sorted[c] = (int)n_valid;                          // the sort groups the kept points by cloud, in input order of the clouds
            n_valid += h_info[c].kept;
            if (h_info[c].kept) shift = std::max(shift, h_info[c].bits);
        }
        h_sorted[n_clouds] = (int)n_valid;
        // the packed word: `shift` bits of key, then the cloud (and the value n_clouds when something was dropped)
        const int end_bit = shift + bit_width(n_valid < n_in ? (unsigned)n_clouds : (unsigned)(n_clouds - 1));
        if (end_bit > 64) {
            mrs::set_error("bad argument: the clouds of one call are sorted as (cloud, key) in 64 bits, and this call needs %d: split it", end_bit);
            return MRS_ERR_ARG;
        }
        if (n_valid > 0) {
            if ((st = arena_reserve(kf, used + n_valid, &old_arena)) != MRS_OK) return st;      // at most one survivor per kept point
            float4* tail = kf->arena.get() + used;
            const size_t b_keys = round256((size_t)n_in * 8), b_vals = round256((size_t)n_in * 4), b_vox = round256((size_t)n_valid * sizeof(float4)),
                         b_part = round256(((size_t)n_valid / 2 + 1) * sizeof(Acc));
            size_t b_sort = 0, b_scan = 0, b_max = 0;
            {
                hipcub::DoubleBuffer<unsigned long long> nk(nullptr, nullptr);
                hipcub::DoubleBuffer<int> nv(nullptr, nullptr);
                int* ni = nullptr;
                MRS_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, b_sort, nk, nv, (int)n_in, 0, end_bit, s));
                MRS_HIP_TRY(hipcub::DeviceScan::InclusiveSum(nullptr, b_scan, ni, ni, (int)n_valid, s));
                MRS_HIP_TRY(hipcub::DeviceScan::InclusiveScan(nullptr, b_max, ni, ni, hipcub::Max(), (int)n_valid, s));
            }
            const size_t b_tmp = round256(std::max(b_sort, std::max(b_scan, b_max)));
            // keys x 2 | values x 2 | voxels | chunk sums | sort / scan workspace.  The run heads, the runs' first positions, the verdicts and
            // their prefix sum live in the halves of the two double buffers the sort left unused.
            mrs::Scratch work;
            if ((st = work.alloc(2 * b_keys + 2 * b_vals + b_vox + b_part + b_tmp, s)) != MRS_OK) return st;
            char* q = work.as<char>();
            unsigned long long* d_keys0 = reinterpret_cast<unsigned long long*>(q); q += b_keys;
            unsigned long long* d_keys1 = reinterpret_cast<unsigned long long*>(q); q += b_keys;
            int* d_vals0 = reinterpret_cast<int*>(q); q += b_vals;
            int* d_vals1 = reinterpret_cast<int*>(q); q += b_vals;
            float4* d_vox = reinterpret_cast<float4*>(q); q += b_vox;
            Acc* d_part = reinterpret_cast<Acc*>(q); q += b_part;
            void* d_tmp = q;

            MRS_HIP_TRY(hipMemcpyAsync(d_sorted, h_sorted, (size_t)(n_clouds + 1) * sizeof(int), hipMemcpyHostToDevice, s));
            marks.mark(3);
            if (vec16) hipLaunchKernelGGL(k_in_keys<true>, dim3(n_tiles), dim3(kThreads), 0, s, raw, L, d_tiles, d_first, d_info, n_clouds, shift, inv, d_keys0, d_vals0);
            else hipLaunchKernelGGL(k_in_keys<false>, dim3(n_tiles), dim3(kThreads), 0, s, raw, L, d_tiles, d_first, d_info, n_clouds, shift, inv, d_keys0, d_vals0);
            marks.mark(4);
            hipcub::DoubleBuffer<unsigned long long> keys(d_keys0, d_keys1);
            hipcub::DoubleBuffer<int> vals(d_vals0, d_vals1);
            MRS_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(d_tmp, b_sort, keys, vals, (int)n_in, 0, end_bit, s));
            marks.mark(5);
            const unsigned long long* d_sorted_keys = keys.Current();
            const int* d_pos = vals.Current();
            int* d_keep = vals.Alternate();                       // first the run heads, then the verdicts
            int* d_rank = reinterpret_cast<int*>(keys.Alternate());
            int* d_start = d_rank + n_valid;                     // the unused key buffer holds 2 n_in ints
            const int blocks = (int)std::min<long long>((n_valid + kThreads - 1) / kThreads, 8192);
            hipLaunchKernelGGL(k_in_heads, dim3(blocks), dim3(kThreads), 0, s, d_sorted_keys, (int)n_valid, d_keep);
            MRS_HIP_TRY(hipcub::DeviceScan::InclusiveScan(d_tmp, b_max, d_keep, d_start, hipcub::Max(), (int)n_valid, s));
            if (vec16) {
                hipLaunchKernelGGL(k_in_chunks<true>, dim3(blocks), dim3(kThreads), 0, s, raw, L, d_sorted_keys, d_pos, d_start, (int)n_valid, d_part);
                hipLaunchKernelGGL(k_in_means<true>, dim3(blocks), dim3(kThreads), 0, s, raw, L, d_sorted_keys, d_pos, d_part, (int)n_valid, f.z_lo, f.z_hi,
                                   f.set_intensity, f.intensity, d_vox, d_keep);
            } else {
                hipLaunchKernelGGL(k_in_chunks<false>, dim3(blocks), dim3(kThreads), 0, s, raw, L, d_sorted_keys, d_pos, d_start, (int)n_valid, d_part);
                hipLaunchKernelGGL(k_in_means<false>, dim3(blocks), dim3(kThreads), 0, s, raw, L, d_sorted_keys, d_pos, d_part, (int)n_valid, f.z_lo, f.z_hi,
                                   f.set_intensity, f.intensity, d_vox, d_keep);
            }
            marks.mark(6);
            MRS_HIP_TRY(hipcub::DeviceScan::InclusiveSum(d_tmp, b_scan, d_keep, d_rank, (int)n_valid, s));
            hipLaunchKernelGGL(k_in_scatter, dim3(blocks), dim3(kThreads), 0, s, d_vox, d_keep, d_rank, (int)n_valid, tail);
            hipLaunchKernelGGL(k_in_counts, dim3((n_clouds + 1 + 63) / 64), dim3(64), 0, s, d_rank, d_sorted, n_clouds, d_counts);
            marks.mark(7);
            MRS_HIP_TRY(hipGetLastError());
            MRS_HIP_TRY(hipMemcpyAsync(h_counts, d_counts, (size_t)(n_clouds + 1) * 8, hipMemcpyDeviceToHost, s));
            MRS_HIP_TRY(hipStreamSynchronize(s));                // synchronisation 2 of 2: the survivors of every cloud
            for (int c = 0; c <= n_clouds; ++c) survivors[c] = h_counts[c];
            if (marks)                                           // events 2 and 3 bracket the first synchronisation: not a step
                fprintf(stderr, "[mrslam] intake steps ms: upload %.4f bounds+grid %.4f keys %.4f sort %.4f means %.4f scan+scatter %.4f points %lld bits %d\n",
                        marks.ms(0), marks.ms(1), marks.ms(3), marks.ms(4), marks.ms(5), marks.ms(6), n_in, end_bit);
        }
    }
    // the store changes only here, after everything that can fail
    for (int c = 0; c < n_clouds; ++c) {
        out_ids[c] = first_id + c;
        out_counts[c] = survivors[c + 1] - survivors[c];
        kf->offsets.push_back(used + survivors[c + 1]);
    }
    kf->poses.insert(kf->poses.end(), h_pose16s, h_pose16s + 16 * (size_t)n_clouds);
    return MRS_OK;
}

}  // namespace

extern "C" {

int mrs_keyframes_ingest(mrs_keyframes* kf, int32_t n_clouds, const void* data, int32_t on_device, const int64_t* h_offsets, int32_t point_step,
                         int32_t off_x, int32_t off_y, int32_t off_z, int32_t off_intensity, float leaf, float z_lo, float z_hi,
                         int32_t set_intensity, float intensity, const float* h_pose16s, int32_t* out_ids, int64_t* out_counts, mrs_stream stream)
{
    MRS_REQUIRE(kf && h_offsets, "null pointer");
    MRS_REQUIRE(n_clouds >= 0 && n_clouds < (1 << 24), "the number of clouds must be 0 .. 2^24 - 1");
    MRS_REQUIRE(n_clouds == 0 || (h_pose16s && out_ids && out_counts), "null pointer");
    MRS_REQUIRE(point_step >= 12 && point_step % 4 == 0, "point_step must be a multiple of 4 and at least 12");
    const int32_t offs[3] = {off_x, off_y, off_z};
    for (int32_t o : offs) MRS_REQUIRE(o >= 0 && o % 4 == 0 && o <= point_step - 4, "a field offset is negative, not a multiple of 4 or beyond point_step - 4");
    MRS_REQUIRE(off_x < off_y && off_y < off_z, "the offsets of x, y, z must ascend");
    MRS_REQUIRE(off_intensity == -1 || (off_intensity >= 0 && off_intensity % 4 == 0 && off_intensity <= point_step - 4),
                "the intensity offset must be -1 (none) or a multiple of 4 in [0, point_step - 4]");
    MRS_REQUIRE(std::isfinite(leaf) && leaf > 0.0f, "the leaf size must be positive and finite");
    MRS_REQUIRE(!std::isnan(z_lo) && !std::isnan(z_hi) && z_lo <= z_hi, "the z limits must not be NaN, and z_lo <= z_hi");
    MRS_REQUIRE(set_intensity == 0 || set_intensity == 1, "set_intensity must be 0 or 1");
    MRS_REQUIRE(!set_intensity || std::isfinite(intensity), "the intensity to set is not finite");
    MRS_REQUIRE(h_offsets[0] == 0, "h_offsets[0] must be 0");
    for (int c = 0; c < n_clouds; ++c) {
        MRS_REQUIRE(h_offsets[c + 1] >= h_offsets[c], "h_offsets must ascend");
        MRS_REQUIRE(h_offsets[c + 1] <= 0x7fffffffll, "more than 2^31 - 1 points in one call: split it");
        MRS_REQUIRE(rigid_finite(h_pose16s + 16 * (size_t)c), "a pose is not finite");
    }
    MRS_REQUIRE(data || h_offsets[n_clouds] == 0, "null pointer");
    MRS_REQUIRE(!on_device || ((uintptr_t)data & 3) == 0, "a device blob must be 4-byte aligned");
    MRS_HIP_TRY(hipSetDevice(kf->ctx->device));
    std::lock_guard<std::mutex> lk(kf->mu);
    const Layout L = {point_step / 4, off_x / 4, off_y / 4, off_z / 4, off_intensity < 0 ? -1 : off_intensity / 4};
    const Filter f = {leaf, z_lo, z_hi, intensity, set_intensity};
    return ingest_locked(kf, n_clouds, data, on_device != 0, h_offsets, point_step, L, f, h_pose16s, out_ids, out_counts, (hipStream_t)stream);
}

int mrs_keyframes_get_points(mrs_keyframes* kf, int32_t id, float* out, int32_t on_device, int64_t capacity_points, int64_t* out_points,
                             mrs_stream stream)
{
    MRS_REQUIRE(kf && out_points, "null pointer");
    MRS_HIP_TRY(hipSetDevice(kf->ctx->device));
    std::lock_guard<std::mutex> lk(kf->mu);
    MRS_REQUIRE(id >= 0 && id < (int)kf->offsets.size() - 1, "keyframe id out of range");
    const long long first = kf->offsets[id], n = kf->offsets[id + 1] - first;
    MRS_REQUIRE(capacity_points >= n, "capacity below the keyframe's point count");
    MRS_REQUIRE(out || n == 0, "null pointer");
    if (n > 0) {
        const size_t bytes = (size_t)n * sizeof(float4);
        if (on_device) {          // `out` may still be in use on the caller's stream, which then waits for the copy
            MRS_TRY(kf->s.join_in((hipStream_t)stream));
            MRS_HIP_TRY(hipMemcpyAsync(out, kf->arena.get() + first, bytes, hipMemcpyDeviceToDevice, kf->s));
            MRS_TRY(kf->s.release_to((hipStream_t)stream));
        } else {
            MRS_HIP_TRY(hipMemcpyAsync(out, kf->arena.get() + first, bytes, hipMemcpyDeviceToHost, kf->s));
            MRS_HIP_TRY(hipStreamSynchronize(kf->s));
        }
    }
    *out_points = n;
    return MRS_OK;
}

}  // extern "C"
