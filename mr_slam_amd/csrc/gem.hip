// gem.hip -- the globally consistent elevation map (C ABI mrs_gem_*).
//
// What it replaces: the submap stack of the elevation node (ElevationMapping::updateLocalMap, ElevationMapping.cpp:653-815), its correction
// after every pose-graph optimisation (updateGlobalMap, :821-962, which rebuilds two std::unordered_map per submap pair on one host thread),
// the elevation branch of GlobalManager::composeGlobalMap (global_manager.cpp:2133-2152) and PointMapLayer::updateBounds
// (pointMap_layer.cpp:100-135).  Here:
//   store   : every closed submap lives in one arena of ten 32-bit columns (gem_cell.hpp: x y z var r g b frontier intensity travers) with a
//             host offset table; the open submap is a second column set that only grows until it is closed;
//   close   : a stable radix sort of (x bits, y bits) with the insertion number as value.  A run's first value is the cell's first
//             insertion, its last value the last writer; a flag at the first insertion, a prefix sum and one gather give the records in
//             ascending order of first insertion;
//   update  : k_gem_move applies T = opt * pose^-1 to every record of the moved submaps in one launch.  The neighbour lists come from the
//             centres on the host (at most MRS_GEM_MAX_SUBMAPS of them).  ONE chain canonicalises everything that takes part: a range pass
//             (so that the sort sees the fewest bits), keys (submap, kx, ky), hipcub::DeviceRadixSort over those bits, heads, a prefix sum and
//             one gather into the second arena, which also snaps x, y and leaves each record's packed key beside it.  Submaps that take no
//             part ride along under the key (submap, position) and come out as they went in;
//   fuse    : k_gem_fuse, one launch per centre submap: a thread per cell of the centre walks the neighbour list in order, binary-searches
//             the neighbour's sorted keys and writes the fused record to both.  Keys are unique on both sides, so no two threads of a launch
//             touch one record; successive launches are ordered by the stream.  No atomics but the matched-cell counter (an integer sum);
//   products: compose / get_submap export columns to records; compose_robots moves every robot's submaps and local map into one cloud and
//             optionally folds equal cells left to right (sort, heads, a thread per run); the costmap scatters (input index, cost) with a
//             64-bit atomicMax per grid cell (a maximum does not depend on the order of arrival) and a second pass resolves it.
// Every call is blocking and works on the legacy default stream.  Nothing here depends on run-to-run order.
#include "common.hpp"
#include "gem_cell.hpp"

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <climits>
#include <cmath>

namespace {

namespace G = mrs::gem;
using u32 = uint32_t;
using u64 = unsigned long long;
constexpr int kThreads = 256;
constexpr int kF = G::kFields;
constexpr long long kMaxRecords = (1ll << 31) - 1024;      // hipcub counts items in int

struct Cols {                                              // ten columns of `stride` words each
    u32* p;
    size_t stride;
    __host__ __device__ u32* col(int c) const { return p + (size_t)c * stride; }
};

inline int blocks_for(long long n) { return (int)std::max<long long>(1, (n + kThreads - 1) / kThreads); }
inline size_t round256(size_t b) { return (b + 255) & ~(size_t)255; }
inline int bit_width(u64 v)
{
    int b = 0;
    while (v) { ++b; v >>= 1; }
    return b;
}

// ---- records in and out -------------------------------------------------------------------------------------------------------------

// records [n][10] -> columns at first + (pos ? pos[t] : t); with `flag`, only the flagged ones
__global__ __launch_bounds__(kThreads) void k_gem_import(const u32* __restrict__ aos, long long n, const int* __restrict__ flag,
                                                         const int* __restrict__ pos, Cols dst, long long first)
{
    const long long t = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (t >= n || (flag && !flag[t])) return;
    const long long d = first + (pos ? pos[t] : t);
#pragma unroll
    for (int c = 0; c < kF; ++c) dst.col(c)[d] = aos[t * kF + c];
}

__global__ __launch_bounds__(kThreads) void k_gem_export(Cols src, long long first, long long n, u32* __restrict__ aos)
{
    const long long t = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (t >= n) return;
#pragma unroll
    for (int c = 0; c < kF; ++c) aos[t * kF + c] = src.col(c)[first + t];
}

__global__ __launch_bounds__(kThreads) void k_gem_leaving(const u32* __restrict__ aos, long long n, float cx, float cy, float dx, float dy, float half,
                                                          int* __restrict__ flag)
{
    const long long t = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (t >= n) return;
    const u32* r = aos + t * kF;
    flag[t] = G::leaves_window(__uint_as_float(r[G::kX]), __uint_as_float(r[G::kY]), __uint_as_float(r[G::kZ]), cx, cy, dx, dy, half) ? 1 : 0;
}

// ---- closing the open submap -----------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kThreads) void k_gem_open_keys(Cols open, int n, u64* __restrict__ keys, int* __restrict__ vals)
{
    const int t = blockIdx.x * kThreads + threadIdx.x;
    if (t >= n) return;
    keys[t] = ((u64)open.col(G::kX)[t] << 32) | (u64)open.col(G::kY)[t];
    vals[t] = t;
}

// head[p] = p at the first position of a run of equal keys, else 0 (an inclusive maximum turns it into every position's run start)
__global__ __launch_bounds__(kThreads) void k_gem_run_heads(const u64* __restrict__ keys, int n, int* __restrict__ head)
{
    const int p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= n) return;
    head[p] = (p > 0 && keys[p] != keys[p - 1]) ? p : 0;
}

// at a run's last position: the cell's first insertion f gets the flag (unless the last writer's elevation is -10) and the last writer
__global__ __launch_bounds__(kThreads) void k_gem_open_runs(const u64* __restrict__ keys, const int* __restrict__ vals, const int* __restrict__ start,
                                                            int n, Cols open, int* __restrict__ flag, int* __restrict__ src)
{
    const int p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= n) return;
    if (p + 1 < n && keys[p + 1] == keys[p]) return;
    const int f = vals[start[p]], l = vals[p];
    flag[f] = __uint_as_float(open.col(G::kZ)[l]) != G::kNoElevation ? 1 : 0;
    src[f] = l;
}

__global__ __launch_bounds__(kThreads) void k_gem_close_gather(Cols open, int n, const int* __restrict__ flag, const int* __restrict__ pos,
                                                               const int* __restrict__ src, Cols dst, long long first)
{
    const int t = blockIdx.x * kThreads + threadIdx.x;
    if (t >= n || !flag[t]) return;
    const long long d = first + pos[t];
    const int s = src[t];
#pragma unroll
    for (int c = 0; c < kF; ++c) dst.col(c)[d] = open.col(c)[s];
}

// ---- update_global -----------------------------------------------------------------------------------------------------------------------

// the submap of record t: the last s with off[s] <= t (empty submaps share an offset with their successor and are skipped)
__device__ __forceinline__ int submap_of(const long long* __restrict__ off, int nsub, long long t)
{
    int lo = 0, hi = nsub;                                 // off[lo] <= t < off[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= t) lo = mid;
        else hi = mid;
    }
    return lo;
}

// records [first, first + n) of the arena: x y z <- T[submap] (x y z); T is [nsub][16]
__global__ __launch_bounds__(kThreads) void k_gem_move(Cols a, long long first, long long n, const long long* __restrict__ off, int nsub,
                                                       const float* __restrict__ T)
{
    const long long t = first + (long long)blockIdx.x * kThreads + threadIdx.x;
    if (t >= first + n) return;
    const float* m = T + (size_t)submap_of(off, nsub, t) * 16;
    float x, y, z;
    G::move_point(m, __uint_as_float(a.col(G::kX)[t]), __uint_as_float(a.col(G::kY)[t]), __uint_as_float(a.col(G::kZ)[t]), &x, &y, &z);
    a.col(G::kX)[t] = __float_as_uint(x);
    a.col(G::kY)[t] = __float_as_uint(y);
    a.col(G::kZ)[t] = __float_as_uint(z);
}

__device__ __forceinline__ int wave_min(int v)
{
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ int wave_max(int v)
{
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}

// range[0..3] = min kx, max kx, min ky, max ky over the keyed records of the submaps that take part (integer minima and maxima: order-free)
__global__ __launch_bounds__(kThreads) void k_gem_key_range(Cols a, long long n, const long long* __restrict__ off, int nsub,
                                                            const unsigned char* __restrict__ part, double res, int* __restrict__ range)
{
    int x0 = INT_MAX, x1 = INT_MIN, y0 = INT_MAX, y1 = INT_MIN;
    for (long long t = (long long)blockIdx.x * kThreads + threadIdx.x; t < n; t += (long long)gridDim.x * kThreads) {
        if (!part[submap_of(off, nsub, t)]) continue;
        int32_t kx, ky;
        if (G::cell_key(__uint_as_float(a.col(G::kX)[t]), res, &kx) && G::cell_key(__uint_as_float(a.col(G::kY)[t]), res, &ky)) {
            x0 = min(x0, kx); x1 = max(x1, kx); y0 = min(y0, ky); y1 = max(y1, ky);
        }
    }
    x0 = wave_min(x0); x1 = wave_max(x1); y0 = wave_min(y0); y1 = wave_max(y1);
    if ((threadIdx.x & 63) == 0 && x0 <= x1) {
        atomicMin(&range[0], x0); atomicMax(&range[1], x1); atomicMin(&range[2], y0); atomicMax(&range[3], y1);
    }
}

// key = submap << low_bits | low.  Taking part: low = (kx - kx0 + 1) << y_bits | (ky - ky0), or 0 without a key; else low = position in the submap
__global__ __launch_bounds__(kThreads) void k_gem_keys(Cols a, long long n, const long long* __restrict__ off, int nsub,
                                                       const unsigned char* __restrict__ part, double res, int kx0, int ky0, int y_bits, int low_bits,
                                                       u64* __restrict__ keys, int* __restrict__ vals)
{
    const long long t = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (t >= n) return;
    const int s = submap_of(off, nsub, t);
    u64 low;
    if (part[s]) {
        int32_t kx, ky;
        const bool ok = G::cell_key(__uint_as_float(a.col(G::kX)[t]), res, &kx) && G::cell_key(__uint_as_float(a.col(G::kY)[t]), res, &ky);
        low = ok ? (((u64)(kx - kx0 + 1) << y_bits) | (u64)(ky - ky0)) : 0ull;
    } else {
        low = (u64)(t - off[s]);
    }
    keys[t] = ((u64)s << low_bits) | low;
    vals[t] = (int)t;
}

// keep[p] for sorted position p: taking part: the first record of its key, keyed, elevation != -10; else always.  Counts the unkeyed.
__global__ __launch_bounds__(kThreads) void k_gem_keep(const u64* __restrict__ keys, const int* __restrict__ vals, long long n, Cols a,
                                                       const unsigned char* __restrict__ part, int y_bits, int low_bits, int* __restrict__ keep,
                                                       u64* __restrict__ dropped)
{
    const long long p = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (p >= n) return;
    const u64 k = keys[p];
    int v = 1;
    if (part[(int)(k >> low_bits)]) {
        const bool keyed = ((k & ((1ull << low_bits) - 1)) >> y_bits) != 0;
        if (!keyed) atomicAdd(dropped, 1ull);
        v = keyed && (p == 0 || keys[p - 1] != k) && __uint_as_float(a.col(G::kZ)[vals[p]]) != G::kNoElevation;
    }
    keep[p] = v;
}

// new_off[s] = survivors before the first record of submap s (the sort keeps every record inside its submap's old range)
__global__ void k_gem_offsets(const long long* __restrict__ off, int nsub, long long n, const int* __restrict__ pos, const int* __restrict__ keep,
                              long long* __restrict__ new_off)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s > nsub) return;
    const long long o = off[s];
    new_off[s] = o < n ? (long long)pos[o] : (long long)pos[n - 1] + keep[n - 1];
}

// survivors to their place in the other arena; a submap that takes part gets snapped x, y and its packed key beside the record
__global__ __launch_bounds__(kThreads) void k_gem_canon_gather(const u64* __restrict__ keys, const int* __restrict__ vals, const int* __restrict__ keep,
                                                               const int* __restrict__ pos, long long n, Cols a, const unsigned char* __restrict__ part,
                                                               int low_bits, double res, Cols b, u64* __restrict__ ckey)
{
    const long long p = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (p >= n || !keep[p]) return;
    const int src = vals[p], dst = pos[p];
    u32 r[kF];
#pragma unroll
    for (int c = 0; c < kF; ++c) r[c] = a.col(c)[src];
    u64 ck = 0;
    if (part[(int)(keys[p] >> low_bits)]) {
        int32_t kx = 0, ky = 0;
        (void)G::cell_key(__uint_as_float(r[G::kX]), res, &kx);       // kept records of such a submap are keyed
        (void)G::cell_key(__uint_as_float(r[G::kY]), res, &ky);
        r[G::kX] = __float_as_uint(G::cell_centre(kx, res));
        r[G::kY] = __float_as_uint(G::cell_centre(ky, res));
        ck = G::pack_key(kx, ky);
    }
#pragma unroll
    for (int c = 0; c < kF; ++c) b.col(c)[dst] = r[c];
    ckey[dst] = ck;
}

// position of `key` in the ascending ckey[lo, hi), or -1
__device__ __forceinline__ long long find_key(const u64* __restrict__ ckey, long long lo, long long hi, u64 key)
{
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        const u64 k = ckey[mid];
        if (k == key) return mid;
        if (k < key) lo = mid + 1;
        else hi = mid;
    }
    return -1;
}

// fuse_pair(new = list[q], old = centre) for q = 1 .. n_list - 1 in order; a thread per cell of the centre
__global__ __launch_bounds__(kThreads) void k_gem_fuse(Cols a, const u64* __restrict__ ckey, const long long* __restrict__ off, const int* __restrict__ list,
                                                       int n_list, int rule, u64* __restrict__ matched)
{
    const int i = list[0];
    const long long cnt = off[i + 1] - off[i], t = (long long)blockIdx.x * kThreads + threadIdx.x;
    int m = 0;
    if (t < cnt) {
        const long long me = off[i] + t;
        const u64 key = ckey[me];
        float z = __uint_as_float(a.col(G::kZ)[me]), var = __uint_as_float(a.col(G::kVar)[me]);
        u32 frontier = a.col(G::kFrontier)[me], rest[5] = {0, 0, 0, 0, 0};
        constexpr int kRest[5] = {G::kR, G::kG, G::kB, G::kIntensity, G::kTravers};
        for (int q = 1; q < n_list; ++q) {
            if (!G::fusable(var)) break;                      // the gate is on this cell's running variance, which no longer changes
            const int j = list[q];
            const long long b = find_key(ckey, off[j], off[j + 1], key);
            if (b < 0) continue;
            G::fuse_zvar(rule, z, var, __uint_as_float(a.col(G::kZ)[b]), __uint_as_float(a.col(G::kVar)[b]), &z, &var);
            frontier = (frontier != 0 && a.col(G::kFrontier)[b] != 0) ? 1u : 0u;
#pragma unroll
            for (int c = 0; c < 5; ++c) rest[c] = a.col(kRest[c])[b];
            a.col(G::kZ)[b] = __float_as_uint(z);
            a.col(G::kVar)[b] = __float_as_uint(var);
            a.col(G::kFrontier)[b] = frontier;
            ++m;
        }
        if (m) {
            a.col(G::kZ)[me] = __float_as_uint(z);
            a.col(G::kVar)[me] = __float_as_uint(var);
            a.col(G::kFrontier)[me] = frontier;
#pragma unroll
            for (int c = 0; c < 5; ++c) a.col(kRest[c])[me] = rest[c];
        }
    }
    for (int o = 32; o > 0; o >>= 1) m += __shfl_xor(m, o);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(matched, (u64)m);
}

// ---- products ------------------------------------------------------------------------------------------------------------------------------

// the n records of a store from `first`, moved by T[submap], as records at out
__global__ __launch_bounds__(kThreads) void k_gem_export_moved(Cols src, long long n, const long long* __restrict__ off, int nsub,
                                                               const float* __restrict__ T, u32* __restrict__ out)
{
    const long long t = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (t >= n) return;
    u32 r[kF];
#pragma unroll
    for (int c = 0; c < kF; ++c) r[c] = src.col(c)[t];
    float x, y, z;
    G::move_point(T + (size_t)submap_of(off, nsub, t) * 16, __uint_as_float(r[G::kX]), __uint_as_float(r[G::kY]), __uint_as_float(r[G::kZ]), &x, &y, &z);
    r[G::kX] = __float_as_uint(x); r[G::kY] = __float_as_uint(y); r[G::kZ] = __float_as_uint(z);
#pragma unroll
    for (int c = 0; c < kF; ++c) out[t * kF + c] = r[c];
}

// records in -> records out, record t moved by T[group of t] (groups by the offsets)
__global__ __launch_bounds__(kThreads) void k_gem_move_records(const u32* __restrict__ in, long long n, const long long* __restrict__ off, int ngroups,
                                                               const float* __restrict__ T, u32* __restrict__ out)
{
    const long long t = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (t >= n) return;
    u32 r[kF];
#pragma unroll
    for (int c = 0; c < kF; ++c) r[c] = in[t * kF + c];
    float x, y, z;
    G::move_point(T + (size_t)submap_of(off, ngroups, t) * 16, __uint_as_float(r[G::kX]), __uint_as_float(r[G::kY]), __uint_as_float(r[G::kZ]), &x, &y, &z);
    r[G::kX] = __float_as_uint(x); r[G::kY] = __float_as_uint(y); r[G::kZ] = __float_as_uint(z);
#pragma unroll
    for (int c = 0; c < kF; ++c) out[t * kF + c] = r[c];
}

__global__ __launch_bounds__(kThreads) void k_gem_record_keys(const u32* __restrict__ rec, long long n, double res, u64* __restrict__ keys, int* __restrict__ vals)
{
    const long long t = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (t >= n) return;
    int32_t kx, ky;
    const bool ok = G::cell_key(__uint_as_float(rec[t * kF + G::kX]), res, &kx) && G::cell_key(__uint_as_float(rec[t * kF + G::kY]), res, &ky);
    keys[t] = ok ? G::pack_key(kx, ky) : 0ull;
    vals[t] = (int)t;
}

__global__ __launch_bounds__(kThreads) void k_gem_merge_heads(const u64* __restrict__ keys, long long n, int* __restrict__ keep, u64* __restrict__ dropped)
{
    const long long p = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (p >= n) return;
    const u64 k = keys[p];
    if (k == 0) atomicAdd(dropped, 1ull);
    keep[p] = k != 0 && (p == 0 || keys[p - 1] != k);
}

// a thread per run of equal keys: the left-to-right fold of its records (old = the running record, new = the next one)
__global__ __launch_bounds__(kThreads) void k_gem_merge_fold(const u64* __restrict__ keys, const int* __restrict__ vals, const int* __restrict__ keep,
                                                             const int* __restrict__ pos, long long n, const u32* __restrict__ rec, int rule, double res,
                                                             u32* __restrict__ out)
{
    const long long p = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (p >= n || !keep[p]) return;
    const u64 k = keys[p];
    u32 r[kF];
#pragma unroll
    for (int c = 0; c < kF; ++c) r[c] = rec[(long long)vals[p] * kF + c];
    for (long long q = p + 1; q < n && keys[q] == k; ++q) {
        const float var = __uint_as_float(r[G::kVar]);
        if (!G::fusable(var)) break;                          // the gate is on the running record, which no longer changes
        const u32* w = rec + (long long)vals[q] * kF;
        float z, v;
        G::fuse_zvar(rule, __uint_as_float(r[G::kZ]), var, __uint_as_float(w[G::kZ]), __uint_as_float(w[G::kVar]), &z, &v);
        r[G::kZ] = __float_as_uint(z);
        r[G::kVar] = __float_as_uint(v);
        r[G::kFrontier] = (r[G::kFrontier] != 0 && w[G::kFrontier] != 0) ? 1u : 0u;
        r[G::kR] = w[G::kR]; r[G::kG] = w[G::kG]; r[G::kB] = w[G::kB]; r[G::kIntensity] = w[G::kIntensity]; r[G::kTravers] = w[G::kTravers];
    }
    const int32_t kx = (int32_t)(k >> 24) - G::kKeyBound, ky = (int32_t)(k & 0xffffffull) - G::kKeyBound;
    r[G::kX] = __float_as_uint(G::cell_centre(kx, res));
    r[G::kY] = __float_as_uint(G::cell_centre(ky, res));
    const long long d = pos[p];
#pragma unroll
    for (int c = 0; c < kF; ++c) out[d * kF + c] = r[c];
}

// grid word = (input index + 1) << 8 | cost; the largest input index wins whatever the order of arrival
__global__ __launch_bounds__(kThreads) void k_gem_cost_scatter(const u32* __restrict__ rec, long long n, double ox, double oy, double res, int sx, int sy,
                                                               int thresh_type, double thresh, u64* __restrict__ grid)
{
    const long long t = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (t >= n) return;
    const u32* r = rec + t * kF;
    int mx, my;
    if (!G::world_to_map(__uint_as_float(r[G::kX]), __uint_as_float(r[G::kY]), ox, oy, res, sx, sy, &mx, &my)) return;
    const u64 w = ((u64)(t + 1) << 8) | (u64)G::cell_cost(__uint_as_float(r[G::kZ]), __uint_as_float(r[G::kTravers]), thresh_type, thresh);
    atomicMax(&grid[(size_t)my * sx + mx], w);
}

__global__ __launch_bounds__(kThreads) void k_gem_cost_resolve(const u64* __restrict__ grid, long long cells, unsigned char* __restrict__ out)
{
    const long long c = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (c >= cells) return;
    const u64 w = grid[c];
    out[c] = w ? (unsigned char)(w & 0xffull) : G::kCostUnknown;
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------------

struct ColumnSet {                                          // owner of ten columns; grows by copy
    mrs::DeviceBuffer<u32> buf;
    size_t stride = 0;
    Cols cols() const { return Cols{buf.get(), stride}; }
    // room for `need` records per column, keeping the first `used`
    int ensure(size_t need, size_t used)
    {
        if (need <= stride) return MRS_OK;
        const size_t cap = std::max(need, stride + stride / 2 + 1024);
        mrs::DeviceBuffer<u32> nb;
        int st = nb.reserve(cap * kF, cap * kF);
        if (st != MRS_OK) return st;
        if (used) MRS_HIP_TRY(hipMemcpy2D(nb.get(), cap * sizeof(u32), buf.get(), stride * sizeof(u32), used * sizeof(u32), kF, hipMemcpyDeviceToDevice));
        buf = std::move(nb);
        stride = cap;
        return MRS_OK;
    }
};

// sort workspace of n items: keys x 2 | values x 2 | two int arrays | hipcub's temporary storage
struct SortSpace {
    mrs::Scratch mem;
    u64 *k0 = nullptr, *k1 = nullptr;
    int *v0 = nullptr, *v1 = nullptr, *a = nullptr, *b = nullptr;
    void* tmp = nullptr;
    size_t tmp_bytes = 0;
    int alloc(long long n)
    {
        size_t b_sort = 0, b_scan = 0, b_max = 0;
        {
            hipcub::DoubleBuffer<u64> nk(nullptr, nullptr);
            hipcub::DoubleBuffer<int> nv(nullptr, nullptr);
            int* ni = nullptr;
            MRS_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, b_sort, nk, nv, (int)n, 0, 64, (hipStream_t) nullptr));
            MRS_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, b_scan, ni, ni, (int)n, (hipStream_t) nullptr));
            MRS_HIP_TRY(hipcub::DeviceScan::InclusiveScan(nullptr, b_max, ni, ni, hipcub::Max(), (int)n, (hipStream_t) nullptr));
        }
        tmp_bytes = round256(std::max(b_sort, std::max(b_scan, b_max)));
        const size_t bk = round256((size_t)n * 8), bv = round256((size_t)n * 4);
        int st = mem.alloc(2 * bk + 4 * bv + tmp_bytes, nullptr);
        if (st != MRS_OK) return st;
        char* q = mem.as<char>();
        k0 = reinterpret_cast<u64*>(q); q += bk;
        k1 = reinterpret_cast<u64*>(q); q += bk;
        v0 = reinterpret_cast<int*>(q); q += bv;
        v1 = reinterpret_cast<int*>(q); q += bv;
        a = reinterpret_cast<int*>(q); q += bv;
        b = reinterpret_cast<int*>(q); q += bv;
        tmp = q;
        return MRS_OK;
    }
    // stable sort of (k0, v0) over bits [0, end_bit); the sorted arrays are returned in *keys / *vals
    int sort(long long n, int end_bit, const u64** keys, const int** vals)
    {
        hipcub::DoubleBuffer<u64> dk(k0, k1);
        hipcub::DoubleBuffer<int> dv(v0, v1);
        size_t bytes = tmp_bytes;
        MRS_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(tmp, bytes, dk, dv, (int)n, 0, end_bit, (hipStream_t) nullptr));
        *keys = dk.Current();
        *vals = dv.Current();
        return MRS_OK;
    }
    int exclusive_sum(const int* in, int* out, long long n)
    {
        size_t bytes = tmp_bytes;
        MRS_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(tmp, bytes, in, out, (int)n, (hipStream_t) nullptr));
        return MRS_OK;
    }
    int inclusive_max(const int* in, int* out, long long n)
    {
        size_t bytes = tmp_bytes;
        MRS_HIP_TRY(hipcub::DeviceScan::InclusiveScan(tmp, bytes, in, out, hipcub::Max(), (int)n, (hipStream_t) nullptr));
        return MRS_OK;
    }
};

// exclusive-sum total: pos[n - 1] + flag[n - 1]
int last_total(const int* d_pos, const int* d_flag, long long n, long long* total)
{
    int h[2] = {0, 0};
    MRS_HIP_TRY(hipMemcpy(&h[0], d_pos + (n - 1), sizeof(int), hipMemcpyDeviceToHost));
    MRS_HIP_TRY(hipMemcpy(&h[1], d_flag + (n - 1), sizeof(int), hipMemcpyDeviceToHost));
    *total = (long long)h[0] + h[1];
    return MRS_OK;
}

// the caller's records on the device: d_cells as they are, h_cells through a scratch upload
int records_on_device(const void* h_cells, const void* d_cells, long long n, mrs::Scratch* up, const u32** out)
{
    if (d_cells) {
        *out = static_cast<const u32*>(d_cells);
        return MRS_OK;
    }
    int st = up->alloc((size_t)n * kF * sizeof(u32), nullptr);
    if (st != MRS_OK) return st;
    MRS_HIP_TRY(hipMemcpy(up->p, h_cells, (size_t)n * kF * sizeof(u32), hipMemcpyHostToDevice));
    *out = up->as<u32>();
    return MRS_OK;
}

// n records at d_rec (device) to the caller's h_out or d_out
int records_out(const u32* d_rec, long long n, void* h_out, void* d_out)
{
    if (n == 0) return MRS_OK;
    if (d_out) MRS_HIP_TRY(hipMemcpy(d_out, d_rec, (size_t)n * kF * sizeof(u32), hipMemcpyDeviceToDevice));
    else MRS_HIP_TRY(hipMemcpy(h_out, d_rec, (size_t)n * kF * sizeof(u32), hipMemcpyDeviceToHost));
    return MRS_OK;
}

}  // namespace

struct mrs_gem {
    mrs_ctx* ctx = nullptr;
    double resolution = 0.2;
    int rule = MRS_GEM_WEIGHTED;
    float radius = 15.0f;
    int min_neighbours = 3;
    ColumnSet arena, spare, open;                           // closed submaps | the other half of update_global's gather | the open submap
    mrs::DeviceBuffer<u64> ckey;                            // packed key per arena record; valid during update_global only
    mrs::DeviceBuffer<u64> counters;                        // dropped, matched
    std::vector<long long> off{0};                          // [submaps + 1]
    std::vector<float> pose, centre;                        // [submaps][16], [submaps][2]
    long long open_n = 0;
    long long dropped = 0, matched = 0;                     // of the last update_global
    int submaps() const { return (int)off.size() - 1; }
};

namespace {

int gem_append(mrs_gem* g, const void* h_cells, const void* d_cells, long long n, const float* window)
{
    MRS_REQUIRE(g, "null pointer");
    MRS_REQUIRE(n >= 0, "n must not be negative");
    if (n == 0) return MRS_OK;
    MRS_REQUIRE((h_cells != nullptr) != (d_cells != nullptr), "pass the cells either as h_cells or as d_cells");
    MRS_REQUIRE(g->open_n + n <= kMaxRecords, "the open submap holds fewer than 2^31 records");
    MRS_HIP_TRY(hipSetDevice(g->ctx->device));
    mrs::Scratch up;
    const u32* rec = nullptr;
    int st = records_on_device(h_cells, d_cells, n, &up, &rec);
    if (st != MRS_OK) return st;
    if ((st = g->open.ensure((size_t)(g->open_n + n), (size_t)g->open_n)) != MRS_OK) return st;
    long long added = n;
    if (window) {
        SortSpace w;                                          // used for its two int arrays and the scan's temporary storage
        if ((st = w.alloc(n)) != MRS_OK) return st;
        hipLaunchKernelGGL(k_gem_leaving, dim3(blocks_for(n)), dim3(kThreads), 0, nullptr, rec, n, window[0], window[1], window[2], window[3], window[4], w.a);
        if ((st = w.exclusive_sum(w.a, w.b, n)) != MRS_OK) return st;
        hipLaunchKernelGGL(k_gem_import, dim3(blocks_for(n)), dim3(kThreads), 0, nullptr, rec, n, w.a, w.b, g->open.cols(), g->open_n);
        MRS_HIP_TRY(hipGetLastError());
        if ((st = last_total(w.b, w.a, n, &added)) != MRS_OK) return st;
    } else {
        hipLaunchKernelGGL(k_gem_import, dim3(blocks_for(n)), dim3(kThreads), 0, nullptr, rec, n, (const int*)nullptr, (const int*)nullptr, g->open.cols(),
                           g->open_n);
        MRS_HIP_TRY(hipGetLastError());
    }
    MRS_HIP_TRY(hipStreamSynchronize(nullptr));
    g->open_n += added;
    return MRS_OK;
}

// `n` records of the arena from `first` to the caller
int gem_export(mrs_gem* g, long long first, long long n, void* h_cells, void* d_cells)
{
    if (n == 0) return MRS_OK;
    if (d_cells) {
        hipLaunchKernelGGL(k_gem_export, dim3(blocks_for(n)), dim3(kThreads), 0, nullptr, g->arena.cols(), first, n, static_cast<u32*>(d_cells));
        MRS_HIP_TRY(hipGetLastError());
        MRS_HIP_TRY(hipStreamSynchronize(nullptr));
        return MRS_OK;
    }
    mrs::Scratch out;
    int st = out.alloc((size_t)n * kF * sizeof(u32), nullptr);
    if (st != MRS_OK) return st;
    hipLaunchKernelGGL(k_gem_export, dim3(blocks_for(n)), dim3(kThreads), 0, nullptr, g->arena.cols(), first, n, out.as<u32>());
    MRS_HIP_TRY(hipGetLastError());
    MRS_HIP_TRY(hipMemcpy(h_cells, out.p, (size_t)n * kF * sizeof(u32), hipMemcpyDeviceToHost));
    return MRS_OK;
}

bool finite16(const float* m)
{
    for (int i = 0; i < 16; ++i)
        if (!std::isfinite(m[i])) return false;
    return true;
}

}  // namespace

extern "C" {

int mrs_gem_create(mrs_ctx* ctx, double resolution, int32_t rule, float radius, int32_t min_neighbours, mrs_gem** out)
{
    MRS_REQUIRE(ctx && out, "null pointer");
    MRS_REQUIRE(std::isfinite(resolution) && resolution > 0.0, "the resolution must be positive and finite");
    MRS_REQUIRE(rule == MRS_GEM_WEIGHTED || rule == MRS_GEM_AS_WRITTEN, "rule is MRS_GEM_WEIGHTED or MRS_GEM_AS_WRITTEN");
    MRS_REQUIRE(std::isfinite(radius) && radius >= 0.0f, "the radius must be finite and not negative");
    MRS_REQUIRE(min_neighbours >= 2, "min_neighbours counts the centre submap itself: at least 2");
    MRS_HIP_TRY(hipSetDevice(ctx->device));
    mrs_gem* g = new mrs_gem();
    g->ctx = ctx;
    g->resolution = resolution;
    g->rule = rule;
    g->radius = radius;
    g->min_neighbours = min_neighbours;
    const int st = g->counters.reserve(2, 2);
    if (st != MRS_OK) {
        delete g;
        return st;
    }
    *out = g;
    return MRS_OK;
}

int mrs_gem_destroy(mrs_gem* gem)
{
    if (!gem) return MRS_OK;
    (void)hipSetDevice(gem->ctx->device);
    (void)hipStreamSynchronize(nullptr);
    delete gem;
    return MRS_OK;
}

int mrs_gem_append_cells(mrs_gem* gem, const void* h_cells, const void* d_cells, int64_t n) { return gem_append(gem, h_cells, d_cells, n, nullptr); }

int mrs_gem_append_leaving(mrs_gem* gem, const void* h_cells, const void* d_cells, int64_t n, const float* h_current2, const float* h_shift2, int32_t length,
                           float resolution)
{
    MRS_REQUIRE(h_current2 && h_shift2, "null pointer");
    const float window[5] = {h_current2[0], h_current2[1], h_shift2[0], h_shift2[1], (float)length * resolution / 2};
    return gem_append(gem, h_cells, d_cells, n, window);
}

int mrs_gem_close_submap(mrs_gem* gem, const float* h_pose16, const float* h_centre2)
{
    MRS_REQUIRE(gem && h_pose16 && h_centre2, "null pointer");
    MRS_REQUIRE(finite16(h_pose16) && std::isfinite(h_centre2[0]) && std::isfinite(h_centre2[1]), "the pose and the centre must be finite");
    if (gem->submaps() >= MRS_GEM_MAX_SUBMAPS) {
        mrs::set_error("a store holds at most %d submaps", MRS_GEM_MAX_SUBMAPS);
        return MRS_ERR_UNSUPPORTED;
    }
    MRS_HIP_TRY(hipSetDevice(gem->ctx->device));
    const long long n = gem->open_n, used = gem->off.back();
    long long kept = 0;
    if (n > 0) {
        SortSpace w;
        int st = w.alloc(n);
        if (st != MRS_OK) return st;
        const Cols open = gem->open.cols();
        const u64* keys = nullptr;
        const int* vals = nullptr;
        hipLaunchKernelGGL(k_gem_open_keys, dim3(blocks_for(n)), dim3(kThreads), 0, nullptr, open, (int)n, w.k0, w.v0);
        if ((st = w.sort(n, 64, &keys, &vals)) != MRS_OK) return st;
        int* other = vals == w.v0 ? w.v1 : w.v0;             // the value buffer the sort left free: run starts, then the last writers
        hipLaunchKernelGGL(k_gem_run_heads, dim3(blocks_for(n)), dim3(kThreads), 0, nullptr, keys, (int)n, w.a);
        if ((st = w.inclusive_max(w.a, other, n)) != MRS_OK) return st;
        MRS_HIP_TRY(hipMemsetAsync(w.a, 0, (size_t)n * sizeof(int), nullptr));
        // w.b receives the last writers; the run starts are read from `other` in the same kernel, so they need an array of their own
        hipLaunchKernelGGL(k_gem_open_runs, dim3(blocks_for(n)), dim3(kThreads), 0, nullptr, keys, vals, other, (int)n, open, w.a, w.b);
        if ((st = w.exclusive_sum(w.a, other, n)) != MRS_OK) return st;
        MRS_HIP_TRY(hipGetLastError());
        if ((st = last_total(other, w.a, n, &kept)) != MRS_OK) return st;
        MRS_REQUIRE(used + kept <= kMaxRecords, "a store holds fewer than 2^31 records");
        if ((st = gem->arena.ensure((size_t)(used + kept), (size_t)used)) != MRS_OK) return st;
        hipLaunchKernelGGL(k_gem_close_gather, dim3(blocks_for(n)), dim3(kThreads), 0, nullptr, open, (int)n, w.a, other, w.b, gem->arena.cols(), used);
        MRS_HIP_TRY(hipGetLastError());
        MRS_HIP_TRY(hipStreamSynchronize(nullptr));
    }
    gem->off.push_back(used + kept);
    gem->pose.insert(gem->pose.end(), h_pose16, h_pose16 + 16);
    gem->centre.insert(gem->centre.end(), h_centre2, h_centre2 + 2);
    gem->open_n = 0;
    return MRS_OK;
}

int mrs_gem_count(mrs_gem* gem, int32_t* h_submaps, int64_t* h_cells, int64_t* h_open)
{
    MRS_REQUIRE(gem, "null pointer");
    if (h_submaps) *h_submaps = gem->submaps();
    if (h_cells) *h_cells = gem->off.back();
    if (h_open) *h_open = gem->open_n;
    return MRS_OK;
}

int mrs_gem_get_submap(mrs_gem* gem, int32_t index, void* h_cells, void* d_cells, int64_t capacity, int64_t* h_n, float* h_pose16, float* h_centre2)
{
    MRS_REQUIRE(gem && h_n, "null pointer");
    MRS_REQUIRE(index >= 0 && index < gem->submaps(), "no such submap");
    MRS_REQUIRE(!(h_cells && d_cells), "pass one of h_cells and d_cells, or neither for the size alone");
    const long long first = gem->off[index], n = gem->off[index + 1] - first;
    *h_n = n;
    if (h_pose16) std::copy(gem->pose.begin() + (size_t)index * 16, gem->pose.begin() + (size_t)index * 16 + 16, h_pose16);
    if (h_centre2) std::copy(gem->centre.begin() + (size_t)index * 2, gem->centre.begin() + (size_t)index * 2 + 2, h_centre2);
    if (!h_cells && !d_cells) return MRS_OK;
    MRS_REQUIRE(capacity >= n, "the output holds fewer records than the submap");
    MRS_HIP_TRY(hipSetDevice(gem->ctx->device));
    return gem_export(gem, first, n, h_cells, d_cells);
}

int mrs_gem_compose(mrs_gem* gem, void* h_cells, void* d_cells, int64_t capacity, int64_t* h_n)
{
    MRS_REQUIRE(gem && h_n, "null pointer");
    MRS_REQUIRE(!(h_cells && d_cells), "pass one of h_cells and d_cells, or neither for the size alone");
    const long long n = gem->off.back();
    *h_n = n;
    if (!h_cells && !d_cells) return MRS_OK;
    MRS_REQUIRE(capacity >= n, "the output holds fewer records than the store");
    MRS_HIP_TRY(hipSetDevice(gem->ctx->device));
    return gem_export(gem, 0, n, h_cells, d_cells);
}

int mrs_gem_stats(mrs_gem* gem, int64_t* h_dropped, int64_t* h_matched)
{
    MRS_REQUIRE(gem, "null pointer");
    if (h_dropped) *h_dropped = gem->dropped;
    if (h_matched) *h_matched = gem->matched;
    return MRS_OK;
}

int mrs_gem_update_global(mrs_gem* gem, const float* h_opt_poses, int32_t n_poses)
{
    MRS_REQUIRE(gem, "null pointer");
    MRS_REQUIRE(n_poses >= 0, "n_poses must not be negative");
    MRS_REQUIRE(h_opt_poses || n_poses == 0, "null pointer");
    const int nsub = gem->submaps(), K = std::min<int>(n_poses, nsub);
    gem->dropped = gem->matched = 0;
    if (K == 0) return MRS_OK;
    for (int i = 0; i < K; ++i) MRS_REQUIRE(finite16(h_opt_poses + (size_t)i * 16), "the poses must be finite");
    MRS_HIP_TRY(hipSetDevice(gem->ctx->device));
    const long long N = gem->off.back();
    const float r2 = gem->radius * gem->radius;
    // development aid (MRS_DEV=1 MRS_GEM_TIMING=1, tools/bench_gem.py): events between the steps, one line on stderr per call
    mrs::StageMarks marks(mrs::dev_env("MRS_GEM_TIMING") != nullptr, nullptr);

    // neighbour lists from the centres, in float32: (distance^2, index) ascending, the centre submap itself first
    std::vector<int> list, list_off(1, 0);
    std::vector<unsigned char> part((size_t)nsub, 0);
    std::vector<std::pair<float, int>> near;
    for (int i = 0; i < K; ++i) {
        near.clear();
        for (int j = 0; j < K; ++j) {
            if (j == i) continue;
            const float dx = gem->centre[(size_t)j * 2] - gem->centre[(size_t)i * 2], dy = gem->centre[(size_t)j * 2 + 1] - gem->centre[(size_t)i * 2 + 1];
            const float d2 = dx * dx + dy * dy;
            if (d2 <= r2) near.emplace_back(d2, j);
        }
        if ((int)near.size() + 1 < gem->min_neighbours) continue;
        std::sort(near.begin(), near.end());
        list.push_back(i);
        part[i] = 1;
        for (const auto& e : near) {
            list.push_back(e.second);
            part[e.second] = 1;
        }
        list_off.push_back((int)list.size());
    }

    // one upload: offsets | corrections | lists | who takes part
    std::vector<float> T((size_t)K * 16, 0.0f);
    for (int i = 1; i < K; ++i) mrs::gem::correction(h_opt_poses + (size_t)i * 16, gem->pose.data() + (size_t)i * 16, T.data() + (size_t)i * 16);
    const size_t b_off = round256((size_t)(nsub + 1) * 8), b_T = round256(T.size() * 4), b_list = round256(list.size() * 4 + 4), b_part = round256((size_t)nsub);
    mrs::Scratch tab;
    int st = tab.alloc(2 * b_off + b_T + b_list + b_part + 256, nullptr);
    if (st != MRS_OK) return st;
    char* q = tab.as<char>();
    long long* d_off = reinterpret_cast<long long*>(q); q += b_off;
    long long* d_new_off = reinterpret_cast<long long*>(q); q += b_off;
    float* d_T = reinterpret_cast<float*>(q); q += b_T;
    int* d_list = reinterpret_cast<int*>(q); q += b_list;
    unsigned char* d_part = reinterpret_cast<unsigned char*>(q); q += b_part;
    int* d_range = reinterpret_cast<int*>(q);
    // everything else the call allocates, before any record or pose changes: a failed allocation leaves the store as it was
    SortSpace w;
    if (!list.empty() && N > 0) {
        if ((st = w.alloc(N)) != MRS_OK) return st;
        if ((st = gem->spare.ensure(gem->arena.stride, 0)) != MRS_OK) return st;
        if ((st = gem->ckey.reserve((size_t)N, gem->arena.stride)) != MRS_OK) return st;
    }
    MRS_HIP_TRY(hipMemcpy(d_off, gem->off.data(), (size_t)(nsub + 1) * 8, hipMemcpyHostToDevice));
    MRS_HIP_TRY(hipMemcpy(d_T, T.data(), T.size() * 4, hipMemcpyHostToDevice));
    if (!list.empty()) MRS_HIP_TRY(hipMemcpy(d_list, list.data(), list.size() * 4, hipMemcpyHostToDevice));
    MRS_HIP_TRY(hipMemcpy(d_part, part.data(), (size_t)nsub, hipMemcpyHostToDevice));
    MRS_HIP_TRY(hipMemsetAsync(gem->counters.get(), 0, 2 * sizeof(u64), nullptr));

    // (a) move submaps 1 .. K - 1
    marks.mark(0);
    const long long first = gem->off[std::min(1, K)], moved = gem->off[K] - first;
    if (moved > 0) hipLaunchKernelGGL(k_gem_move, dim3(blocks_for(moved)), dim3(kThreads), 0, nullptr, gem->arena.cols(), first, moved, d_off, nsub, d_T);
    MRS_HIP_TRY(hipGetLastError());
    for (int i = 1; i < K; ++i) std::copy(h_opt_poses + (size_t)i * 16, h_opt_poses + (size_t)i * 16 + 16, gem->pose.begin() + (size_t)i * 16);
    if (list.empty() || N == 0) {
        MRS_HIP_TRY(hipStreamSynchronize(nullptr));
        return MRS_OK;
    }

    // (c) canonical form of every submap that takes part, in one chain
    marks.mark(1);
    const int h_init[4] = {INT_MAX, INT_MIN, INT_MAX, INT_MIN};
    int h_range[4];
    MRS_HIP_TRY(hipMemcpy(d_range, h_init, sizeof(h_init), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_gem_key_range, dim3(std::min(blocks_for(N), 2048)), dim3(kThreads), 0, nullptr, gem->arena.cols(), N, d_off, nsub, d_part,
                       gem->resolution, d_range);
    MRS_HIP_TRY(hipGetLastError());
    MRS_HIP_TRY(hipMemcpy(h_range, d_range, sizeof(h_range), hipMemcpyDeviceToHost));
    if (h_range[0] > h_range[1]) h_range[0] = h_range[1] = h_range[2] = h_range[3] = 0;            // no keyed record at all
    long long longest_raw = 1;
    for (int s = 0; s < nsub; ++s)
        if (!part[s]) longest_raw = std::max(longest_raw, gem->off[s + 1] - gem->off[s]);
    const int y_bits = bit_width((u64)((long long)h_range[3] - h_range[2])), x_bits = bit_width((u64)((long long)h_range[1] - h_range[0] + 1));
    const int low_bits = std::max(std::max(x_bits + y_bits, bit_width((u64)(longest_raw - 1))), 1), end_bit = low_bits + bit_width((u64)(nsub - 1));
    marks.mark(2);
    const u64* keys = nullptr;
    const int* vals = nullptr;
    hipLaunchKernelGGL(k_gem_keys, dim3(blocks_for(N)), dim3(kThreads), 0, nullptr, gem->arena.cols(), N, d_off, nsub, d_part, gem->resolution, h_range[0],
                       h_range[2], y_bits, low_bits, w.k0, w.v0);
    marks.mark(3);
    if ((st = w.sort(N, end_bit, &keys, &vals)) != MRS_OK) return st;
    marks.mark(4);
    hipLaunchKernelGGL(k_gem_keep, dim3(blocks_for(N)), dim3(kThreads), 0, nullptr, keys, vals, N, gem->arena.cols(), d_part, y_bits, low_bits, w.a,
                       gem->counters.get());
    if ((st = w.exclusive_sum(w.a, w.b, N)) != MRS_OK) return st;
    hipLaunchKernelGGL(k_gem_offsets, dim3((nsub + 1 + 63) / 64), dim3(64), 0, nullptr, d_off, nsub, N, w.b, w.a, d_new_off);
    hipLaunchKernelGGL(k_gem_canon_gather, dim3(blocks_for(N)), dim3(kThreads), 0, nullptr, keys, vals, w.a, w.b, N, gem->arena.cols(), d_part, low_bits,
                       gem->resolution, gem->spare.cols(), gem->ckey.get());
    MRS_HIP_TRY(hipGetLastError());
    std::vector<long long> new_off((size_t)nsub + 1);
    MRS_HIP_TRY(hipMemcpy(new_off.data(), d_new_off, new_off.size() * 8, hipMemcpyDeviceToHost));
    std::swap(gem->arena, gem->spare);
    gem->off = new_off;
    marks.mark(5);

    // (b) one launch per centre submap with enough neighbours, in index order
    for (size_t c = 0; c + 1 < list_off.size(); ++c) {
        const int i = list[list_off[c]];
        const long long cnt = new_off[i + 1] - new_off[i];
        if (cnt == 0) continue;
        hipLaunchKernelGGL(k_gem_fuse, dim3(blocks_for(cnt)), dim3(kThreads), 0, nullptr, gem->arena.cols(), gem->ckey.get(), d_new_off, d_list + list_off[c],
                           list_off[c + 1] - list_off[c], gem->rule, gem->counters.get() + 1);
    }
    MRS_HIP_TRY(hipGetLastError());
    marks.mark(6);
    u64 h_counters[2] = {0, 0};
    MRS_HIP_TRY(hipMemcpy(h_counters, gem->counters.get(), sizeof(h_counters), hipMemcpyDeviceToHost));
    gem->dropped = (long long)h_counters[0];
    gem->matched = (long long)h_counters[1];
    if (marks)
        fprintf(stderr, "[mrslam] gem update steps ms: move %.4f range %.4f keys %.4f sort %.4f heads+gather %.4f fuse %.4f records %lld bits %d launches %zu\n",
                marks.ms(0), marks.ms(1), marks.ms(2), marks.ms(3), marks.ms(4), marks.ms(5), N, end_bit, list_off.size() - 1);
    return MRS_OK;
}

int mrs_gem_compose_robots(mrs_ctx* ctx, mrs_gem* const* stores, int32_t n_robots, const float* h_poses, const void* h_local_cells,
                           const void* d_local_cells, const int64_t* h_local_offsets, const float* h_refs, int32_t merge_cells, int32_t rule,
                           double resolution, void* h_cells, void* d_cells, int64_t capacity, int64_t* h_n, int64_t* h_dropped)
{
    MRS_REQUIRE(ctx && stores && h_n, "null pointer");
    MRS_REQUIRE(n_robots >= 1, "at least one robot");
    MRS_REQUIRE(!(h_cells && d_cells), "pass one of h_cells and d_cells, or neither for the size bound alone");
    MRS_REQUIRE(rule == MRS_GEM_WEIGHTED || rule == MRS_GEM_AS_WRITTEN, "rule is MRS_GEM_WEIGHTED or MRS_GEM_AS_WRITTEN");
    MRS_REQUIRE(!merge_cells || (std::isfinite(resolution) && resolution > 0.0), "the resolution must be positive and finite");
    long long total = 0, n_sub = 0;
    for (int r = 0; r < n_robots; ++r) {
        MRS_REQUIRE(stores[r] && stores[r]->ctx == ctx, "every store belongs to this context");
        total += stores[r]->off.back();
        n_sub += stores[r]->submaps();
    }
    MRS_REQUIRE(h_poses || n_sub == 0, "null pointer");
    const long long n_local = h_local_offsets ? h_local_offsets[n_robots] : 0;
    if (h_local_offsets) {
        MRS_REQUIRE(h_local_offsets[0] == 0, "the local-map offsets start at 0");
        for (int r = 0; r < n_robots; ++r) MRS_REQUIRE(h_local_offsets[r] <= h_local_offsets[r + 1], "the local-map offsets must not decrease");
        MRS_REQUIRE(n_local == 0 || (((h_local_cells != nullptr) != (d_local_cells != nullptr)) && h_refs),
                    "pass the local maps either as h_local_cells or as d_local_cells, with h_refs");
    }
    const long long M = total + n_local;
    MRS_REQUIRE(M <= kMaxRecords, "one composition holds fewer than 2^31 records");
    *h_n = M;
    if (h_dropped) *h_dropped = 0;
    if (!h_cells && !d_cells) return MRS_OK;                  // M bounds the result with and without merge_cells
    MRS_REQUIRE(capacity >= M, "the output holds fewer records than the composition may have");
    if (M == 0) return MRS_OK;
    MRS_HIP_TRY(hipSetDevice(ctx->device));

    // the concatenation as records: robots' submaps in (robot, submap) order, then the local maps.  One upload carries every table:
    // each robot's submap offsets | the local maps' offsets | the submap poses | the reference poses
    mrs::Scratch cat, tab, up;
    int st = MRS_OK;
    u32* d_cat = static_cast<u32*>(d_cells);                  // without merge_cells the concatenation is the result
    if (!d_cat || merge_cells) {
        if ((st = cat.alloc((size_t)M * kF * sizeof(u32), nullptr)) != MRS_OK) return st;
        d_cat = cat.as<u32>();
    }
    std::vector<long long> offs;
    std::vector<size_t> off_at((size_t)n_robots);
    for (int r = 0; r < n_robots; ++r) {
        off_at[r] = offs.size();
        offs.insert(offs.end(), stores[r]->off.begin(), stores[r]->off.end());
    }
    const size_t local_at = offs.size();
    if (n_local > 0) offs.insert(offs.end(), h_local_offsets, h_local_offsets + n_robots + 1);
    const size_t b_offs = round256(offs.size() * 8), n_T = (size_t)n_sub * 16 + (n_local > 0 ? (size_t)n_robots * 16 : 0);
    std::vector<char> h_tab(b_offs + n_T * 4 + 16, 0);
    memcpy(h_tab.data(), offs.data(), offs.size() * 8);
    if (n_sub > 0) memcpy(h_tab.data() + b_offs, h_poses, (size_t)n_sub * 64);
    if (n_local > 0) memcpy(h_tab.data() + b_offs + (size_t)n_sub * 64, h_refs, (size_t)n_robots * 64);
    if ((st = tab.alloc(h_tab.size(), nullptr)) != MRS_OK) return st;
    const u32* d_local = static_cast<const u32*>(d_local_cells);
    if (n_local > 0 && !d_local) {
        if ((st = up.alloc((size_t)n_local * kF * sizeof(u32), nullptr)) != MRS_OK) return st;
        MRS_HIP_TRY(hipMemcpy(up.p, h_local_cells, (size_t)n_local * kF * sizeof(u32), hipMemcpyHostToDevice));
        d_local = up.as<u32>();
    }
    MRS_HIP_TRY(hipMemcpy(tab.p, h_tab.data(), h_tab.size(), hipMemcpyHostToDevice));
    const long long* d_offs = tab.as<long long>();
    const float* d_T = reinterpret_cast<const float*>(tab.as<char>() + b_offs);
    long long base = 0, pose0 = 0;
    for (int r = 0; r < n_robots; ++r) {
        mrs_gem* g = stores[r];
        const int ns = g->submaps();
        const long long n = g->off.back();
        if (n > 0)
            hipLaunchKernelGGL(k_gem_export_moved, dim3(blocks_for(n)), dim3(kThreads), 0, nullptr, g->arena.cols(), n, d_offs + off_at[r], ns,
                               d_T + (size_t)pose0 * 16, d_cat + base * kF);
        base += n;
        pose0 += ns;
    }
    if (n_local > 0)
        hipLaunchKernelGGL(k_gem_move_records, dim3(blocks_for(n_local)), dim3(kThreads), 0, nullptr, d_local, n_local, d_offs + local_at, n_robots,
                           d_T + (size_t)n_sub * 16, d_cat + base * kF);
    MRS_HIP_TRY(hipGetLastError());
    if (!merge_cells) {
        MRS_HIP_TRY(hipStreamSynchronize(nullptr));
        return d_cells ? MRS_OK : records_out(d_cat, M, h_cells, nullptr);
    }

    // merge_cells: one grid over the concatenation, equal keys folded left to right
    SortSpace w;
    mrs::Scratch merged, cnt;
    if ((st = w.alloc(M)) != MRS_OK) return st;
    if ((st = merged.alloc((size_t)M * kF * sizeof(u32), nullptr)) != MRS_OK) return st;
    if ((st = cnt.alloc(sizeof(u64), nullptr)) != MRS_OK) return st;
    MRS_HIP_TRY(hipMemsetAsync(cnt.p, 0, sizeof(u64), nullptr));
    const u64* keys = nullptr;
    const int* vals = nullptr;
    hipLaunchKernelGGL(k_gem_record_keys, dim3(blocks_for(M)), dim3(kThreads), 0, nullptr, d_cat, M, resolution, w.k0, w.v0);
    if ((st = w.sort(M, 48, &keys, &vals)) != MRS_OK) return st;
    hipLaunchKernelGGL(k_gem_merge_heads, dim3(blocks_for(M)), dim3(kThreads), 0, nullptr, keys, M, w.a, cnt.as<u64>());
    if ((st = w.exclusive_sum(w.a, w.b, M)) != MRS_OK) return st;
    hipLaunchKernelGGL(k_gem_merge_fold, dim3(blocks_for(M)), dim3(kThreads), 0, nullptr, keys, vals, w.a, w.b, M, d_cat, rule, resolution, merged.as<u32>());
    MRS_HIP_TRY(hipGetLastError());
    long long cells = 0;
    u64 h_cnt = 0;
    if ((st = last_total(w.b, w.a, M, &cells)) != MRS_OK) return st;
    MRS_HIP_TRY(hipMemcpy(&h_cnt, cnt.p, sizeof(u64), hipMemcpyDeviceToHost));
    *h_n = cells;
    if (h_dropped) *h_dropped = (long long)h_cnt;
    return records_out(merged.as<u32>(), cells, h_cells, d_cells);
}

int mrs_gem_costmap(mrs_ctx* ctx, const void* h_cloud, const void* d_cloud, int64_t n, double origin_x, double origin_y, int32_t size_x, int32_t size_y,
                    double resolution, int32_t thresh_type, double thresh, uint8_t* h_grid, uint8_t* d_grid)
{
    MRS_REQUIRE(ctx, "null pointer");
    MRS_REQUIRE(n >= 0 && n <= kMaxRecords, "n must lie in [0, 2^31)");
    MRS_REQUIRE(n == 0 || (h_cloud != nullptr) != (d_cloud != nullptr), "pass the cloud either as h_cloud or as d_cloud");
    MRS_REQUIRE((h_grid != nullptr) != (d_grid != nullptr), "pass the grid either as h_grid or as d_grid");
    MRS_REQUIRE(size_x >= 1 && size_y >= 1 && (long long)size_x * size_y <= (1ll << 28), "the grid has between 1 and 2^28 cells");
    MRS_REQUIRE(std::isfinite(origin_x) && std::isfinite(origin_y) && std::isfinite(resolution) && resolution > 0.0, "origin and resolution must be finite");
    MRS_REQUIRE(thresh_type == 0 || thresh_type == 1, "thresh_type is 0 (traversability) or 1 (elevation)");
    MRS_HIP_TRY(hipSetDevice(ctx->device));
    const long long cells = (long long)size_x * size_y;
    mrs::Scratch up, grid, out;
    int st = grid.alloc((size_t)cells * sizeof(u64), nullptr);
    if (st != MRS_OK) return st;
    MRS_HIP_TRY(hipMemsetAsync(grid.p, 0, (size_t)cells * sizeof(u64), nullptr));
    if (n > 0) {
        const u32* rec = nullptr;
        if ((st = records_on_device(h_cloud, d_cloud, n, &up, &rec)) != MRS_OK) return st;
        hipLaunchKernelGGL(k_gem_cost_scatter, dim3(blocks_for(n)), dim3(kThreads), 0, nullptr, rec, n, origin_x, origin_y, resolution, size_x, size_y,
                           thresh_type, thresh, grid.as<u64>());
    }
    unsigned char* d_out = d_grid;
    if (!d_out) {
        if ((st = out.alloc((size_t)cells, nullptr)) != MRS_OK) return st;
        d_out = out.as<unsigned char>();
    }
    hipLaunchKernelGGL(k_gem_cost_resolve, dim3(blocks_for(cells)), dim3(kThreads), 0, nullptr, grid.as<u64>(), cells, d_out);
    MRS_HIP_TRY(hipGetLastError());
    if (h_grid) MRS_HIP_TRY(hipMemcpy(h_grid, d_out, (size_t)cells, hipMemcpyDeviceToHost));
    else MRS_HIP_TRY(hipStreamSynchronize(nullptr));
    return MRS_OK;
}

}  // extern "C"
