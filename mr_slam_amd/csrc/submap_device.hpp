// submap_device.hpp -- what the consumers of a keyframe store share: the store itself (struct mrs_keyframes), the point arithmetic of DESIGN.md
// section 4.11 (the point moved, the cell, the grid of a set of cell bounds, the key, the mean) and the order-preserving float bits of the
// cell bounds.  Included by submap.hip (row G0), mapcompose.hip (row G8) and intake.hip (row G10).
#pragma once
#include "common.hpp"

#include <algorithm>
#include <cmath>

struct mrs_keyframes {
    mrs::HandleStream s;                      // first: destroyed last, after the buffers whose work it carried
    mrs_ctx* ctx = nullptr;
    mrs::DeviceBuffer<float4> arena;
    std::vector<long long> offsets{0};        // [n + 1] first point of every keyframe
    std::vector<float> poses;                 // [n][16] row-major
    mrs::PinnedBuffer<char> h_stage;          // host points on their way in, the tables of a call, the offsets on their way out
    std::mutex mu;

    ~mrs_keyframes() { if (s) (void)hipStreamSynchronize(s); }      // nothing queued outlives the buffers
};

namespace mrs {
namespace kfdev {

// total order of floats as unsigned ints (for atomicMin / atomicMax on cells kept as the floats floorf returned)
__device__ __forceinline__ unsigned order_bits(float f)
{
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float order_float(unsigned u)
{
    return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}

constexpr float kFltMax = 3.402823466e38f;
constexpr long long kMaxArenaPoints = 1ll << 34;      // 256 GiB of float4: no size computed from a point count can wrap

__device__ __forceinline__ bool finite3(float x, float y, float z)      // false for NaN and inf
{
    return fabsf(x) <= kFltMax && fabsf(y) <= kFltMax && fabsf(z) <= kFltMax;
}

// the voxel cell of one coordinate, kept as the float floorf returned
__device__ __forceinline__ float cell_of(float v, float inv) { return floorf(v * inv); }

// minimum / maximum of the ordered cell bits across the wave (every lane ends with the wave's values)
__device__ __forceinline__ void wave_minmax3(unsigned lo[3], unsigned hi[3])
{
#pragma unroll
    for (int a = 0; a < 3; ++a)
        for (int o = 32; o > 0; o >>= 1) {
            lo[a] = min(lo[a], (unsigned)__shfl_xor((int)lo[a], o, 64));
            hi[a] = max(hi[a], (unsigned)__shfl_xor((int)hi[a], o, 64));
        }
}

// The grid of a set of kept points from the ordered bits of its minimum cell (b[0..2]) and maximum cell (b[3..5]): the minimum cell, the key
// multipliers and the number of bits of the largest key the grid can hold (at least 1).  false: a cell beyond +-2^62 (or v * inv overflowed
// to inf), or div.x * div.y * div.z not below 2^63.
__device__ __forceinline__ bool grid_from_bounds(const unsigned* b, long long mn[3], long long& mul_y, long long& mul_z, int& bits)
{
    long long div[3];
    for (int a = 0; a < 3; ++a) {
        const float lo = order_float(b[a]), hi = order_float(b[3 + a]);
        if (!(fabsf(lo) < 4.6e18f && fabsf(hi) < 4.6e18f)) return false;
        mn[a] = (long long)lo;
        div[a] = (long long)hi - mn[a] + 1;
    }
    const long long kMax = 0x7fffffffffffffffll;
    if (div[1] > kMax / div[0]) return false;
    mul_y = div[0];
    mul_z = div[0] * div[1];
    if (div[2] > kMax / mul_z) return false;
    const unsigned long long last = (unsigned long long)(mul_z * div[2]) - 1ull;
    bits = last == 0ull ? 1 : 64 - __clzll((long long)last);
    return true;
}

// 64-bit key of a kept point on a grid
__device__ __forceinline__ unsigned long long voxel_key(float x, float y, float z, float inv, long long mn_x, long long mn_y, long long mn_z,
                                                        long long mul_y, long long mul_z)
{
    const long long cx = (long long)cell_of(x, inv) - mn_x, cy = (long long)cell_of(y, inv) - mn_y, cz = (long long)cell_of(z, inv) - mn_z;
    return (unsigned long long)(cx + cy * mul_y + cz * mul_z);
}

// a voxel's output point from the float64 sums of its m points: one division and one rounding to float32 per channel
__device__ __forceinline__ float4 mean_of(double sx, double sy, double sz, double sw, double m)
{
    return make_float4((float)(sx / m), (float)(sy / m), (float)(sz / m), (float)(sw / m));
}

// the point moved into the centre keyframe's frame (one rounding per operation, in this order) and the pass-through verdict
__device__ __forceinline__ bool move_and_crop(const float4 p, const float* __restrict__ T, float crop, float& x, float& y, float& z)
{
    x = ((T[0] * p.x + T[1] * p.y) + T[2] * p.z) + T[3];
    y = ((T[4] * p.x + T[5] * p.y) + T[6] * p.z) + T[7];
    z = ((T[8] * p.x + T[9] * p.y) + T[10] * p.z) + T[11];
    return finite3(x, y, z) && x >= -crop && x <= crop && y >= -crop && y <= crop;
}

inline size_t round256(size_t b) { return (b + 255) & ~(size_t)255; }

// the handle's pinned staging buffer grown to `bytes` (doubling); lock held
inline int stage_reserve(mrs_keyframes* kf, size_t bytes)
{
    if (bytes <= kf->h_stage.capacity()) return MRS_OK;
    size_t cap = std::max(kf->h_stage.capacity(), (size_t)1 << 20);
    while (cap < bytes) cap *= 2;
    MRS_HIP_TRY(hipStreamSynchronize(kf->s));
    return kf->h_stage.reserve(bytes, cap);
}

// Room for `want` points: a new arena (doubling), what is there copied on the device; lock held.  Without `old` the call waits for the copy and
// frees the previous arena.  With it the previous arena is handed to the caller, who keeps it until the handle's stream has been synchronised:
// the growth then costs no synchronisation of its own.
inline int arena_reserve(mrs_keyframes* kf, long long want, mrs::DeviceBuffer<float4>* old = nullptr)
{
    MRS_REQUIRE(want >= 0 && want <= kMaxArenaPoints, "more than 2^34 points in one keyframe store");
    if ((size_t)want <= kf->arena.capacity()) return MRS_OK;
    size_t cap = std::max(kf->arena.capacity(), (size_t)1024);
    while (cap < (size_t)want) cap *= 2;
    mrs::DeviceBuffer<float4> grown;
    int st = grown.reserve(cap, cap);
    if (st != MRS_OK) return st;
    const long long used = kf->offsets.back();
    if (used > 0) MRS_HIP_TRY(hipMemcpyAsync(grown.get(), kf->arena.get(), (size_t)used * sizeof(float4), hipMemcpyDeviceToDevice, kf->s));
    if (old) *old = std::move(kf->arena);
    else MRS_HIP_TRY(hipStreamSynchronize(kf->s));
    kf->arena = std::move(grown);
    return MRS_OK;
}

inline bool rigid_finite(const float* P)
{
    for (int i = 0; i < 16; ++i)
        if (!std::isfinite(P[i])) return false;
    return true;
}

}  // namespace kfdev
}  // namespace mrs
