// submap_device.hpp -- what the consumers of a keyframe store share: the store itself (struct mrs_keyframes), the point arithmetic of DESIGN.md
// section 4.11 and the order-preserving float bits of the cell bounds.  Included by submap.hip (row G0) and mapcompose.hip (row G8).
#pragma once
#include "common.hpp"

#include <algorithm>

struct mrs_keyframes {
    mrs_ctx* ctx = nullptr;
    mrs::DeviceBuffer<float4> arena;
    std::vector<long long> offsets{0};        // [n + 1] first point of every keyframe
    std::vector<float> poses;                 // [n][16] row-major
    void* h_stage = nullptr;                  // pinned: host points on their way in, the tables of a call, the offsets on their way out
    size_t stage_bytes = 0;
    hipStream_t s = nullptr;
    hipEvent_t ev_in = nullptr, ev_out = nullptr;
    std::mutex mu;
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

// the point moved into the centre keyframe's frame (one rounding per operation, in this order) and the pass-through verdict
__device__ __forceinline__ bool move_and_crop(const float4 p, const float* __restrict__ T, float crop, float& x, float& y, float& z)
{
    x = ((T[0] * p.x + T[1] * p.y) + T[2] * p.z) + T[3];
    y = ((T[4] * p.x + T[5] * p.y) + T[6] * p.z) + T[7];
    z = ((T[8] * p.x + T[9] * p.y) + T[10] * p.z) + T[11];
    const bool finite = fabsf(x) <= 3.402823466e38f && fabsf(y) <= 3.402823466e38f && fabsf(z) <= 3.402823466e38f;      // false for NaN and inf
    return finite && x >= -crop && x <= crop && y >= -crop && y <= crop;
}

inline size_t round256(size_t b) { return (b + 255) & ~(size_t)255; }

// the handle's pinned staging buffer grown to `bytes` (doubling); lock held
inline int stage_reserve(mrs_keyframes* kf, size_t bytes)
{
    if (bytes <= kf->stage_bytes) return MRS_OK;
    size_t cap = std::max(kf->stage_bytes, (size_t)1 << 20);
    while (cap < bytes) cap *= 2;
    MRS_HIP_TRY(hipStreamSynchronize(kf->s));
    if (kf->h_stage) (void)hipHostFree(kf->h_stage);
    kf->h_stage = nullptr; kf->stage_bytes = 0;
    MRS_HIP_TRY(hipHostMalloc(&kf->h_stage, cap, hipHostMallocDefault));
    kf->stage_bytes = cap;
    return MRS_OK;
}

}  // namespace kfdev
}  // namespace mrs
