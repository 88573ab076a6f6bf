// gem_cell.hpp -- the per-cell arithmetic of the global elevation map (gem.hip): cell key, snapped position, the window
// predicate of the open submap, the two fusion rules and the costmap verdict.  Host and device compile the same text (a stand-alone host
// program exercises it under the sanitizers: tests/cpp/gem_cell_main.cpp), and the library is built with -ffp-contract=off, so every
// operation below is one IEEE operation in the order written.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define MRS_GEM_HD __host__ __device__ inline
#else
#define MRS_GEM_HD inline
#endif

namespace mrs {
namespace gem {

constexpr int kFields = 10;                  // x y z var | r g b frontier | intensity travers, 32 bits each
enum Field { kX = 0, kY, kZ, kVar, kR, kG, kB, kFrontier, kIntensity, kTravers };
constexpr int kKeyBound = 1 << 23;           // a cell key k is accepted iff |k| < 2^23
constexpr float kNoElevation = -10.0f;       // the reference's "no data" elevation

// Cell key of one coordinate (ElevationMapping.cpp:1229): k = ceil((double)v / resolution).  False for a non-finite v or a key outside
// the bound; *k is written only when true.
MRS_GEM_HD bool cell_key(float v, double resolution, int32_t* k)
{
    const double c = std::ceil((double)v / resolution);
    if (!(c > -(double)kKeyBound && c < (double)kKeyBound)) return false;     // NaN and +-inf fail both compares
    *k = (int32_t)c;
    return true;
}

// centre of cell k as the reference stores it: (float)(k * resolution - resolution / 2.0)
MRS_GEM_HD float cell_centre(int32_t k, double resolution)
{
    return (float)((double)k * resolution - resolution / 2.0);
}

// (kx, ky) as one sortable word of 48 bits: each key offset by 2^23 into [1, 2^24 - 1]; 0 is free for "no key"
MRS_GEM_HD uint64_t pack_key(int32_t kx, int32_t ky)
{
    return ((uint64_t)(uint32_t)(kx + kKeyBound) << 24) | (uint64_t)(uint32_t)(ky + kKeyBound);
}

// The window predicate of updateLocalMap (ElevationMapping.cpp:770-779) as written, in float: which cells of the previous window enter the
// open submap for a shift (dx, dy) of the window to (cx, cy); half = length * resolution / 2.
MRS_GEM_HD bool leaves_window(float px, float py, float elevation, float cx, float cy, float dx, float dy, float half)
{
    if (!(elevation != kNoElevation)) return false;
    const float xl = cx - half, xh = cx + half, yl = cy - half, yh = cy + half;
    return ((px < xl || py < yl) && (dx > 0 && dy > 0)) || ((px > xh || py > yh) && (dx < 0 && dy < 0)) ||
           ((px < xl || py > yh) && (dx > 0 && dy < 0)) || ((px > xh || py < yl) && (dx < 0 && dy > 0)) ||
           ((px < xl) && (dx > 0 && dy == 0)) || ((px > xh) && (dx < 0 && dy == 0)) ||
           ((py < yl) && (dy > 0 && dx == 0)) || ((py > yh) && (dy < 0 && dx == 0));
}

// the gate of ElevationMapping.cpp:910 on the old record's variance (false for NaN)
MRS_GEM_HD bool fusable(float var_old) { return var_old > 0.0f && var_old < 1.0f; }

enum Rule { kWeighted = 0, kAsWritten = 1 };

// Elevation and variance of the fused record from old (zo, vo) and new (zn, vn), in double, stored to float.
// kAsWritten: the reference's expressions with C precedence (:913-914); kWeighted: the inverse-variance mean they evidently mean.
MRS_GEM_HD void fuse_zvar(int rule, float zo_, float vo_, float zn_, float vn_, float* z, float* var)
{
    const double zo = zo_, zn = zn_, vo2 = (double)vo_ * (double)vo_, vn2 = (double)vn_ * (double)vn_;
    if (rule == kAsWritten) {
        *z = (float)(((vn2 * zo) + ((vo2 * zn) / vo2)) + vn2);
        *var = (float)(((vo2 * vn2) / vo2) + vn2);
    } else {
        const double s = vo2 + vn2;
        *z = (float)(((vn2 * zo) + (vo2 * zn)) / s);
        *var = (float)((vo2 * vn2) / s);
    }
}

// x' = ((m0 x + m1 y) + m2 z) + m3 for the three rows of a row-major 4x4 (or 3x4) float matrix
MRS_GEM_HD void move_point(const float* m, float x, float y, float z, float* ox, float* oy, float* oz)
{
    *ox = ((m[0] * x + m[1] * y) + m[2] * z) + m[3];
    *oy = ((m[4] * x + m[5] * y) + m[6] * z) + m[7];
    *oz = ((m[8] * x + m[9] * y) + m[10] * z) + m[11];
}

// T = opt * inverse(pose) in float32 for rigid row-major 4x4 matrices: inverse = (R^T, -(R^T t)), each sum left to right
inline void correction(const float* opt, const float* pose, float* T)
{
    float inv[16];
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) inv[r * 4 + c] = pose[c * 4 + r];
        inv[r * 4 + 3] = -((pose[0 * 4 + r] * pose[3] + pose[1 * 4 + r] * pose[7]) + pose[2 * 4 + r] * pose[11]);
    }
    inv[12] = inv[13] = inv[14] = 0.0f;
    inv[15] = 1.0f;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c)
            T[r * 4 + c] = ((opt[r * 4 + 0] * inv[0 * 4 + c] + opt[r * 4 + 1] * inv[1 * 4 + c]) + opt[r * 4 + 2] * inv[2 * 4 + c]) + opt[r * 4 + 3] * inv[3 * 4 + c];
    T[12] = T[13] = T[14] = 0.0f;
    T[15] = 1.0f;
}

constexpr uint8_t kCostFree = 0, kCostLethal = 254, kCostUnknown = 255;

// costmap_2d::Costmap2D::worldToMap restated: false below the origin or at / past the size
MRS_GEM_HD bool world_to_map(float x, float y, double ox, double oy, double resolution, int size_x, int size_y, int* mx, int* my)
{
    const double px = x, py = y;
    if (px != px || py != py) return false;                                  // isnan (pointMap_layer.cpp:110)
    if (px < ox || py < oy) return false;
    const double fx = (px - ox) / resolution, fy = (py - oy) / resolution;
    if (!(fx < (double)size_x && fy < (double)size_y)) return false;         // also keeps the casts in range
    *mx = (int)fx;
    *my = (int)fy;
    return true;
}

// pointMap_layer.cpp:120-132: thresh_type 0 compares the traversability, 1 the elevation
MRS_GEM_HD uint8_t cell_cost(float z, float travers, int thresh_type, double thresh)
{
    const bool known = z != -10.0f && z != 10.0f && travers != -10.0f;
    const bool hit = thresh_type == 0 ? (double)travers < thresh : (double)z > thresh;
    return known && hit ? kCostLethal : kCostFree;
}

}  // namespace gem
}  // namespace mrs
