// fpfh.hip -- radius neighbours, SPFH / FPFH histograms and ISS keypoints of a ragged batch of clouds (C ABI mrs_radius_*, mrs_fpfh_*,
// mrs_iss_*).
//
// What it replaces: RING_ros/FPFH.py:33-105 -- get_spfh and describe, one Python call per keypoint and one per neighbour of a keypoint, on
// the lists of sklearn's KDTree.query_radius -- and the ISS module that file imports and the reference does not ship.
//   rows   : a uniform grid of cell size r (1 + 2^-10) per cloud: cell of every point in fp64, key = cloud | z | y | x cell (16 bits each),
//            one stable radix sort of (key, point).  A query walks the 9 (y, z) cell rows around it; the three x cells of a row are one
//            run of the sorted keys, found with one binary search inside the cloud's segment.  k_radius_walk counts, the caller
//            allocates, k_radius_walk fills; k_row_rank then puts every row into ascending order (rank of an entry = the entries of the
//            row below it; 16 lanes per row).  The membership test is fp64 on the widened float32 coordinates, (dx dx + dy dy) + dz dz
//            <= r r: a pure function of the two points and r, so a row does not depend on the batch, the grid or the launch.
//   spfh   : 16 lanes per point, a lane per neighbour in turn; alpha, phi, theta in fp64 in the reference's operation order (no
//            contraction), bins by np.histogram's rule against the edges of linspace (made on the host, staged in LDS); integer LDS
//            adds, so the counts do not depend on the order.  Each third is divided by its own sum.
//   fpfh   : 32 lanes per keypoint, lanes = bins (three bins per lane at most), a loop over the row in row order: the weighted sum has
//            one order, whatever the launch.  The norm is added in bin order.
//   iss    : a thread per point: mean and covariance of the row plus the point in fp64, eigenvalues by eig3.hpp; then the non-maximum
//            test over the rows at the second radius.
// No float atomics anywhere; everything is a function of the inputs alone.
#include "common.hpp"
#include "eig3.hpp"

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>

namespace {

constexpr int kMaxBins = MRS_FPFH_MAX_BINS;
constexpr int kThreads = 256;
constexpr int kCellMax = 65535;                 // 16 bits per axis; cells past it are clamped (more candidates, the same rows)
constexpr int kSpfhLanes = 16, kSpfhPer = kThreads / kSpfhLanes;
constexpr int kFpfhLanes = 32, kFpfhPer = kThreads / kFpfhLanes;
static_assert(3 * kMaxBins <= 3 * kFpfhLanes, "a lane of k_describe holds three bins at most");
typedef unsigned long long u64;

// the cloud of packed point i: the last c with offs[c] <= i (clouds without points are stepped over)
__device__ __forceinline__ int find_cloud(const int64_t* __restrict__ offs, int batch, int64_t i)
{
    int lo = 0, hi = batch;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (offs[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ int64_t clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ u64 cell_key(int c, int z, int y, int x) { return ((u64)c << 48) | ((u64)z << 32) | ((u64)y << 16) | (u64)x; }

// ---- rows --------------------------------------------------------------------------------------------------------------------------
// lo[c][3]: the smallest finite coordinate of cloud c per axis (+inf without one).  A workgroup per cloud.
__global__ __launch_bounds__(1024) void k_cloud_min(const float* __restrict__ pts, int stride, const int64_t* __restrict__ offs,
                                                    float* __restrict__ lo)
{
    __shared__ float part[16][3];
    const int c = blockIdx.x;
    float m[3] = {INFINITY, INFINITY, INFINITY};
    for (int64_t i = offs[c] + threadIdx.x; i < offs[c + 1]; i += 1024) {
        const float* q = pts + (size_t)i * stride;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float v = q[a];
            if (fabsf(v) < INFINITY) m[a] = fminf(m[a], v);
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a)
        for (int o = 32; o > 0; o >>= 1) m[a] = fminf(m[a], __shfl_xor(m[a], o, 64));
    if ((threadIdx.x & 63) == 0)
        for (int a = 0; a < 3; ++a) part[threadIdx.x >> 6][a] = m[a];
    __syncthreads();
    if (threadIdx.x < 3) {
        float v = part[0][threadIdx.x];
        for (int w = 1; w < 16; ++w) v = fminf(v, part[w][threadIdx.x]);
        lo[3 * c + threadIdx.x] = v;
    }
}

// cell of one coordinate: floor((v - lo) / cell) in fp64, clamped; a coordinate that is not finite goes to cell 0 (it is nobody's neighbour)
__device__ __forceinline__ int cell_of(float v, float lo, double inv_cell)
{
    const double q = ((double)v - (double)lo) * inv_cell;
    if (!(q >= 1.0)) return 0;
    return q >= (double)kCellMax ? kCellMax : (int)q;
}

__global__ void k_cell_keys(const float* __restrict__ pts, int stride, const int64_t* __restrict__ offs, int batch, int n,
                            const float* __restrict__ lo, double inv_cell, u64* __restrict__ keys, int* __restrict__ vals)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int c = find_cloud(offs, batch, i);
    const float* q = pts + (size_t)i * stride;
    keys[i] = cell_key(c, cell_of(q[2], lo[3 * c + 2], inv_cell), cell_of(q[1], lo[3 * c + 1], inv_cell), cell_of(q[0], lo[3 * c], inv_cell));
    vals[i] = i;
}

// the points in sorted order, widened: x, y, z and the packed index (exact in a double)
__global__ void k_gather_cells(const float* __restrict__ pts, int stride, int n, const int* __restrict__ vals, double4* __restrict__ sorted)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const int i = vals[t];
    const float* q = pts + (size_t)i * stride;
    sorted[t] = make_double4((double)q[0], (double)q[1], (double)q[2], (double)i);
}

// One thread per point, in sorted order (neighbouring threads walk neighbouring cells).  FILL = false: cnt[i] = the row's length;
// FILL = true: the members go to tmp[row_start[i] ..) as cloud-local indices, in the order of the walk (at most the row's length of them).
template <bool FILL>
__global__ __launch_bounds__(kThreads) void k_radius_walk(const u64* __restrict__ keys, const double4* __restrict__ sorted,
                                                          const int64_t* __restrict__ offs, int n, double r2, int64_t* __restrict__ cnt,
                                                          const int64_t* __restrict__ row_start, int64_t total, int32_t* __restrict__ tmp)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const u64 key = keys[t];
    const int c = (int)(key >> 48), cz = (int)(key >> 32) & 0xffff, cy = (int)(key >> 16) & 0xffff, cx = (int)key & 0xffff;
    const int64_t seg0 = offs[c], seg1 = offs[c + 1];        // the cloud's points are one segment of the sorted arrays too
    const double4 p = sorted[t];
    const int i = (int)p.w;
    int64_t out = 0, cap = 0;
    if (FILL) {
        out = clamp64(row_start[i], 0, total);
        cap = clamp64(row_start[i + 1], out, total);
    }
    int64_t found = 0;
    for (int dz = -1; dz <= 1; ++dz) {
        const int z = cz + dz;
        if (z < 0 || z > kCellMax) continue;
        for (int dy = -1; dy <= 1; ++dy) {
            const int y = cy + dy;
            if (y < 0 || y > kCellMax) continue;
            const u64 k_lo = cell_key(c, z, y, max(cx - 1, 0)), k_hi = cell_key(c, z, y, min(cx + 1, kCellMax));
            int64_t a = seg0, b = seg1;                      // first u in [seg0, seg1) with keys[u] >= k_lo
            while (a < b) {
                const int64_t mid = (a + b) >> 1;
                if (keys[mid] < k_lo) a = mid + 1; else b = mid;
            }
            for (int64_t u = a; u < seg1 && keys[u] <= k_hi; ++u) {
                if (u == t) continue;
                const double4 q = sorted[u];
                const double dx = q.x - p.x, ddy = q.y - p.y, ddz = q.z - p.z;
                const double d2 = (dx * dx + ddy * ddy) + ddz * ddz;
                if (d2 <= r2) {
                    if (FILL) {
                        if (out + found < cap) tmp[out + found] = (int32_t)((int64_t)q.w - seg0);
                    }
                    ++found;
                }
            }
        }
    }
    if (!FILL) cnt[i] = found;
}

// 16 lanes per row: entry e goes to position (number of entries of the row below it); the entries of a row are distinct
__global__ __launch_bounds__(kThreads) void k_row_rank(const int64_t* __restrict__ row_start, int n, int64_t total,
                                                       const int32_t* __restrict__ tmp, int32_t* __restrict__ index)
{
    const int64_t g = (int64_t)blockIdx.x * (kThreads / 16) + (threadIdx.x >> 4);
    const int c = threadIdx.x & 15;
    if (g >= n) return;
    const int64_t s = clamp64(row_start[g], 0, total), e = clamp64(row_start[g + 1], s, total);
    for (int64_t k = s + c; k < e; k += 16) {
        const int32_t v = tmp[k];
        int64_t rank = 0;
        for (int64_t u = s; u < e; ++u) rank += tmp[u] < v ? 1 : 0;
        index[s + rank] = v;
    }
}

struct Grid {
    mrs::Scratch lo, keys_in, keys, vals_in, vals, sorted, tmp;
};

int build_grid(const float* d_points, int stride, const int64_t* d_offsets, int batch, int n, double radius, Grid& G, hipStream_t s)
{
    int st;
    if ((st = G.lo.alloc((size_t)batch * 3 * sizeof(float), s)) != MRS_OK) return st;
    if ((st = G.keys_in.alloc((size_t)n * 8, s)) != MRS_OK) return st;
    if ((st = G.keys.alloc((size_t)n * 8, s)) != MRS_OK) return st;
    if ((st = G.vals_in.alloc((size_t)n * 4, s)) != MRS_OK) return st;
    if ((st = G.vals.alloc((size_t)n * 4, s)) != MRS_OK) return st;
    if ((st = G.sorted.alloc((size_t)n * sizeof(double4), s)) != MRS_OK) return st;
    // a little more than r: |dx| <= r (1 + a few ulp) keeps the two cells at most one apart whatever the rounding of the quotients
    const double inv_cell = 1.0 / (radius * (1.0 + 1.0 / 1024.0));
    const unsigned blocks = (unsigned)((n + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(k_cloud_min, dim3(batch), dim3(1024), 0, s, d_points, stride, d_offsets, G.lo.as<float>());
    hipLaunchKernelGGL(k_cell_keys, dim3(blocks), dim3(kThreads), 0, s, d_points, stride, d_offsets, batch, n, G.lo.as<float>(), inv_cell,
                       G.keys_in.as<u64>(), G.vals_in.as<int>());
    int key_bits = 48;
    while ((1ll << (key_bits - 48)) < batch) ++key_bits;
    size_t bytes = 0;
    MRS_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, G.keys_in.as<u64>(), G.keys.as<u64>(), G.vals_in.as<int>(), G.vals.as<int>(), n,
                                                   0, key_bits, s));
    if ((st = G.tmp.alloc(bytes, s)) != MRS_OK) return st;
    MRS_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(G.tmp.p, bytes, G.keys_in.as<u64>(), G.keys.as<u64>(), G.vals_in.as<int>(), G.vals.as<int>(), n,
                                                   0, key_bits, s));
    hipLaunchKernelGGL(k_gather_cells, dim3(blocks), dim3(kThreads), 0, s, d_points, stride, n, G.vals.as<int>(), G.sorted.as<double4>());
    MRS_HIP_TRY(hipGetLastError());
    return MRS_OK;
}

int check_batch(const mrs_ctx* ctx, const void* d_points, int stride, const int64_t* d_offsets, const int64_t* h_offsets, int batch,
                double radius, int64_t* n_out)
{
    MRS_REQUIRE(ctx && d_offsets && h_offsets, "null pointer");
    MRS_REQUIRE(batch >= 1 && batch <= mrs::kMaxGridY && stride >= 3, "batch must be within [1, 65535] and stride_floats >= 3");
    MRS_REQUIRE(radius > 0.0 && radius < INFINITY, "radius must be positive and finite");
    MRS_REQUIRE(h_offsets[0] == 0, "offsets start at 0");
    for (int b = 0; b < batch; ++b) MRS_REQUIRE(h_offsets[b + 1] >= h_offsets[b], "offsets must be non-decreasing");
    MRS_REQUIRE(h_offsets[batch] < (1ll << 31) - 1, "fewer than 2^31 - 1 points per call");
    MRS_REQUIRE(d_points || h_offsets[batch] == 0, "null pointer");
    *n_out = h_offsets[batch];
    return MRS_OK;
}

// ---- histograms --------------------------------------------------------------------------------------------------------------------
struct Edges {                                   // np.linspace(lo, hi, bins + 1): fl(fl(i step) + lo), the last one hi itself
    double unit[kMaxBins + 1], angle[kMaxBins + 1];
};

void make_edges(int bins, Edges& E)
{
    const double lo[2] = {-1.0, -M_PI}, hi[2] = {1.0, M_PI};
    for (int a = 0; a < 2; ++a) {
        double* e = a ? E.angle : E.unit;
        const double step = (hi[a] - lo[a]) / (double)bins;
        for (int i = 0; i <= kMaxBins; ++i) {
            const double v = (double)i * step;
            e[i] = i < bins ? v + lo[a] : hi[a];
        }
    }
}

// np.histogram's bin of v for `bins` equal bins with the given edges: the i with e[i] <= v < e[i + 1], the last bin closed on the right;
// -1 for a value outside [e[0], e[bins]] or NaN
__device__ __forceinline__ int hist_bin(double v, const double* e, int bins)
{
    if (!(v >= e[0] && v <= e[bins])) return -1;
    int i = (int)((v - e[0]) / (e[bins] - e[0]) * (double)bins);
    i = min(max(i, 0), bins - 1);
    while (i > 0 && v < e[i]) --i;
    while (i < bins - 1 && v >= e[i + 1]) ++i;
    return i;
}

struct RowSpan {
    int64_t base, s, e;
    unsigned cloud_n;
};

__device__ __forceinline__ RowSpan row_span(const int64_t* __restrict__ offs, int batch, int64_t n, int64_t i, const int64_t* __restrict__ row_start,
                                            int64_t total, int* __restrict__ bad)
{
    RowSpan r;
    const int c = find_cloud(offs, batch, i);
    r.base = offs[c];
    const int64_t end = offs[c + 1] < n ? offs[c + 1] : n;     // offsets that disagree with n cannot lead past the n points either
    r.cloud_n = end > r.base ? (unsigned)(end - r.base) : 0u;
    const int64_t s = row_start[i], e = row_start[i + 1];
    r.s = clamp64(s, 0, total);
    r.e = clamp64(e, r.s, total);
    if (bad && (r.s != s || r.e != e)) *bad = 1;
    return r;
}

__global__ __launch_bounds__(kThreads) void k_spfh(const float* __restrict__ pts, int stride, const float* __restrict__ nrm,
                                                   const int64_t* __restrict__ offs, int batch, int64_t n,
                                                   const int64_t* __restrict__ row_start, const int32_t* __restrict__ index, int64_t total,
                                                   int bins, Edges E, int32_t* __restrict__ counts, double* __restrict__ spfh, int* __restrict__ bad)
{
    __shared__ int hist[kSpfhPer][3 * kMaxBins];
    __shared__ double edge[2][kMaxBins + 1];
    const int t = threadIdx.x, grp = t / kSpfhLanes, c = t % kSpfhLanes, nb = 3 * bins;
    for (int k = t; k < kSpfhPer * 3 * kMaxBins; k += kThreads) (&hist[0][0])[k] = 0;
    for (int k = t; k <= kMaxBins; k += kThreads) { edge[0][k] = E.unit[k]; edge[1][k] = E.angle[k]; }
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * kSpfhPer + grp;
    if (i < n) {
        const RowSpan R = row_span(offs, batch, n, i, row_start, total, c == 0 ? bad : nullptr);
        const float* pi = pts + (size_t)i * stride;
        const double px = pi[0], py = pi[1], pz = pi[2];
        const double u0 = nrm[3 * i], u1 = nrm[3 * i + 1], u2 = nrm[3 * i + 2];
        for (int64_t k = R.s + c; k < R.e; k += kSpfhLanes) {
            const int32_t jl = index[k];
            if ((unsigned)jl >= R.cloud_n) { *bad = 1; continue; }
            const int64_t j = R.base + jl;
            if (j == i) continue;
            const float* pj = pts + (size_t)j * stride;
            double d0 = (double)pj[0] - px, d1 = (double)pj[1] - py, d2 = (double)pj[2] - pz;
            const double len = sqrt((d0 * d0 + d1 * d1) + d2 * d2);
            if (len == 0.0) continue;
            d0 = d0 / len; d1 = d1 / len; d2 = d2 / len;
            const double m0 = nrm[3 * j], m1 = nrm[3 * j + 1], m2 = nrm[3 * j + 2];
            const double v0 = u1 * d2 - u2 * d1, v1 = u2 * d0 - u0 * d2, v2 = u0 * d1 - u1 * d0;
            const double w0 = u1 * v2 - u2 * v1, w1 = u2 * v0 - u0 * v2, w2 = u0 * v1 - u1 * v0;
            const double alpha = (v0 * m0 + v1 * m1) + v2 * m2;
            const double phi = (u0 * d0 + u1 * d1) + u2 * d2;
            const double theta = atan2((w0 * m0 + w1 * m1) + w2 * m2, (u0 * m0 + u1 * m1) + u2 * m2);
            const int ba = hist_bin(alpha, edge[0], bins), bp = hist_bin(phi, edge[0], bins), bt = hist_bin(theta, edge[1], bins);
            if (ba >= 0) atomicAdd(&hist[grp][ba], 1);
            if (bp >= 0) atomicAdd(&hist[grp][bins + bp], 1);
            if (bt >= 0) atomicAdd(&hist[grp][2 * bins + bt], 1);
        }
    }
    __syncthreads();
    if (i < n) {
        int sum[3] = {0, 0, 0};
        for (int b = 0; b < bins; ++b) { sum[0] += hist[grp][b]; sum[1] += hist[grp][bins + b]; sum[2] += hist[grp][2 * bins + b]; }
        for (int b = c; b < nb; b += kSpfhLanes) {
            const int v = hist[grp][b], sm = sum[b / bins];
            if (counts) counts[i * nb + b] = v;
            spfh[i * nb + b] = sm > 0 ? (double)v / (double)sm : 0.0;
        }
    }
}

__global__ __launch_bounds__(kThreads) void k_describe(const float* __restrict__ pts, int stride, const int64_t* __restrict__ offs, int batch,
                                                       int64_t n, const int64_t* __restrict__ row_start, const int32_t* __restrict__ index,
                                                       int64_t total, int bins, const double* __restrict__ spfh,
                                                       const int64_t* __restrict__ keypoints, int64_t n_key, double* __restrict__ out)
{
    __shared__ double fl[kFpfhPer][3 * kMaxBins];
    const int t = threadIdx.x, grp = t / kFpfhLanes, c = t % kFpfhLanes, nb = 3 * bins;
    const int64_t kk = (int64_t)blockIdx.x * kFpfhPer + grp;
    const bool live = kk < n_key;
    const int64_t i = live ? (keypoints ? keypoints[kk] : kk) : -1;
    const bool ok = live && i >= 0 && i < n;
    double f[3] = {0.0, 0.0, 0.0};
    if (ok) {
        const RowSpan R = row_span(offs, batch, n, i, row_start, total, nullptr);
        const float* pi = pts + (size_t)i * stride;
        const double px = pi[0], py = pi[1], pz = pi[2];
        double acc[3] = {0.0, 0.0, 0.0};
        int kept = 0;
        for (int64_t k = R.s; k < R.e; ++k) {                 // every lane of the group walks the whole row, in row order
            const int32_t jl = index[k];
            if ((unsigned)jl >= R.cloud_n) continue;
            const int64_t j = R.base + jl;
            if (j == i) continue;
            const float* pj = pts + (size_t)j * stride;
            const double d0 = (double)pj[0] - px, d1 = (double)pj[1] - py, d2 = (double)pj[2] - pz;
            const double len = sqrt((d0 * d0 + d1 * d1) + d2 * d2);
            if (len == 0.0) continue;
            const double w = 1.0 / len;
            ++kept;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const int b = c + kFpfhLanes * r;
                if (b < nb) acc[r] = acc[r] + w * spfh[j * nb + b];
            }
        }
        if (kept > 0) {
            const double inv_k = 1.0 / (double)kept;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const int b = c + kFpfhLanes * r;
                if (b < nb) f[r] = spfh[i * nb + b] + inv_k * acc[r];
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const int b = c + kFpfhLanes * r;
        if (b < nb) fl[grp][b] = f[r];
    }
    __syncthreads();
    if (!live) return;
    double ss = 0.0;
    for (int b = 0; b < nb; ++b) ss = ss + fl[grp][b] * fl[grp][b];
    const double norm = sqrt(ss);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const int b = c + kFpfhLanes * r;
        if (b < nb) out[kk * nb + b] = norm == 0.0 ? 0.0 : f[r] / norm;
    }
}

// ---- ISS ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_iss_saliency(const float* __restrict__ pts, int stride, const int64_t* __restrict__ offs, int batch,
                                                           int64_t n, const int64_t* __restrict__ row_start, const int32_t* __restrict__ index,
                                                           int64_t total, int min_neighbors, double g21, double g32, double* __restrict__ sal)
{
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const RowSpan R = row_span(offs, batch, n, i, row_start, total, nullptr);
    const float* pi = pts + (size_t)i * stride;
    const double px = pi[0], py = pi[1], pz = pi[2];
    const int64_t il = i - R.base;
    // members in row order with the point itself put in before the first entry above it: ascending for ascending rows, so that two points
    // with the same member set get the same bits
    double sx = 0.0, sy = 0.0, sz = 0.0;
    int64_t m = 0;
    bool self_in = false;
    for (int64_t k = R.s; k < R.e; ++k) {
        const int32_t jl = index[k];
        if ((unsigned)jl >= R.cloud_n || jl == il) continue;
        if (!self_in && jl > il) { sx += px; sy += py; sz += pz; ++m; self_in = true; }
        const float* pj = pts + (size_t)(R.base + jl) * stride;
        sx += (double)pj[0]; sy += (double)pj[1]; sz += (double)pj[2];
        ++m;
    }
    if (!self_in) { sx += px; sy += py; sz += pz; ++m; }
    if (m < min_neighbors) { sal[i] = 0.0; return; }
    const double mx = sx / (double)m, my = sy / (double)m, mz = sz / (double)m;
    double c00 = 0.0, c01 = 0.0, c02 = 0.0, c11 = 0.0, c12 = 0.0, c22 = 0.0;
    auto add = [&](double x, double y, double z) __attribute__((always_inline)) {
        const double a = x - mx, b = y - my, c = z - mz;
        c00 += a * a; c01 += a * b; c02 += a * c; c11 += b * b; c12 += b * c; c22 += c * c;
    };
    self_in = false;
    for (int64_t k = R.s; k < R.e; ++k) {
        const int32_t jl = index[k];
        if ((unsigned)jl >= R.cloud_n || jl == il) continue;
        if (!self_in && jl > il) { add(px, py, pz); self_in = true; }
        const float* pj = pts + (size_t)(R.base + jl) * stride;
        add((double)pj[0], (double)pj[1], (double)pj[2]);
    }
    if (!self_in) add(px, py, pz);
    const double inv = 1.0 / (double)m;
    const double cov[9] = {c00 * inv, c01 * inv, c02 * inv, c01 * inv, c11 * inv, c12 * inv, c02 * inv, c12 * inv, c22 * inv};
    double w[3];
    mrs::sym3_eigvals(cov, w);
    sal[i] = (w[1] < g21 * w[0] && w[2] < g32 * w[1]) ? w[2] : 0.0;
}

__global__ __launch_bounds__(kThreads) void k_iss_nonmax(const int64_t* __restrict__ offs, int batch, int64_t n,
                                                         const int64_t* __restrict__ row_start, const int32_t* __restrict__ index, int64_t total,
                                                         const double* __restrict__ sal, uint8_t* __restrict__ keep)
{
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const RowSpan R = row_span(offs, batch, n, i, row_start, total, nullptr);
    const double si = sal[i];
    bool k = si > 0.0;
    for (int64_t u = R.s; k && u < R.e; ++u) {
        const int32_t jl = index[u];
        if ((unsigned)jl >= R.cloud_n) continue;
        const int64_t j = R.base + jl;
        if (j == i) continue;
        const double sj = sal[j];
        k = si > sj || (si == sj && i < j);
    }
    keep[i] = k ? 1 : 0;
}

int check_rows(const mrs_ctx* ctx, const int64_t* d_offsets, int batch, int64_t n, const int64_t* d_row_start, const int32_t* d_index,
               int64_t total)
{
    MRS_REQUIRE(ctx && d_offsets && d_row_start, "null pointer");
    MRS_REQUIRE(batch >= 1 && batch <= mrs::kMaxGridY, "batch must be within [1, 65535]");
    MRS_REQUIRE(n >= 0 && n < (1ll << 31) - 1 && total >= 0 && total < (1ll << 31), "n and total must fit 31 bits");
    MRS_REQUIRE(d_index || total == 0, "null pointer");
    return MRS_OK;
}

int spfh_impl(mrs_ctx* ctx, const float* d_points, int stride, const float* d_normals, const int64_t* d_offsets, int batch, int64_t n,
              const int64_t* d_row_start, const int32_t* d_index, int64_t total, int bins, int32_t* d_counts, double* d_spfh, hipStream_t s,
              bool report)
{
    int st = check_rows(ctx, d_offsets, batch, n, d_row_start, d_index, total);
    if (st != MRS_OK) return st;
    MRS_REQUIRE(stride >= 3 && bins >= 1 && bins <= kMaxBins, "stride_floats >= 3 and bins in 1..32");
    MRS_REQUIRE(n == 0 || (d_points && d_normals && d_spfh), "null pointer");
    if (n == 0) return MRS_OK;
    MRS_HIP_TRY(hipSetDevice(ctx->device));
    mrs::Scratch bad;
    if ((st = bad.alloc(sizeof(int), s)) != MRS_OK) return st;
    MRS_HIP_TRY(hipMemsetAsync(bad.p, 0, sizeof(int), s));
    Edges E;
    make_edges(bins, E);
    hipLaunchKernelGGL(k_spfh, dim3((unsigned)((n + kSpfhPer - 1) / kSpfhPer)), dim3(kThreads), 0, s, d_points, stride, d_normals, d_offsets, batch,
                       n, d_row_start, d_index, total, bins, E, d_counts, d_spfh, bad.as<int>());
    MRS_HIP_TRY(hipGetLastError());
    if (report) {
        int h_bad = 0;
        MRS_HIP_TRY(hipMemcpyAsync(&h_bad, bad.p, sizeof(int), hipMemcpyDeviceToHost, s));
        MRS_HIP_TRY(hipStreamSynchronize(s));
        MRS_REQUIRE(h_bad == 0, "a row entry outside its cloud, or row bounds outside [0, total]");
    }
    return MRS_OK;
}

}  // namespace

extern "C" {

int mrs_radius_count(mrs_ctx* ctx, const float* d_points, int32_t stride_floats, const int64_t* d_offsets, const int64_t* h_offsets,
                     int32_t batch, double radius, int64_t* d_row_start, int64_t* h_total, mrs_stream stream)
{
    int64_t n64 = 0;
    int st = check_batch(ctx, d_points, stride_floats, d_offsets, h_offsets, batch, radius, &n64);
    if (st != MRS_OK) return st;
    MRS_REQUIRE(d_row_start && h_total, "null pointer");
    MRS_HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    const int n = (int)n64;
    *h_total = 0;
    if (n == 0) {
        MRS_HIP_TRY(hipMemsetAsync(d_row_start, 0, sizeof(int64_t), s));
        MRS_HIP_TRY(hipStreamSynchronize(s));
        return MRS_OK;
    }
    Grid G;
    if ((st = build_grid(d_points, stride_floats, d_offsets, batch, n, radius, G, s)) != MRS_OK) return st;
    mrs::Scratch cnt, tmp;
    if ((st = cnt.alloc((size_t)(n + 1) * sizeof(int64_t), s)) != MRS_OK) return st;
    MRS_HIP_TRY(hipMemsetAsync(cnt.as<int64_t>() + n, 0, sizeof(int64_t), s));
    hipLaunchKernelGGL(k_radius_walk<false>, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, G.keys.as<u64>(),
                       G.sorted.as<double4>(), d_offsets, n, radius * radius, cnt.as<int64_t>(), (const int64_t*)nullptr, (int64_t)0,
                       (int32_t*)nullptr);
    size_t bytes = 0;
    MRS_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, cnt.as<int64_t>(), d_row_start, n + 1, s));
    if ((st = tmp.alloc(bytes, s)) != MRS_OK) return st;
    MRS_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(tmp.p, bytes, cnt.as<int64_t>(), d_row_start, n + 1, s));
    MRS_HIP_TRY(hipGetLastError());
    MRS_HIP_TRY(hipMemcpyAsync(h_total, d_row_start + n, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    MRS_HIP_TRY(hipStreamSynchronize(s));
    if (*h_total > (1ll << 31) - 1) {
        mrs::set_error("the rows hold %lld entries, more than 2^31 - 1: search a smaller radius or fewer clouds per call", (long long)*h_total);
        return MRS_ERR_UNSUPPORTED;
    }
    return MRS_OK;
}

int mrs_radius_fill(mrs_ctx* ctx, const float* d_points, int32_t stride_floats, const int64_t* d_offsets, const int64_t* h_offsets,
                    int32_t batch, double radius, const int64_t* d_row_start, int64_t total, int32_t* d_index, mrs_stream stream)
{
    int64_t n64 = 0;
    int st = check_batch(ctx, d_points, stride_floats, d_offsets, h_offsets, batch, radius, &n64);
    if (st != MRS_OK) return st;
    MRS_REQUIRE(d_row_start && total >= 0 && total <= (1ll << 31) - 1 && (d_index || total == 0), "null pointer, or total outside [0, 2^31 - 1]");
    const int n = (int)n64;
    if (n == 0 || total == 0) return MRS_OK;
    MRS_HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    Grid G;
    if ((st = build_grid(d_points, stride_floats, d_offsets, batch, n, radius, G, s)) != MRS_OK) return st;
    mrs::Scratch tmp;
    if ((st = tmp.alloc((size_t)total * sizeof(int32_t), s)) != MRS_OK) return st;
    // a row_start that is not the one of mrs_radius_count leaves entries unwritten: they are defined (cloud-local 0) all the same
    MRS_HIP_TRY(hipMemsetAsync(tmp.p, 0, (size_t)total * sizeof(int32_t), s));
    MRS_HIP_TRY(hipMemsetAsync(d_index, 0, (size_t)total * sizeof(int32_t), s));
    hipLaunchKernelGGL(k_radius_walk<true>, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, G.keys.as<u64>(),
                       G.sorted.as<double4>(), d_offsets, n, radius * radius, (int64_t*)nullptr, d_row_start, total, tmp.as<int32_t>());
    hipLaunchKernelGGL(k_row_rank, dim3((unsigned)(((int64_t)n + kThreads / 16 - 1) / (kThreads / 16))), dim3(kThreads), 0, s, d_row_start, n, total,
                       tmp.as<int32_t>(), d_index);
    MRS_HIP_TRY(hipGetLastError());
    return MRS_OK;
}

int mrs_fpfh_spfh(mrs_ctx* ctx, const float* d_points, int32_t stride_floats, const float* d_normals, const int64_t* d_offsets,
                  int32_t batch, int64_t n, const int64_t* d_row_start, const int32_t* d_index, int64_t total, int32_t bins,
                  int32_t* d_counts, double* d_spfh, mrs_stream stream)
{
    return spfh_impl(ctx, d_points, stride_floats, d_normals, d_offsets, batch, n, d_row_start, d_index, total, bins, d_counts, d_spfh,
                     (hipStream_t)stream, false);
}

int mrs_fpfh_spfh_from_neighbors(mrs_ctx* ctx, const float* d_points, int32_t stride_floats, const float* d_normals,
                                 const int64_t* d_offsets, int32_t batch, int64_t n, const int64_t* d_row_start, const int32_t* d_index,
                                 int64_t total, int32_t bins, int32_t* d_counts, double* d_spfh, mrs_stream stream)
{
    return spfh_impl(ctx, d_points, stride_floats, d_normals, d_offsets, batch, n, d_row_start, d_index, total, bins, d_counts, d_spfh,
                     (hipStream_t)stream, true);
}

int mrs_fpfh_describe(mrs_ctx* ctx, const float* d_points, int32_t stride_floats, const int64_t* d_offsets, int32_t batch, int64_t n,
                      const int64_t* d_row_start, const int32_t* d_index, int64_t total, int32_t bins, const double* d_spfh,
                      const int64_t* d_keypoints, int64_t n_keypoints, double* d_fpfh, mrs_stream stream)
{
    int st = check_rows(ctx, d_offsets, batch, n, d_row_start, d_index, total);
    if (st != MRS_OK) return st;
    MRS_REQUIRE(stride_floats >= 3 && bins >= 1 && bins <= kMaxBins, "stride_floats >= 3 and bins in 1..32");
    const int64_t K = d_keypoints ? n_keypoints : n;
    MRS_REQUIRE(K >= 0 && K < (1ll << 31), "the number of keypoints must fit 31 bits");
    MRS_REQUIRE(K == 0 || (d_fpfh && (n == 0 || (d_points && d_spfh))), "null pointer");
    if (K == 0) return MRS_OK;
    MRS_HIP_TRY(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_describe, dim3((unsigned)((K + kFpfhPer - 1) / kFpfhPer)), dim3(kThreads), 0, (hipStream_t)stream, d_points, stride_floats,
                       d_offsets, batch, n, d_row_start, d_index, total, bins, d_spfh, d_keypoints, K, d_fpfh);
    MRS_HIP_TRY(hipGetLastError());
    return MRS_OK;
}

int mrs_iss_saliency(mrs_ctx* ctx, const float* d_points, int32_t stride_floats, const int64_t* d_offsets, int32_t batch, int64_t n,
                     const int64_t* d_row_start, const int32_t* d_index, int64_t total, int32_t min_neighbors, double gamma21,
                     double gamma32, double* d_saliency, mrs_stream stream)
{
    int st = check_rows(ctx, d_offsets, batch, n, d_row_start, d_index, total);
    if (st != MRS_OK) return st;
    MRS_REQUIRE(stride_floats >= 3 && min_neighbors >= 1, "stride_floats >= 3 and min_neighbors >= 1");
    MRS_REQUIRE(gamma21 > 0.0 && gamma32 > 0.0 && gamma21 < INFINITY && gamma32 < INFINITY, "the ratios must be positive and finite");
    MRS_REQUIRE(n == 0 || (d_points && d_saliency), "null pointer");
    if (n == 0) return MRS_OK;
    MRS_HIP_TRY(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_iss_saliency, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, (hipStream_t)stream, d_points, stride_floats,
                       d_offsets, batch, n, d_row_start, d_index, total, min_neighbors, gamma21, gamma32, d_saliency);
    MRS_HIP_TRY(hipGetLastError());
    return MRS_OK;
}

int mrs_iss_nonmax(mrs_ctx* ctx, const int64_t* d_offsets, int32_t batch, int64_t n, const int64_t* d_row_start, const int32_t* d_index,
                   int64_t total, const double* d_saliency, uint8_t* d_keep, mrs_stream stream)
{
    int st = check_rows(ctx, d_offsets, batch, n, d_row_start, d_index, total);
    if (st != MRS_OK) return st;
    MRS_REQUIRE(n == 0 || (d_saliency && d_keep), "null pointer");
    if (n == 0) return MRS_OK;
    MRS_HIP_TRY(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_iss_nonmax, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, (hipStream_t)stream, d_offsets, batch, n,
                       d_row_start, d_index, total, d_saliency, d_keep);
    MRS_HIP_TRY(hipGetLastError());
    return MRS_OK;
}

}  // extern "C"
