// m2dp.hip -- the M2DP descriptor of a batch of raw 3-D clouds (C ABI mrs_m2dp_*).
//
// What it replaces: RING_ros/pr_methods/M2DP.py:43-124 -- sklearn's PCA().fit_transform(cloud), then a Python loop over 4 x 16 planes that
// projects the whole cloud onto each plane and calls np.histogram2d (16 theta x 8 rho bins), then np.linalg.svd of the 64 x 128 signature
// matrix; the descriptor is concat(u0, v0).  0.11 s per 20 000-point scan there, linear in the point count.
// Here, per call and for the whole batch:
//   moments   : three fixed-order passes over the points (sums -> mean; centred products -> covariance; rotated squared norms -> maxRho),
//               each a workgroup per 4096-point chunk of a scan writing ONE partial, and a finishing kernel that adds a scan's partials in
//               chunk order: no floating-point atomics, and a scan's result does not depend on where in the batch it stands;
//   PCA       : eig3.hpp's closed-form eigenvectors of the 3 x 3 covariance, sklearn's sign rule (largest-magnitude coefficient positive);
//   signature : k_m2dp_hist, one workgroup per (scan, 1024-point tile).  Every point is loaded, centred and rotated ONCE into LDS; then a
//               lane IS a plane (its two in-plane axes live in registers) and a wave walks its quarter of the tile reading each point as an
//               LDS broadcast, so the 64 LDS atomics of a point go to 64 different histogram rows (row stride 129 words: 64 different
//               banks) instead of piling onto one row.  int32 counters, flushed with global integer atomics: order-independent, exact;
//   SVD       : one workgroup per scan, power iteration on C C^T (C = the integer counts, in LDS) as two matrix-vector products, iterated
//               until the step ||u_k+1 - u_k|| is below 2^-48 and then six more (each shrinks the error by sigma2^2 / sigma1^2 ~ 0.2-0.4).
// Everything is fp64.  Exactness against the reference: the bin a (point, plane) pair falls in is decided by comparisons whose operands
// carry ~1e-15 relative error (rotation, projection, squared edges), so only pairs within ~1e-15 maxRho of a bin edge can land in the
// neighbouring bin; theta bins come from the octant and two slope comparisons (tan(pi/8), tan(3 pi/8)) instead of atan2, rho bins from
// x^2 + y^2 against the squared edges instead of a square root.  Bin indices are sums of comparison results: non-finite input cannot
// index out of bounds.
#include "common.hpp"
#include "eig3.hpp"

#include <algorithm>

namespace {

constexpr int kPlanes = 64, kBins = 128, kDesc = 192;
constexpr int kTile = MRS_M2DP_TILE_POINTS;
constexpr int kHistStride = kBins + 1;        // words from one plane's histogram to the next in LDS
constexpr int kThreads = 256;
constexpr int kChunk = 4096;                  // points per workgroup of the moment passes
constexpr int kPart = 6;                      // doubles per partial
// per-scan state, doubles: the first 16 are what mrs_m2dp_pca_batch returns
constexpr int kState = 24, kMean = 0, kRot = 3, kMaxRho = 12, kEig = 13, kEdge = 16;   // kEdge + k, k = 1..7: squared rho edge, squared again

template <class T>
__device__ __forceinline__ void load_point(const T* __restrict__ pts, int stride, int64_t i, double& x, double& y, double& z)
{
    const T* q = pts + (size_t)i * stride;
    x = (double)q[0]; y = (double)q[1]; z = (double)q[2];
}

// cloud_pca row of one point: (p - mean) . components^T
__device__ __forceinline__ void rotate(const double* __restrict__ st, double x, double y, double z, double& c0, double& c1, double& c2)
{
    const double dx = x - st[kMean], dy = y - st[kMean + 1], dz = z - st[kMean + 2];
    c0 = dx * st[kRot + 0] + dy * st[kRot + 1] + dz * st[kRot + 2];
    c1 = dx * st[kRot + 3] + dy * st[kRot + 4] + dz * st[kRot + 5];
    c2 = dx * st[kRot + 6] + dy * st[kRot + 7] + dz * st[kRot + 8];
}

// fixed-order tree over the workgroup; the result is in v[] of every thread
template <int K, bool MAX>
__device__ __forceinline__ void block_reduce(double* v, double* sm)
{
    const int t = threadIdx.x;
#pragma unroll
    for (int k = 0; k < K; ++k) sm[k * kThreads + t] = v[k];
    __syncthreads();
    for (int o = kThreads / 2; o > 0; o >>= 1) {
        if (t < o) {
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const double a = sm[k * kThreads + t], b = sm[k * kThreads + t + o];
                sm[k * kThreads + t] = MAX ? (b > a ? b : a) : a + b;
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = sm[k * kThreads];
}

// PASS 0: sum of x, y, z; 1: the six centred second moments; 2: max of |cloud_pca row|^2.  One partial per (scan, chunk).
template <class T, int PASS>
__global__ __launch_bounds__(kThreads) void k_m2dp_moments(const T* __restrict__ pts, int stride, const int64_t* __restrict__ offs,
                                                           const double* __restrict__ state, int cmax, double* __restrict__ part)
{
    __shared__ double sm[kThreads * kPart];
    const int b = blockIdx.y, c = blockIdx.x;
    const int64_t o0 = offs[b], n = offs[b + 1] - o0, i0 = (int64_t)c * kChunk;
    if (n < 3 || i0 >= n) return;
    const int64_t i1 = i0 + kChunk < n ? i0 + kChunk : n;
    const double* st = state + (size_t)b * kState;
    constexpr int K = PASS == 0 ? 3 : (PASS == 1 ? 6 : 1);
    double acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.0;
    for (int64_t i = i0 + threadIdx.x; i < i1; i += kThreads) {
        double x, y, z;
        load_point(pts, stride, o0 + i, x, y, z);
        if constexpr (PASS == 0) {
            acc[0] += x; acc[1] += y; acc[2] += z;
        } else if constexpr (PASS == 1) {
            const double dx = x - st[kMean], dy = y - st[kMean + 1], dz = z - st[kMean + 2];
            acc[0] += dx * dx; acc[1] += dx * dy; acc[2] += dx * dz; acc[3] += dy * dy; acc[4] += dy * dz; acc[5] += dz * dz;
        } else {
            double c0, c1, c2;
            rotate(st, x, y, z, c0, c1, c2);
            const double r2 = c0 * c0 + c1 * c1 + c2 * c2;
            acc[0] = r2 > acc[0] ? r2 : acc[0];
        }
    }
    block_reduce<K, PASS == 2>(acc, sm);
    if (threadIdx.x == 0) {
        double* out = part + ((size_t)b * cmax + c) * kPart;
#pragma unroll
        for (int k = 0; k < K; ++k) out[k] = acc[k];
    }
}

// one thread per scan: a scan's partials in chunk order -> its state
template <int PASS>
__global__ void k_m2dp_finish(const int64_t* __restrict__ offs, int batch, int cmax, const double* __restrict__ part, double* __restrict__ state)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    const int64_t n = offs[b + 1] - offs[b];
    double* st = state + (size_t)b * kState;
    if (n < 3) {
        if (PASS == 0)
            for (int k = 0; k < kState; ++k) st[k] = 0.0;
        return;
    }
    const int chunks = (int)((n + kChunk - 1) / kChunk);
    const double* p = part + (size_t)b * cmax * kPart;
    constexpr int K = PASS == 0 ? 3 : (PASS == 1 ? 6 : 1);
    double acc[K];
    for (int k = 0; k < K; ++k) acc[k] = 0.0;
    for (int c = 0; c < chunks; ++c)
        for (int k = 0; k < K; ++k) {
            const double v = p[(size_t)c * kPart + k];
            acc[k] = PASS == 2 ? (v > acc[k] ? v : acc[k]) : acc[k] + v;
        }
    if constexpr (PASS == 0) {
        for (int k = 0; k < 3; ++k) st[kMean + k] = acc[k] / (double)n;
    } else if constexpr (PASS == 1) {
        const double inv = 1.0 / (double)(n - 1);
        const double cov[9] = {acc[0] * inv, acc[1] * inv, acc[2] * inv, acc[1] * inv, acc[3] * inv, acc[4] * inv, acc[2] * inv, acc[4] * inv, acc[5] * inv};
        double w[3], v[9];
        mrs::sym3_eigvecs_desc(cov, w, v);
        for (int r = 0; r < 3; ++r) {           // svd_flip on the components: the largest-magnitude coefficient (the first of equals) positive
            int m = 0;
            for (int k = 1; k < 3; ++k)
                if (fabs(v[3 * r + k]) > fabs(v[3 * r + m])) m = k;
            const double sgn = v[3 * r + m] < 0.0 ? -1.0 : 1.0;
            for (int k = 0; k < 3; ++k) st[kRot + 3 * r + k] = sgn * v[3 * r + k];
            st[kEig + r] = w[r];
        }
    } else {
        const double max_rho = sqrt(acc[0]);
        st[kMaxRho] = max_rho;
        // rhoList = linspace(0, sqrt(maxRho), 9)^2: edge k = (k step)^2; a point's rho^2 is compared with the edge squared once more.  The
        // last edge (+ 0.001, above every rho) needs no comparison: the bin index stops at 7.
        const double step = sqrt(max_rho) / 8.0;
        st[kEdge] = 0.0;
        for (int k = 1; k < 8; ++k) {
            const double e = (k * step) * (k * step);
            st[kEdge + k] = e * e;
        }
    }
}

// The signature matrix.  grid (tiles, batch); counts int32 [batch][64][128], zeroed by the caller.
template <class T>
__global__ __launch_bounds__(kThreads) void k_m2dp_hist(const T* __restrict__ pts, int stride, const int64_t* __restrict__ offs,
                                                        const double* __restrict__ state, int* __restrict__ counts)
{
    __shared__ int hist[kPlanes * kHistStride];
    __shared__ double pt[kTile * 3];
    const int b = blockIdx.y, t = threadIdx.x;
    const int64_t o0 = offs[b], n = offs[b + 1] - o0, i0 = (int64_t)blockIdx.x * kTile;
    if (n < 3 || i0 >= n) return;
    const int m = (int)(i0 + kTile < n ? kTile : n - i0);          // points of this tile
    const double* st = state + (size_t)b * kState;
    for (int i = t; i < kPlanes * kHistStride; i += kThreads) hist[i] = 0;
    for (int i = t; i < m; i += kThreads) {
        double x, y, z, c0, c1, c2;
        load_point(pts, stride, o0 + i0 + i, x, y, z);
        rotate(st, x, y, z, c0, c1, c2);
        pt[3 * i] = c0; pt[3 * i + 1] = c1; pt[3 * i + 2] = c2;
    }
    // this lane's plane: azimuth linspace(-pi/2, pi/2, 4)[lane / 16], elevation linspace(0, pi/2, 16)[lane % 16]; normal vecN,
    // px = (1, 0, 0) - vecN.x vecN, py = vecN x px  (M2DP.py:54-70)
    const int lane = t & 63, wave = t >> 6;
    const int ai = lane >> 4, ei = lane & 15;
    const double half_pi = 1.5707963267948966;
    const double az = ai == 3 ? half_pi : ai * ((half_pi - -half_pi) / 3.0) + -half_pi;
    const double el = ei == 15 ? half_pi : ei * (half_pi / 15.0);
    const double nx = cos(el) * cos(az), ny = cos(el) * sin(az), nz = sin(el);
    const double px0 = 1.0 - nx * nx, px1 = 0.0 - nx * ny, px2 = 0.0 - nx * nz;
    const double py0 = ny * px2 - nz * px1, py1 = nz * px0 - nx * px2, py2 = nx * px1 - ny * px0;
    double e2[8];
#pragma unroll
    for (int k = 1; k < 8; ++k) e2[k] = st[kEdge + k];
    const double t1 = 0.41421356237309503, t3 = 2.414213562373095;   // tan(pi / 8), tan(3 pi / 8)
    __syncthreads();
    int* row = hist + lane * kHistStride;
    for (int i = wave; i < m; i += kThreads / 64) {
        const double c0 = pt[3 * i], c1 = pt[3 * i + 1], c2 = pt[3 * i + 2];       // one address per wave: LDS broadcast
        const double x = c0 * px0 + c1 * px1 + c2 * px2;
        const double y = c0 * py0 + c1 * py1 + c2 * py2;
        const double r2 = x * x + y * y;
        int rb = 0;
#pragma unroll
        for (int k = 1; k < 8; ++k) rb += r2 >= e2[k] ? 1 : 0;
        // theta = atan2(y, x) in 16 bins of pi / 8 from -pi: the angle within the quadrant by slope, then the quadrant
        const double ax = fabs(x), ay = fabs(y);
        const int sub = (ay >= ax * t1 ? 1 : 0) + (ay >= ax ? 1 : 0) + (ay >= ax * t3 ? 1 : 0);
        const bool xn = x < 0.0, yn = y < 0.0;
        const int tb = yn ? (xn ? sub : 7 - sub) : (xn ? 15 - sub : 8 + sub);
        atomicAdd(row + rb * 16 + tb, 1);
    }
    __syncthreads();
    int* out = counts + (size_t)b * kPlanes * kBins;
    for (int i = t; i < kPlanes * kBins; i += kThreads) {
        const int v = hist[(i >> 7) * kHistStride + (i & (kBins - 1))];
        if (v) atomicAdd(out + i, v);
    }
}

// Leading singular pair of the signature matrix.  One workgroup per scan; desc double [batch][192], A double [batch][64][128] or null.
__global__ __launch_bounds__(kThreads) void k_m2dp_svd(const int* __restrict__ counts, const int64_t* __restrict__ offs, double* __restrict__ desc,
                                                      double* __restrict__ A)
{
    __shared__ int cm[kPlanes * kHistStride];
    __shared__ double u[kPlanes], un[kPlanes], w[kBins], tmp[kThreads];
    const int b = blockIdx.x, t = threadIdx.x;
    const int64_t n = offs[b + 1] - offs[b];
    double* d = desc + (size_t)b * kDesc;
    double* a = A ? A + (size_t)b * kPlanes * kBins : nullptr;
    if (n < 3) {
        if (t < kDesc) d[t] = 0.0;
        if (a)
            for (int i = t; i < kPlanes * kBins; i += kThreads) a[i] = 0.0;
        return;
    }
    const int* c = counts + (size_t)b * kPlanes * kBins;
    for (int i = t; i < kPlanes * kBins; i += kThreads) {
        const int v = c[i];
        cm[(i >> 7) * kHistStride + (i & (kBins - 1))] = v;
        if (a) a[i] = (double)v / (double)n;                         // hist / cloud_pca.shape[0]
    }
    if (t < kPlanes) u[t] = 0.125;
    // u <- C C^T u / ||C C^T u||: the singular vectors of A = C / n are those of C.  C is non-negative, so the leading pair is too and the
    // all-positive start has a component along it.
    const double tol2 = 0x1p-96;                                     // (2^-48)^2: a few ulps per component, above the rounding floor of a step
    int extra = 0;
    bool zero = false;
    for (int it = 0; it < 2000; ++it) {
        __syncthreads();
        if (t < kBins) {
            double s = 0.0;
            for (int i = 0; i < kPlanes; ++i) s += (double)cm[i * kHistStride + t] * u[i];
            w[t] = s;
        }
        __syncthreads();
        {
            const int r = t >> 2, q = (t & 3) * 32;
            double s = 0.0;
            for (int k = 0; k < 32; ++k) s += (double)cm[r * kHistStride + q + k] * w[q + k];
            tmp[t] = s;
        }
        __syncthreads();
        if (t < kPlanes) un[t] = (tmp[4 * t] + tmp[4 * t + 1]) + (tmp[4 * t + 2] + tmp[4 * t + 3]);
        __syncthreads();
        double nrm2 = 0.0;
        for (int i = 0; i < kPlanes; ++i) nrm2 += un[i] * un[i];    // the same sum in every thread
        if (!(nrm2 > 0.0) || !(nrm2 < INFINITY)) { zero = true; break; }
        const double inv = 1.0 / sqrt(nrm2);
        if (t < kPlanes) {
            const double v = un[t] * inv, dd = v - u[t];
            tmp[t] = dd * dd;
            u[t] = v;
        }
        __syncthreads();
        double step2 = 0.0;
        for (int i = 0; i < kPlanes; ++i) step2 += tmp[i];
        if (step2 <= tol2 && ++extra > 6) break;
    }
    __syncthreads();
    if (t < kBins) {
        double s = 0.0;
        for (int i = 0; i < kPlanes; ++i) s += (double)cm[i * kHistStride + t] * u[i];
        w[t] = s;
    }
    __syncthreads();
    double wn2 = 0.0, su = 0.0;
    for (int k = 0; k < kBins; ++k) wn2 += w[k] * w[k];
    for (int i = 0; i < kPlanes; ++i) su += u[i];
    zero = zero || !(wn2 > 0.0) || !(wn2 < INFINITY);
    const double sgn = su < 0.0 ? -1.0 : 1.0;                        // the product's sign rule: sum(u0) >= 0
    const double winv = zero ? 0.0 : sgn / sqrt(wn2);
    if (t < kPlanes) d[t] = zero ? 0.0 : sgn * u[t];
    if (t < kBins) d[kPlanes + t] = w[t] * winv;
}

template <class T>
void launch_moments(int pass, const T* p, int stride, const int64_t* d_offs, const double* state, int cmax, int batch, double* part, hipStream_t s)
{
    const dim3 grid(cmax, batch), block(kThreads);
    if (pass == 0) hipLaunchKernelGGL((k_m2dp_moments<T, 0>), grid, block, 0, s, p, stride, d_offs, state, cmax, part);
    else if (pass == 1) hipLaunchKernelGGL((k_m2dp_moments<T, 1>), grid, block, 0, s, p, stride, d_offs, state, cmax, part);
    else hipLaunchKernelGGL((k_m2dp_moments<T, 2>), grid, block, 0, s, p, stride, d_offs, state, cmax, part);
}

// d_desc null: the PCA stage only (d_pca set)
template <class T>
int m2dp_impl(const T* p, int stride, const int64_t* d_offs, int64_t longest, int batch, double* d_desc, double* d_A, double* d_pca, hipStream_t s)
{
    const int cmax = (int)std::max<int64_t>(1, (longest + kChunk - 1) / kChunk);
    const int tiles = (int)std::max<int64_t>(1, (longest + kTile - 1) / kTile);
    mrs::Scratch state, part, counts;
    int st = state.alloc((size_t)batch * kState * sizeof(double), s);
    if (st != MRS_OK) return st;
    if ((st = part.alloc((size_t)batch * cmax * kPart * sizeof(double), s)) != MRS_OK) return st;
    const dim3 fgrid((batch + 63) / 64), fblock(64);
    launch_moments(0, p, stride, d_offs, state.as<double>(), cmax, batch, part.as<double>(), s);
    hipLaunchKernelGGL(k_m2dp_finish<0>, fgrid, fblock, 0, s, d_offs, batch, cmax, part.as<double>(), state.as<double>());
    launch_moments(1, p, stride, d_offs, state.as<double>(), cmax, batch, part.as<double>(), s);
    hipLaunchKernelGGL(k_m2dp_finish<1>, fgrid, fblock, 0, s, d_offs, batch, cmax, part.as<double>(), state.as<double>());
    launch_moments(2, p, stride, d_offs, state.as<double>(), cmax, batch, part.as<double>(), s);
    hipLaunchKernelGGL(k_m2dp_finish<2>, fgrid, fblock, 0, s, d_offs, batch, cmax, part.as<double>(), state.as<double>());
    MRS_HIP_TRY(hipGetLastError());
    if (d_pca)
        MRS_HIP_TRY(hipMemcpy2DAsync(d_pca, 16 * sizeof(double), state.p, kState * sizeof(double), 16 * sizeof(double), batch,
                                     hipMemcpyDeviceToDevice, s));
    if (!d_desc) return MRS_OK;
    const size_t cbytes = (size_t)batch * kPlanes * kBins * sizeof(int);
    if ((st = counts.alloc(cbytes, s)) != MRS_OK) return st;
    MRS_HIP_TRY(hipMemsetAsync(counts.p, 0, cbytes, s));
    hipLaunchKernelGGL(k_m2dp_hist<T>, dim3(tiles, batch), dim3(kThreads), 0, s, p, stride, d_offs, state.as<double>(), counts.as<int>());
    hipLaunchKernelGGL(k_m2dp_svd, dim3(batch), dim3(kThreads), 0, s, counts.as<int>(), d_offs, d_desc, d_A);
    MRS_HIP_TRY(hipGetLastError());
    return MRS_OK;
}

int m2dp_entry(mrs_ctx* ctx, const void* d_points, int32_t is_double, int32_t stride, const int64_t* d_offsets, const int64_t* h_offsets,
               int32_t batch, double* d_desc, double* d_A, double* d_pca, mrs_stream stream)
{
    MRS_REQUIRE(ctx && d_offsets && h_offsets && (d_desc || d_pca), "null pointer");
    MRS_REQUIRE(batch > 0 && batch <= mrs::kMaxGridY && stride >= 3, "batch must be within [1, 65535] and stride >= 3");
    int64_t longest = 0;
    for (int b = 0; b < batch; ++b) {
        MRS_REQUIRE(h_offsets[b + 1] >= h_offsets[b], "offsets must be non-decreasing");
        longest = std::max(longest, h_offsets[b + 1] - h_offsets[b]);
    }
    MRS_REQUIRE(h_offsets[0] >= 0 && longest < (1ll << 31), "fewer than 2^31 points per cloud");
    MRS_REQUIRE(d_points || longest == 0, "null pointer");
    MRS_HIP_TRY(hipSetDevice(ctx->device));
    return is_double ? m2dp_impl<double>((const double*)d_points, stride, d_offsets, longest, batch, d_desc, d_A, d_pca, (hipStream_t)stream)
                     : m2dp_impl<float>((const float*)d_points, stride, d_offsets, longest, batch, d_desc, d_A, d_pca, (hipStream_t)stream);
}

}  // namespace

extern "C" {

int mrs_m2dp_batch(mrs_ctx* ctx, const void* d_points, int32_t is_double, int32_t stride, const int64_t* d_offsets, const int64_t* h_offsets,
                   int32_t batch, double* d_desc, double* d_A, mrs_stream stream)
{
    MRS_REQUIRE(d_desc, "null pointer");
    return m2dp_entry(ctx, d_points, is_double, stride, d_offsets, h_offsets, batch, d_desc, d_A, nullptr, stream);
}

int mrs_m2dp_pca_batch(mrs_ctx* ctx, const void* d_points, int32_t is_double, int32_t stride, const int64_t* d_offsets, const int64_t* h_offsets,
                       int32_t batch, double* d_pca, mrs_stream stream)
{
    MRS_REQUIRE(d_pca, "null pointer");
    return m2dp_entry(ctx, d_points, is_double, stride, d_offsets, h_offsets, batch, nullptr, nullptr, d_pca, stream);
}

int mrs_m2dp_host(mrs_ctx* ctx, const void* h_points, int32_t is_double, int32_t stride, int32_t n, double* h_desc, double* h_A)
{
    MRS_REQUIRE(ctx && h_desc && (h_points || n == 0), "null pointer");
    MRS_REQUIRE(n >= 0 && stride >= 3, "n must not be negative and stride >= 3");
    if (n < 3) {                                                    // M2DP.py:100-109: zeros, no device work
        memset(h_desc, 0, kDesc * sizeof(double));
        if (h_A) memset(h_A, 0, (size_t)kPlanes * kBins * sizeof(double));
        return MRS_OK;
    }
    MRS_HIP_TRY(hipSetDevice(ctx->device));
    const size_t in_bytes = (size_t)n * stride * (is_double ? 8 : 4);
    const size_t out_doubles = kDesc + (size_t)kPlanes * kBins;
    mrs::Scratch in, out, offs;
    int st = in.alloc(in_bytes, nullptr);
    if (st != MRS_OK) return st;
    if ((st = out.alloc(out_doubles * sizeof(double), nullptr)) != MRS_OK) return st;
    if ((st = offs.alloc(2 * sizeof(int64_t), nullptr)) != MRS_OK) return st;
    const int64_t h_offs[2] = {0, n};
    MRS_HIP_TRY(hipMemcpy(in.p, h_points, in_bytes, hipMemcpyHostToDevice));
    MRS_HIP_TRY(hipMemcpy(offs.p, h_offs, sizeof(h_offs), hipMemcpyHostToDevice));
    st = mrs_m2dp_batch(ctx, in.p, is_double, stride, offs.as<int64_t>(), h_offs, 1, out.as<double>(), h_A ? out.as<double>() + kDesc : nullptr, nullptr);
    if (st != MRS_OK) return st;
    MRS_HIP_TRY(hipMemcpy(h_desc, out.p, kDesc * sizeof(double), hipMemcpyDeviceToHost));
    if (h_A) MRS_HIP_TRY(hipMemcpy(h_A, out.as<double>() + kDesc, (size_t)kPlanes * kBins * sizeof(double), hipMemcpyDeviceToHost));
    return MRS_OK;
}

}  // extern "C"
