// gicp_device.hpp -- device code of the batched GICP refinement for gfx950: constants, kernel-argument structs
// and kernels.  Included by gicp.hip only (handle, launch helpers and C entry points), so everything stays in one translation unit.
//
// Behaviour reproduced: fast_gicp's FastGICP (un-vendored submodule of the reference; algorithm
// per SURVEY.md App. A.2) as configured at Mapping/src/global_manager/src/global_manager.cpp:
// 2435-2443 and LoopDetection/src/RING_ros/main_RING.py:81-104:
//   G2 calculate_covariances : kNN (k) in the own cloud, covariance of the neighbours (double),
//                              PLANE regularisation U diag(1,1,1e-3) V^T == I - 0.999 n n^T
//   G3 update_correspondences: 1-NN of the float-transformed source point, reject d^2 >= max^2,
//                              M_i = (C_B + R C_A R^T)^-1
//   G4 linearize             : e = b - T a, J = [skew(T a) | -I], H += J^T M J, b += J^T M e
//   G5 LM optimiser          : LsqRegistration::step_lm / is_converged / se3_exp
//   G6 getFitnessScore       : mean squared NN distance with d^2 <= max_range
//
// Design: kd-tree-free.  Every nearest-neighbour query is an exact brute-force scan: target
// points are staged through LDS in tiles of 1024 float4 and read back as wave-wide broadcasts
// (one ds_read_b128 per candidate per wave), four source points per lane, ~7 VALU ops per
// (source, target) pair; at 120k x 120k the un-culled scan runs at ~95 % of the VALU issue peak.
// Both clouds are stored in Morton order (rocPRIM radix sort at set_clouds time), so a tile of 1024
// consecutive points is spatially compact and carries an axis-aligned bounding box: a workgroup
// (1024 consecutive, i.e. equally compact, queries; a wave owns 4 x 64 consecutive ones) visits the tiles
// in order of increasing box-to-box distance, stops at the first tile beyond its largest search radius,
// and inside a staged tile every wave skips the 128- and 16-candidate sub-tiles (boxes built while
// staging) that none of its lanes can use.  Every query starts from the neighbour it had in the previous
// pass (any target point is an upper bound).  The culling is conservative, so the neighbours are still
// the exact ones.  The scan is VALU-bound (7 lane-ops per surviving (source, target) pair);
// the per-point 3x3 algebra and the 28-term fp64 reductions (wave __shfl butterflies -> one
// partial per workgroup -> fixed-order final sum) are noise next to it.  All pairs of a batch
// advance together; the Levenberg-Marquardt bookkeeping runs on the device (one lane per
// pair), so the host only polls two counters (pairs to linearise, pairs in an LM trial).
// LM trial semantics are upstream's: linearize(x0) is the only step that searches (one NN pass per
// outer iteration); every trial pose delta * x0 is scored by compute_error, i.e. on the cached
// correspondences with the Mahalanobis matrices of the linearisation pose (recomputed on the fly
// from x0 -- the same values, cheaper than storing 48 B per point).
#pragma once
#include <cfloat>
#include <cmath>

#include "common.hpp"
#include "nn_core.hpp"
#include "eig3.hpp"

namespace {

constexpr int kTile = 1024;      // target points per LDS tile
constexpr int kNNThreads = 256;  // lanes per workgroup
constexpr int kPts = 4;          // source points per lane
constexpr int kTerms = 28;       // 21 (H upper) + 6 (b) + 1 (error)

struct LmState {
    double x[16];      // accepted pose (row-major 4x4) = linearisation pose of the current outer iteration
    double xi[16];     // pose being evaluated: == x while linearising (phase 0), the LM candidate in phase 1
    double delta[16];  // last increment
    double H[36];      // linearisation at x
    double b[6];
    double d[6];       // last LM step
    double y0;
    double lambda;
    double nu;
    double final_H[36];
    int phase;         // 0: linearize at x (NN search + H, b, y0), 1: LM trial (compute_error at xi), 2: done
    int inner;
    int outer;
    int trials;
    int converged;
    int failed;
    int active;
    int pad;
};

struct GicpParams {
    double max_corr2;     // squared correspondence distance threshold (inf if unbounded)
    double rot_eps, trans_eps;
    double conv_factor;   // upstream is_converged: factor 10 on both scaled deltas
    double lm_init_factor;
    int max_iter;
    int lm_max_iter;
    int force_iters;      // >0: run exactly this many outer iterations, no convergence test
    int k;
    double voxel_res;     // > 0: VGICP (voxelised target, G7); 0: GICP
    int voxel_neighbors;  // 1, 7 or 27 (DIRECT1 / DIRECT7 / DIRECT27)
    float cert_margin;    // metres the round-4 search looks beyond the neighbour it found (what later passes certify against)
    float motion_switch;  // round-4 schedule: a pair whose last step moved it farther than this (metres) is searched by the round-3 kernel
    int pad2;
};

// How far the last accepted LM increment moved the source cloud: |translation| + rotation angle x 60 m (metres, an upper estimate for
// points within 60 m of the origin).  Decides which search a pair gets in the round-4 schedule (nn_pass).
__device__ __forceinline__ float pair_motion(const LmState& S)
{
    const double tx = S.delta[3], ty = S.delta[7], tz = S.delta[11];
    const double c = fmin(fmax(0.5 * (S.delta[0] + S.delta[5] + S.delta[10] - 1.0), -1.0), 1.0);
    return (float)(sqrt(tx * tx + ty * ty + tz * tz) + 60.0 * sqrt(fmax(2.0 - 2.0 * c, 0.0)));
}

__device__ __forceinline__ double wave_sum_d(double v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ float dist2(float qx, float qy, float qz, const float4& b)
{
    const float dx = qx - b.x, dy = qy - b.y, dz = qz - b.z;
    return __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
}

// PLANE regularisation (the only one implemented, fast_gicp's default): C = U diag(1, 1, 1e-3) V^T = I - 0.999 n n^T with n the unit normal.
// The library keeps n (3 doubles, 24 B per point) instead of the 6 doubles of C: every reader rebuilds C with THESE expressions (fp64,
// no contraction: -ffp-contract=off), i.e. the very doubles the covariance kernels used to store -- half the bytes k_linearize streams and gathers.
constexpr int kCovDoubles = 3;
__host__ __device__ __forceinline__ void cov6_from_normal(const double* __restrict__ n, double (&c)[6])
{
    const double n0 = n[0], n1 = n[1], n2 = n[2];
    c[0] = 1.0 - 0.999 * n0 * n0;
    c[1] = -0.999 * n0 * n1;
    c[2] = -0.999 * n0 * n2;
    c[3] = 1.0 - 0.999 * n1 * n1;
    c[4] = -0.999 * n1 * n2;
    c[5] = 1.0 - 0.999 * n2 * n2;
}

// Bounding boxes of the Morton-ordered cloud at two granularities, in global memory (built once per set_clouds by k_boxes):
//   tile t  = points [1024 t, 1024 t + 1024),  mini 64 t + m = points [1024 t + 16 m, + 16)   (slots past the cloud: empty boxes, lo = +inf, hi = -inf)
struct Hier {
    const float4* tlo;  // [ntiles]
    const float4* thi;
    const float4* mlo;  // [64 * ntiles]
    const float4* mhi;
    int ntiles;
};

__device__ __forceinline__ float box_point_d2(const float4& lo, const float4& hi, float x, float y, float z)
{
    const float dx = fmaxf(fmaxf(lo.x - x, x - hi.x), 0.0f);
    const float dy = fmaxf(fmaxf(lo.y - y, y - hi.y), 0.0f);
    const float dz = fmaxf(fmaxf(lo.z - z, z - hi.z), 0.0f);
    return dx * dx + dy * dy + dz * dz;
}

// lower bound of the squared distance between any point of box (lo, hi) and any point of box (qlo, qhi)
__device__ __forceinline__ float box_box_d2(const float4& lo, const float4& hi, const float (&qlo)[3], const float (&qhi)[3])
{
    const float dx = fmaxf(fmaxf(lo.x - qhi[0], qlo[0] - hi.x), 0.0f);
    const float dy = fmaxf(fmaxf(lo.y - qhi[1], qlo[1] - hi.y), 0.0f);
    const float dz = fmaxf(fmaxf(lo.z - qhi[2], qlo[2] - hi.z), 0.0f);
    return dx * dx + dy * dy + dz * dz;
}

// bounding box of a wave's live queries (every lane returns the same values; +inf / -inf without live queries)
__device__ __forceinline__ void wave_bbox(float (&lo)[3], float (&hi)[3])
{
#pragma unroll
    for (int a = 0; a < 3; ++a)
        for (int o = 32; o > 0; o >>= 1) {
            lo[a] = fminf(lo[a], __shfl_xor(lo[a], o, 64));
            hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], o, 64));
        }
}

__device__ __forceinline__ float wave_max(float v)
{
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// ---- the traversal of the k-NN selection ------------------------------------------------------------------------------------------
// No LDS tile, no workgroup barrier: a WAVE (its queries are 64 consecutive Morton-ordered points, i.e. spatially compact) walks the
// two-level box hierarchy on its own.  What bounded the round-3 / round-4 form of this walk (one bounding box per wave, a per-mini test, then
// the mini's candidates) was not arithmetic but the LENGTH OF ITS DEPENDENCY CHAINS: a workgroup of k_knn_cov<30> lived 0.9 ms (0.55 ms now)
// because every mini cost two dependent round trips to the L2 (its box -> test -> its 16 candidates -> distances), taken one after the other.
// And a wave whose 64 queries straddle a jump of the Morton curve has a bounding box the size of the scene: tested against THAT box, every mini
// of the cloud passed the coarse test and was then rejected one round trip at a time -- 3 ms for one wave, the tail of the whole launch.
//   * coarse tests against QUAD boxes: the queries of 4 consecutive lanes share a box and a bound (16 per wave; a jump of the curve
//     spoils one of them, not the wave).  Lane l tests tile / mini l against the 16 quads (v_readlane broadcasts, ~20 VALU instructions
//     per quad): one ballot per 64 boxes and NO per-mini test afterwards -- whatever passes is evaluated;
//   * tiles nearest first (smallest box distance to any quad) inside a chunk of 64 tiles, the chunk of the wave's own tile first; the
//     bounds are asked again before every tile (`bound()`), so a lane whose seed was poor holds the walk only until its neighbours' tile
//     has been seen;
//   * the 16 candidates of a mini arrive by scalar loads in two halves, the next half REQUESTED BEFORE the current one is evaluated
//     (scalar loads return out of order, so only lgkmcnt(0) exists: an empty asm that reads one register of the current half makes the
//     compiler wait for it before the next requests are issued -- everything outstanding during the arithmetic belongs to the next half).
// Conservative at every level (0.9999 slack on the box distances), so the neighbours found are the exact ones.
#ifndef MRS_KNN_QUAD
#define MRS_KNN_QUAD 4
#endif
constexpr int kQL = MRS_KNN_QUAD;        // lanes per group of the coarse tests (4: "quads"; 8 was measured: see DESIGN.md 4)
constexpr int kQG = 64 / kQL;
__device__ __forceinline__ float lane_f(float v, int l) { return __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(v), l)); }
__device__ __forceinline__ float first_f(float v) { return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(v))); }

// box of the live queries of this lane's group of 4 consecutive lanes (empty: +inf / -inf)
__device__ __forceinline__ void quad_box(bool live, const float4& q, float (&lo)[3], float (&hi)[3])
{
    lo[0] = live ? q.x : INFINITY; lo[1] = live ? q.y : INFINITY; lo[2] = live ? q.z : INFINITY;
    hi[0] = live ? q.x : -INFINITY; hi[1] = live ? q.y : -INFINITY; hi[2] = live ? q.z : -INFINITY;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int o = 1; o < kQL; o <<= 1) {
            lo[a] = fminf(lo[a], __shfl_xor(lo[a], o, 64));
            hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], o, 64));
        }
}
__device__ __forceinline__ float quad_max(float v)
{
#pragma unroll
    for (int o = 1; o < kQL; o <<= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// does THIS lane's box (blo, bhi) come within the bound of any query of the wave?  16 quad tests (box against the quad's box and largest
// bound); a quad in `wide` (its box is larger than its bound: the 4 points straddle a jump of the Morton curve, and everything between the
// two ends of the jump would "touch" the box) is tested query by query instead.  dmin: the smallest distance seen.
__device__ __forceinline__ bool quads_hit(const float4& blo, const float4& bhi, const float (&qlo)[3], const float (&qhi)[3], float qT,
                                          unsigned wide, const float4& q, float T, float& dmin)
{
    bool hit = false;
    dmin = INFINITY;
#pragma unroll
    for (int g = 0; g < kQG; ++g) {
        if (wide >> g & 1) {        // wave-uniform
#pragma unroll
            for (int l = kQL * g; l < kQL * g + kQL; ++l) {
                const float d = box_point_d2(blo, bhi, lane_f(q.x, l), lane_f(q.y, l), lane_f(q.z, l));
                hit |= d * 0.9999f <= lane_f(T, l);         // a dead lane's T is -1
                dmin = fminf(dmin, lane_f(T, l) >= 0.0f ? d : INFINITY);
            }
        } else {
            const float l[3] = {lane_f(qlo[0], kQL * g), lane_f(qlo[1], kQL * g), lane_f(qlo[2], kQL * g)};
            const float h[3] = {lane_f(qhi[0], kQL * g), lane_f(qhi[1], kQL * g), lane_f(qhi[2], kQL * g)};
            const float d = box_box_d2(blo, bhi, l, h);
            hit |= d * 0.9999f <= lane_f(qT, kQL * g);
            dmin = fminf(dmin, d);
        }
    }
    return hit;
}

// quads whose box is larger than their bound (bit g: lanes 4g .. 4g + 3)
__device__ __forceinline__ unsigned wide_quads(const float (&qlo)[3], const float (&qhi)[3], float qT)
{
    const float ex = qhi[0] - qlo[0], ey = qhi[1] - qlo[1], ez = qhi[2] - qlo[2];
    const bool w = ex * ex + ey * ey + ez * ez > qT;           // (an empty quad: -inf extents, inf > -1: tested lane by lane, every lane dead)
    const unsigned long long m = __ballot(w);
    unsigned out = 0;
#pragma unroll
    for (int g = 0; g < kQG; ++g) out |= (unsigned)(m >> (kQL * g) & 1ull) << g;
    return out;
}

struct Cand8 { float4 c[8]; };
__device__ __forceinline__ void cand_request(Cand8& o, const float4* __restrict__ pts, int j0)       // wave-uniform j0: scalar loads
{
#pragma unroll
    for (int u = 0; u < 8; ++u) o.c[u] = pts[j0 + u];       // 128 contiguous bytes; past the cloud's end: the next cloud's points or the 16 points of
                                                            // slack behind the last one (prepare_side), masked in cand_dist
    asm volatile("" ::: "memory");        // the requests stay where they are written
}
__device__ __forceinline__ void cand_arrived(const Cand8& a)
{
    // a use of the half: the compiler's s_waitcnt lgkmcnt(0) lands HERE, before the next requests.  The .w lanes (never read by the arithmetic)
    // are named too: left dead, the register allocator hands them out as scratch while the loads are in flight, and every such write
    // costs a wait for everything outstanding
    asm volatile("" ::"s"(a.c[0].x), "s"(a.c[0].w), "s"(a.c[1].w), "s"(a.c[2].w), "s"(a.c[3].w), "s"(a.c[4].w), "s"(a.c[5].w), "s"(a.c[6].w), "s"(a.c[7].w) : "memory");
}
__device__ __forceinline__ void cand_dist(const Cand8& a, int j0, int n, float qx, float qy, float qz, float (&dd)[8])
{
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const float dx = qx - a.c[u].x, dy = qy - a.c[u].y, dz = qz - a.c[u].z;
        dd[u] = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
    }
    if (j0 + 8 > n) {           // the cloud's last points (wave-uniform): what was read beyond them does not exist
#pragma unroll
        for (int u = 0; u < 8; ++u) dd[u] = j0 + u < n ? dd[u] : INFINITY;
    }
}

// the candidates of the minis `ids(r)`, r = 0 .. count - 1 (wave-uniform), 8 at a time: visit(first index, the 8 candidates).  The visitor
// starts with cand_pin() on a coordinate of its query: its arithmetic then stays behind the requests for the next 8.
__device__ __forceinline__ void cand_pin(float& x) { asm volatile("" : "+v"(x)); }      // (volatile asm statements keep their order)
template <class Ids, class Visit>
__device__ __forceinline__ void stream_minis(const float4* __restrict__ pts, int count, Ids ids, Visit visit)
{
    if (count <= 0) return;
    Cand8 A, B;
    int j0 = ids(0) * 16;
    cand_request(A, pts, j0);
    for (int r = 0; r < count; ++r) {
        cand_arrived(A);
        cand_request(B, pts, j0 + 8);
        visit(j0, A);
        cand_arrived(B);
        const int jn = r + 1 < count ? ids(r + 1) * 16 : j0;
        if (r + 1 < count) cand_request(A, pts, jn);
        visit(j0 + 8, B);
        j0 = jn;
    }
}

// Walk of the hierarchy for the 64 queries of a wave.  bound(): the lane's current bound (called by the whole wave before every tile; it may
// do wave-wide bookkeeping first); a dead lane's bound is ignored.  visit(first index, 8 candidates): see stream_minis.  NEAREST: tiles nearest
// first (pass 1: bounds shrink); otherwise tiles and minis in index order (pass 2 without the list of pass 1: candidates must arrive in
// ascending index order).  rec(id): every mini visited.
template <bool NEAREST, class Bound, class Visit, class Rec>
__device__ __forceinline__ void knn_walk(const float4* __restrict__ pts, int n, const Hier& H, bool live, const float4& q, int home_tile,
                                         Bound bound, Visit visit, Rec rec)
{
    const int lane = threadIdx.x & 63;
    float qlo[3], qhi[3];
    quad_box(live, q, qlo, qhi);
    const int nchunks = (H.ntiles + 63) >> 6;
    const int hc = min(home_tile, H.ntiles - 1) >> 6;
    for (int ci = 0; ci < nchunks; ++ci) {
        const int ch = !NEAREST ? ci : (ci == 0 ? hc : (ci <= hc ? ci - 1 : ci));       // NEAREST: the chunk of the wave's own tile first
        const int t = ch * 64 + lane;
        float T = bound();
        T = live ? T : -1.0f;
        float qT = quad_max(T);
        unsigned wide = wide_quads(qlo, qhi, qT);
        float key = INFINITY;           // box distance of a tile still to be visited; +inf: not (or no longer) a candidate
        {
            const int tc = min(t, H.ntiles - 1);
            float dmin;
            const bool hit = quads_hit(H.tlo[tc], H.thi[tc], qlo, qhi, qT, wide, q, T, dmin);
            if (hit && t < H.ntiles) key = dmin;
        }
        unsigned long long tmask = __ballot(key < INFINITY);
        while (tmask) {
            int tl;
            if (NEAREST) {
                float best = key;
                for (int o = 32; o > 0; o >>= 1) best = fminf(best, __shfl_xor(best, o, 64));
                best = first_f(best);
                tl = (int)__builtin_ctzll(__ballot(key == best));
                T = bound();
                T = live ? T : -1.0f;
                qT = quad_max(T);
                wide = wide_quads(qlo, qhi, qT);
                if (!(best * 0.9999f <= first_f(wave_max(T)))) break;        // every tile left is at least as far from every query
            } else {
                tl = (int)__builtin_ctzll(tmask);
            }
            tmask &= ~(1ull << tl);
            if (lane == tl) key = INFINITY;
            const int tt = ch * 64 + tl;
            float dmin;
            const bool mh = quads_hit(H.mlo[tt * 64 + lane], H.mhi[tt * 64 + lane], qlo, qhi, qT, wide, q, T, dmin);
            // (minis past the cloud's end have empty boxes, at distance +inf -- which an infinite bound, a cloud smaller than k, would accept)
            const unsigned long long mmask = __ballot(mh && (tt * 64 + lane) * 16 < n);
            const int cnt = __builtin_popcountll(mmask);
            unsigned long long left = mmask;         // ids(r) is asked for r = 0, 1, 2, ... in turn
            stream_minis(pts, cnt, [&](int) { const int m = (int)__builtin_ctzll(left); left &= left - 1; rec(tt * 64 + m); return tt * 64 + m; }, visit);
        }
    }
}

// Exact 1-NN of P query points per lane over the Morton-ordered cloud tgt[0..m): squared distance and (sorted-space) index; `maxc2` is
// the rejection radius (inf = none).  seed: any valid target index per query (last pass's neighbour, or the Morton seed of a cold
// start): its distance is the initial bound.  Waves are independent (no barrier inside).
constexpr int kNNRejMax = 256;     // minis a wave of nn_scan may reject before it changes to the quad-box walk
template <int P>
__device__ __forceinline__ void nn_scan(const float4* __restrict__ tgt, int m, const Hier& H, float maxc2,
                                        const float (&qx)[P], const float (&qy)[P], const float (&qz)[P],
                                        const bool (&live)[P], float (&best)[P], int (&bidx)[P], const int (&seed)[P])
{
    int grp[P];
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    float r = 0.0f;
#pragma unroll
    for (int p = 0; p < P; ++p) {
        best[p] = INFINITY; grp[p] = -1;
        if (live[p]) {
            lo[0] = fminf(lo[0], qx[p]); hi[0] = fmaxf(hi[0], qx[p]);
            lo[1] = fminf(lo[1], qy[p]); hi[1] = fmaxf(hi[1], qy[p]);
            lo[2] = fminf(lo[2], qz[p]); hi[2] = fmaxf(hi[2], qz[p]);
            // warm start: any target point is an upper bound; last pass's neighbour is nearly always the winner
            if (seed[p] >= 0 && seed[p] < m) { best[p] = dist2(qx[p], qy[p], qz[p], tgt[seed[p]]); grp[p] = seed[p] & ~7; }
            r = fmaxf(r, fminf(best[p], maxc2));
        }
    }
    wave_bbox(lo, hi);
    const float reach = wave_max(r);
    // the P queries of a lane share one traversal: `need` / `visit` loop over them
    auto need = [&](const float4& blo, const float4& bhi) {
        bool w = false;
#pragma unroll
        for (int p = 0; p < P; ++p) w |= live[p] && box_point_d2(blo, bhi, qx[p], qy[p], qz[p]) * 0.9999f <= fminf(best[p], maxc2);
        return w;
    };
    const int lane = threadIdx.x & 63;
    // A wave whose queries straddle a jump of the Morton curve has a box the size of the scene: every mini passes the two coarse tests and is
    // then rejected by `need`, one dependent round trip each (such a workgroup lived 1.4 ms, the median one 0.08 ms: the tail of every
    // launch, and most of a small one).  The walk counts its rejections; past kNNRejMax it is abandoned for the k-NN selection's walk
    // (quad boxes, per-query tests at the jump, nearest tile first), which starts over with the bounds found so far.
    int rejected = 0;
    for (int tb = 0; tb < H.ntiles && rejected <= kNNRejMax; tb += 64) {
        const int t = tb + lane;
        bool hit = false;
        if (t < H.ntiles) hit = box_box_d2(H.tlo[t], H.thi[t], lo, hi) * 0.9999f <= reach;
        unsigned long long tmask = __ballot(hit);
        while (tmask && rejected <= kNNRejMax) {
            const int tt = tb + (int)__builtin_ctzll(tmask);
            tmask &= tmask - 1;
            const bool mhit = box_box_d2(H.mlo[tt * 64 + lane], H.mhi[tt * 64 + lane], lo, hi) * 0.9999f <= reach;
            unsigned long long mmask = __ballot(mhit);
            while (mmask) {
                const int mm = (int)__builtin_ctzll(mmask);
                mmask &= mmask - 1;
                if (!__any(need(H.mlo[tt * 64 + mm], H.mhi[tt * 64 + mm]))) { ++rejected; continue; }
                const int j0 = tt * kTile + mm * 16;
                float4 c16[16];        // all 16 candidates requested before the first use (wave-uniform addresses: scalar loads)
#pragma unroll
                for (int u = 0; u < 16; ++u) c16[u] = j0 + u < m ? tgt[j0 + u] : make_float4(INFINITY, INFINITY, INFINITY, 0.f);
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const float4* c = c16 + 8 * h;
#pragma unroll
                    for (int p = 0; p < P; ++p) {
                        float d[8];
#pragma unroll
                        for (int u = 0; u < 8; ++u) d[u] = dist2(qx[p], qy[p], qz[p], c[u]);
                        const float mn = fminf(fminf(fminf(d[0], d[1]), fminf(d[2], d[3])), fminf(fminf(d[4], d[5]), fminf(d[6], d[7])));
                        if (mn < best[p]) { best[p] = mn; grp[p] = j0 + 8 * h; }
                    }
                }
            }
        }
    }
    if (rejected > kNNRejMax) {
#pragma unroll
        for (int p = 0; p < P; ++p) {
            const float4 q = make_float4(qx[p], qy[p], qz[p], 0.f);
            const int home_tile = __builtin_amdgcn_readfirstlane(max(seed[p], 0)) >> 10;
            knn_walk<true>(tgt, m, H, live[p], q, home_tile, [&]() { return fminf(best[p], maxc2); },
                           [&](int j0, const Cand8& cand) {
                               float x = q.x, d[8];
                               cand_pin(x);
                               cand_dist(cand, j0, m, x, q.y, q.z, d);
                               const float mn = fminf(fminf(fminf(d[0], d[1]), fminf(d[2], d[3])), fminf(fminf(d[4], d[5]), fminf(d[6], d[7])));
                               if (live[p] && mn < best[p]) { best[p] = mn; grp[p] = j0; }
                           },
                           [](int) {});
        }
    }
    // resolve the index inside the winning group of 8
#pragma unroll
    for (int p = 0; p < P; ++p) {
        bidx[p] = -1;
        if (grp[p] >= 0) {
            for (int u = 7; u >= 0; --u) {
                const int j = grp[p] + u;
                if (j < m && dist2(qx[p], qy[p], qz[p], tgt[j]) == best[p]) bidx[p] = j;
            }
        }
    }
}

// ---- Morton ordering of the clouds (set_clouds) ------------------------------------------------
__device__ __forceinline__ int float_to_ordered(float f)
{
    const int i = __float_as_int(f);
    return i >= 0 ? i : i ^ 0x7fffffff;
}
__device__ __forceinline__ float ordered_to_float(int i) { return __int_as_float(i >= 0 ? i : i ^ 0x7fffffff); }

// per-cloud bounding box: bbox[c] = {min x,y,z, max x,y,z} as ordered ints (pre-set to +-max)
__global__ void k_cloud_bbox(const float* __restrict__ src, int stride, const int64_t* __restrict__ offs, int* __restrict__ bbox)
{
    const int c = blockIdx.y;
    const int64_t o = offs[c];
    const int n = (int)(offs[c + 1] - o);
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float* p = src + (size_t)(o + i) * stride;
#pragma unroll
        for (int a = 0; a < 3; ++a) { lo[a] = fminf(lo[a], p[a]); hi[a] = fmaxf(hi[a], p[a]); }
    }
    // wave butterflies -> one partial per wave in LDS -> ONE set of atomics per workgroup (six hot addresses per cloud)
    __shared__ float red[4][6];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        for (int s = 32; s > 0; s >>= 1) {
            lo[a] = fminf(lo[a], __shfl_xor(lo[a], s, 64));
            hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], s, 64));
        }
        if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][a] = lo[a]; red[threadIdx.x >> 6][3 + a] = hi[a]; }
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const int a = threadIdx.x;
        if (a < 3)
            atomicMin(&bbox[6 * c + a], float_to_ordered(fminf(fminf(red[0][a], red[1][a]), fminf(red[2][a], red[3][a]))));
        else
            atomicMax(&bbox[6 * c + a], float_to_ordered(fmaxf(fmaxf(red[0][a], red[1][a]), fmaxf(red[2][a], red[3][a]))));
    }
}

__device__ __forceinline__ unsigned long long spread3(unsigned v)  // 14 bits -> every third bit
{
    unsigned long long x = v & 0x3fffu;
    x = (x | (x << 32)) & 0x1f00000000ffffull;
    x = (x | (x << 16)) & 0x1f0000ff0000ffull;
    x = (x | (x << 8)) & 0x100f00f00f00f00full;
    x = (x | (x << 4)) & 0x10c30c30c30c30c3ull;
    x = (x | (x << 2)) & 0x1249249249249249ull;
    return x;
}

// 42-bit Morton code of (x, y, z) on the cubic grid (origin lo, scale sc) of a cloud
__device__ __forceinline__ unsigned long long morton42(float x, float y, float z, const float (&lo)[3], float sc)
{
    const float p[3] = {x, y, z};
    unsigned q[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float v = (p[a] - lo[a]) * sc;
        q[a] = v >= 0.0f ? (unsigned)fminf(v, 16383.0f) : 0u;  // NaN -> 0
    }
    return spread3(q[0]) | (spread3(q[1]) << 1) | (spread3(q[2]) << 2);
}

__device__ __forceinline__ float morton_grid(const int* __restrict__ bbox, int c, float (&lo)[3])
{
    float ext = 0.0f;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        lo[a] = ordered_to_float(bbox[6 * c + a]);
        ext = fmaxf(ext, ordered_to_float(bbox[6 * c + 3 + a]) - lo[a]);
    }
    return ext > 0.0f ? 16383.0f / ext : 0.0f;
}

// Cold start of the NN scan: the target point whose Morton code is closest to the query's (binary search over the
// Morton-ordered cloud, codes recomputed from the points) or its predecessor, whichever is nearer.  Any index is
// a valid upper bound; this one is usually within a cell or two of the true neighbour.
__device__ __forceinline__ int morton_seed(const float4* __restrict__ tgt, int m, float qx, float qy, float qz,
                                           const float (&lo)[3], float sc)
{
    const unsigned long long key = morton42(qx, qy, qz, lo, sc);
    int a = 0, b = m;  // first index with code >= key
    while (a < b) {
        const int mid = (a + b) >> 1;
        const float4 t = tgt[mid];
        if (morton42(t.x, t.y, t.z, lo, sc) < key) a = mid + 1; else b = mid;
    }
    const int j1 = min(a, m - 1), j0 = max(j1 - 1, 0);
    return dist2(qx, qy, qz, tgt[j0]) < dist2(qx, qy, qz, tgt[j1]) ? j0 : j1;
}

// key = cloud id (high bits) | 42-bit Morton code on a cubic grid spanning the cloud's bounding box
__global__ void k_morton_keys(const float* __restrict__ src, int stride, const int64_t* __restrict__ offs,
                              const int* __restrict__ bbox, unsigned long long* __restrict__ keys, int* __restrict__ vals)
{
    const int c = blockIdx.y;
    const int64_t o = offs[c];
    const int n = (int)(offs[c + 1] - o);
    float lo[3];
    const float sc = morton_grid(bbox, c, lo);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float* p = src + (size_t)(o + i) * stride;
        keys[o + i] = ((unsigned long long)c << 42) | morton42(p[0], p[1], p[2], lo, sc);
        vals[o + i] = (int)(o + i);
    }
}

// dst[k] = point perm[k]; .w carries its ORIGINAL cloud-local index
__global__ void k_gather_sorted(const float* __restrict__ src, int stride, const int64_t* __restrict__ offs,
                                const int* __restrict__ perm, float4* __restrict__ dst)
{
    const int c = blockIdx.y;
    const int64_t o = offs[c];
    const int n = (int)(offs[c + 1] - o);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int g = perm[o + i];
        const float* p = src + (size_t)g * stride;
        dst[o + i] = make_float4(p[0], p[1], p[2], __int_as_float(g - (int)o));
    }
}

// bounding boxes of every 1024-point tile and of its 64 minis of 16 points; tile_base[c] = first tile of cloud c (minis: 64 x that)
__global__ __launch_bounds__(256) void k_boxes(const float4* __restrict__ pts, const int64_t* __restrict__ offs, const int* __restrict__ tile_base,
                                               float4* __restrict__ tlo, float4* __restrict__ thi, float4* __restrict__ mlo,
                                               float4* __restrict__ mhi)
{
    __shared__ float red[4][6];
    const int c = blockIdx.y;
    const int64_t o = offs[c];
    const int n = (int)(offs[c + 1] - o);
    const int t = blockIdx.x;
    if (t * kTile >= n) return;
    const size_t tile = (size_t)tile_base[c] + t;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
#pragma unroll
    for (int j = 0; j < kTile / 256; ++j) {
        const int i = t * kTile + j * 256 + (int)threadIdx.x;      // 16 consecutive lanes = one mini
        const bool in = i < n;
        const float4 p = pts[o + (in ? i : 0)];
        float b[6] = {in ? p.x : INFINITY, in ? p.y : INFINITY, in ? p.z : INFINITY, in ? p.x : -INFINITY, in ? p.y : -INFINITY, in ? p.z : -INFINITY};
#pragma unroll
        for (int a = 0; a < 3; ++a)
            for (int s = 1; s < 16; s <<= 1) {
                b[a] = fminf(b[a], __shfl_xor(b[a], s, 64));
                b[3 + a] = fmaxf(b[3 + a], __shfl_xor(b[3 + a], s, 64));
            }
        if ((threadIdx.x & 15) == 0) {
            const size_t mi = tile * 64 + (size_t)((j * 256 + (int)threadIdx.x) >> 4);
            mlo[mi] = make_float4(b[0], b[1], b[2], 0.f);
            mhi[mi] = make_float4(b[3], b[4], b[5], 0.f);
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) { lo[a] = fminf(lo[a], b[a]); hi[a] = fmaxf(hi[a], b[3 + a]); }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        for (int s = 32; s > 0; s >>= 1) {
            lo[a] = fminf(lo[a], __shfl_xor(lo[a], s, 64));
            hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], s, 64));
        }
        if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][a] = lo[a]; red[threadIdx.x >> 6][3 + a] = hi[a]; }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float l[3], h[3];
        for (int a = 0; a < 3; ++a) {
            l[a] = fminf(fminf(red[0][a], red[1][a]), fminf(red[2][a], red[3][a]));
            h[a] = fmaxf(fmaxf(red[0][3 + a], red[1][3 + a]), fmaxf(red[2][3 + a], red[3][3 + a]));
        }
        tlo[tile] = make_float4(l[0], l[1], l[2], 0.f);
        thi[tile] = make_float4(h[0], h[1], h[2], 0.f);
    }
}

// smallest_eigvec / sym3_eigvals: eig3.hpp (closed form + Rayleigh-quotient steps; the cyclic Jacobi of rounds 1-5 is gone)

// ---- exact k nearest neighbours in two passes ----------------------------------------------------------------------------------
// A sorted insertion that carries the index costs ~8 VALU instructions per slot and, in SIMT, every lane of a wave pays for every
// lane's insertions.  Here the scan keeps only the KMAX smallest DISTANCES, sorted, by a chain of v_med3_f32
// (dk[s] = med3(dk[s-1], d, dk[s]): one instruction per slot, no predicate: a distance beyond the list leaves it unchanged).
//   pass 1 (the k-th distance tau): seed = the 64 neighbours along the Morton curve; then the hierarchy walk.  A candidate closer than
//     the lane's bound T = dk[KMAX - 1] is only NOTED in a lane-private LDS buffer (one predicated ds_write); the chain runs when some
//     lane's buffer is more than half full: once per candidate a LANE accepted, not once per candidate ANY lane of the wave accepted
//     (rounds 3-4: ~480 chain passes per wave, 15 k of its 44 k VALU instructions; now ~50).  T is refreshed at every flush; a stale T
//     is a valid bound (bounds only shrink), it merely lets a few more candidates through;
//   pass 2 (the indices): tau is exact, and so is the number of candidates strictly inside it (nless = #{dk[s] < tau}); the walk over
//     the minis pass 1 noted appends every candidate with d < tau and the first kk - nless exact ties with tau (they arrive in
//     ascending index order): never more than kk entries, whatever the number of duplicates (no overflow path);
//   order: the rank of a collected candidate is the number of dk[s] below its distance (+ the equal ones already placed: a bit mask),
//     2 VALU instructions per slot in place of the 8 of a (distance, index) insertion, and no index registers.
// Exactly equal distances resolve to the smaller (Morton-space) index.  The whole workgroup must call it together.

__device__ int g_knn_norec;        // development aid (MRS_KNN_REC=0): pass 2 walks the hierarchy again instead of revisiting pass 1's minis

constexpr int kHome = 64;         // Morton-curve neighbours that seed the bound (the walk skips exactly that index range)
constexpr int kKnnBuf = 16;       // LDS slots per lane for noted candidates (in the first slots of the index list: pass 1 is over before pass 2 writes)
constexpr int kKnnRec = 64;       // minis a wave can note in pass 1 for pass 2 (more: pass 2 walks the hierarchy again)
constexpr int kKnnBlk = 64;       // neighbour lists leave the selection in blocks of 64 points, slot-major (knn_at)

template <int KMAX>
__device__ __forceinline__ void dist_insert(float (&dk)[KMAX], float d)
{
#pragma unroll
    for (int s = KMAX - 1; s > 0; --s) dk[s] = __builtin_amdgcn_fmed3f(dk[s - 1], d, dk[s]);
    dk[0] = fminf(dk[0], d);
}

// (distance, index) ordered insertion (k_knn_select, the round-4 search core)
template <int KMAX>
__device__ __forceinline__ void knn_insert_tie(float (&dk)[KMAX], int (&ik)[KMAX], float d, int j)
{
#pragma unroll
    for (int s = KMAX - 1; s > 0; --s) {
        const bool up = dk[s - 1] > d || (dk[s - 1] == d && ik[s - 1] > j);
        const bool here = !up && (dk[s] > d || (dk[s] == d && ik[s] > j));
        dk[s] = up ? dk[s - 1] : (here ? d : dk[s]);
        ik[s] = up ? ik[s - 1] : (here ? j : ik[s]);
    }
    if (dk[0] > d || (dk[0] == d && ik[0] > j)) { dk[0] = d; ik[0] = j; }
}

// Neighbour lists between the selection and its consumers (k_cov_from_knn, k_feat_from_knn): cloud-local sorted-space indices, per cloud
// in blocks of 64 points, slot-major inside a block -- entry (point i, slot s) of cloud c (first point o) lies at
//   knn[(o + 64 c) k + (i / 64) 64 k + 64 s + i % 64]
// so that a wave's loads of one slot are ONE 256-byte row (as [point][k] every lane walked its own 4 k bytes: 64 lines per load
// instruction, re-fetched from HBM whenever the L1 / L2 lost them: k_feat_from_knn read 1.1 KB per point).  Room: knn_ints().
__host__ __device__ inline size_t knn_ints(int64_t points, int64_t clouds, int k) { return (size_t)(points + kKnnBlk * clouds) * (size_t)k; }
__device__ __forceinline__ size_t knn_at(int64_t o, int c, int i, int k, int s)
{
    return (size_t)(o + (int64_t)kKnnBlk * c) * k + (size_t)(i >> 6) * (kKnnBlk * k) + (size_t)(s << 6) + (size_t)(i & 63);
}

// The k nearest of point i (itself included) in (distance, index) order: emit(rank, index) once per neighbour, ranks 0 .. found - 1;
// returns the number found (< k only in a cloud with fewer than k points).  list: KMAX x kNNThreads ints of LDS, slot-major.
template <int KMAX, class Emit>
__device__ __forceinline__ int knn_two_pass(int* __restrict__ list, const float4* __restrict__ pts, int n, const Hier& H,
                                            int i, bool live, const float4& q, int k, int* __restrict__ rec_ids /* wave-private, kKnnRec ints of LDS, or null */,
                                            Emit emit)
{
    static_assert(KMAX <= 32 && KMAX >= kKnnBuf, "rank mask is 32 bits; the note buffer lives in the list");
    const int tid = (int)threadIdx.x;
    float dk[KMAX];
#pragma unroll
    for (int s = 0; s < KMAX; ++s) dk[s] = INFINITY;
    // pass 1: the KMAX smallest distances.  Seed: the 64 neighbours along the Morton curve, 8 loads in flight at a time
    const int home = max(0, min(i - kHome / 2, n - kHome));
    for (int u0 = 0; u0 < kHome; u0 += 8) {
        if (home + u0 >= n) break;             // n < kHome: wave-uniform
        float4 hp[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) hp[u] = pts[(live && home + u0 + u < n) ? home + u0 + u : 0];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const float d = dist2(q.x, q.y, q.z, hp[u]);
            dist_insert<KMAX>(dk, (live && home + u0 + u < n && d == d) ? d : INFINITY);
        }
    }
    const int home_tile = __builtin_amdgcn_readfirstlane(i) >> 10;      // kTile = 1024
    float* const buf = reinterpret_cast<float*>(list);
    int nb = 0;                     // candidates noted since the last flush
    auto flush = [&]() {
#pragma unroll 1
        for (int s = 0; s < kKnnBuf; ++s) {
            if (!__any(s < nb)) break;
            const float v = s < nb ? buf[s * kNNThreads + tid] : INFINITY;
            dist_insert<KMAX>(dk, v);
        }
        nb = 0;
    };
    int nrec = 0;       // wave-uniform
    knn_walk<true>(pts, n, H, live, q, home_tile,
               [&]() { if (__any(nb > 0)) flush(); return dk[KMAX - 1]; },       // before every tile: bounds up to date
               [&](int j0, const Cand8& cand) {
                   float qx = q.x, dd[8];
                   cand_pin(qx);
                   cand_dist(cand, j0, n, qx, q.y, q.z, dd);
                   const float T = dk[KMAX - 1];
                   const float mn = fminf(fminf(fminf(dd[0], dd[1]), fminf(dd[2], dd[3])), fminf(fminf(dd[4], dd[5]), fminf(dd[6], dd[7])));
                   if (!__any(live && mn < T)) return;
#pragma unroll
                   for (int u = 0; u < 8; ++u) {
                       const bool use = live && (unsigned)(j0 + u - home) >= (unsigned)kHome && dd[u] < T;       // NaN: false
                       if (use) { buf[nb * kNNThreads + tid] = dd[u]; ++nb; }
                   }
                   if (__any(nb > kKnnBuf - 8)) flush();
               },
               [&](int id) {       // every mini within some quad's bound of the moment (a superset of the minis within the final bounds)
                   if (rec_ids && nrec < kKnnRec && (threadIdx.x & 63) == 0) rec_ids[nrec] = id;
                   ++nrec;
               });
    if (__any(nb > 0)) flush();
    // pass 2: the candidates within the k-th distance, home range included, in ascending index order
    const int kk = k < KMAX ? k : KMAX;
    float tau = dk[KMAX - 1];
    int nless = 0;
#pragma unroll
    for (int s = 0; s < KMAX - 1; ++s) tau = (s == kk - 1) ? dk[s] : tau;
#pragma unroll
    for (int s = 0; s < KMAX; ++s) {
        dk[s] = s < kk ? dk[s] : INFINITY;        // the ranks below count dk[s] < d over every slot
        nless += dk[s] < tau ? 1 : 0;
    }
    if (!live) tau = -1.0f;
    const int room = kk - nless;                  // exact ties with tau that belong to the k nearest
    int cnt = 0, nt = 0;
    auto visit2 = [&](int j0, const Cand8& cand) {
        float qx = q.x, dd[8];
        cand_pin(qx);
        cand_dist(cand, j0, n, qx, q.y, q.z, dd);
        const float mn = fminf(fminf(fminf(dd[0], dd[1]), fminf(dd[2], dd[3])), fminf(fminf(dd[4], dd[5]), fminf(dd[6], dd[7])));
        if (!__any(mn <= tau)) return;
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (dd[u] <= tau && dd[u] < INFINITY) {     // tau is +inf for a cloud with fewer than k points: padding stays out
                const bool tie = dd[u] == tau;
                if (!tie || nt < room) {
                    list[cnt * kNNThreads + tid] = j0 + u;
                    ++cnt;
                    nt += tie ? 1 : 0;
                }
            }
    };
    if (rec_ids && nrec <= kKnnRec) {       // the minis pass 1 visited, without walking the hierarchy again -- in INDEX order (ties resolve by arrival)
        nnc::wave_lds_sync();
        const int lane = threadIdx.x & 63;
        const int id = lane < nrec ? rec_ids[lane] : 0x7fffffff;
        int rank = 0;
        for (int m = 0; m < nrec; ++m) rank += __builtin_amdgcn_readlane(id, m) < id ? 1 : 0;
        nnc::wave_lds_sync();
        if (lane < nrec) rec_ids[rank] = id;
        nnc::wave_lds_sync();
        // (no box test: nearly every one of them holds a candidate of some lane, and the test would be a round trip per mini)
        stream_minis(pts, nrec, [&](int r) { return __builtin_amdgcn_readfirstlane(rec_ids[r]); }, visit2);
    } else {
        knn_walk<false>(pts, n, H, live, q, 0, [&]() { return tau; }, visit2, [](int) {});
    }
    cnt = min(cnt, kk);       // (cannot exceed it: nless candidates are closer than tau, at most room ties were taken)
    // order: rank = #{dk < d} + the equal ones placed before (entries arrive in ascending index order)
    int most = cnt;
    for (int o = 32; o > 0; o >>= 1) most = max(most, __shfl_xor(most, o, 64));
    unsigned used = 0;
    int j = cnt > 0 ? list[tid] : 0;
    float4 pj = pts[j];
#pragma unroll 1
    for (int c = 0; c < most; ++c) {
        const bool h = c < cnt;
        const int jn = c + 1 < cnt ? list[(c + 1) * kNNThreads + tid] : 0;
        const float4 pn = pts[jn];          // the next entry's point is on its way while this one is ranked
        const float d = dist2(q.x, q.y, q.z, pj);
        int r = 0;
#pragma unroll
        for (int s = 0; s < KMAX; ++s) r += dk[s] < d ? 1 : 0;
        r = min(r, 31);
        r += __builtin_ctz(~(used >> r));
        if (h && r < kk) {
            used |= 1u << r;
            emit(r, j);
        }
        j = jn; pj = pn;
    }
    return cnt;
}

// G2 / N1 selection: exact kNN (KMAX slots, the first k are used) on the Morton-ordered cloud with tile / mini culling (bound = the lane's
// current KMAX-th distance).  grid = (blocks, clouds); cloud c spans pts[offs[c] .. offs[c+1]).  The neighbours go to knn (layout: knn_at)
// as cloud-local SORTED-space indices, -1 in the slots a cloud with fewer than k points cannot fill; k_cov_from_knn / k_feat_from_knn do
// the fp64 tails (without their state the selection keeps fewer registers alive: more waves per SIMD).
template <int KMAX, int WAVES = (KMAX <= 20 ? 6 : (KMAX <= 30 ? 5 : 4))>
__global__ __launch_bounds__(kNNThreads) __attribute__((amdgpu_waves_per_eu(WAVES, WAVES))) void k_knn_cov(const float4* __restrict__ pts_all,
                                                        const int64_t* __restrict__ offs, const int* __restrict__ tile_base,
                                                        const float4* __restrict__ tlo, const float4* __restrict__ thi,
        const float4* __restrict__ mlo, const float4* __restrict__ mhi, int k, int* __restrict__ knn)
{
    __shared__ int knn_list[KMAX * kNNThreads];
    __shared__ int knn_rec[kNNThreads / 64][kKnnRec];
    const int c = blockIdx.y;
    const int64_t o = offs[c];
    const int n = (int)(offs[c + 1] - o);
    const float4* pts = pts_all + o;
    Hier H;
    H.tlo = tlo + tile_base[c]; H.thi = thi + tile_base[c];
    H.mlo = mlo + (size_t)64 * tile_base[c]; H.mhi = mhi + (size_t)64 * tile_base[c];
    H.ntiles = (n + kTile - 1) / kTile;
    for (int base = blockIdx.x * kNNThreads; base < n; base += gridDim.x * kNNThreads) {
        const int i = base + threadIdx.x;
        const bool live = i < n;
        const float4 q = pts[live ? i : 0];
        int* const out = knn + knn_at(o, c, live ? i : 0, k, 0);
        const int found = knn_two_pass<KMAX>(knn_list, pts, n, H, i, live, q, k, g_knn_norec ? nullptr : knn_rec[threadIdx.x >> 6],
                                             [&](int r, int j) { out[r << 6] = j; });
        if (live && found < k)
            for (int s = found; s < k; ++s) out[s << 6] = -1;
    }
}


// ---- RING++ point-feature front-end -----------------------------------
// calculate_features (generate_bev_pointfeat_cython/src/kernel.cu:16-104) for one point, given its
// 5 eigenvalues (3-D descending, 2-D descending) and the z of its k neighbours.
__device__ __forceinline__ void point_features(const float* e, const float* nz, int k, float* f)
{
    const float e0 = e[0], e1 = e[1], e2 = e[2];
    const float sum = e0 + e1 + e2, prod = e0 * e1 * e2, sum2 = e[3] + e[4];
    f[0] = e2 / sum;                                                  // C_
    f[1] = (float)pow((double)(prod / (sum * sum * sum)), 1.0 / 3.0);  // O_
    f[2] = (e0 - e1) / e0;                                            // L_
    float ent = 0.0f;
    ent += (e0 / sum) * logf(e0 / sum);
    ent += (e1 / sum) * logf(e1 / sum);
    ent += (e2 / sum) * logf(e2 / sum);
    f[3] = -ent;                                                      // E_
    f[4] = (e1 - e2) / e0;                                            // P_
    f[5] = e2 / e0;                                                   // S_
    f[6] = (e0 - e2) / e0;                                            // A_
    f[7] = sum;                                                       // X_
    f[8] = (float)((double)(3 * k) / (4.0 * M_PI * (double)prod));    // D_
    f[9] = sum2;                                                      // S_2
    f[10] = e[4] / e[3];                                              // L_2
    float mean = 0.0f, mn = 10000.0f;
    for (int i = 0; i < k; ++i) { mean += nz[i]; mn = fminf(mn, nz[i]); }
    mean /= (float)k;
    float dz = -100000.0f, vz = 0.0f;
    for (int i = 0; i < k; ++i) {
        dz = fmaxf(dz, nz[i] - mn);
        const float d = fabsf(nz[i] - mean);
        vz += d * d;
    }
    f[11] = dz;                                                       // dZ_
    f[12] = vz / (float)k;                                            // vZ_
}

// drop-in kernel of voxelfeat.GPUFeatureExtractor: neighbours and eigenvalues supplied by the caller
__global__ void k_features_from_neighbors(const float* __restrict__ pts /* [n][3] */, int n, int k,
                                          const int* __restrict__ knn, const float* __restrict__ eig,
                                          float* __restrict__ feat /* [n][13] */)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        float nz[32];
        for (int j = 0; j < k; ++j) nz[j] = pts[(size_t)knn[(size_t)i * k + j] * 3 + 2];
        float f[13];
        point_features(eig + (size_t)i * 5, nz, k, f);
        for (int j = 0; j < 13; ++j) feat[(size_t)i * 13 + j] = f[j];
    }
}

__device__ __forceinline__ bool inv3_sym(const double* a, double* r)
{
    // a: full 3x3 symmetric, r: full 3x3
    const double c0 = a[4] * a[8] - a[5] * a[7], c1 = a[5] * a[6] - a[3] * a[8], c2 = a[3] * a[7] - a[4] * a[6];
    const double det = a[0] * c0 + a[1] * c1 + a[2] * c2;
    if (det == 0.0) return false;
    const double id = 1.0 / det;
    r[0] = c0 * id; r[1] = (a[2] * a[7] - a[1] * a[8]) * id; r[2] = (a[1] * a[5] - a[2] * a[4]) * id;
    r[3] = c1 * id; r[4] = (a[0] * a[8] - a[2] * a[6]) * id; r[5] = (a[2] * a[3] - a[0] * a[5]) * id;
    r[6] = c2 * id; r[7] = (a[1] * a[6] - a[0] * a[7]) * id; r[8] = (a[0] * a[4] - a[1] * a[3]) * id;
    return true;
}

// G3a: exact 1-NN of every (float-)transformed source point (tile-culled brute force).
// grid = (blocks, pairs).  Kept free of the fp64 algebra so that it runs at full occupancy.  P source points per
// lane: 2 in a batch, 1 for a single pair so that its ~235 workgroups become ~470 (see launch_nn_scan).
// corr[so + i] = target index (sorted space), or -1 when d^2 >= max_corr^2.
template <int P>
__global__ __launch_bounds__(kNNThreads) void k_nn_scan(
    const float4* __restrict__ src_all, const int64_t* __restrict__ src_offs,
    const float4* __restrict__ tgt_all, const int64_t* __restrict__ tgt_offs,
    const int* __restrict__ tgt_tile_base, const float4* __restrict__ tlo, const float4* __restrict__ thi,
        const float4* __restrict__ mlo, const float4* __restrict__ mhi,
    const LmState* __restrict__ st, GicpParams prm, int* __restrict__ corr, int* __restrict__ nn_seed,
    const int* __restrict__ tgt_bbox, float* __restrict__ lb_out, int gate)
{
    const int pair = blockIdx.y;
    const LmState& S = st[pair];
    if (!S.active || S.phase != 0) return;   // LM trials reuse the cached correspondences (upstream compute_error)
    if (gate && !(pair_motion(S) > prm.motion_switch)) return;   // round-4 schedule: this pair is certified / searched by k_nn_scan_g
    const int64_t so = src_offs[pair], to = tgt_offs[pair];
    const int n = (int)(src_offs[pair + 1] - so), m = (int)(tgt_offs[pair + 1] - to);
    const float4* src = src_all + so;
    const float4* tgt = tgt_all + to;
    Hier H;
    H.tlo = tlo + tgt_tile_base[pair]; H.thi = thi + tgt_tile_base[pair];
    H.mlo = mlo + (size_t)64 * tgt_tile_base[pair]; H.mhi = mhi + (size_t)64 * tgt_tile_base[pair];
    H.ntiles = (m + kTile - 1) / kTile;
    const float maxc2 = prm.max_corr2 < 3.0e38 ? (float)prm.max_corr2 * 1.0001f : INFINITY;
    float Tf[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) Tf[i] = (float)S.x[i];
    float glo[3];
    const float gsc = morton_grid(tgt_bbox, pair, glo);
    const int per_block = kNNThreads * P;
    for (int base = blockIdx.x * per_block; base < n; base += gridDim.x * per_block) {
        float qx[P], qy[P], qz[P];
        int si[P], seed[P];
        bool live[P];
#pragma unroll
        for (int p = 0; p < P; ++p) {
            // a wave owns 4 x 64 CONSECUTIVE (Morton-ordered, i.e. spatially compact) source points
            si[p] = base + (threadIdx.x >> 6) * (64 * P) + p * 64 + (threadIdx.x & 63);
            live[p] = si[p] < n;
            const float4 a = src[live[p] ? si[p] : 0];
            qx[p] = Tf[0] * a.x + Tf[1] * a.y + Tf[2] * a.z + Tf[3];
            qy[p] = Tf[4] * a.x + Tf[5] * a.y + Tf[6] * a.z + Tf[7];
            qz[p] = Tf[8] * a.x + Tf[9] * a.y + Tf[10] * a.z + Tf[11];
            seed[p] = live[p] ? nn_seed[so + si[p]] : -1;   // last pass's nearest neighbour (the rejected ones too)
            if (live[p] && seed[p] < 0 && m > 0) seed[p] = morton_seed(tgt, m, qx[p], qy[p], qz[p], glo, gsc);  // cold start
        }
        float best[P];
        int bidx[P];
        nn_scan<P>(tgt, m, H, maxc2, qx, qy, qz, live, best, bidx, seed);
#pragma unroll
        for (int p = 0; p < P; ++p)
            if (live[p]) {
                corr[so + si[p]] = (bidx[p] >= 0 && (double)best[p] < prm.max_corr2) ? bidx[p] : -1;
                nn_seed[so + si[p]] = bidx[p];
                if (lb_out) lb_out[so + si[p]] = 0.0f;     // this search leaves no certificate
            }
    }
}

// G3b + G4: Mahalanobis matrices, residuals and the 28 fp64 sums for the correspondences found by
// k_nn_scan.  grid = (blocks, pairs), one source point per lane; partial[pair][block][28].
// Two poses: the Mahalanobis matrices belong to the linearisation pose S.x (upstream caches them in
// update_correspondences), the residuals to the evaluated pose S.xi.  Phase 0: xi == x, all 28 sums
// (FastGICP::linearize); phase 1: only the error sum (FastGICP::compute_error of an LM trial).
// Three waves per SIMD (142 registers, no spills): the normals of the lane's NEXT point (own 24 B streamed, neighbour's 24 B gathered) travel one
// point ahead like the points themselves, instead of being requested where the algebra needs them (four waves spill, in either form)
__global__ __launch_bounds__(kNNThreads) __attribute__((amdgpu_waves_per_eu(3, 3))) void k_linearize(
    const float4* __restrict__ src_all, const int64_t* __restrict__ src_offs, const double* __restrict__ src_cov,
    const float4* __restrict__ tgt_all, const int64_t* __restrict__ tgt_offs, const double* __restrict__ tgt_cov,
    const LmState* __restrict__ st, const int* __restrict__ corr, double* __restrict__ partial, int max_blocks, int trial_only)
{
    __shared__ double red[kNNThreads / 64][kTerms];
    const int pair = blockIdx.y;
    const LmState& S = st[pair];
    if (!S.active) return;
    if (trial_only && S.phase == 0) return;     // a tick enqueued WITHOUT its search kernels (mrs_gicp_batch_align, one pair): a pair that needs a
                                                // linearisation sits this tick out (k_lm_update leaves its state alone) and takes the next, full one
    const int64_t so = src_offs[pair], to = tgt_offs[pair];
    const int n = (int)(src_offs[pair + 1] - so);
    const float4* src = src_all + so;
    const float4* tgt = tgt_all + to;
    double* pout = partial + ((size_t)pair * max_blocks + blockIdx.x) * kTerms;
    const bool error_only = S.phase == 1;
    double T[12], TL[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) { T[i] = S.xi[i]; TL[i] = S.x[i]; }
    double acc[kTerms];
#pragma unroll
    for (int i = 0; i < kTerms; ++i) acc[i] = 0.0;
    const int per_block = kNNThreads * kPts;  // same point -> block mapping as the scan (fixed summation order)
    for (int base = blockIdx.x * per_block; base < n; base += gridDim.x * per_block) {
        // software pipeline over the lane's kPts points (a rolled loop: one copy of the algebra): the correspondence index travels two
        // points ahead, the point's own data and its gathered neighbour one point ahead of the algebra (the gathers are what the kernel
        // waits for); the order of the sums does not change
        auto idx_of = [&](int p) { const int i = base + p * kNNThreads + (int)threadIdx.x; return (p < kPts && i < n) ? corr[so + i] : -1; };
        int j_cur = idx_of(0), j_nx = idx_of(1);
        float4 a_nx = make_float4(0.f, 0.f, 0.f, 0.f), b_nx = a_nx;
        double na_nx[3] = {0.0, 0.0, 0.0}, nb_nx[3] = {0.0, 0.0, 0.0};
        auto fetch_normals = [&](int i_next, int j_next) {
            const double* pa = src_cov + kCovDoubles * (size_t)(so + i_next);
            const double* pb = tgt_cov + kCovDoubles * (size_t)(to + j_next);
            na_nx[0] = pa[0]; na_nx[1] = pa[1]; na_nx[2] = pa[2];
            nb_nx[0] = pb[0]; nb_nx[1] = pb[1]; nb_nx[2] = pb[2];
        };
        if (j_cur >= 0) {
            a_nx = src[base + threadIdx.x]; b_nx = tgt[j_cur];
            fetch_normals(base + (int)threadIdx.x, j_cur);
        }
#pragma unroll 1
        for (int p = 0; p < kPts; ++p) {
            const int i = base + p * kNNThreads + threadIdx.x;
            const int j = j_cur;
            const float4 a = a_nx, bb = b_nx;
            const double na[3] = {na_nx[0], na_nx[1], na_nx[2]}, nbv[3] = {nb_nx[0], nb_nx[1], nb_nx[2]};
            j_cur = j_nx;
            j_nx = idx_of(p + 2);
            if (j_cur >= 0) {
                a_nx = src[i + kNNThreads]; b_nx = tgt[j_cur];
                fetch_normals(i + kNNThreads, j_cur);
            }
            if (j < 0) continue;
            double ca[6], cb[6];
            cov6_from_normal(na, ca);
            cov6_from_normal(nbv, cb);
            const double CA[9] = {ca[0], ca[1], ca[2], ca[1], ca[3], ca[4], ca[2], ca[4], ca[5]};
            double RC[9], RCR[9], M[9];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    RC[3 * r + c] = TL[4 * r] * CA[c] + TL[4 * r + 1] * CA[3 + c] + TL[4 * r + 2] * CA[6 + c];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    RCR[3 * r + c] = RC[3 * r] * TL[4 * c] + RC[3 * r + 1] * TL[4 * c + 1] + RC[3 * r + 2] * TL[4 * c + 2];
            RCR[0] += cb[0]; RCR[1] += cb[1]; RCR[2] += cb[2];
            RCR[3] += cb[1]; RCR[4] += cb[3]; RCR[5] += cb[4];
            RCR[6] += cb[2]; RCR[7] += cb[4]; RCR[8] += cb[5];
            if (!inv3_sym(RCR, M)) continue;
            double ta[3], e[3], Me[3];
#pragma unroll
            for (int r = 0; r < 3; ++r)
                ta[r] = T[4 * r] * (double)a.x + T[4 * r + 1] * (double)a.y + T[4 * r + 2] * (double)a.z + T[4 * r + 3];
            e[0] = (double)bb.x - ta[0]; e[1] = (double)bb.y - ta[1]; e[2] = (double)bb.z - ta[2];
#pragma unroll
            for (int r = 0; r < 3; ++r) Me[r] = M[3 * r] * e[0] + M[3 * r + 1] * e[1] + M[3 * r + 2] * e[2];
            acc[27] += e[0] * Me[0] + e[1] * Me[1] + e[2] * Me[2];
            if (error_only) continue;
            const double J[18] = {0, -ta[2], ta[1], -1, 0, 0,
                                  ta[2], 0, -ta[0], 0, -1, 0,
                                  -ta[1], ta[0], 0, 0, 0, -1};
            double MJ[18];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 6; ++c)
                    MJ[6 * r + c] = M[3 * r] * J[c] + M[3 * r + 1] * J[6 + c] + M[3 * r + 2] * J[12 + c];
#pragma unroll
            for (int r = 0; r < 6; ++r) {
#pragma unroll
                for (int c = r; c < 6; ++c)
                    acc[r * 6 - (r * (r - 1)) / 2 + (c - r)] += J[r] * MJ[c] + J[6 + r] * MJ[6 + c] + J[12 + r] * MJ[12 + c];
            }
#pragma unroll
            for (int r = 0; r < 6; ++r) acc[21 + r] += J[r] * Me[0] + J[6 + r] * Me[1] + J[12 + r] * Me[2];
        }
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int i = 0; i < kTerms; ++i) {
        const double v = wave_sum_d(acc[i]);
        if (lane == 0) red[wave][i] = v;
    }
    __syncthreads();
    if (threadIdx.x < kTerms) {
        double v = 0;
        for (int w = 0; w < kNNThreads / 64; ++w) v += red[w][threadIdx.x];
        pout[threadIdx.x] = v;
    }
}


// ================================================================================================================================
// Round 4 search core (nn_core.hpp): octree-cell leaves + query groups.  The kernels below replace k_nn_scan / k_knn_cov;
// the round-3 kernels stay selectable (mrs_gicp_batch_set_search(h, 0)) for A/B runs and as a cross-check in the tests.
struct HierArrays {
    const float4* llo; const float4* lhi; const float4* tlo; const float4* thi; const float4* slo; const float4* shi;
    const int* leaf_first; const int* tile_first; const int* super_first;   // [clouds + 1]
};

__device__ __forceinline__ nnc::LeafHier cloud_hier(const HierArrays& A, int c)
{
    nnc::LeafHier H;
    const int l0 = A.leaf_first[c], t0 = A.tile_first[c], s0 = A.super_first[c];
    H.llo = A.llo + l0; H.lhi = A.lhi + l0; H.nleaf = A.leaf_first[c + 1] - l0;
    H.tlo = A.tlo + t0; H.thi = A.thi + t0; H.ntile = A.tile_first[c + 1] - t0;
    H.slo = A.slo + s0; H.shi = A.shi + s0; H.nsuper = A.super_first[c + 1] - s0;
    return H;
}

// G3a, round 4: exact 1-NN of every (float-)transformed source point.  One query per lane; semantics of k_nn_scan (corr = target index in
// sorted space or -1 when d^2 >= max_corr^2; nn_seed = the neighbour found, warm start of the next pass), ties to the smaller index.
// Certificates (round 4).  After a search the lane knows lb = a lower bound of the distance from its query to every target point OTHER
// than the neighbour found: the second smallest distance it evaluated, or the radius it searched (neighbour distance + a margin), whichever
// is smaller.  When the pose changes, a query moves by delta = |T_new a - T_prev a|, so every other point is still at least lb - delta
// away; if the old neighbour's new distance is below that, it is still THE nearest neighbour -- exactly, by the triangle inequality --
// and no search is needed (k_nn_certify).  Queries that cannot be certified go to a per-pair work list and are searched as before.
// Late iterations of an alignment move the cloud by less than the gap between a point's nearest and second nearest neighbour, so most of
// their passes reduce to one streaming kernel.  Float evaluation error is covered by a relative 1e-5 + absolute (1e-6 m + 4 ulps of the
// largest coordinate) slack on both sides -- certificates are exact up to that evaluation error; an exact tie (two points at one distance) leaves no gap and is always searched, so ties still resolve to the smaller index.
struct CertArrays {
    float* lb;             // [source points] lower bound described above (0: none)
    float* t_prev;         // [pairs][12] pose of the pair's last nearest-neighbour pass (float, like the searches use it)
    int* work;             // [source points] per pair (at the pair's source offset): source indices that need a search
    int* bcount;           // [pairs][nb] entries in the work list of each block of 1024 consecutive source points (its list starts at the block)
    int nb;                // blocks of the longest source cloud
    unsigned long long* searched;   // [pairs][kStatStride] statistics of an align(), slots 0 / 1 of every pair: queries searched, queries due (points of the
                                    // pairs that searched, per pass).  One 128-byte line per pair: 30 000 workgroups adding to ONE word serialise in its L2
                                    // channel (~12 ns each: 0.7 ms of a 0.77 ms k_nn_certify); the host sums the pairs
};

__device__ __forceinline__ void pose_f(const LmState& S, float (&Tf)[12])
{
#pragma unroll
    for (int i = 0; i < 12; ++i) Tf[i] = (float)S.x[i];
}

constexpr int kStatStride = 16;    // unsigned long longs per pair in CertArrays::searched (128 bytes)
constexpr int kCertBlock = 1024;   // consecutive source points whose uncertified members form one work list (searched by one workgroup)

// One workgroup per 1024 consecutive source points of every pair that is about to search: certify the old neighbour or put the point on
// the block's work list, in index order (lists of consecutive points keep the search's waves spatially compact; appended with atomics in
// completion order, the waves of a sparse list spanned the whole cloud and tested ~1000 tiles each).
__global__ __launch_bounds__(256) void k_nn_certify(const float4* __restrict__ src_all, const int64_t* __restrict__ src_offs,
                                                   const float4* __restrict__ tgt_all, const int64_t* __restrict__ tgt_offs,
                                                   const LmState* __restrict__ st, GicpParams prm, int* __restrict__ corr,
                                                   const int* __restrict__ nn_seed, CertArrays C)
{
    __shared__ int wcnt[16];
    const int pair = blockIdx.y;
    const LmState& S = st[pair];
    if (!S.active || S.phase != 0) return;
    if (pair_motion(S) > prm.motion_switch) return;      // a pair that moved this far goes to the round-3 kernel (nn_pass)
    const int64_t so = src_offs[pair], to = tgt_offs[pair];
    const int n = (int)(src_offs[pair + 1] - so), m = (int)(tgt_offs[pair + 1] - to);
    const int b0 = (int)blockIdx.x * kCertBlock;
    if (b0 >= n) return;
    const float4* src = src_all + so;
    const float4* tgt = tgt_all + to;
    float Tf[12], Tp[12];
    pose_f(S, Tf);
#pragma unroll
    for (int i = 0; i < 12; ++i) Tp[i] = C.t_prev[12 * pair + i];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int rank[4];
    bool need[4];
    // the four points of a lane: every load of a stage is requested before the first one is used (the gathers are what the kernel waits for)
    float4 a[4], nb[4];
    int seed[4];
    float lb[4];
    bool live[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int i = b0 + j * 256 + (int)threadIdx.x;
        live[j] = i < n;
        a[j] = src[live[j] ? i : b0];
        seed[j] = live[j] ? nn_seed[so + i] : -1;
        lb[j] = live[j] ? C.lb[so + i] : 0.0f;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) nb[j] = tgt[(seed[j] >= 0 && seed[j] < m) ? seed[j] : 0];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int i = b0 + j * 256 + (int)threadIdx.x;
        bool certified = false;
        if (live[j] && seed[j] >= 0 && seed[j] < m && lb[j] > 0.0f) {
            const float qx = Tf[0] * a[j].x + Tf[1] * a[j].y + Tf[2] * a[j].z + Tf[3];
            const float qy = Tf[4] * a[j].x + Tf[5] * a[j].y + Tf[6] * a[j].z + Tf[7];
            const float qz = Tf[8] * a[j].x + Tf[9] * a[j].y + Tf[10] * a[j].z + Tf[11];
            const float dx = qx - (Tp[0] * a[j].x + Tp[1] * a[j].y + Tp[2] * a[j].z + Tp[3]);
            const float dy = qy - (Tp[4] * a[j].x + Tp[5] * a[j].y + Tp[6] * a[j].z + Tp[7]);
            const float dz = qz - (Tp[8] * a[j].x + Tp[9] * a[j].y + Tp[10] * a[j].z + Tp[11]);
            const float delta = sqrtf(dx * dx + dy * dy + dz * dz);
            // slack for the float evaluation of T a on both sides of the comparison: 1e-5 relative + 1e-6 m + 4 ulps of the largest
            // coordinate (an ulp at lidar range is 4e-6 m at 60 m: an absolute micrometre alone would rest on this kernel and the search
            // rounding T a identically).  A certificate is exact up to that evaluation error; what fails the test is searched.
            const float slack = 1e-6f + 4.0f * FLT_EPSILON * fmaxf(fmaxf(fabsf(qx), fabsf(qy)), fabsf(qz));
            const float lbn = lb[j] - delta * 1.00001f - slack;
            const float d1sq = dist2(qx, qy, qz, nb[j]);
            if (sqrtf(d1sq) * 1.00001f + slack < lbn) {       // (false for NaN)
                certified = true;
                corr[so + i] = (double)d1sq < prm.max_corr2 ? seed[j] : -1;
                C.lb[so + i] = lbn;
            }
        }
        need[j] = live[j] && !certified;
        const unsigned long long mk = __ballot(need[j]);
        rank[j] = (int)__popcll(mk & ((1ull << lane) - 1ull));
        if (lane == 0) wcnt[j * 4 + wave] = (int)__popcll(mk);
    }
    __syncthreads();
    int total = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        int off = 0;
        for (int u = 0; u < j * 4 + wave; ++u) off += wcnt[u];
        if (need[j]) C.work[so + b0 + off + rank[j]] = b0 + j * 256 + (int)threadIdx.x;
    }
    if (threadIdx.x == 0) {
        for (int u = 0; u < 16; ++u) total += wcnt[u];
        C.bcount[(size_t)pair * C.nb + blockIdx.x] = total;
        const int members = min(kCertBlock, n - b0);
        atomicAdd(&C.searched[(size_t)pair * kStatStride], (unsigned long long)(2 * total > members ? members : total));
        atomicAdd(&C.searched[(size_t)pair * kStatStride + 1], (unsigned long long)members);
    }
}

// the pose of this pass becomes t_prev of every pair that searched; the work-list sizes go to the statistics
__global__ void k_nn_store_pose(const LmState* __restrict__ st, int n_pairs, CertArrays C, int worklists, const int64_t* __restrict__ src_offs,
                                float motion_switch)
{
    const int pair = blockIdx.x * blockDim.x + threadIdx.x;
    if (pair >= n_pairs) return;
    const LmState& S = st[pair];
    if (!S.active || S.phase != 0) return;
    float Tf[12];
    pose_f(S, Tf);
#pragma unroll
    for (int i = 0; i < 12; ++i) C.t_prev[12 * pair + i] = Tf[i];
    const int n_src = (int)(src_offs[pair + 1] - src_offs[pair]);
    if (worklists && !(pair_motion(S) > motion_switch)) return;        // counted block by block in k_nn_certify
    C.searched[(size_t)pair * kStatStride] += (unsigned long long)n_src;      // this pair's own line, one thread per pair, stream-ordered
    C.searched[(size_t)pair * kStatStride + 1] += (unsigned long long)n_src;
}

// G3a, round 4: exact 1-NN of every (float-)transformed source point.  One query per lane; semantics of k_nn_scan (corr = target index in
// sorted space or -1 when d^2 >= max_corr^2; nn_seed = the neighbour found, warm start of the next pass), ties to the smaller index.
// WORK: the queries are the entries of the pair's work list (k_nn_certify) instead of all source points.  Always leaves the certificate
// bound of every query it searched in C.lb.
template <bool WORK>
__global__ __launch_bounds__(kNNThreads) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_nn_scan_g(
    const float4* __restrict__ src_all, const int64_t* __restrict__ src_offs,
    const float4* __restrict__ tgt_all, const int64_t* __restrict__ tgt_offs, HierArrays HA,
    const LmState* __restrict__ st, GicpParams prm, int* __restrict__ corr, int* __restrict__ nn_seed,
    const int* __restrict__ tgt_bbox, CertArrays C)
{
    __shared__ nnc::GrpLds lds[kNNThreads / 64];
    const int pair = blockIdx.y;
    const LmState& S = st[pair];
    if (!S.active || S.phase != 0) return;
    if (WORK && pair_motion(S) > prm.motion_switch) return;
    const int64_t so = src_offs[pair], to = tgt_offs[pair];
    const int n_src = (int)(src_offs[pair + 1] - so), m = (int)(tgt_offs[pair + 1] - to);
    // one workgroup per block of 1024 consecutive source points: its work list, or (no lists, or more than half of the block listed) all of it
    const int b0 = (int)blockIdx.x * kCertBlock;
    if (b0 >= n_src) return;
    const int members = min(kCertBlock, n_src - b0);
    const int listed_n = WORK ? C.bcount[(size_t)pair * C.nb + blockIdx.x] : members;
    const bool listed = WORK && 2 * listed_n <= members;
    const int n = listed ? listed_n : members;
    const float4* src = src_all + so;
    const float4* tgt = tgt_all + to;
    const nnc::LeafHier H = cloud_hier(HA, pair);
    const float maxc2 = prm.max_corr2 < 3.0e38 ? (float)prm.max_corr2 * 1.0001f : INFINITY;
    float Tf[12];
    pose_f(S, Tf);
    float glo[3];
    const float gsc = morton_grid(tgt_bbox, pair, glo);
    nnc::GrpLds& L = lds[threadIdx.x >> 6];
    for (int base = 0; base < n; base += kNNThreads) {
        const int w = base + (int)threadIdx.x;
        const bool live = w < n;
        const int i = listed ? C.work[so + b0 + (live ? w : 0)] : b0 + (live ? w : 0);
        const float4 a = src[i];
        const float qx = Tf[0] * a.x + Tf[1] * a.y + Tf[2] * a.z + Tf[3];
        const float qy = Tf[4] * a.x + Tf[5] * a.y + Tf[6] * a.z + Tf[7];
        const float qz = Tf[8] * a.x + Tf[9] * a.y + Tf[10] * a.z + Tf[11];
        // margin of the search radius beyond the neighbour's distance: what a later pass may certify against.  The volume searched grows
        // with the cube of the radius, so it stays small: it pays in the late passes of an alignment, where a point moves by well under a
        // millimetre per pass (a 6 cm margin made the searches of the early passes 70 times as long and certified nothing there)
        const float margin = prm.cert_margin;
        int seed = live ? nn_seed[so + i] : -1;
        if (live && seed < 0 && m > 0) seed = morton_seed(tgt, m, qx, qy, qz, glo, gsc);   // cold start
        // any target point is an upper bound: last pass's neighbour is nearly always the winner again.  Its distance is formed inside the
        // search's first radius evaluation, after the search has requested the top of the hierarchy: the two loads overlap
        const bool has_seed = live && seed >= 0 && seed < m;
        const float4 sp = tgt[has_seed ? seed : 0];
        float best = INFINITY, second = INFINITY;
        int bidx = -1;
        auto radius2 = [&]() {       // squared search radius: (distance of the best candidate so far + margin)^2, capped by the threshold
            const float r = sqrtf(fminf(has_seed ? dist2(qx, qy, qz, sp) : INFINITY, best)) + margin;
            return fminf(maxc2, r * r);
        };
        nnc::grp_search(tgt, H, L, qx, qy, qz, live, radius2,
                        [&](int j, float d, bool ok) {
                            if (!ok) return;
                            second = __builtin_amdgcn_fmed3f(best, d, second);      // second smallest of everything evaluated
                            if (d < best) { best = d; bidx = j; }
                        });
        if (live) {
            corr[so + i] = (bidx >= 0 && (double)best < prm.max_corr2) ? bidx : -1;
            nn_seed[so + i] = bidx;
            // every point that was not evaluated lies beyond the final radius (radii only shrink while the search runs)
            C.lb[so + i] = bidx >= 0 ? fminf(sqrtf(second), sqrtf(radius2()) * 0.9999f) : 0.0f;
        }
    }
}

template <int KMAX>
__device__ __forceinline__ float kth_of(const float (&dk)[KMAX], int k)
{
    float v = dk[KMAX - 1];
#pragma unroll
    for (int s = 0; s < KMAX - 1; ++s) v = (s == k - 1) ? dk[s] : v;
    return v;
}

// G2 / N1, round 4: exact k nearest neighbours (the point itself included) of every point of every cloud, as cloud-local sorted-space
// indices in (distance, index) order, layout knn_at(); -1 in the slots a cloud with fewer than k points cannot fill.
// Seed: the group's 32 (64 for k > 16) neighbours along the Morton curve give a bound close to the final one; pass 1: the KMAX smallest
// DISTANCES (v_med3 chain, no indices) over the leaves within the shrinking bound -> tau = the exact k-th distance; pass 2: every candidate
// within tau, strictly closer ones from the bottom of a k-slot LDS list, exact ties from its top (they arrive in ascending index order, and a
// tie is only kept while the list still has room for it: at most k - #closer can be needed), so a cluster of duplicates can neither
// overflow the list nor push a closer point out; selection: (distance, index) insertion of the <= k collected.
template <int KMAX>
__global__ __launch_bounds__(kNNThreads) void k_knn_select(const float4* __restrict__ pts_all, const int64_t* __restrict__ offs, HierArrays HA,
                                                           int k, int* __restrict__ knn)
{
    __shared__ nnc::GrpLds lds[kNNThreads / 64];
    __shared__ int lst[KMAX * kNNThreads];          // slot-major: slot s of lane t at lst[s * kNNThreads + t]
    const int c = blockIdx.y;
    const int64_t o = offs[c];
    const int n = (int)(offs[c + 1] - o);
    const float4* pts = pts_all + o;
    const nnc::LeafHier H = cloud_hier(HA, c);
    nnc::GrpLds& L = lds[threadIdx.x >> 6];
    constexpr int HS = KMAX <= 16 ? 32 : 64;
    constexpr int GS = 8;
    const int tid = (int)threadIdx.x;
    for (int base = blockIdx.x * kNNThreads; base < n; base += gridDim.x * kNNThreads) {
        const int i = base + tid;
        const bool live = i < n;
        const float4 q = pts[live ? i : 0];
        float dk[KMAX];
#pragma unroll
        for (int s = 0; s < KMAX; ++s) dk[s] = INFINITY;
        // seed phase: HS consecutive points around the group's queries
        const int hc = min(HS, n);
        const int h0 = max(0, min(base + (tid & ~(GS - 1)) + GS / 2 - HS / 2, n - hc));
        nnc::grp_eval_range(pts, L, q.x, q.y, q.z, h0, hc, [&](int, float d, bool ok) { dist_insert<KMAX>(dk, (ok && live && d == d) ? d : INFINITY); });
        // pass 1: the k-th distance
        nnc::grp_search(pts, H, L, q.x, q.y, q.z, live, [&]() { return kth_of<KMAX>(dk, k); },
                            [&](int j, float d, bool ok) {
                                const bool use = ok && live && (unsigned)(j - h0) >= (unsigned)hc && d == d;
                                dist_insert<KMAX>(dk, use ? d : INFINITY);
                            });
        const float tau = live ? kth_of<KMAX>(dk, k) : -1.0f;
        // pass 2: indices within tau
        int nlt = 0, ntie = 0;
        nnc::grp_search(pts, H, L, q.x, q.y, q.z, live, [&]() { return tau; },
                            [&](int j, float d, bool ok) {
                                if (!(ok && live)) return;
                                if (d < tau) {
                                    lst[min(nlt, KMAX - 1) * kNNThreads + tid] = j;     // at most k - 1 of these; a tie in the way was not needed
                                    ++nlt;
                                    ntie = min(ntie, k - nlt);
                                } else if (d == tau && d < INFINITY && nlt + ntie < k) {
                                    lst[(k - 1 - ntie) * kNNThreads + tid] = j;
                                    ++ntie;
                                }
                            });
        // selection in (distance, index) order
        int ik[KMAX];
#pragma unroll
        for (int s = 0; s < KMAX; ++s) { dk[s] = INFINITY; ik[s] = -1; }
        int most = max(nlt, ntie);
        for (int w = 32; w > 0; w >>= 1) most = max(most, __shfl_xor(most, w, 64));
        for (int e = 0; e < most; ++e) {
            const bool ha = e < nlt, hb = e < ntie;
            const int ja = ha ? lst[e * kNNThreads + tid] : 0;
            const int jb = hb ? lst[(k - 1 - e) * kNNThreads + tid] : 0;
            const float da = dist2(q.x, q.y, q.z, pts[ja]), db = dist2(q.x, q.y, q.z, pts[jb]);
            if (ha) knn_insert_tie<KMAX>(dk, ik, da, ja);
            if (hb) knn_insert_tie<KMAX>(dk, ik, db, jb);
        }
        if (live) {
            int* out = knn + knn_at(o, c, i, k, 0);
#pragma unroll
            for (int s = 0; s < KMAX; ++s)
                if (s < k) out[s << 6] = ik[s];
        }
    }
}

// Second moments of a point's k neighbours in ONE pass over them: sums of d and d d^T with d = p - q taken about the query point q
// (fp64; |d| is a neighbourhood radius, so the subtraction  sum d d^T - n m m^T  cancels a few digits of 16 at most), instead of a pass
// for the mean and a second one about it: half the gathers (30 random 16-byte reads per point instead of 60).
// Memory schedule (round 6): rounds 1-5 walked the slots one by one behind two data-dependent branches each, so that a wave sat out an index
// load AND a dependent gather per neighbour, ~30 round trips in a row (10 k cycles per wave for ~4 k cycles of arithmetic).  Now the slots
// are taken in chunks of kMomChunk: the indices of a chunk (one coalesced 256-byte row per slot and wave; slots past k re-read slot k - 1) are
// requested two chunks ahead of the sums and its points one chunk ahead, so that loads of 2 x kMomChunk neighbours are in flight while a chunk is summed.  An empty slot (-1: a cloud with fewer than k points)
// gathers the query itself and contributes exact zeros, so the sums are those of the slot-by-slot loop bit for bit.
// cv: full symmetric 3x3 of  sum (p - mean)(p - mean)^T  (not yet divided); returns the number of neighbours.
constexpr int kMomChunk = 5;      // 15 / 20 / 30 neighbours (GICP default, the oracle's k, RING++) are whole chunks
template <int KMAX, bool WANT_Z>
__device__ __forceinline__ int neighbour_moments(const float4* __restrict__ pts, const int* __restrict__ nb /* slot s at nb[64 s] */, int k, int self,
                                                 const float4& q, double (&cv)[9], float (&nz)[KMAX])
{
#pragma clang fp contract(fast)
    constexpr int NCH = (KMAX + kMomChunk - 1) / kMomChunk;
    int idx[3][kMomChunk];                                 // chunk c lives in [c % 3]: indices run two chunks ahead of the sums, points one
    float px[2][kMomChunk], py[2][kMomChunk], pz[2][kMomChunk];
    auto indices = [&](int c) {
#pragma unroll
        for (int j = 0; j < kMomChunk; ++j) idx[c % 3][j] = nb[min(c * kMomChunk + j, k - 1) << 6];
    };
    auto gather = [&](int c) {
#pragma unroll
        for (int j = 0; j < kMomChunk; ++j) {
            const int id = idx[c % 3][j];
            const float4 p = pts[id >= 0 ? id : self];
            px[c & 1][j] = p.x; py[c & 1][j] = p.y; pz[c & 1][j] = p.z;
        }
    };
    double sd[3] = {0, 0, 0}, sc[6] = {0, 0, 0, 0, 0, 0};
    int cnt = 0;
    indices(0);
    if (NCH > 1) indices(1);
    gather(0);
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        if (c * kMomChunk < k) {                                       // uniform: k is a kernel argument
            if (c + 2 < NCH && (c + 2) * kMomChunk < k) indices(c + 2);
            if (c + 1 < NCH && (c + 1) * kMomChunk < k) gather(c + 1);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < kMomChunk; ++j) {
                const int s = c * kMomChunk + j;
                const bool ok = s < k && idx[c % 3][j] >= 0;
                const float fx = px[c & 1][j], fy = py[c & 1][j], fz = pz[c & 1][j];
                const double dx = ok ? (double)fx - (double)q.x : 0.0, dy = ok ? (double)fy - (double)q.y : 0.0, dz = ok ? (double)fz - (double)q.z : 0.0;
                sd[0] += dx; sd[1] += dy; sd[2] += dz;
                sc[0] += dx * dx; sc[1] += dx * dy; sc[2] += dx * dz;
                sc[3] += dy * dy; sc[4] += dy * dz; sc[5] += dz * dz;
                if (WANT_Z && s < KMAX) nz[s] = ok ? fz : 0.0f;
                cnt += ok ? 1 : 0;
            }
        } else if (WANT_Z) {
#pragma unroll
            for (int j = 0; j < kMomChunk; ++j)
                if (c * kMomChunk + j < KMAX) nz[c * kMomChunk + j] = 0.0f;
        }
    }
    const double inv = 1.0 / (double)cnt;
    cv[0] = sc[0] - sd[0] * sd[0] * inv; cv[1] = sc[1] - sd[0] * sd[1] * inv; cv[2] = sc[2] - sd[0] * sd[2] * inv;
    cv[4] = sc[3] - sd[1] * sd[1] * inv; cv[5] = sc[4] - sd[1] * sd[2] * inv; cv[8] = sc[5] - sd[2] * sd[2] * inv;
    cv[3] = cv[1]; cv[6] = cv[2]; cv[7] = cv[5];
    return cnt;
}

// G2 tail: covariance of the k neighbours (fp64) + PLANE regularisation.  One point per lane; knn = the selection's output (knn_at).
// knn_out optional, ORIGINAL indexing.
__global__ __launch_bounds__(256) void k_cov_from_knn(const float4* __restrict__ pts_all, const int64_t* __restrict__ offs, int k,
                                                     const int* __restrict__ knn, double* __restrict__ cov_all, int* __restrict__ knn_out)
{
    const int c = blockIdx.y;
    const int64_t o = offs[c];
    const int n = (int)(offs[c + 1] - o);
    const float4* pts = pts_all + o;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int* nb = knn + knn_at(o, c, i, k, 0);       // slot s at nb[64 s]: one row per wave and slot
        const float4 q = pts[i];
        double cv[9];
        float unused[32];
        const int cnt = neighbour_moments<32, false>(pts, nb, k, i, q, cv, unused);
        for (int a = 0; a < 9; ++a) cv[a] /= cnt;
        double nrm[3];
        mrs::smallest_eigvec(cv, nrm);
        double* out = cov_all + kCovDoubles * (size_t)(o + i);      // the unit normal: C = I - 0.999 n n^T is rebuilt by the readers (cov6_from_normal)
        out[0] = nrm[0]; out[1] = nrm[1]; out[2] = nrm[2];
        if (knn_out) {
            const int oi = __float_as_int(q.w);
            for (int s = 0; s < k; ++s) knn_out[(size_t)(o + oi) * k + s] = nb[s << 6] >= 0 ? __float_as_int(pts[nb[s << 6]].w) : -1;
        }
    }
}

// N1 tail: covariance P^T P / (k - 1) (util.py:123-131) -> eigenvalues of the 3x3 and of its xy 2x2 block, both descending (util.py:134-158) ->
// the 13 hand-crafted features of every point from its k neighbours.  Outputs in the caller's ORIGINAL point order; feat_planes (optional)
// receives the channel-major [9][n] planes x,y,z,C,O,E,L2,dZ,vZ that generate_RINGplusplus feeds to the feature BEV (util.py:220-228).
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) void k_feat_from_knn(const float4* __restrict__ pts_all, const int64_t* __restrict__ offs, int k,
                                                      const int* __restrict__ knn, int* __restrict__ knn_out, float* __restrict__ eig_out,
                                                      float* __restrict__ feat_out, float* __restrict__ feat_planes)
{
    const int c = blockIdx.y;
    const int64_t o = offs[c];
    const int n = (int)(offs[c + 1] - o);
    const float4* pts = pts_all + o;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int* nb = knn + knn_at(o, c, i, k, 0);       // slot s at nb[64 s]
        const float4 q = pts[i];
        const int oi = __float_as_int(q.w);
        double cv[9];
        float nz[32];
        const int cnt = neighbour_moments<32, true>(pts, nb, k, i, q, cv, nz);
        for (int a = 0; a < 9; ++a) cv[a] /= (double)(cnt - 1);
        double w[3];
        mrs::sym3_eigvals(cv, w);
        const double hm = 0.5 * (cv[0] + cv[4]), hd = 0.5 * (cv[0] - cv[4]);
        const double rad = sqrt(hd * hd + cv[1] * cv[1]);
        float e[5] = {(float)w[0], (float)w[1], (float)w[2], (float)(hm + rad), (float)(hm - rad)};
        float f[13];
        point_features(e, nz, cnt, f);     // cnt = min(k, n): a cloud with fewer than k points gives what k = n gives (no phantom neighbours at z = 0)
        const size_t gi = (size_t)(o + oi);
        if (knn_out)
            for (int s = 0; s < k; ++s) knn_out[gi * k + s] = nb[s << 6] >= 0 ? __float_as_int(pts[nb[s << 6]].w) : -1;
        if (eig_out) for (int j = 0; j < 5; ++j) eig_out[gi * 5 + j] = e[j];
        if (feat_out) for (int j = 0; j < 13; ++j) feat_out[gi * 13 + j] = f[j];
        if (feat_planes) {
            float* pl = feat_planes + (size_t)9 * o;  // scan-local channel-major planes
            pl[0 * (size_t)n + oi] = q.x; pl[1 * (size_t)n + oi] = q.y; pl[2 * (size_t)n + oi] = q.z;
            pl[3 * (size_t)n + oi] = f[0]; pl[4 * (size_t)n + oi] = f[1]; pl[5 * (size_t)n + oi] = f[3];
            pl[6 * (size_t)n + oi] = f[10]; pl[7 * (size_t)n + oi] = f[11]; pl[8 * (size_t)n + oi] = f[12];
        }
    }
}

// ---- G7: voxelised GICP (fast_gicp FastVGICP / FastVGICPCuda; Koide et al., ICRA 2021) ---------------------
// The target is summarised per voxel of edge `res`: mean of its points and mean of their (regularised)
// covariances (ADDITIVE accumulation).  A transformed source point corresponds to the voxel that contains it
// (DIRECT1) and optionally its 6 / 26 neighbours; each correspondence is a distribution-to-distribution term
// weighted by sqrt(points in the voxel).  max_correspondence_distance is not used.  Parity unpinned: restated
// from the publication and SURVEY.md row G7 (the submodule is absent).  Conventions of upstream's CUDA voxel map:
// voxel coordinate = floor(x / resolution - 0.5) in float arithmetic on the float-transformed point
// (calc_voxel_coord); correspondences and (C_voxel + R C_A R^T)^-1 belong to the linearisation pose, LM trials
// (compute_error) only re-evaluate the residuals (x_linearized / x_eval in upstream's kernels).
__device__ __forceinline__ int voxel_coord_f(float v, float res) { return (int)floorf(v / res - 0.5f); }

__device__ __forceinline__ unsigned long long voxel_key(int cloud, int ix, int iy, int iz)
{
    return ((unsigned long long)cloud << 48) | ((unsigned long long)(ix & 0xffff) << 32) |
           ((unsigned long long)(iy & 0xffff) << 16) | (unsigned long long)(iz & 0xffff);
}

__global__ void k_vox_keys(const float4* __restrict__ pts, const int64_t* __restrict__ offs, double res,
                           unsigned long long* __restrict__ keys, int* __restrict__ vals)
{
    const int c = blockIdx.y;
    const int64_t o = offs[c];
    const int n = (int)(offs[c + 1] - o);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float4 p = pts[o + i];
        const float resf = (float)res;
        keys[o + i] = voxel_key(c, voxel_coord_f(p.x, resf) + 32768, voxel_coord_f(p.y, resf) + 32768,
                                voxel_coord_f(p.z, resf) + 32768);
        vals[o + i] = (int)(o + i);
    }
}

__global__ void k_vox_heads(const unsigned long long* __restrict__ keys, size_t n, int* __restrict__ head)
{
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        head[i] = (i == 0 || keys[i] != keys[i - 1]) ? 1 : 0;
}

// one lane per voxel head: key, mean (w = count) and mean covariance of the voxel
__global__ void k_vox_build(const float4* __restrict__ pts, const double* __restrict__ cov, const unsigned long long* __restrict__ keys,
                            const int* __restrict__ perm, const int* __restrict__ head, const int* __restrict__ slot, size_t n,
                            unsigned long long* __restrict__ vkeys, float4* __restrict__ vmean, double* __restrict__ vcov)
{
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        if (!head[i]) continue;
        const unsigned long long k = keys[i];
        double m[3] = {0, 0, 0}, c[6] = {0, 0, 0, 0, 0, 0};
        int cnt = 0;
        for (size_t j = i; j < n && keys[j] == k; ++j) {
            const float4 p = pts[perm[j]];
            m[0] += (double)p.x; m[1] += (double)p.y; m[2] += (double)p.z;
            double cp[6];
            cov6_from_normal(cov + kCovDoubles * (size_t)perm[j], cp);
            for (int a = 0; a < 6; ++a) c[a] += cp[a];
            ++cnt;
        }
        const int v = slot[i];
        vkeys[v] = k;
        vmean[v] = make_float4((float)(m[0] / cnt), (float)(m[1] / cnt), (float)(m[2] / cnt), (float)cnt);
        for (int a = 0; a < 6; ++a) vcov[6 * (size_t)v + a] = c[a] / cnt;
    }
}

// G7 linearisation: voxel lookup (binary search in the sorted voxel keys) fused with the 28 fp64 sums.
__global__ __launch_bounds__(kNNThreads) void k_linearize_voxel(
    const float4* __restrict__ src_all, const int64_t* __restrict__ src_offs, const double* __restrict__ src_cov,
    const unsigned long long* __restrict__ vkeys, const float4* __restrict__ vmean, const double* __restrict__ vcov,
    int n_voxels, const LmState* __restrict__ st, GicpParams prm, double* __restrict__ partial, int max_blocks)
{
    __shared__ double red[kNNThreads / 64][kTerms];
    const int pair = blockIdx.y;
    const LmState& S = st[pair];
    if (!S.active) return;
    const int64_t so = src_offs[pair];
    const int n = (int)(src_offs[pair + 1] - so);
    const float4* src = src_all + so;
    double* pout = partial + ((size_t)pair * max_blocks + blockIdx.x) * kTerms;
    const bool error_only = S.phase == 1;
    double T[12], TL[12];
    float Tf[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) { T[i] = S.xi[i]; TL[i] = S.x[i]; Tf[i] = (float)S.x[i]; }
    double acc[kTerms];
#pragma unroll
    for (int i = 0; i < kTerms; ++i) acc[i] = 0.0;
    const int per_block = kNNThreads * kPts;
    const int nn = prm.voxel_neighbors;
    const float resf = (float)prm.voxel_res;
    for (int base = blockIdx.x * per_block; base < n; base += gridDim.x * per_block) {
#pragma unroll 1
        for (int p = 0; p < kPts; ++p) {
            const int i = base + p * kNNThreads + threadIdx.x;
            if (i >= n) continue;
            const float4 a = src[i];
            double ta[3];
#pragma unroll
            for (int r = 0; r < 3; ++r)
                ta[r] = T[4 * r] * (double)a.x + T[4 * r + 1] * (double)a.y + T[4 * r + 2] * (double)a.z + T[4 * r + 3];
            // voxel of the float-transformed point at the LINEARISATION pose
            const int cx = voxel_coord_f(Tf[0] * a.x + Tf[1] * a.y + Tf[2] * a.z + Tf[3], resf) + 32768,
                      cy = voxel_coord_f(Tf[4] * a.x + Tf[5] * a.y + Tf[6] * a.z + Tf[7], resf) + 32768,
                      cz = voxel_coord_f(Tf[8] * a.x + Tf[9] * a.y + Tf[10] * a.z + Tf[11], resf) + 32768;
            double ca[6];
            cov6_from_normal(src_cov + kCovDoubles * (size_t)(so + i), ca);
            const double CA[9] = {ca[0], ca[1], ca[2], ca[1], ca[3], ca[4], ca[2], ca[4], ca[5]};
            double RC[9], RCRa[9];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    RC[3 * r + c] = TL[4 * r] * CA[c] + TL[4 * r + 1] * CA[3 + c] + TL[4 * r + 2] * CA[6 + c];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    RCRa[3 * r + c] = RC[3 * r] * TL[4 * c] + RC[3 * r + 1] * TL[4 * c + 1] + RC[3 * r + 2] * TL[4 * c + 2];
#pragma unroll 1
            for (int o = 0; o < 27; ++o) {
                const int dx = o % 3 - 1, dy = (o / 3) % 3 - 1, dz = o / 9 - 1;
                const int man = abs(dx) + abs(dy) + abs(dz);
                if ((nn == 1 && man != 0) || (nn == 7 && man > 1)) continue;
                const unsigned long long key = voxel_key(pair, cx + dx, cy + dy, cz + dz);
                int lo = 0, hi = n_voxels;  // first index with vkeys >= key
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (vkeys[mid] < key) lo = mid + 1; else hi = mid;
                }
                if (lo >= n_voxels || vkeys[lo] != key) continue;
                const float4 vm = vmean[lo];
                const double* cb = vcov + 6 * (size_t)lo;
                double RCR[9], M[9];
                RCR[0] = RCRa[0] + cb[0]; RCR[1] = RCRa[1] + cb[1]; RCR[2] = RCRa[2] + cb[2];
                RCR[3] = RCRa[3] + cb[1]; RCR[4] = RCRa[4] + cb[3]; RCR[5] = RCRa[5] + cb[4];
                RCR[6] = RCRa[6] + cb[2]; RCR[7] = RCRa[7] + cb[4]; RCR[8] = RCRa[8] + cb[5];
                if (!inv3_sym(RCR, M)) continue;
                const double w = sqrt((double)vm.w);
                double e[3] = {(double)vm.x - ta[0], (double)vm.y - ta[1], (double)vm.z - ta[2]}, Me[3];
#pragma unroll
                for (int r = 0; r < 3; ++r) Me[r] = M[3 * r] * e[0] + M[3 * r + 1] * e[1] + M[3 * r + 2] * e[2];
                acc[27] += w * (e[0] * Me[0] + e[1] * Me[1] + e[2] * Me[2]);
                if (error_only) continue;
                const double J[18] = {0, -ta[2], ta[1], -1, 0, 0,
                                      ta[2], 0, -ta[0], 0, -1, 0,
                                      -ta[1], ta[0], 0, 0, 0, -1};
                double MJ[18];
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int c = 0; c < 6; ++c)
                        MJ[6 * r + c] = M[3 * r] * J[c] + M[3 * r + 1] * J[6 + c] + M[3 * r + 2] * J[12 + c];
#pragma unroll
                for (int r = 0; r < 6; ++r) {
#pragma unroll
                    for (int c = r; c < 6; ++c)
                        acc[r * 6 - (r * (r - 1)) / 2 + (c - r)] += w * (J[r] * MJ[c] + J[6 + r] * MJ[6 + c] + J[12 + r] * MJ[12 + c]);
                }
#pragma unroll
                for (int r = 0; r < 6; ++r) acc[21 + r] += w * (J[r] * Me[0] + J[6 + r] * Me[1] + J[12 + r] * Me[2]);
            }
        }
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int i = 0; i < kTerms; ++i) {
        const double v = wave_sum_d(acc[i]);
        if (lane == 0) red[wave][i] = v;
    }
    __syncthreads();
    if (threadIdx.x < kTerms) {
        double v = 0;
        for (int w = 0; w < kNNThreads / 64; ++w) v += red[w][threadIdx.x];
        pout[threadIdx.x] = v;
    }
}

// ---- device-side LM bookkeeping (one lane per pair) ------------------------------------------
__device__ void mul4d(const double* a, const double* b, double* c)
{
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double s = 0;
            for (int k = 0; k < 4; ++k) s += a[4 * i + k] * b[4 * k + j];
            c[4 * i + j] = s;
        }
}

__device__ void se3_exp_d(const double* a, double* T)
{
    const double wx = a[0], wy = a[1], wz = a[2];
    const double theta_sq = wx * wx + wy * wy + wz * wz;
    double imag, real, theta = 0;
    if (theta_sq < 1e-10) {
        const double t4 = theta_sq * theta_sq;
        imag = 0.5 - (1.0 / 48.0) * theta_sq + (1.0 / 3840.0) * t4;
        real = 1.0 - (1.0 / 8.0) * theta_sq + (1.0 / 384.0) * t4;
    } else {
        theta = sqrt(theta_sq);
        imag = sin(0.5 * theta) / theta;
        real = cos(0.5 * theta);
    }
    double qw = real, qx = imag * wx, qy = imag * wy, qz = imag * wz;
    const double nq = sqrt(qw * qw + qx * qx + qy * qy + qz * qz);
    qw /= nq; qx /= nq; qy /= nq; qz /= nq;
    const double R[9] = {1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qz * qw), 2 * (qx * qz + qy * qw),
                         2 * (qx * qy + qz * qw), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qx * qw),
                         2 * (qx * qz - qy * qw), 2 * (qy * qz + qx * qw), 1 - 2 * (qx * qx + qy * qy)};
    double V[9];
    if (theta < 1e-10) {
        for (int i = 0; i < 9; ++i) V[i] = R[i];
    } else {
        const double O[9] = {0, -wz, wy, wz, 0, -wx, -wy, wx, 0};
        double O2[9];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) O2[3 * i + j] = O[3 * i] * O[j] + O[3 * i + 1] * O[3 + j] + O[3 * i + 2] * O[6 + j];
        const double c1 = (1.0 - cos(theta)) / theta_sq, c2 = (theta - sin(theta)) / (theta_sq * theta);
        for (int i = 0; i < 9; ++i) V[i] = (i % 4 == 0 ? 1.0 : 0.0) + c1 * O[i] + c2 * O2[i];
    }
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) T[4 * i + j] = R[3 * i + j];
        T[4 * i + 3] = V[3 * i] * a[3] + V[3 * i + 1] * a[4] + V[3 * i + 2] * a[5];
    }
    T[12] = T[13] = T[14] = 0; T[15] = 1;
}

__device__ bool solve6_d(const double* Hin, const double* rhs, double* x)
{
    double L[36], D[6];
    for (int i = 0; i < 36; ++i) L[i] = 0;
    for (int j = 0; j < 6; ++j) {
        double d = Hin[6 * j + j];
        for (int k = 0; k < j; ++k) d -= L[6 * j + k] * L[6 * j + k] * D[k];
        D[j] = d;
        if (d == 0.0 || !(d == d)) return false;
        for (int i = j + 1; i < 6; ++i) {
            double s = Hin[6 * i + j];
            for (int k = 0; k < j; ++k) s -= L[6 * i + k] * L[6 * j + k] * D[k];
            L[6 * i + j] = s / d;
        }
    }
    double y[6];
    for (int i = 0; i < 6; ++i) { double s = rhs[i]; for (int k = 0; k < i; ++k) s -= L[6 * i + k] * y[k]; y[i] = s; }
    for (int i = 0; i < 6; ++i) y[i] /= D[i];
    for (int i = 5; i >= 0; --i) { double s = y[i]; for (int k = i + 1; k < 6; ++k) s -= L[6 * k + i] * x[k]; x[i] = s; }
    return true;
}

__device__ bool is_converged_d(const GicpParams& p, const double* delta)
{
    double mr = 0, mt = 0;
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) mr = fmax(mr, p.conv_factor * fabs(delta[4 * i + j] - (i == j ? 1.0 : 0.0)) / p.rot_eps);
        mt = fmax(mt, p.conv_factor * fabs(delta[4 * i + 3]) / p.trans_eps);
    }
    return fmax(mr, mt) < 1.0;
}

// propose the next candidate from (H, b, lambda); marks the pair failed if the solve breaks down
__device__ void propose(LmState& S)
{
    double Hl[36], rhs[6];
    for (int i = 0; i < 36; ++i) Hl[i] = S.H[i];
    for (int i = 0; i < 6; ++i) { Hl[7 * i] += S.lambda; rhs[i] = -S.b[i]; }
    if (!solve6_d(Hl, rhs, S.d)) { S.failed = 1; S.active = 0; S.phase = 2; return; }
    se3_exp_d(S.d, S.delta);
    mul4d(S.delta, S.x, S.xi);
    ++S.trials;
}

// LsqRegistration::step_lm / computeTransformation bookkeeping; grid = pairs, 64 lanes each.
//   phase 0 result = linearize(x0): H, b, y0 -> first LM candidate, phase 1
//   phase 1 result = compute_error(delta * x0) on the cached correspondences -> rho -> accept (x0 <- xi, next
//   outer iteration linearises again: phase 0) or reject (lambda *= nu, next candidate, stay in phase 1)
// n_next[0] counts the pairs that need a linearisation next tick, n_next[1] the pairs in an LM trial, n_next[2] those of [0] that moved
// farther than prm.motion_switch in the step just accepted.
constexpr int kLmThreads = 256;     // four waves share the 28 terms of the final sum (rounds 1-5: one wave, 28 dependent reductions in a row)
__global__ __launch_bounds__(kLmThreads) void k_lm_update(LmState* __restrict__ st, const double* __restrict__ partial, const int* __restrict__ nblocks,
                            int max_blocks, GicpParams prm, int* __restrict__ n_next, int trial_only)
{
    const int pair = blockIdx.x;
    LmState& S = st[pair];
    if (!S.active) return;
    if (trial_only && S.phase == 0) {                   // see k_linearize: the pair waits for the next full tick; it still counts as "to linearise"
        if (threadIdx.x == 0) {
            atomicAdd(&n_next[0], 1);
            if (pair_motion(S) > prm.motion_switch) atomicAdd(&n_next[2], 1);
        }
        return;
    }
    __shared__ double sum[kTerms];
    {   // fixed-order (deterministic) final sum of the per-workgroup partials: lane l adds blocks l, l + 64, ...
        // in ascending order, then one wave butterfly per term; wave w takes the terms t0 + w, t0 + w + 4, ... (the order INSIDE a term is
        // what fixes its bits, and that is unchanged)
        const double* p = partial + (size_t)pair * max_blocks * kTerms;
        const int nb = nblocks[pair];
        const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
        for (int t = (S.phase == 1 ? kTerms - 1 : 0) + wave; t < kTerms; t += kLmThreads / 64) {
            double v = 0;
            for (int b = lane; b < nb; b += 64) v += p[(size_t)b * kTerms + t];
            v = wave_sum_d(v);
            if (lane == 0) sum[t] = v;
        }
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const double y = sum[27];
    const int limit = prm.force_iters > 0 ? prm.force_iters : prm.max_iter;
    if (S.phase == 0) n_next[3] = 1;                    // this tick carried a linearisation (= a nearest-neighbour pass): counted by the host

    if (S.phase == 0) {
        int t = 0;
        for (int r = 0; r < 6; ++r)
            for (int c = r; c < 6; ++c) { S.H[6 * r + c] = sum[t]; S.H[6 * c + r] = sum[t]; ++t; }
        for (int r = 0; r < 6; ++r) S.b[r] = sum[21 + r];
        S.y0 = y;
        if (S.lambda < 0.0) {
            double mx = 0;
            for (int i = 0; i < 6; ++i) mx = fmax(mx, fabs(S.H[7 * i]));
            S.lambda = prm.lm_init_factor * mx;
        }
        S.nu = 2.0;
        S.inner = 0;
        S.phase = 1;
        propose(S);
    } else {
        double denom = 0;
        for (int i = 0; i < 6; ++i) denom += S.d[i] * (S.lambda * S.d[i] - S.b[i]);
        const double rho = (S.y0 - y) / denom;
        bool stepped = false;   // step_lm returned true: one outer iteration is complete
        if (!(rho == rho)) {
            S.failed = 1; S.active = 0; S.phase = 2;
        } else if (rho < 0) {
            if (is_converged_d(prm, S.delta)) {
                stepped = true;     // returns true without moving; the outer loop then sees a converged delta
            } else {
                S.lambda = S.nu * S.lambda;
                S.nu = 2 * S.nu;
                ++S.inner;
                if (S.inner >= prm.lm_max_iter) { S.failed = 1; S.active = 0; S.phase = 2; }  // "lm not converged"
                else propose(S);
            }
        } else {
            for (int i = 0; i < 16; ++i) S.x[i] = S.xi[i];
            const double w = 2 * rho - 1;
            S.lambda = S.lambda * fmax(1.0 / 3.0, 1.0 - w * w * w);
            for (int i = 0; i < 36; ++i) S.final_H[i] = S.H[i];
            stepped = true;
        }
        if (stepped) {
            ++S.outer;
            const bool conv = prm.force_iters > 0 ? false : is_converged_d(prm, S.delta);
            if (conv) S.converged = 1;
            if (conv || S.outer >= limit) { S.active = 0; S.phase = 2; }
            else {
                for (int i = 0; i < 16; ++i) S.xi[i] = S.x[i];
                S.phase = 0;
            }
        }
    }
    if (S.active) atomicAdd(&n_next[S.phase == 0 ? 0 : 1], 1);
    if (S.active && S.phase == 0 && pair_motion(S) > prm.motion_switch) atomicAdd(&n_next[2], 1);   // pairs whose next search is a broad one
}

// G6: fitness partials: [pair][block][2] = (sum of d^2 <= max_range, count)
__global__ __launch_bounds__(kNNThreads) void k_fitness(const float4* __restrict__ src_all,
                                                        const int64_t* __restrict__ src_offs,
                                                        const float4* __restrict__ tgt_all,
                                                        const int64_t* __restrict__ tgt_offs,
                                                        const int* __restrict__ tgt_tile_base,
                                                        const float4* __restrict__ tlo, const float4* __restrict__ thi,
        const float4* __restrict__ mlo, const float4* __restrict__ mhi,
                                                        const double* __restrict__ poses /* [pairs][16] */,
                                                        double max_range, double* __restrict__ partial, int max_blocks,
                                                        const int* __restrict__ nn_seed /* optional warm start */)
{
    __shared__ double red[kNNThreads / 64][2];
    const int pair = blockIdx.y;
    const int64_t so = src_offs[pair], to = tgt_offs[pair];
    const int n = (int)(src_offs[pair + 1] - so), m = (int)(tgt_offs[pair + 1] - to);
    const float4* src = src_all + so;
    const float4* tgt = tgt_all + to;
    Hier H;
    H.tlo = tlo + tgt_tile_base[pair]; H.thi = thi + tgt_tile_base[pair];
    H.mlo = mlo + (size_t)64 * tgt_tile_base[pair]; H.mhi = mhi + (size_t)64 * tgt_tile_base[pair];
    H.ntiles = (m + kTile - 1) / kTile;
    const float maxc2 = max_range < 3.0e38 ? (float)max_range * 1.0001f : INFINITY;
    float Tf[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) Tf[i] = (float)poses[(size_t)pair * 16 + i];
    constexpr int PF = 2;  // source points per lane (see launch_nn_scan); the grid-stride loop covers any grid
    const int per_block = kNNThreads * PF;
    double s = 0, c = 0;
    for (int base = blockIdx.x * per_block; base < n; base += gridDim.x * per_block) {
        float qx[PF], qy[PF], qz[PF];
        int si[PF];
        bool live[PF];
#pragma unroll
        for (int p = 0; p < PF; ++p) {
            si[p] = base + (threadIdx.x >> 6) * (64 * PF) + p * 64 + (threadIdx.x & 63);
            live[p] = si[p] < n;
            const float4 a = src[live[p] ? si[p] : 0];
            qx[p] = Tf[0] * a.x + Tf[1] * a.y + Tf[2] * a.z + Tf[3];
            qy[p] = Tf[4] * a.x + Tf[5] * a.y + Tf[6] * a.z + Tf[7];
            qz[p] = Tf[8] * a.x + Tf[9] * a.y + Tf[10] * a.z + Tf[11];
        }
        float best[PF];
        int bidx[PF];
        int seed[PF];   // the neighbours of the last alignment pass: valid upper bounds at any pose
#pragma unroll
        for (int p = 0; p < PF; ++p) seed[p] = (nn_seed && live[p]) ? nn_seed[so + si[p]] : -1;
        nn_scan<PF>(tgt, m, H, maxc2, qx, qy, qz, live, best, bidx, seed);
#pragma unroll
        for (int p = 0; p < PF; ++p)
            if (live[p] && bidx[p] >= 0 && (double)best[p] <= max_range) { s += (double)best[p]; c += 1.0; }
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    s = wave_sum_d(s); c = wave_sum_d(c);
    if (lane == 0) { red[wave][0] = s; red[wave][1] = c; }
    __syncthreads();
    if (threadIdx.x < 2) {
        double v = 0;
        for (int w = 0; w < kNNThreads / 64; ++w) v += red[w][threadIdx.x];
        partial[((size_t)pair * max_blocks + blockIdx.x) * 2 + threadIdx.x] = v;
    }
}

// corr (sorted space) -> caller's indexing: out[so + orig_src] = orig_tgt (or -1)
__global__ void k_corr_to_original(const float4* __restrict__ src_all, const int64_t* __restrict__ src_offs,
                                   const float4* __restrict__ tgt_all, const int64_t* __restrict__ tgt_offs,
                                   const int* __restrict__ corr, int* __restrict__ out)
{
    const int pair = blockIdx.y;
    const int64_t so = src_offs[pair], to = tgt_offs[pair];
    const int n = (int)(src_offs[pair + 1] - so);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int j = corr[so + i];
        out[so + __float_as_int(src_all[so + i].w)] = j >= 0 ? __float_as_int(tgt_all[to + j].w) : -1;
    }
}

}  // namespace
