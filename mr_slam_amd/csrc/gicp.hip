// gicp.hip -- host side of the batched GICP refinement: the handle (owning device buffers), the launch helpers and the C entry points.
// The kernels and the design notes are in gicp_device.hpp, included here and nowhere else (one translation unit).
// Four registration methods run on the one handle, each an Estimator behind the one tick driver (run_ticks): fast_gicp's LM-GICP and its voxelised
// variant, point-to-point ICP (row G9, icp_device.hpp), PCL-style GICP (row G11, pclgicp_device.hpp) and point-to-plane ICP (row G12,
// icp_plane_device.hpp; the normals' entry points follow the covariances').
#include <hipcub/hipcub.hpp>

#include <cstdlib>
#include <functional>
#include <type_traits>

#include "common.hpp"
#include "gicp_device.hpp"
#include "icp_device.hpp"
#include "icp_plane_device.hpp"
#include "pclgicp_device.hpp"

// Small batches (<= kLmWindowPairs pairs: ONE registration at a time is how the nodes call it, main_RING.py:81-104, global_manager.cpp:2016-2021)
// run the LM schedule in windows of kLmWindow ticks without a host round trip in between: every kernel of a tick gates itself on the pair's
// device-side state (active / phase / motion), so a tick launched for a pair that has converged, or the search kernels of a tick that is an LM
// trial, are empty launches.  The host reads the per-tick counters once per window instead of copying + synchronising after every tick
// (rounds 1-5: ~10 round trips of 40-60 us per registration of two 35 k-point clouds).  Same kernels on the same state: same bits.
constexpr int kLmWindowPairs = 8;
constexpr int kLmWindow = 4;
constexpr int kLmWindowMax = 16;
constexpr int kNormalsGiven = -1;     // GicpCloud::nrm_key
using mrs::DeviceBuffer;

// The clouds of one side of a batch (0: sources, 1: targets), in Morton order, with everything built from them.  All device memory is owned
// here: dropping a GicpCloud frees it.  The buffers are kept across setInput* calls and only re-allocated when the clouds outgrow them.
struct GicpCloud {
    bool ready = false;               // set_clouds / set_clouds_from completed: the members below describe the side's current clouds
    std::vector<int64_t> offs;        // host copy of the cloud offsets [n_pairs + 1]
    int64_t longest = 0;              // points of the largest cloud
    int max_tiles = 0;                // 1024-point tiles of the largest cloud
    bool cov_valid = false;
    bool hier_valid = false;
    int nrm_key = 0;                  // the normals in `nrm`: 0 none, kNormalsGiven the caller's (set_normals), else the k they were computed with
    double nrm_vp[3] = {0, 0, 0};     // ... and their viewpoint
    DeviceBuffer<int64_t> d_offs;
    DeviceBuffer<float4> pts;         // total + total / 8 points (+ 16: a mini's 16 candidates are read whole, cand_request)
    DeviceBuffer<float4> nrm;         // sorted space: (unit normal, curvature) of every point (row G12), allocated by the first call that fills it
    DeviceBuffer<double> cov;         // sorted space: the unit normal of every point (kCovDoubles = 3 doubles; cov6_from_normal); none under no_cov
    DeviceBuffer<int> tile_base;      // [n_pairs] first tile of each cloud
    DeviceBuffer<int> bbox;           // [n_pairs][6] bounding box of each cloud (ordered ints), the Morton grid
    DeviceBuffer<float4> tlo, thi;    // tile bounding boxes (tiles + tiles / 8 + 1)
    DeviceBuffer<float4> mlo, mhi;    // boxes of the 64 minis (16 points) of every tile
    // round-4 search structure (nn_core.hpp): octree-cell leaves of <= 16 points, tiles of 64 leaves, supers of 64 tiles, per cloud
    DeviceBuffer<float4> llo, lhi, t2lo, t2hi, slo, shi;
    DeviceBuffer<int> leaf_first, tile_first, super_first;          // [n_pairs + 1] each
    std::vector<int> h_leaf_first, h_tile_first, h_super_first;     // host copies (set_clouds_from re-bases them)
    HierArrays hier() const
    {
        return HierArrays{llo.get(), lhi.get(), t2lo.get(), t2hi.get(), slo.get(), shi.get(), leaf_first.get(), tile_first.get(), super_first.get()};
    }
};

// Device-side state of an alignment.  corr, seed and the certificates are sized with the source side's points (prepare_side).
struct GicpLmBuffers {
    DeviceBuffer<LmState> state;
    DeviceBuffer<double> partial;     // [n_pairs][>= max_blocks][kTerms]
    DeviceBuffer<int> nblocks, nactive;
    DeviceBuffer<int> corr;           // [total source points] correspondences of the current evaluation
    DeviceBuffer<int> seed;           // [total source points] last nearest neighbour (warm start of the next NN pass)
    size_t n_seed = 0;
    int max_blocks = 0;               // workgroups per pair of the reduction kernels for the CURRENT clouds (ensure_state)
};

struct GicpCertBuffers {              // see CertArrays
    DeviceBuffer<float> lb, t_prev;
    DeviceBuffer<int> work, bcount;
    DeviceBuffer<unsigned long long> searched;
    int nb = 0;                       // row stride of bcount
    CertArrays view() const { return CertArrays{lb.get(), t_prev.get(), work.get(), bcount.get(), nb, searched.get()}; }
};

struct GicpVoxelMap {                 // G7 voxel map of the targets (sorted keys, all pairs)
    DeviceBuffer<unsigned long long> keys;
    DeviceBuffer<float4> mean;
    DeviceBuffer<double> cov;
    int n = 0;
    double res_built = 0.0;
};

// ------------------------------------------------------------------------------------------------
struct mrs_gicp_batch {
    mrs_ctx* ctx = nullptr;
    int n_pairs = 0;
    GicpParams prm;
    GicpCloud side[2];              // [0] sources, [1] targets
    GicpLmBuffers lm;
    GicpCertBuffers cert;
    GicpVoxelMap vox;
    double last_nn_passes = 0;
    int search_core = 1;            // 1: octree leaves + query groups (round 4), 0: round-3 wave-shared traversal (A/B, cross-check)
    int cold_core = 0;              // search_core 1: kernel of the FIRST pass of an align() (0: round-3 kernel, 1: round-4 kernel)
    bool use_certificates = true;   // search_core 1: certify unchanged neighbours before searching (k_nn_certify)
    double last_searched = 0;       // share of (source point, pass) that needed a search in the last align()
    bool no_cov = false;            // RING++ front end: no covariance buffers
    int big_movers = 1;             // pairs whose last step exceeded motion_switch (counted by k_lm_update): do they need the round-3 kernel?
    bool clouds_set() const { return side[0].ready && side[1].ready; }
};

namespace {

// dst[seg.dst + i] = src[seg.src + i], i < seg.count, for every segment (one per pair; blockIdx.y): how set_clouds_from moves a stored cloud's
// arrays into a pair's slot.  seg = {src offset, dst offset, count} in units of T.
template <class T>
__global__ void k_copy_segments(const T* __restrict__ src, T* __restrict__ dst, const int64_t* __restrict__ seg, int64_t scale)
{
    const int64_t so = seg[3 * blockIdx.y] * scale, dofs = seg[3 * blockIdx.y + 1] * scale, n = seg[3 * blockIdx.y + 2] * scale;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) dst[dofs + i] = src[so + i];
}

int blocks_for_points(int n) { return (n + kNNThreads * kPts - 1) / (kNNThreads * kPts); }
constexpr int kLinChunks = 4;    // blocks of 1024 points per workgroup of the reduction kernels (ensure_state)

// ---- allocation ----

// a buffer of exactly n elements, whatever it held before
template <class T>
int fresh(DeviceBuffer<T>& b, size_t n)
{
    b.reset();
    return b.reserve(n, n);
}

// Room for the octree-cell hierarchy of a side of P clouds: the three [P + 1] tables and, grow-only with 1/8 slack, the box arrays of the given
// numbers of leaves, tiles and supers (0: the tables only -- build_leaf_hier learns the counts from a kernel that writes the tables).
int reserve_hier(GicpCloud& S, int P, int leaves, int tiles, int supers)
{
    int st = MRS_OK;
    for (DeviceBuffer<int>* first : {&S.leaf_first, &S.tile_first, &S.super_first})
        if (st == MRS_OK) st = first->reserve((size_t)P + 1, (size_t)P + 1);
    auto boxes = [&st](DeviceBuffer<float4>& lo, DeviceBuffer<float4>& hi, int need) {
        const size_t cap = (size_t)(need + need / 8 + 1);
        if (st == MRS_OK) st = lo.reserve((size_t)need, cap);
        if (st == MRS_OK) st = hi.reserve((size_t)need, cap);
    };
    boxes(S.llo, S.lhi, leaves);
    boxes(S.t2lo, S.t2hi, tiles);
    boxes(S.slo, S.shi, supers);
    return st;
}

// Octree-cell leaves + tiles + supers of every cloud of side `w` from the sorted keys (set_clouds).  Synchronises (the leaf counts size the arrays).
int build_leaf_hier(mrs_gicp_batch* h, int w, const unsigned long long* d_keys, int64_t total, hipStream_t s)
{
    const int P = h->n_pairs;
    GicpCloud& S = h->side[w];
    mrs::Scratch cellhead, cellstart, head, leafid, tmp;
    int st;
    for (mrs::Scratch* b : {&cellhead, &cellstart, &head, &leafid})
        if ((st = b->alloc((size_t)total * sizeof(int), s)) != MRS_OK) return st;
    const int fb = (int)std::min<int64_t>((total + 255) / 256, 8192);
    hipLaunchKernelGGL(nnc::k_leaf_level, dim3(fb), dim3(256), 0, s, d_keys, (size_t)total, cellhead.as<int>());
    size_t b1 = 0, b2 = 0;
    MRS_HIP_TRY(hipcub::DeviceScan::InclusiveScan(nullptr, b1, cellhead.as<int>(), cellstart.as<int>(), hipcub::Max(), (int)total, s));
    MRS_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, b2, head.as<int>(), leafid.as<int>(), (int)total, s));
    if ((st = tmp.alloc(std::max(b1, b2), s)) != MRS_OK) return st;
    MRS_HIP_TRY(hipcub::DeviceScan::InclusiveScan(tmp.p, b1, cellhead.as<int>(), cellstart.as<int>(), hipcub::Max(), (int)total, s));
    hipLaunchKernelGGL(nnc::k_leaf_heads, dim3(fb), dim3(256), 0, s, cellstart.as<int>(), (size_t)total, head.as<int>());
    MRS_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(tmp.p, b2, head.as<int>(), leafid.as<int>(), (int)total, s));
    if ((st = reserve_hier(S, P, 0, 0, 0)) != MRS_OK) return st;
    hipLaunchKernelGGL(nnc::k_leaf_first, dim3((P + 1 + 255) / 256), dim3(256), 0, s, head.as<int>(), leafid.as<int>(), S.d_offs.get(), P,
                       S.leaf_first.get());
    MRS_HIP_TRY(hipGetLastError());
    // tiles: octree cells of <= 256 points (every leaf cell lies inside one of them)
    mrs::Scratch tpre, thead, tid;
    if ((st = tpre.alloc((size_t)total, s)) != MRS_OK) return st;
    if ((st = thead.alloc((size_t)total * sizeof(int), s)) != MRS_OK) return st;
    if ((st = tid.alloc((size_t)total * sizeof(int), s)) != MRS_OK) return st;
    hipLaunchKernelGGL(nnc::k_tile_prefix, dim3(fb), dim3(256), 0, s, d_keys, (size_t)total, tpre.as<signed char>());
    hipLaunchKernelGGL(nnc::k_tile_heads, dim3((unsigned)std::min<int64_t>((total + 1023) / 1024, 16384)), dim3(1024), 0, s, d_keys,
                       (const signed char*)tpre.as<signed char>(), (size_t)total, thead.as<int>());
    MRS_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(tmp.p, b2, thead.as<int>(), tid.as<int>(), (int)total, s));
    hipLaunchKernelGGL(nnc::k_leaf_first, dim3((P + 1 + 255) / 256), dim3(256), 0, s, thead.as<int>(), tid.as<int>(), S.d_offs.get(), P,
                       S.tile_first.get());
    MRS_HIP_TRY(hipGetLastError());
    std::vector<int> lf(P + 1), tf(P + 1), sf(P + 1);
    MRS_HIP_TRY(hipMemcpyAsync(lf.data(), S.leaf_first.get(), lf.size() * sizeof(int), hipMemcpyDeviceToHost, s));
    MRS_HIP_TRY(hipMemcpyAsync(tf.data(), S.tile_first.get(), tf.size() * sizeof(int), hipMemcpyDeviceToHost, s));
    MRS_HIP_TRY(hipStreamSynchronize(s));
    int most_supers = 0;
    sf[0] = 0;
    for (int c = 0; c < P; ++c) {
        const int nt = tf[c + 1] - tf[c], ns = (nt + 63) / 64;
        sf[c + 1] = sf[c] + ns;
        most_supers = std::max(most_supers, ns);
    }
    S.h_leaf_first = lf; S.h_tile_first = tf; S.h_super_first = sf;
    if ((st = reserve_hier(S, P, lf[P], tf[P], sf[P])) != MRS_OK) return st;
    MRS_HIP_TRY(hipMemcpyAsync(S.super_first.get(), sf.data(), sf.size() * sizeof(int), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(nnc::k_leaf_boxes, dim3(fb), dim3(256), 0, s, (const float4*)S.pts.get(), d_keys, head.as<int>(), leafid.as<int>(),
                       S.d_offs.get(), (size_t)total, S.llo.get(), S.lhi.get());
    hipLaunchKernelGGL(nnc::k_tile_boxes, dim3(fb), dim3(256), 0, s, d_keys, (const int*)thead.as<int>(), (const int*)tid.as<int>(),
                       (const int*)head.as<int>(), (const int*)leafid.as<int>(), (const int*)S.leaf_first.get(), (const int64_t*)S.d_offs.get(),
                       (size_t)total, (const float4*)S.llo.get(), (const float4*)S.lhi.get(), S.t2lo.get(), S.t2hi.get());
    hipLaunchKernelGGL(nnc::k_group_boxes, dim3(most_supers, P), dim3(64), 0, s, (const float4*)S.t2lo.get(), (const float4*)S.t2hi.get(),
                       (const int*)S.tile_first.get(), (const int*)S.super_first.get(), S.slo.get(), S.shi.get());
    MRS_HIP_TRY(hipGetLastError());
    MRS_HIP_TRY(hipStreamSynchronize(s));     // tf / sf are temporaries
    return MRS_OK;
}

// ---- the one launch site of every kernel that more than one entry point starts ----
// (kept after build_leaf_hier and before the entry points: the compiler emits template kernels in the order of their first use.  For the same
// reason one of them, launch_pcl_sums, stands further down, in front of the tick driver.)

// The round-3 scan of every source point.  Source points per lane: fewer points per wave = a more compact query set = sharper sub-tile
// culling; more = every LDS candidate read serves more distance evaluations.  Measured (120k x 120k, MI355X):
// 2 beats 4 at every batch size (23.5k vs 21.4k it/s at 256 pairs, 14.3k vs 11.1k at 16) and 1 only wins when a
// single pair would otherwise leave most CUs idle.
void launch_nn_scan(mrs_gicp_batch* h, const GicpParams& prm, float* lb_out, int gate, hipStream_t s)
{
    const GicpCloud &S = h->side[0], &T = h->side[1];
    const int P = h->n_pairs, longest_src = (int)S.longest;
    const int cus = h->ctx->num_cu > 0 ? h->ctx->num_cu : 256;
    auto wgs = [&](int pts) { return (long)P * ((longest_src + kNNThreads * pts - 1) / (kNNThreads * pts)); };
    auto launch = [&](auto kernel, int pts) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)(wgs(pts) / P), P), dim3(kNNThreads), 0, s, S.pts.get(), S.d_offs.get(), T.pts.get(), T.d_offs.get(),
                           T.tile_base.get(), T.tlo.get(), T.thi.get(), T.mlo.get(), T.mhi.get(), h->lm.state.get(), prm, h->lm.corr.get(),
                           h->lm.seed.get(), T.bbox.get(), lb_out, gate);
    };
    if (wgs(2) >= 3L * cus)
        launch(k_nn_scan<2>, 2);
    else
        launch(k_nn_scan<1>, 1);
}

// one workgroup per 1024 source points: grid of k_nn_certify and k_nn_scan_g
dim3 cert_grid(const mrs_gicp_batch* h) { return dim3((unsigned)(((int)h->side[0].longest + kCertBlock - 1) / kCertBlock), h->n_pairs); }

// work_lists: only the queries that k_nn_certify left on the work lists (else every point)
void launch_nn_scan_g(mrs_gicp_batch* h, const GicpParams& prm, bool work_lists, hipStream_t s)
{
    const GicpCloud &S = h->side[0], &T = h->side[1];
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, cert_grid(h), dim3(kNNThreads), 0, s, S.pts.get(), S.d_offs.get(), T.pts.get(), T.d_offs.get(), T.hier(),
                           h->lm.state.get(), prm, h->lm.corr.get(), h->lm.seed.get(), T.bbox.get(), h->cert.view());
    };
    if (!work_lists)
        launch(k_nn_scan_g<false>);
    else
        launch(k_nn_scan_g<true>);
}

void launch_nn_certify(mrs_gicp_batch* h, const GicpParams& prm, hipStream_t s)
{
    const GicpCloud &S = h->side[0], &T = h->side[1];
    hipLaunchKernelGGL(k_nn_certify, cert_grid(h), dim3(256), 0, s, S.pts.get(), S.d_offs.get(), T.pts.get(), T.d_offs.get(), h->lm.state.get(),
                       prm, h->lm.corr.get(), h->lm.seed.get(), h->cert.view());
}

void launch_nn_store_pose(mrs_gicp_batch* h, int worklists, hipStream_t s)
{
    hipLaunchKernelGGL(k_nn_store_pose, dim3((h->n_pairs + 255) / 256), dim3(256), 0, s, h->lm.state.get(), h->n_pairs, h->cert.view(), worklists,
                       h->side[0].d_offs.get(), h->prm.motion_switch);
}

void launch_linearize(mrs_gicp_batch* h, int trial_only, hipStream_t s)
{
    const GicpCloud &S = h->side[0], &T = h->side[1];
    hipLaunchKernelGGL(k_linearize, dim3(h->lm.max_blocks, h->n_pairs), dim3(kNNThreads), 0, s, S.pts.get(), S.d_offs.get(), S.cov.get(), T.pts.get(),
                       T.d_offs.get(), T.cov.get(), h->lm.state.get(), h->lm.corr.get(), h->lm.partial.get(), h->lm.max_blocks, trial_only);
}

void launch_linearize_voxel(mrs_gicp_batch* h, hipStream_t s)
{
    const GicpCloud& S = h->side[0];
    hipLaunchKernelGGL(k_linearize_voxel, dim3(h->lm.max_blocks, h->n_pairs), dim3(kNNThreads), 0, s, S.pts.get(), S.d_offs.get(), S.cov.get(),
                       h->vox.keys.get(), h->vox.mean.get(), h->vox.cov.get(), h->vox.n, h->lm.state.get(), h->prm, h->lm.partial.get(),
                       h->lm.max_blocks);
}

// The update kernels share one contract for the tick's counters n_next: [0] pairs that iterate again, [2] those of [0] that moved far, [3] the tick
// carried a search.  Only k_lm_update writes [1] (pairs in an LM trial).
void launch_lm_update(mrs_gicp_batch* h, int* n_next, int trial_only, hipStream_t s)
{
    GicpLmBuffers& L = h->lm;
    hipLaunchKernelGGL(k_lm_update, dim3(h->n_pairs), dim3(kLmThreads), 0, s, L.state.get(), L.partial.get(), L.nblocks.get(), L.max_blocks, h->prm,
                       n_next, trial_only);
}

// one ICP iteration's sums; plane: point-to-plane (row G12) instead of point-to-point (row G9)
void launch_icp_sums(mrs_gicp_batch* h, bool plane, hipStream_t s)
{
    const GicpCloud &S = h->side[0], &T = h->side[1];
    GicpLmBuffers& L = h->lm;
    const dim3 grid(L.max_blocks, h->n_pairs);
    if (plane)
        hipLaunchKernelGGL(k_icp_plane_sums, grid, dim3(kNNThreads), 0, s, S.pts.get(), S.d_offs.get(), T.pts.get(), T.nrm.get(), T.d_offs.get(),
                           L.state.get(), L.corr.get(), L.partial.get(), L.max_blocks);
    else
        hipLaunchKernelGGL(k_icp_sums, grid, dim3(kNNThreads), 0, s, S.pts.get(), S.d_offs.get(), T.pts.get(), T.d_offs.get(), L.state.get(),
                           L.corr.get(), L.partial.get(), L.max_blocks);
}

void launch_icp_update(mrs_gicp_batch* h, bool plane, const IcpParams& dp, int* n_next, hipStream_t s)
{
    GicpLmBuffers& L = h->lm;
    if (plane)
        hipLaunchKernelGGL(k_icp_plane_update, dim3(h->n_pairs), dim3(kLmThreads), 0, s, L.state.get(), L.partial.get(), L.nblocks.get(),
                           L.max_blocks, dp, n_next);
    else
        hipLaunchKernelGGL(k_icp_update, dim3(h->n_pairs), dim3(kLmThreads), 0, s, L.state.get(), L.partial.get(), L.nblocks.get(), L.max_blocks,
                           dp, n_next);
}

void launch_pcl_update(mrs_gicp_batch* h, const PclGicpParams& dp, int* n_next, hipStream_t s)
{
    GicpLmBuffers& L = h->lm;
    hipLaunchKernelGGL(k_pclgicp_update, dim3(h->n_pairs), dim3(kLmThreads), 0, s, L.state.get(), L.partial.get(), L.nblocks.get(), L.max_blocks,
                       h->side[1].bbox.get(), dp, n_next);
}

// the correspondences of the last search as indices into the clouds as they were given (d_corr: one int per source point)
void launch_corr_to_original(mrs_gicp_batch* h, int32_t* d_corr, hipStream_t s)
{
    const GicpCloud &S = h->side[0], &T = h->side[1];
    hipLaunchKernelGGL(k_corr_to_original, dim3(64, h->n_pairs), dim3(256), 0, s, S.pts.get(), S.d_offs.get(), T.pts.get(), T.d_offs.get(),
                       h->lm.corr.get(), d_corr);
}

// f(integral_constant<KMAX>) for the smallest list size that holds k neighbours.  WITH_30: the rung of RING++'s k (k_knn_cov: 30 list slots =
// 30 KB of LDS = five workgroups per compute unit; 32: four).
template <bool WITH_30, class F>
void dispatch_kmax(int k, F&& f)
{
    if (k <= 16) return f(std::integral_constant<int, 16>{});
    if (k <= 20) return f(std::integral_constant<int, 20>{});
    if constexpr (WITH_30)
        if (k <= 30) return f(std::integral_constant<int, 30>{});
    return f(std::integral_constant<int, 32>{});
}

// k nearest neighbours of every point of side `w` (k_knn_select) into knn (layout: knn_at)
int launch_knn_select(mrs_gicp_batch* h, int w, int k, int* d_knn, hipStream_t s)
{
    const GicpCloud& S = h->side[w];
    const dim3 grid((unsigned)((S.longest + kNNThreads - 1) / kNNThreads), h->n_pairs);
    dispatch_kmax<false>(k, [&](auto kmax) {
        hipLaunchKernelGGL((k_knn_select<decltype(kmax)::value>), grid, dim3(kNNThreads), 0, s, S.pts.get(), S.d_offs.get(), S.hier(), k, d_knn);
    });
    MRS_HIP_TRY(hipGetLastError());
    return MRS_OK;
}

// the selection kernel of the default search setting over clouds [c0, c0 + nc) of side w; knn: see knn_at (cloud numbers count from c0)
void launch_knn_cov(mrs_gicp_batch* h, int w, int c0, int nc, int k, int* d_knn, hipStream_t s)
{
    const GicpCloud& S = h->side[w];
    const dim3 g((unsigned)((S.longest + kNNThreads - 1) / kNNThreads), nc);
    dispatch_kmax<true>(k, [&](auto kmax) {
        hipLaunchKernelGGL((k_knn_cov<decltype(kmax)::value>), g, dim3(kNNThreads), 0, s, S.pts.get(), S.d_offs.get() + c0, S.tile_base.get() + c0,
                           S.tlo.get(), S.thi.get(), S.mlo.get(), S.mhi.get(), k, d_knn);
    });
}

// One nearest-neighbour pass for every pair in phase 0 (h->lm.state): fills h->lm.corr / h->lm.seed.  prm: the searches' parameters (the
// correspondence distance above all): the handle's own for GICP, a copy with ICP's distance for ICP.
// mode 0: first pass of an align(), 1: later pass, 2: one plain search with the selected core (linearize hook).
// search_core 0: the round-3 kernel, every point, every pass.  search_core 1 (round-4 schedule):
//   * first pass, and every pair whose last step moved it by more than prm.motion_switch: the round-3 kernel -- a search whose radius
//     is decimetres is a broad search, and brute force over fat minis is at its best there (measured: 17 against 26 ms for 5 cold
//     passes of 64 pairs); it leaves no certificates;
//   * the other pairs: certify the previous pass's neighbours, search what could not be certified (k_nn_scan_g leaves certificates).
int nn_pass(mrs_gicp_batch* h, const GicpParams& prm, int mode, hipStream_t s)
{
    MRS_REQUIRE(h->search_core == 0 || h->side[1].hier_valid, "target hierarchy missing: set the target clouds after choosing the search setting");
    float* const lb = h->search_core == 1 ? h->cert.lb.get() : nullptr;
    if (h->search_core == 0) {
        launch_nn_scan(h, prm, lb, 0, s);
    } else if (mode == 0 && h->cold_core == 0) {
        launch_nn_scan(h, prm, lb, 0, s);
        launch_nn_store_pose(h, 0, s);
    } else if (mode != 1 || !h->use_certificates) {
        launch_nn_scan_g(h, prm, false, s);
        launch_nn_store_pose(h, 0, s);
    } else {
        if (h->big_movers > 0) launch_nn_scan(h, prm, lb, 1, s);
        launch_nn_certify(h, prm, s);
        launch_nn_scan_g(h, prm, true, s);
        launch_nn_store_pose(h, 1, s);
    }
    MRS_HIP_TRY(hipGetLastError());
    return MRS_OK;
}

// MRS_DEV=1 MRS_KNN_REC=0: pass 2 of the selection walks the hierarchy again (what it does when pass 1 noted too many minis)
int knn_dev_switches(hipStream_t s)
{
    const char* const e = mrs::dev_env("MRS_KNN_REC");      // read per call (the tests flip it)
    const int off = (e && atoi(e) == 0) ? 1 : 0;
    static int cur = 0;
    if (off != cur) {
        MRS_HIP_TRY(hipStreamSynchronize(s));
        MRS_HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_knn_norec), &off, sizeof(off)));
        cur = off;
    }
    return MRS_OK;
}

// The k nearest neighbours of every point of side `which` (the selection kernel of the handle's search setting), handed to
// tail(first cloud, clouds, lists) -- the launch of a consumer such as k_cov_from_knn -- through scratch memory.
template <class Tail>
int knn_then(mrs_gicp_batch* h, int32_t which, int k, hipStream_t s, Tail&& tail)
{
    const GicpCloud& S = h->side[which];
    if (h->search_core == 1 && h->cold_core == 1) {     // setting 3: the round-4 k-NN kernel (slower than the round-3 one on the bench's scans)
        MRS_REQUIRE(S.hier_valid, "search setting 3 was selected after set_clouds: set the clouds again");
        mrs::Scratch knn;
        int st = knn.alloc(knn_ints(S.offs[h->n_pairs], h->n_pairs, k) * sizeof(int), s);
        if (st != MRS_OK) return st;
        if ((st = launch_knn_select(h, which, k, knn.as<int>(), s)) != MRS_OK) return st;
        tail(0, h->n_pairs, (const int*)knn.as<int>());
        MRS_HIP_TRY(hipGetLastError());
        return MRS_OK;
    }
    int st = knn_dev_switches(s);
    if (st != MRS_OK) return st;
    // the neighbour indices pass from the selection to its consumer through scratch memory: clouds are processed in chunks so that
    // it stays below ~512 MB (256 clouds x 120 k points x k = 15 would be 1.8 GB held by the scratch cache for the life of the process)
    const int64_t per_cloud = (int64_t)(knn_ints(S.longest, 1, k) * sizeof(int));
    const int chunk = (int)std::max<int64_t>(1, std::min<int64_t>(h->n_pairs, (512ll << 20) / per_cloud));
    mrs::Scratch knn;
    if ((st = knn.alloc((size_t)chunk * per_cloud, s)) != MRS_OK) return st;
    for (int c0 = 0; c0 < h->n_pairs; c0 += chunk) {
        const int nc = std::min(chunk, h->n_pairs - c0);
        // the kernels index knn by GLOBAL point number (knn_at: (offs[c] + 64 c) k with c counted from the chunk's first cloud): shift the
        // chunk's buffer so that the chunk's first point lands on its start
        int* const kn = knn.as<int>() - (size_t)S.offs[c0] * k;
        launch_knn_cov(h, which, c0, nc, k, kn, s);
        tail(c0, nc, (const int*)kn);
    }
    MRS_HIP_TRY(hipGetLastError());
    return MRS_OK;
}

}  // namespace

// Everything of set_clouds that does not look at the points: checks, (re)allocation of the side's buffers, offsets and tile bases, reset of
// the warm-start seeds.  Leaves the side not `ready`: the caller fills in the points.
static int prepare_side(mrs_gicp_batch* h, int32_t which, const int64_t* h_offsets, hipStream_t s)
{
    MRS_REQUIRE(h && h_offsets, "null pointer");
    MRS_REQUIRE(which == 0 || which == 1, "which must be 0 (source) or 1 (target)");
    MRS_REQUIRE(h_offsets[0] == 0, "offsets[0] must be 0");
    const int P = h->n_pairs;
    for (int i = 0; i < P; ++i) {
        MRS_REQUIRE(h_offsets[i + 1] > h_offsets[i], "every cloud needs at least one point");
        MRS_REQUIRE(h_offsets[i + 1] - h_offsets[i] < (1ll << 28), "cloud too large (2^28 points at most)");
    }
    MRS_HIP_TRY(hipSetDevice(h->ctx->device));
    const int64_t total = h_offsets[P];
    MRS_REQUIRE(total < (1ll << 31), "more than 2^31 points in one batch");
    MRS_REQUIRE(P < (1 << 21), "too many pairs for the 64-bit sort key");
    std::vector<int> tile_base(P);
    int tiles = 0, longest_tiles = 0;
    int64_t longest = 0;
    for (int i = 0; i < P; ++i) {
        const int64_t n = h_offsets[i + 1] - h_offsets[i];
        const int nt = (int)((n + kTile - 1) / kTile);
        tile_base[i] = tiles;
        tiles += nt;
        longest_tiles = std::max(longest_tiles, nt);
        longest = std::max(longest, n);
    }
    GicpCloud& S = h->side[which];
    S.ready = false;
    // a registration object is fed a new cloud per loop candidate (ICPCheck, global_manager.cpp:2018-2019): keep the device
    // buffers and only grow them (each hipFree synchronises the device, each hipMalloc costs tens of microseconds)
    if ((size_t)total + 16 > S.pts.capacity() || (size_t)tiles > S.tlo.capacity() || !S.d_offs) {
        S = GicpCloud{};        // the hierarchy goes too: reserve_hier sizes it again
        const size_t cap = (size_t)(total + total / 8), capt = (size_t)(tiles + tiles / 8 + 1);
        int st = MRS_OK;
        auto alloc = [&st](auto& buf, size_t n) { if (st == MRS_OK) st = fresh(buf, n); };
        alloc(S.d_offs, (size_t)P + 1);
        alloc(S.pts, cap + 16);
        if (!h->no_cov) alloc(S.cov, cap * kCovDoubles);
        alloc(S.tile_base, (size_t)P);
        alloc(S.tlo, capt);
        alloc(S.thi, capt);
        alloc(S.mlo, capt * 64);
        alloc(S.mhi, capt * 64);
        alloc(S.bbox, (size_t)P * 6);
        if (which == 0 && !h->no_cov) {       // correspondences, seeds and certificates belong to alignments: the RING++ front end's containers (no_cov) never read them
            alloc(h->lm.corr, cap);
            alloc(h->lm.seed, cap);
            alloc(h->cert.lb, cap);
            alloc(h->cert.work, cap + kCertBlock);
            if (st == MRS_OK) st = h->cert.t_prev.reserve((size_t)P * 12, (size_t)P * 12);
            if (st == MRS_OK) st = h->cert.searched.reserve((size_t)P * kStatStride, (size_t)P * kStatStride);
        }
        if (st != MRS_OK) {
            S = GicpCloud{};    // no half-allocated side: the next call starts over
            return st;
        }
    }
    S.offs.assign(h_offsets, h_offsets + P + 1);
    S.longest = longest;
    S.max_tiles = longest_tiles;
    S.cov_valid = false;
    S.hier_valid = false;
    S.nrm_key = 0;
    if (which == 1) h->vox.res_built = 0.0;   // new targets: their voxel map is built again (set_clouds_from delivers covariances, so compute_covariances does not run)
    if (which == 0) h->lm.n_seed = (size_t)total;
    if (h->lm.seed) MRS_HIP_TRY(hipMemsetAsync(h->lm.seed.get(), 0xff, h->lm.n_seed * sizeof(int), s));  // -1: no warm start across clouds
    MRS_HIP_TRY(hipMemcpyAsync(S.d_offs.get(), h_offsets, (P + 1) * sizeof(int64_t), hipMemcpyHostToDevice, s));
    MRS_HIP_TRY(hipMemcpyAsync(S.tile_base.get(), tile_base.data(), P * sizeof(int), hipMemcpyHostToDevice, s));
    // per-cloud bounding boxes armed for k_cloud_bbox (ordered ints: min = +max, max = -max)
    std::vector<int> box_init((size_t)P * 6);
    for (int i = 0; i < P; ++i)
        for (int a = 0; a < 3; ++a) { box_init[6 * i + a] = INT32_MAX; box_init[6 * i + 3 + a] = INT32_MIN; }
    MRS_HIP_TRY(hipMemcpyAsync(S.bbox.get(), box_init.data(), box_init.size() * sizeof(int), hipMemcpyHostToDevice, s));
    MRS_HIP_TRY(hipStreamSynchronize(s));   // tile_base, box_init and h_offsets are temporaries
    return MRS_OK;
}

extern "C" {

int mrs_gicp_batch_set_search(mrs_gicp_batch* h, int32_t core)
{
    MRS_REQUIRE(h, "null handle");
    MRS_REQUIRE(core >= 0 && core <= 3, "core must be 0 .. 3");
    const int base = core == 0 ? 0 : 1;
    if ((core == 3) != (h->search_core == 1 && h->cold_core == 1)) h->side[0].cov_valid = h->side[1].cov_valid = false;   // the k-NN kernel changes
    h->search_core = base;
    h->use_certificates = core == 1 || core == 3;
    h->cold_core = core == 3 ? 1 : 0;
    return MRS_OK;
}

double mrs_gicp_batch_last_searched_fraction(const mrs_gicp_batch* h) { return h ? h->last_searched : 1.0; }

void mrs_gicp_default_params(mrs_gicp_params* p)
{
    if (!p) return;
    p->k_correspondences = 20;          // fast_gicp default; Mapping sets 15 (global_manager.cpp:2442)
    p->max_correspondence_distance = DBL_MAX;
    p->max_iterations = 64;
    p->rotation_epsilon = 2e-3;
    p->transformation_epsilon = 5e-4;
    p->lm_max_iterations = 10;
    p->lm_init_lambda_factor = 1e-9;
    p->convergence_factor = 10.0;       // upstream LsqRegistration::is_converged scales both deltas by 10
    p->force_iterations = 0;
    p->voxel_resolution = 0.0;          // FastVGICP(Cuda) default is 1.0; Mapping sets 0.5 (global_manager.cpp:2450)
    p->voxel_neighbors = 1;             // DIRECT1 (global_manager.cpp:2452)
}

int mrs_gicp_batch_create(mrs_ctx* ctx, int32_t n_pairs, mrs_gicp_batch** out)
{
    MRS_REQUIRE(ctx && out, "null pointer");
    MRS_REQUIRE(n_pairs > 0, "n_pairs must be positive");
    MRS_REQUIRE(n_pairs <= mrs::kMaxGridY, "at most 65535 pairs per batch (create several batches)");
    *out = nullptr;
    MRS_HIP_TRY(hipSetDevice(ctx->device));
    mrs_gicp_batch* h = new mrs_gicp_batch();
    h->ctx = ctx;
    h->n_pairs = n_pairs;
    mrs_gicp_params d;
    mrs_gicp_default_params(&d);
    *out = h;
    return mrs_gicp_batch_set_params(h, &d);
}

int mrs_gicp_batch_destroy(mrs_gicp_batch* h)
{
    if (!h) return MRS_OK;
    (void)hipSetDevice(h->ctx->device);
    delete h;       // its members free the device memory
    return MRS_OK;
}

int mrs_gicp_batch_set_params(mrs_gicp_batch* h, const mrs_gicp_params* p)
{
    MRS_REQUIRE(h && p, "null pointer");
    MRS_REQUIRE(p->k_correspondences >= 3 && p->k_correspondences <= 32, "k_correspondences must be in [3, 32]");
    MRS_REQUIRE(p->max_iterations > 0 && p->lm_max_iterations > 0, "iteration limits must be positive");
    MRS_REQUIRE(p->max_correspondence_distance > 0, "max_correspondence_distance must be positive");
    if (p->k_correspondences != h->prm.k) h->side[0].cov_valid = h->side[1].cov_valid = false;
    h->prm.k = p->k_correspondences;
    h->prm.max_corr2 = p->max_correspondence_distance >= 1e150 ? INFINITY
                                                               : p->max_correspondence_distance * p->max_correspondence_distance;
    h->prm.max_iter = p->max_iterations;
    h->prm.rot_eps = p->rotation_epsilon;
    h->prm.trans_eps = p->transformation_epsilon;
    h->prm.lm_max_iter = p->lm_max_iterations;
    h->prm.lm_init_factor = p->lm_init_lambda_factor;
    MRS_REQUIRE(p->convergence_factor >= 0.0, "convergence_factor must be >= 0 (0 selects upstream's 10)");
    h->prm.conv_factor = p->convergence_factor > 0.0 ? p->convergence_factor : 10.0;
    h->prm.force_iters = p->force_iterations;
    MRS_REQUIRE(p->voxel_resolution >= 0.0, "voxel_resolution must be >= 0");
    MRS_REQUIRE(p->voxel_neighbors == 1 || p->voxel_neighbors == 7 || p->voxel_neighbors == 27, "voxel_neighbors must be 1, 7 or 27");
    h->prm.cert_margin = 0.004f;
    h->prm.motion_switch = 0.02f;
    h->prm.voxel_res = p->voxel_resolution;
    h->prm.voxel_neighbors = p->voxel_neighbors;
    return MRS_OK;
}

int mrs_gicp_batch_set_clouds(mrs_gicp_batch* h, int32_t which, const float* d_points, int32_t stride_floats,
                              const int64_t* h_offsets, mrs_stream stream)
{
    MRS_REQUIRE(h && d_points && h_offsets, "null pointer");
    MRS_REQUIRE(stride_floats >= 3, "stride_floats must be >= 3");
    hipStream_t s = (hipStream_t)stream;
    int st = prepare_side(h, which, h_offsets, s);
    if (st != MRS_OK) return st;
    GicpCloud& S = h->side[which];
    const int64_t total = h_offsets[h->n_pairs];

    // Morton order: per-cloud bounding box -> 64-bit keys (cloud id | Morton code) -> stable radix sort
    mrs::Scratch keys_in, keys_out, vals_in, vals_out, tmp;
    if ((st = keys_in.alloc((size_t)total * 8, s)) != MRS_OK) return st;
    if ((st = keys_out.alloc((size_t)total * 8, s)) != MRS_OK) return st;
    if ((st = vals_in.alloc((size_t)total * 4, s)) != MRS_OK) return st;
    if ((st = vals_out.alloc((size_t)total * 4, s)) != MRS_OK) return st;
    // (the boxes were armed by prepare_side, in the same host synchronisation as the offsets: one round trip less per cloud)
    const dim3 pg((unsigned)std::min<int64_t>((S.longest + 255) / 256, 1024), h->n_pairs);
    hipLaunchKernelGGL(k_cloud_bbox, dim3(std::min(pg.x, 64u), pg.y), dim3(256), 0, s, d_points, stride_floats, S.d_offs.get(), S.bbox.get());
    hipLaunchKernelGGL(k_morton_keys, pg, dim3(256), 0, s, d_points, stride_floats, S.d_offs.get(), S.bbox.get(),
                       keys_in.as<unsigned long long>(), vals_in.as<int>());
    int key_bits = 42;                       // 42-bit Morton code + the bits of the cloud id: fewer radix passes than 64
    while ((1ll << (key_bits - 42)) < h->n_pairs) ++key_bits;
    size_t tmp_bytes = 0;
    MRS_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, keys_in.as<unsigned long long>(),
                                                   keys_out.as<unsigned long long>(), vals_in.as<int>(), vals_out.as<int>(),
                                                   (int)total, 0, key_bits, s));
    if ((st = tmp.alloc(tmp_bytes, s)) != MRS_OK) return st;
    MRS_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(tmp.p, tmp_bytes, keys_in.as<unsigned long long>(),
                                                   keys_out.as<unsigned long long>(), vals_in.as<int>(), vals_out.as<int>(),
                                                   (int)total, 0, key_bits, s));
    hipLaunchKernelGGL(k_gather_sorted, pg, dim3(256), 0, s, d_points, stride_floats, S.d_offs.get(), vals_out.as<int>(), S.pts.get());
    hipLaunchKernelGGL(k_boxes, dim3(S.max_tiles, h->n_pairs), dim3(256), 0, s, S.pts.get(), S.d_offs.get(), S.tile_base.get(), S.tlo.get(),
                       S.thi.get(), S.mlo.get(), S.mhi.get());
    MRS_HIP_TRY(hipGetLastError());
    // the octree-cell hierarchy serves the round-4 searches: correspondences search the TARGETS (which == 1); the sources need it only
    // for the round-4 k-NN kernel (setting 3)
    if (which == 1 || (h->search_core == 1 && h->cold_core == 1)) {
        if ((st = build_leaf_hier(h, which, keys_out.as<unsigned long long>(), total, s)) != MRS_OK) return st;
        S.hier_valid = true;
    }
    MRS_HIP_TRY(hipStreamSynchronize(s));
    S.ready = true;
    return MRS_OK;
}

/* Pair i's cloud of side `which` := cloud h_ids[i] of side `store_which` of `store` (a batch used as a container of unique submaps):
 * sorted points, covariances, tile / mini boxes and the octree-cell hierarchy are COPIED on the device (a few MB per cloud) instead of
 * being rebuilt -- a submap that takes part in several pairs (the node checks a new scan against several stored candidates,
 * main_RING.py:81-104, global_manager.cpp:2016-2021) pays for its Morton sort and its covariances once. */
int mrs_gicp_batch_set_clouds_from(mrs_gicp_batch* h, int32_t which, mrs_gicp_batch* store, int32_t store_which, const int32_t* h_ids,
                                   mrs_stream stream)
{
    MRS_REQUIRE(h && store && h_ids, "null pointer");
    MRS_REQUIRE(h != store, "a batch cannot be its own store");
    MRS_REQUIRE(which == 0 || which == 1, "which must be 0 (source) or 1 (target)");
    MRS_REQUIRE(store_which == 0 || store_which == 1, "store_which must be 0 or 1");
    MRS_REQUIRE(h->ctx->device == store->ctx->device, "batch and store live on different devices");
    const GicpCloud& F = store->side[store_which];
    MRS_REQUIRE(F.ready, "the store holds no clouds on that side");
    MRS_REQUIRE(!h->no_cov && !store->no_cov, "covariance-free containers cannot take part");
    MRS_REQUIRE(h->prm.k == store->prm.k, "batch and store use different k_correspondences");
    const int P = h->n_pairs, U = store->n_pairs;
    for (int i = 0; i < P; ++i) MRS_REQUIRE(h_ids[i] >= 0 && h_ids[i] < U, "cloud id outside the store");
    const bool need_hier = which == 1 || (h->search_core == 1 && h->cold_core == 1);
    MRS_REQUIRE(!need_hier || F.hier_valid, "the store side has no octree-cell hierarchy (store the clouds as targets)");
    MRS_HIP_TRY(hipSetDevice(h->ctx->device));
    hipStream_t s = (hipStream_t)stream;
    int st;
    if (!F.cov_valid && (st = mrs_gicp_batch_compute_covariances(store, store_which, nullptr, stream)) != MRS_OK) return st;
    const std::vector<int64_t>& so = F.offs;
    std::vector<int64_t> offs(P + 1, 0);
    for (int i = 0; i < P; ++i) offs[i + 1] = offs[i] + (so[h_ids[i] + 1] - so[h_ids[i]]);
    if ((st = prepare_side(h, which, offs.data(), s)) != MRS_OK) return st;
    GicpCloud& S = h->side[which];
    // segment tables {source offset, destination offset, count}: points, 1024-point tiles, and the three levels of the hierarchy
    std::vector<int> stile(U + 1, 0);
    for (int u = 0; u < U; ++u) stile[u + 1] = stile[u] + (int)((so[u + 1] - so[u] + kTile - 1) / kTile);
    std::vector<int64_t> seg((size_t)5 * 3 * P);
    std::vector<int> lf(P + 1, 0), tf(P + 1, 0), sf(P + 1, 0);
    int dtile = 0;
    int64_t most[5] = {0, 0, 0, 0, 0};
    for (int i = 0; i < P; ++i) {
        const int u = h_ids[i];
        const int64_t cnt[5] = {so[u + 1] - so[u], stile[u + 1] - stile[u],
                                need_hier ? F.h_leaf_first[u + 1] - F.h_leaf_first[u] : 0,
                                need_hier ? F.h_tile_first[u + 1] - F.h_tile_first[u] : 0,
                                need_hier ? F.h_super_first[u + 1] - F.h_super_first[u] : 0};
        const int64_t from[5] = {so[u], stile[u], need_hier ? F.h_leaf_first[u] : 0, need_hier ? F.h_tile_first[u] : 0,
                                 need_hier ? F.h_super_first[u] : 0};
        const int64_t to[5] = {offs[i], dtile, lf[i], tf[i], sf[i]};
        for (int a = 0; a < 5; ++a) {
            seg[((size_t)a * P + i) * 3] = from[a]; seg[((size_t)a * P + i) * 3 + 1] = to[a]; seg[((size_t)a * P + i) * 3 + 2] = cnt[a];
            most[a] = std::max(most[a], cnt[a]);
        }
        dtile += (int)cnt[1];
        lf[i + 1] = lf[i] + (int)cnt[2]; tf[i + 1] = tf[i] + (int)cnt[3]; sf[i + 1] = sf[i] + (int)cnt[4];
    }
    mrs::Scratch dseg;
    if ((st = dseg.alloc(seg.size() * sizeof(int64_t), s)) != MRS_OK) return st;
    MRS_HIP_TRY(hipMemcpyAsync(dseg.p, seg.data(), seg.size() * sizeof(int64_t), hipMemcpyHostToDevice, s));
    auto table = [&](int a) { return dseg.as<int64_t>() + (size_t)a * P * 3; };
    auto copy4 = [&](const DeviceBuffer<float4>& src, const DeviceBuffer<float4>& dst, int a, int64_t scale) {
        const unsigned bx = (unsigned)std::max<int64_t>(1, std::min<int64_t>((most[a] * scale + 1023) / 1024, 256));
        hipLaunchKernelGGL(k_copy_segments<float4>, dim3(bx, P), dim3(256), 0, s, (const float4*)src.get(), dst.get(), (const int64_t*)table(a), scale);
    };
    copy4(F.pts, S.pts, 0, 1);
    {   // the normals: 3 doubles per point
        const unsigned bx = (unsigned)std::max<int64_t>(1, std::min<int64_t>((most[0] * kCovDoubles + 1023) / 1024, 256));
        hipLaunchKernelGGL(k_copy_segments<double>, dim3(bx, P), dim3(256), 0, s, (const double*)F.cov.get(), S.cov.get(), (const int64_t*)table(0),
                           (int64_t)kCovDoubles);
    }
    copy4(F.tlo, S.tlo, 1, 1);
    copy4(F.thi, S.thi, 1, 1);
    copy4(F.mlo, S.mlo, 1, 64);
    copy4(F.mhi, S.mhi, 1, 64);
    {   // the clouds' bounding boxes (the Morton grids): 6 ints per cloud
        std::vector<int64_t> bseg((size_t)3 * P);
        for (int i = 0; i < P; ++i) { bseg[3 * i] = 6 * (int64_t)h_ids[i]; bseg[3 * i + 1] = 6 * (int64_t)i; bseg[3 * i + 2] = 6; }
        mrs::Scratch dbs;
        if ((st = dbs.alloc(bseg.size() * sizeof(int64_t), s)) != MRS_OK) return st;
        MRS_HIP_TRY(hipMemcpyAsync(dbs.p, bseg.data(), bseg.size() * sizeof(int64_t), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_copy_segments<int>, dim3(1, P), dim3(64), 0, s, (const int*)F.bbox.get(), S.bbox.get(), (const int64_t*)dbs.p, (int64_t)1);
        MRS_HIP_TRY(hipStreamSynchronize(s));     // bseg / dbs are temporaries
    }
    if (need_hier) {
        if ((st = reserve_hier(S, P, lf[P], tf[P], sf[P])) != MRS_OK) return st;
        MRS_HIP_TRY(hipMemcpyAsync(S.leaf_first.get(), lf.data(), lf.size() * sizeof(int), hipMemcpyHostToDevice, s));
        MRS_HIP_TRY(hipMemcpyAsync(S.tile_first.get(), tf.data(), tf.size() * sizeof(int), hipMemcpyHostToDevice, s));
        MRS_HIP_TRY(hipMemcpyAsync(S.super_first.get(), sf.data(), sf.size() * sizeof(int), hipMemcpyHostToDevice, s));
        copy4(F.llo, S.llo, 2, 1);
        copy4(F.lhi, S.lhi, 2, 1);
        copy4(F.t2lo, S.t2lo, 3, 1);
        copy4(F.t2hi, S.t2hi, 3, 1);
        copy4(F.slo, S.slo, 4, 1);
        copy4(F.shi, S.shi, 4, 1);
        S.h_leaf_first = lf; S.h_tile_first = tf; S.h_super_first = sf;
        S.hier_valid = true;
    }
    MRS_HIP_TRY(hipGetLastError());
    MRS_HIP_TRY(hipStreamSynchronize(s));         // the tables are temporaries
    S.cov_valid = true;
    S.ready = true;
    return MRS_OK;
}

/* host-array form of set_clouds (what a pcl::PointCloud / numpy caller holds): staged through a scratch buffer */
int mrs_gicp_batch_set_clouds_host(mrs_gicp_batch* h, int32_t which, const float* h_points, int32_t stride_floats, const int64_t* h_offsets)
{
    MRS_REQUIRE(h && h_points && h_offsets, "null pointer");
    MRS_REQUIRE(stride_floats >= 3, "stride_floats must be >= 3");
    MRS_REQUIRE(h_offsets[0] == 0 && h_offsets[h->n_pairs] > 0, "offsets must start at 0 and hold points");
    MRS_HIP_TRY(hipSetDevice(h->ctx->device));
    const size_t bytes = (size_t)h_offsets[h->n_pairs] * stride_floats * sizeof(float);
    mrs::Scratch stage;
    int st = stage.alloc(bytes, nullptr);
    if (st != MRS_OK) return st;
    MRS_HIP_TRY(hipMemcpy(stage.p, h_points, bytes, hipMemcpyHostToDevice));
    st = mrs_gicp_batch_set_clouds(h, which, stage.as<float>(), stride_floats, h_offsets, nullptr);
    if (st != MRS_OK) return st;
    MRS_HIP_TRY(hipStreamSynchronize(nullptr));     // the staging buffer goes back to the cache only after set_clouds has read it
    return MRS_OK;
}

int mrs_gicp_batch_compute_covariances(mrs_gicp_batch* h, int32_t which, int32_t* d_knn_out, mrs_stream stream)
{
    MRS_REQUIRE(h, "null handle");
    MRS_REQUIRE(which == 0 || which == 1, "which must be 0 or 1");
    GicpCloud& S = h->side[which];
    MRS_REQUIRE(S.ready, "set_clouds first");
    MRS_HIP_TRY(hipSetDevice(h->ctx->device));
    hipStream_t s = (hipStream_t)stream;
    const int k = h->prm.k;
    const int st = knn_then(h, which, k, s, [&](int c0, int nc, const int* kn) {
        hipLaunchKernelGGL(k_cov_from_knn, dim3((unsigned)((S.longest + 255) / 256), nc), dim3(256), 0, s, (const float4*)S.pts.get(),
                           (const int64_t*)S.d_offs.get() + c0, k, kn, S.cov.get(), d_knn_out);
    });
    if (st != MRS_OK) return st;
    S.cov_valid = true;
    if (which == 1) h->vox.res_built = 0.0;
    return MRS_OK;
}

int mrs_gicp_batch_get_covariances(mrs_gicp_batch* h, int32_t which, double* h_cov6)
{
    MRS_REQUIRE(h && h_cov6, "null pointer");
    MRS_REQUIRE(which == 0 || which == 1, "which must be 0 or 1");
    const GicpCloud& S = h->side[which];
    MRS_REQUIRE(S.cov_valid, "covariances not computed");
    MRS_HIP_TRY(hipSetDevice(h->ctx->device));
    MRS_HIP_TRY(hipDeviceSynchronize());
    const size_t total = (size_t)S.offs[h->n_pairs];
    std::vector<double> sorted(total * kCovDoubles);
    std::vector<float4> pts(total);
    MRS_HIP_TRY(hipMemcpy(sorted.data(), S.cov.get(), total * kCovDoubles * sizeof(double), hipMemcpyDeviceToHost));
    MRS_HIP_TRY(hipMemcpy(pts.data(), S.pts.get(), total * sizeof(float4), hipMemcpyDeviceToHost));
    for (int c = 0; c < h->n_pairs; ++c) {  // the library stores clouds in Morton order; .w = original index
        const int64_t o = S.offs[c];
        for (int64_t i = o; i < S.offs[c + 1]; ++i) {
            int orig;
            memcpy(&orig, &pts[i].w, sizeof(int));
            double c6[6];
            cov6_from_normal(&sorted[(size_t)i * kCovDoubles], c6);      // the doubles the device kernels work with
            memcpy(h_cov6 + (size_t)(o + orig) * 6, c6, 6 * sizeof(double));
        }
    }
    return MRS_OK;
}

/* ---- surface normals (row G12, contract A of DESIGN.md 4.16; kernels: icp_plane_device.hpp) ---- */

static int normals_room(mrs_gicp_batch* h, int32_t which)
{
    GicpCloud& S = h->side[which];
    return S.nrm.reserve((size_t)S.offs[h->n_pairs], S.pts.capacity());     // grow-only, sized like the points
}

int mrs_gicp_batch_compute_normals(mrs_gicp_batch* h, int32_t which, int32_t k, const double* h_viewpoint, mrs_stream stream)
{
    MRS_REQUIRE(h, "null handle");
    MRS_REQUIRE(which == 0 || which == 1, "which must be 0 or 1");
    MRS_REQUIRE(k >= 3 && k <= 32, "normal_k must be in [3, 32]");
    GicpCloud& S = h->side[which];
    MRS_REQUIRE(S.ready, "set_clouds first");
    const double zero[3] = {0.0, 0.0, 0.0};
    const double* const v = h_viewpoint ? h_viewpoint : zero;
    if (S.nrm_key == k && memcmp(S.nrm_vp, v, sizeof(zero)) == 0) return MRS_OK;
    MRS_HIP_TRY(hipSetDevice(h->ctx->device));
    hipStream_t s = (hipStream_t)stream;
    int st = normals_room(h, which);
    if (st != MRS_OK) return st;
    S.nrm_key = 0;
    st = knn_then(h, which, k, s, [&](int c0, int nc, const int* kn) {
        hipLaunchKernelGGL(k_normals_from_knn, dim3((unsigned)((S.longest + 255) / 256), nc), dim3(256), 0, s, (const float4*)S.pts.get(),
                           (const int64_t*)S.d_offs.get() + c0, k, kn, v[0], v[1], v[2], S.nrm.get());
    });
    if (st != MRS_OK) return st;
    S.nrm_key = k;
    memcpy(S.nrm_vp, v, sizeof(zero));
    return MRS_OK;
}

int mrs_gicp_batch_get_normals(mrs_gicp_batch* h, int32_t which, float* h_normals4)
{
    MRS_REQUIRE(h && h_normals4, "null pointer");
    MRS_REQUIRE(which == 0 || which == 1, "which must be 0 or 1");
    const GicpCloud& S = h->side[which];
    MRS_REQUIRE(S.ready && S.nrm_key != 0, "normals neither computed nor given");
    MRS_HIP_TRY(hipSetDevice(h->ctx->device));
    MRS_HIP_TRY(hipDeviceSynchronize());
    const size_t total = (size_t)S.offs[h->n_pairs];
    std::vector<float4> nrm(total), pts(total);
    MRS_HIP_TRY(hipMemcpy(nrm.data(), S.nrm.get(), total * sizeof(float4), hipMemcpyDeviceToHost));
    MRS_HIP_TRY(hipMemcpy(pts.data(), S.pts.get(), total * sizeof(float4), hipMemcpyDeviceToHost));
    for (int c = 0; c < h->n_pairs; ++c) {  // the library stores clouds in Morton order; .w = original index
        const int64_t o = S.offs[c];
        for (int64_t i = o; i < S.offs[c + 1]; ++i) {
            int orig;
            memcpy(&orig, &pts[i].w, sizeof(int));
            memcpy(h_normals4 + (size_t)(o + orig) * 4, &nrm[i], sizeof(float4));
        }
    }
    return MRS_OK;
}

int mrs_gicp_batch_set_normals(mrs_gicp_batch* h, int32_t which, const float* d_normals, int32_t stride_floats, mrs_stream stream)
{
    MRS_REQUIRE(h && d_normals, "null pointer");
    MRS_REQUIRE(which == 0 || which == 1, "which must be 0 or 1");
    MRS_REQUIRE(stride_floats >= 3, "stride_floats must be >= 3");
    GicpCloud& S = h->side[which];
    MRS_REQUIRE(S.ready, "set_clouds first");
    MRS_HIP_TRY(hipSetDevice(h->ctx->device));
    hipStream_t s = (hipStream_t)stream;
    const int st = normals_room(h, which);
    if (st != MRS_OK) return st;
    S.nrm_key = 0;
    hipLaunchKernelGGL(k_normals_scatter, dim3((unsigned)((S.longest + 255) / 256), h->n_pairs), dim3(256), 0, s, (const float4*)S.pts.get(),
                       (const int64_t*)S.d_offs.get(), d_normals, stride_floats, S.nrm.get());
    MRS_HIP_TRY(hipGetLastError());
    S.nrm_key = kNormalsGiven;
    S.nrm_vp[0] = S.nrm_vp[1] = S.nrm_vp[2] = 0.0;
    return MRS_OK;
}

int mrs_gicp_batch_set_normals_host(mrs_gicp_batch* h, int32_t which, const float* h_normals, int32_t stride_floats)
{
    MRS_REQUIRE(h && h_normals, "null pointer");
    MRS_REQUIRE(which == 0 || which == 1, "which must be 0 or 1");
    MRS_REQUIRE(stride_floats >= 3, "stride_floats must be >= 3");
    MRS_REQUIRE(h->side[which].ready, "set_clouds first");
    MRS_HIP_TRY(hipSetDevice(h->ctx->device));
    const size_t bytes = (size_t)h->side[which].offs[h->n_pairs] * stride_floats * sizeof(float);
    mrs::Scratch stage;
    int st = stage.alloc(bytes, nullptr);
    if (st != MRS_OK) return st;
    MRS_HIP_TRY(hipMemcpy(stage.p, h_normals, bytes, hipMemcpyHostToDevice));
    if ((st = mrs_gicp_batch_set_normals(h, which, stage.as<float>(), stride_floats, nullptr)) != MRS_OK) return st;
    MRS_HIP_TRY(hipStreamSynchronize(nullptr));     // the staging buffer goes back to the cache only after the kernel has read it
    return MRS_OK;
}

// what the last alignment's searches did: mrs_gicp_batch_last_nn_passes / _last_searched_fraction
static int record_search_stats(mrs_gicp_batch* h, long nn_ticks)
{
    h->last_nn_passes = (double)nn_ticks;
    h->last_searched = 1.0;
    if (h->search_core == 1 && h->cert.searched && h->prm.voxel_res <= 0.0 && nn_ticks > 0) {
        std::vector<unsigned long long> stat((size_t)h->n_pairs * kStatStride);
        MRS_HIP_TRY(hipMemcpy(stat.data(), h->cert.searched.get(), stat.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        unsigned long long q[2] = {0, 0};
        for (int p = 0; p < h->n_pairs; ++p) { q[0] += stat[(size_t)p * kStatStride]; q[1] += stat[(size_t)p * kStatStride + 1]; }
        if (q[1]) h->last_searched = (double)q[0] / (double)q[1];
    }
    return MRS_OK;
}

static int ensure_state(mrs_gicp_batch* h)
{
    const GicpCloud& S = h->side[0];
    const size_t P = (size_t)h->n_pairs;
    // workgroups of the reduction kernels (k_linearize, k_linearize_voxel, k_fitness) per pair: every workgroup walks kLinChunks blocks of 1024
    // points before its 28 wave reductions + LDS round (one per 1024 points, the ds_bpermute butterflies were 38 % of the LDS pipe's time and
    // a third of the kernel's instructions: profiles/r04_pmc.json).  The partial sums are added in workgroup order (k_lm_update): a fixed order
    // for a given cloud size and batch size, the same for every search setting.
    // A small batch (the node's one pair at a time: 39 blocks of 1024 points) cannot afford that: 10 workgroups on 256 compute units; below four
    // workgroups per compute unit every block of 1024 points gets its own workgroup (k_linearize 25.7 -> 11 us per launch for one pair of 39 k points).
    const int cus = h->ctx->num_cu > 0 ? h->ctx->num_cu : 256;
    const int chunks = (int64_t)h->n_pairs * blocks_for_points((int)S.longest) >= (int64_t)4 * kLinChunks * cus ? kLinChunks : 1;
    const int mb = (blocks_for_points((int)S.longest) + chunks - 1) / chunks;
    int st;
    if ((st = h->lm.state.reserve(P, P)) != MRS_OK) return st;
    if ((st = h->lm.nblocks.reserve(P, P)) != MRS_OK) return st;
    if ((st = h->lm.nactive.reserve(kLmWindowMax * 4, kLmWindowMax * 4)) != MRS_OK) return st;
    if ((st = h->lm.partial.reserve(P * mb * kTerms, P * mb * kTerms)) != MRS_OK) return st;
    h->lm.max_blocks = mb;   // grid AND row stride of lm.partial: a function of the clouds at hand only (the block -> points mapping, hence the order
                             // of the sums, must not depend on what the object held before)
    const size_t cb = (size_t)((S.longest + kCertBlock - 1) / kCertBlock);
    if ((st = h->cert.bcount.reserve(P * cb, P * cb)) != MRS_OK) return st;
    h->cert.nb = (int)(h->cert.bcount.capacity() / P);      // grow-only, like the buffer: the row stride of the largest clouds so far
    std::vector<int> nb(h->n_pairs);
    for (int i = 0; i < h->n_pairs; ++i) nb[i] = std::min(blocks_for_points((int)(S.offs[i + 1] - S.offs[i])), h->lm.max_blocks);
    MRS_HIP_TRY(hipMemcpy(h->lm.nblocks.get(), nb.data(), nb.size() * sizeof(int), hipMemcpyHostToDevice));
    return MRS_OK;
}

static int build_voxel_map(mrs_gicp_batch* h, hipStream_t s)
{
    const GicpCloud& T = h->side[1];
    GicpVoxelMap& V = h->vox;
    if (V.res_built == h->prm.voxel_res && V.keys) return MRS_OK;
    MRS_REQUIRE(h->n_pairs < 65536, "VGICP supports at most 65535 pairs per batch");
    const size_t total = (size_t)T.offs[h->n_pairs];
    mrs::Scratch keys_in, keys_out, vals_in, vals_out, head, slot, tmp;
    int st;
    if ((st = keys_in.alloc(total * 8, s)) != MRS_OK) return st;
    if ((st = keys_out.alloc(total * 8, s)) != MRS_OK) return st;
    if ((st = vals_in.alloc(total * 4, s)) != MRS_OK) return st;
    if ((st = vals_out.alloc(total * 4, s)) != MRS_OK) return st;
    if ((st = head.alloc(total * 4, s)) != MRS_OK) return st;
    if ((st = slot.alloc(total * 4, s)) != MRS_OK) return st;
    hipLaunchKernelGGL(k_vox_keys, dim3((unsigned)std::min<int64_t>((T.longest + 255) / 256, 1024), h->n_pairs), dim3(256), 0, s,
                       T.pts.get(), T.d_offs.get(), h->prm.voxel_res, keys_in.as<unsigned long long>(), vals_in.as<int>());
    size_t b1 = 0, b2 = 0;
    MRS_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, b1, keys_in.as<unsigned long long>(), keys_out.as<unsigned long long>(),
                                                   vals_in.as<int>(), vals_out.as<int>(), (int)total, 0, 64, s));
    MRS_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, b2, head.as<int>(), slot.as<int>(), (int)total, s));
    if ((st = tmp.alloc(std::max(b1, b2), s)) != MRS_OK) return st;
    MRS_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(tmp.p, b1, keys_in.as<unsigned long long>(), keys_out.as<unsigned long long>(),
                                                   vals_in.as<int>(), vals_out.as<int>(), (int)total, 0, 64, s));
    const int fb = (int)std::min<size_t>((total + 255) / 256, 4096);
    hipLaunchKernelGGL(k_vox_heads, dim3(fb), dim3(256), 0, s, keys_out.as<unsigned long long>(), total, head.as<int>());
    MRS_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(tmp.p, b2, head.as<int>(), slot.as<int>(), (int)total, s));
    int last_head = 0, last_slot = 0;
    MRS_HIP_TRY(hipMemcpyAsync(&last_head, head.as<int>() + (total - 1), 4, hipMemcpyDeviceToHost, s));
    MRS_HIP_TRY(hipMemcpyAsync(&last_slot, slot.as<int>() + (total - 1), 4, hipMemcpyDeviceToHost, s));
    MRS_HIP_TRY(hipStreamSynchronize(s));
    V.n = last_head + last_slot;
    if ((st = fresh(V.keys, (size_t)V.n)) != MRS_OK) return st;
    if ((st = fresh(V.mean, (size_t)V.n)) != MRS_OK) return st;
    if ((st = fresh(V.cov, (size_t)V.n * 6)) != MRS_OK) return st;
    hipLaunchKernelGGL(k_vox_build, dim3(fb), dim3(256), 0, s, T.pts.get(), T.cov.get(), keys_out.as<unsigned long long>(),
                       vals_out.as<int>(), head.as<int>(), slot.as<int>(), total, V.keys.get(), V.mean.get(), V.cov.get());
    MRS_HIP_TRY(hipGetLastError());
    MRS_HIP_TRY(hipStreamSynchronize(s));
    V.res_built = h->prm.voxel_res;
    return MRS_OK;
}

int mrs_gicp_batch_get_voxel_map(mrs_gicp_batch* h, int32_t* h_n_voxels, int32_t* h_pair, int32_t* h_coord, float* h_mean, int32_t* h_count,
                                 double* h_cov6, mrs_stream stream)
{
    MRS_REQUIRE(h && h_n_voxels, "null pointer");
    MRS_REQUIRE(h->clouds_set(), "set source and target clouds first");
    MRS_REQUIRE(h->prm.voxel_res > 0.0, "voxel_resolution is 0: plain GICP has no voxel map");
    MRS_HIP_TRY(hipSetDevice(h->ctx->device));
    hipStream_t s = (hipStream_t)stream;
    int st;
    for (int w = 0; w < 2; ++w)     // like linearize
        if (!h->side[w].cov_valid) { st = mrs_gicp_batch_compute_covariances(h, w, nullptr, stream); if (st != MRS_OK) return st; }
    if ((st = build_voxel_map(h, s)) != MRS_OK) return st;
    const GicpVoxelMap& V = h->vox;
    *h_n_voxels = V.n;
    if (!h_pair && !h_coord && !h_mean && !h_count && !h_cov6) return MRS_OK;
    const size_t n = (size_t)V.n;
    std::vector<unsigned long long> keys(n);
    std::vector<float4> mean(n);
    MRS_HIP_TRY(hipMemcpyAsync(keys.data(), V.keys.get(), n * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    MRS_HIP_TRY(hipMemcpyAsync(mean.data(), V.mean.get(), n * sizeof(float4), hipMemcpyDeviceToHost, s));
    if (h_cov6) MRS_HIP_TRY(hipMemcpyAsync(h_cov6, V.cov.get(), n * 6 * sizeof(double), hipMemcpyDeviceToHost, s));
    MRS_HIP_TRY(hipStreamSynchronize(s));
    for (size_t v = 0; v < n; ++v) {
        const unsigned long long k = keys[v];   // voxel_key: pair | x | y | z, the coordinates offset by 32768
        if (h_pair) h_pair[v] = (int32_t)(k >> 48);
        if (h_coord)
            for (int a = 0; a < 3; ++a) h_coord[3 * v + a] = (int32_t)((k >> (32 - 16 * a)) & 0xffff) - 32768;
        if (h_mean) { h_mean[3 * v] = mean[v].x; h_mean[3 * v + 1] = mean[v].y; h_mean[3 * v + 2] = mean[v].z; }
        if (h_count) h_count[v] = (int32_t)mean[v].w;
    }
    return MRS_OK;
}

/* ---- alignments: one tick driver (run_ticks) and the frame around it (run_alignment), four estimators ---- */

// The context slot (second stream, two events, pinned buffer) an alignment of a small batch borrows for the duration of the call when it needs
// one: for covariances side by side (the stream and the events) or for a window's counters (the pinned buffer).  It goes back
// idle: on the normal way out it is (the last window was synchronised); on any other way out work may still run on its stream, or a window's
// counters may still be on their way into its pinned buffer from `s`, so both streams are drained first.
struct AlignSide {
    mrs_ctx* ctx; hipStream_t s; std::unique_ptr<mrs::SideSlot> sl; bool completed;
    ~AlignSide()
    {
        if (!completed && sl) {
            (void)hipStreamSynchronize(sl->stream);
            (void)hipStreamSynchronize(s);
        }
        mrs::side_release(ctx, std::move(sl));
    }
};

// both clouds of a small batch are new (every registration of the nodes): a cloud of 30-40 k points fills 150 of the 256 compute units with one
// wave per SIMD, so the two k-NN + covariance passes run side by side on two streams instead of back to back
static bool covariances_side_by_side(const mrs_gicp_batch* h)
{
    return h->n_pairs <= kLmWindowPairs && !h->side[0].cov_valid && !h->side[1].cov_valid && !mrs::dev_env("MRS_GICP_SERIAL_COV");
}

// The covariances the handle does not hold yet, enqueued on `s`.  sl: the call's slot when they run side by side, else null.
static int covariances_first(mrs_gicp_batch* h, mrs::SideSlot* sl, hipStream_t s)
{
    int st;
    if (sl) {
        mrs::HandleStream& side = sl->stream;
        MRS_TRY(side.join_in(s));                                    // fork
        st = mrs_gicp_batch_compute_covariances(h, 1, nullptr, (mrs_stream)side.s);
        if (st != MRS_OK) return st;
        MRS_HIP_TRY(hipEventRecord(side.ev_out, side));              // join: recorded here, waited for behind the other cloud's pass
        st = mrs_gicp_batch_compute_covariances(h, 0, nullptr, (mrs_stream)s);
        if (st != MRS_OK) return st;
        MRS_HIP_TRY(hipStreamWaitEvent(s, side.ev_out, 0));
    }
    for (int w = 0; w < 2; ++w)
        if (!h->side[w].cov_valid) { st = mrs_gicp_batch_compute_covariances(h, w, nullptr, (mrs_stream)s); if (st != MRS_OK) return st; }
    return MRS_OK;
}

namespace {

// A launch site of the section further up that has to stand down here: k_pclgicp_sums<0, kPclTerms> is first used behind set_clouds_from's
// k_copy_segments<...>, and the compiler emits template kernels in the order of their first use.
void launch_pcl_sums(mrs_gicp_batch* h, hipStream_t s)
{
    const GicpCloud &S = h->side[0], &T = h->side[1];
    GicpLmBuffers& L = h->lm;
    // one launch over all 74 terms: it has no scratch at 2 waves per SIMD, so the two-range form is not needed
    hipLaunchKernelGGL((k_pclgicp_sums<0, kPclTerms>), dim3(L.max_blocks, h->n_pairs), dim3(kNNThreads), 0, s, S.pts.get(), S.d_offs.get(),
                       S.cov.get(), T.pts.get(), T.d_offs.get(), T.cov.get(), T.bbox.get(), L.state.get(), L.corr.get(), L.partial.get(), L.max_blocks);
}

// One registration method as the tick driver sees it.  A tick is one search of the pairs that iterate (nn_pass) and the estimator's two kernels:
// the sums over the correspondences and the per-pair update, which writes the tick's counters (see launch_lm_update).
struct Estimator {
    GicpParams sp;              // the searches' parameters: the handle's, with the call's own correspondence distance for ICP and PCL-GICP
    long max_ticks = 0;
    bool covariances = false;   // reads the clouds' covariances
    bool searches = true;       // false: the voxelised LM estimator, which looks its correspondences up in the targets' voxel map
    bool may_window = true;     // every kernel of a tick gates itself on the pair's device-side state (k_linearize_voxel does not)
    bool alternate = false;     // LM on ONE pair: windows enqueue every second tick without its search (trial_only)
    std::function<void(int* n_next, int trial_only, hipStream_t s)> tick;       // launches the sums and the update
};

// ticks per window; MRS_DEV=1 MRS_GICP_WINDOW=n (0 or 1: the per-tick schedule)
int lm_window()
{
    const char* const v = mrs::dev_env("MRS_GICP_WINDOW");
    return v ? std::max(0, std::min(kLmWindowMax, atoi(v))) : kLmWindow;
}

// ticks per window of this call, 0: the per-tick schedule
int window_of(const mrs_gicp_batch* h, const Estimator& est)
{
    const int window = h->n_pairs <= kLmWindowPairs && est.may_window ? lm_window() : 0;
    return window > 1 ? window : 0;
}

// The estimator's ticks until no pair iterates or max_ticks is reached; *nn_ticks: the ticks that carried a search.  With a slot, a small
// batch runs them in windows (see kLmWindowPairs) and the host reads a window's counters once; whatever is left, and every other batch, runs tick
// by tick.  The per-tick loop is written for LM, whose ticks are linearisations (next[0]) or trials (next[1]); for the three estimators without
// trials next[1] stays 0 and `next[0] > 0` is the loop's own condition.
int run_ticks(mrs_gicp_batch* h, const Estimator& est, mrs::SideSlot* slot, hipStream_t s, long* nn_ticks)
{
    int* const counters = h->lm.nactive.get();      // [kLmWindowMax][4]
    int st;
    long ticks = 0;
    *nn_ticks = 0;
    int next[3] = {h->n_pairs, 0, h->n_pairs};      // pairs to iterate (LM: to linearise), pairs in an LM trial, pairs of [0] that moved far
    const int window = slot ? window_of(h, est) : 0;
    if (window > 0) {
        static_assert(kLmWindowMax * 4 <= mrs::kSidePinnedInts, "the slot's pinned buffer holds a window's counters");
        int* const h_win = slot->pinned.get();
        const long bound = est.alternate ? 2 * est.max_ticks : est.max_ticks;      // a sat-out tick does no work: the bound counts work ticks
        while (next[0] + next[1] > 0 && ticks < bound) {
            MRS_HIP_TRY(hipMemsetAsync(counters, 0, (size_t)window * 4 * sizeof(int), s));
            for (int t = 0; t < window; ++t) {
                // ONE pair alternates between a linearisation and (at least) one LM trial: every second tick is enqueued without its four
                // search kernels (an empty launch still costs ~5 us on the stream: 20 us per trial tick, ~160 us per registration).  If the
                // pair needs a linearisation on such a tick after all (it only does after a rejected trial shifted the rhythm) it sits the
                // tick out -- k_linearize / k_lm_update leave it alone -- and takes the next one: same transitions, same bits.
                const int trial_only = (est.alternate && ((ticks + t) & 1)) ? 1 : 0;
                h->big_movers = 1;                      // the broad search gates itself on the pair's motion (k_nn_scan: gate)
                if (!trial_only && (st = nn_pass(h, est.sp, (ticks == 0 && t == 0) ? 0 : 1, s)) != MRS_OK) return st;
                est.tick(counters + 4 * t, trial_only, s);
            }
            MRS_HIP_TRY(hipGetLastError());
            MRS_HIP_TRY(hipMemcpyAsync(h_win, counters, (size_t)window * 4 * sizeof(int), hipMemcpyDeviceToHost, s));
            MRS_HIP_TRY(hipStreamSynchronize(s));
            for (int t = 0; t < window; ++t) *nn_ticks += h_win[4 * t + 3];
            for (int i = 0; i < 3; ++i) next[i] = h_win[4 * (window - 1) + i];
            ticks += window;
        }
    }
    while (next[0] + next[1] > 0 && ticks < est.max_ticks) {
        MRS_HIP_TRY(hipMemsetAsync(counters, 0, 4 * sizeof(int), s));
        if (est.searches && next[0] > 0) {   // only linearisations search; LM trials score the cached correspondences
            h->big_movers = next[2];
            if ((st = nn_pass(h, est.sp, *nn_ticks == 0 ? 0 : 1, s)) != MRS_OK) return st;
        }
        if (next[0] > 0) ++*nn_ticks;
        est.tick(counters, 0, s);
        MRS_HIP_TRY(hipGetLastError());
        MRS_HIP_TRY(hipMemcpyAsync(next, counters, 3 * sizeof(int), hipMemcpyDeviceToHost, s));
        MRS_HIP_TRY(hipStreamSynchronize(s));
        ++ticks;
    }
    return MRS_OK;
}

// Every pair active at its pose (h_poses; null: the identity).  narrow: through float, as the references' align() takes a Matrix4f guess.
// y0_max: the previous iteration's error starts at DBL_MAX (ICP).
void init_states(std::vector<LmState>& init, const double* h_poses, bool narrow, bool y0_max)
{
    for (size_t p = 0; p < init.size(); ++p) {
        LmState& S = init[p];
        memset(&S, 0, sizeof(LmState));
        for (int i = 0; i < 16; ++i) {
            const double g = h_poses ? h_poses[p * 16 + i] : (i % 5 == 0 ? 1.0 : 0.0);
            S.x[i] = S.xi[i] = narrow ? (double)(float)g : g;
        }
        if (y0_max) S.y0 = DBL_MAX;
        S.active = 1;
    }
}

// what an alignment hands back, per pair (all but `final` optional)
struct AlignOut {
    double* final; int32_t *converged, *iterations, *state; double* hessian;
};

int read_results(mrs_gicp_batch* h, std::vector<LmState>& states, const AlignOut& out)
{
    MRS_HIP_TRY(hipMemcpy(states.data(), h->lm.state.get(), states.size() * sizeof(LmState), hipMemcpyDeviceToHost));
    for (size_t p = 0; p < states.size(); ++p) {
        const LmState& S = states[p];
        for (int i = 0; i < 16; ++i) out.final[p * 16 + i] = (double)(float)S.x[i];  // final_transformation_ is float
        if (out.converged) out.converged[p] = S.converged;
        if (out.iterations) out.iterations[p] = S.outer;
        if (out.state) out.state[p] = S.inner;
        if (out.hessian) memcpy(out.hessian + p * 36, S.final_H, sizeof(S.final_H));
    }
    return MRS_OK;
}

// An alignment from `states` (init_states) to `out`, behind the caller's checks and its ensure_state -- device-side state first: its
// (blocking) upload of the per-pair block counts would otherwise wait for the covariance kernels enqueued here and keep the host from enqueuing
// the first ticks behind them.
int run_alignment(mrs_gicp_batch* h, const Estimator& est, std::vector<LmState>& states, const AlignOut& out, hipStream_t s)
{
    int st;
    const bool fork = est.covariances && covariances_side_by_side(h);
    AlignSide side{h->ctx, s, {}, false};
    if ((fork || window_of(h, est) > 0) && (st = mrs::side_acquire(h->ctx, &side.sl)) != MRS_OK) return st;
    if (est.covariances && (st = covariances_first(h, fork ? side.sl.get() : nullptr, s)) != MRS_OK) return st;
    if (!est.searches && (st = build_voxel_map(h, s)) != MRS_OK) return st;
    MRS_HIP_TRY(hipMemcpyAsync(h->lm.state.get(), states.data(), states.size() * sizeof(LmState), hipMemcpyHostToDevice, s));
    if (h->cert.searched) MRS_HIP_TRY(hipMemsetAsync(h->cert.searched.get(), 0, (size_t)h->n_pairs * kStatStride * sizeof(unsigned long long), s));
    long nn_ticks = 0;
    if ((st = run_ticks(h, est, side.sl.get(), s, &nn_ticks)) != MRS_OK) return st;
    // every tick loop ends in a synchronisation of `s` and runs at least once (n_pairs >= 1, max_ticks >= 1): nothing is in flight here
    if ((st = record_search_stats(h, nn_ticks)) != MRS_OK) return st;
    if ((st = read_results(h, states, out)) != MRS_OK) return st;
    side.completed = true;
    return MRS_OK;
}

// The one-iteration hooks' prelude: the states at the given poses uploaded, a tick's counters cleared, one plain search with the handle's
// search setting (sp null: none)
int step_prelude(mrs_gicp_batch* h, const std::vector<LmState>& init, const GicpParams* sp, hipStream_t s)
{
    MRS_HIP_TRY(hipMemcpyAsync(h->lm.state.get(), init.data(), init.size() * sizeof(LmState), hipMemcpyHostToDevice, s));
    MRS_HIP_TRY(hipMemsetAsync(h->lm.nactive.get(), 0, 4 * sizeof(int), s));
    return sp ? nn_pass(h, *sp, 2, s) : MRS_OK;
}

// ... and what their epilogues share: the correspondences in the caller's numbering if wanted, and the states on their way back if wanted
// (the hook adds its own copies and synchronises)
int step_epilogue(mrs_gicp_batch* h, int32_t* d_corr, std::vector<LmState>* states, hipStream_t s)
{
    if (d_corr) launch_corr_to_original(h, d_corr, s);
    MRS_HIP_TRY(hipGetLastError());
    if (states) MRS_HIP_TRY(hipMemcpyAsync(states->data(), h->lm.state.get(), states->size() * sizeof(LmState), hipMemcpyDeviceToHost, s));
    return MRS_OK;
}

// The ICP and PCL-GICP profile hooks' prelude: the states at the given poses on the device, the timer's events, and one plain search of every
// source point (the handle's search setting, warm) timed alone into ms
int profile_prelude(mrs_gicp_batch* h, const std::vector<LmState>& init, const GicpParams& sp, mrs::RepTimer& timer, int reps, float& ms,
                    hipStream_t s)
{
    MRS_HIP_TRY(hipMemcpyAsync(h->lm.state.get(), init.data(), init.size() * sizeof(LmState), hipMemcpyHostToDevice, s));
    MRS_HIP_TRY(hipStreamSynchronize(s));
    MRS_TRY(timer.create());
    int nn_st = MRS_OK;
    const int st = timer.timed(ms, reps, s, [&]() { const int r = nn_pass(h, sp, 2, s); if (r != MRS_OK) nn_st = r; });
    return st != MRS_OK ? st : nn_st;
}

// out_counts[0]: source points, [1]: those with a correspondence after the last search.  Blocking.
int count_correspondences(mrs_gicp_batch* h, int64_t* out_counts)
{
    std::vector<int> corr(h->lm.n_seed);
    MRS_HIP_TRY(hipMemcpy(corr.data(), h->lm.corr.get(), corr.size() * sizeof(int), hipMemcpyDeviceToHost));
    int64_t c = 0;
    for (int v : corr) c += v >= 0;
    out_counts[0] = (int64_t)corr.size(); out_counts[1] = c;
    return MRS_OK;
}

}  // namespace

/* fast_gicp's LM-GICP, voxelised when the handle's voxel_resolution is positive.  An outer iteration is a linearisation and up to lm_max_iter
 * trials, a tick each. */
int mrs_gicp_batch_align(mrs_gicp_batch* h, const double* h_guess, double* h_final, int32_t* h_converged,
                         int32_t* h_iterations, double* h_hessian, mrs_stream stream)
{
    MRS_REQUIRE(h && h_final, "null pointer");
    MRS_REQUIRE(h->clouds_set(), "set source and target clouds first");
    MRS_HIP_TRY(hipSetDevice(h->ctx->device));
    const int st = ensure_state(h);
    if (st != MRS_OK) return st;
    std::vector<LmState> init(h->n_pairs);
    init_states(init, h_guess, true, false);
    for (LmState& S : init) { S.lambda = -1.0; S.nu = 2.0; }
    const bool voxel = h->prm.voxel_res > 0.0;
    const int limit = h->prm.force_iters > 0 ? h->prm.force_iters : h->prm.max_iter;
    Estimator est;
    est.sp = h->prm;
    est.max_ticks = (long)limit * (h->prm.lm_max_iter + 1) + 1;
    est.covariances = true;
    est.searches = est.may_window = !voxel;
    est.alternate = h->n_pairs == 1;
    est.tick = [h, voxel](int* n_next, int trial_only, hipStream_t s) {
        if (voxel)
            launch_linearize_voxel(h, s);
        else
            launch_linearize(h, trial_only, s);
        launch_lm_update(h, n_next, trial_only, s);
    };
    return run_alignment(h, est, init,AlignOut{h_final, h_converged, h_iterations, nullptr, h_hessian}, (hipStream_t)stream);
}

/* ---- point-to-point ICP (row G9; kernels: icp_device.hpp) ---- */

void mrs_icp_default_params(mrs_icp_params* p)
{
    if (!p) return;
    p->max_iterations = 10;                             // pcl::Registration; Mapping sets icp_iters (global_manager.cpp:892, :2431)
    p->force_iterations = 0;
    p->max_correspondence_distance = sqrt(DBL_MAX);     // Mapping: 2.0 (:891) and 100 (:2430)
    p->transformation_epsilon = 0.0;                    // Mapping: 1e-3 (:893, :2432)
    p->rotation_epsilon = 0.0;
    p->euclidean_fitness_epsilon = -DBL_MAX;            // never fires; Mapping: 1e-3 (:894, :2433)
}

namespace {

int icp_check_params(const mrs_icp_params* p)
{
    MRS_REQUIRE(p->max_iterations > 0, "max_iterations must be positive");
    MRS_REQUIRE(p->force_iterations >= 0, "force_iterations must be >= 0");
    MRS_REQUIRE(p->max_correspondence_distance > 0, "max_correspondence_distance must be positive");
    return MRS_OK;
}

IcpParams icp_device_params(const mrs_gicp_batch* h, const mrs_icp_params* p)
{
    IcpParams d;
    d.crit.trans_eps = p->transformation_epsilon;
    d.crit.rot_thr = mrs::icp_rotation_threshold(p->rotation_epsilon, p->transformation_epsilon);
    d.crit.fit_eps = p->euclidean_fitness_epsilon;
    d.crit.max_iter = p->max_iterations;
    d.crit.force_iters = p->force_iterations;
    d.motion_switch = h->prm.motion_switch;
    d.pad = 0;
    return d;
}

// The searches' parameters of an ICP call: the handle's (search margins, motion switch) with ICP's own correspondence distance.
GicpParams icp_search_params(const mrs_gicp_batch* h, const mrs_icp_params* p)
{
    GicpParams sp = h->prm;
    sp.max_corr2 = p->max_correspondence_distance >= 1e150 ? INFINITY : p->max_correspondence_distance * p->max_correspondence_distance;
    return sp;
}

// state, block counts and a partial buffer for the terms of the estimator at hand (29 for point-to-plane: one more than GICP's 28)
int icp_ensure_state(mrs_gicp_batch* h, bool plane)
{
    const int st = ensure_state(h);
    if (st != MRS_OK || !plane) return st;
    const size_t need = (size_t)h->n_pairs * h->lm.max_blocks * kIcpPlaneTerms;
    return h->lm.partial.reserve(need, need);
}

// The target normals of a point-to-plane call: those the handle holds, else computed with the call's k and viewpoint.
int icp_plane_normals(mrs_gicp_batch* h, const mrs_icp_plane_params* p, mrs_stream stream)
{
    MRS_REQUIRE(p->normal_k >= 3 && p->normal_k <= 32, "normal_k must be in [3, 32]");
    if (h->side[1].nrm_key != 0) return MRS_OK;
    return mrs_gicp_batch_compute_normals(h, 1, p->normal_k, p->viewpoint, stream);
}

mrs_icp_params icp_params_of(const mrs_icp_plane_params* p)
{
    mrs_icp_params q;
    q.max_iterations = p->max_iterations;
    q.force_iterations = p->force_iterations;
    q.max_correspondence_distance = p->max_correspondence_distance;
    q.transformation_epsilon = p->transformation_epsilon;
    q.rotation_epsilon = p->rotation_epsilon;
    q.euclidean_fitness_epsilon = p->euclidean_fitness_epsilon;
    return q;
}

int icp_align(mrs_gicp_batch* h, const mrs_icp_params* p, bool plane, const double* h_guess, double* h_final, int32_t* h_converged,
              int32_t* h_iterations, int32_t* h_state, mrs_stream stream)
{
    MRS_HIP_TRY(hipSetDevice(h->ctx->device));
    const int st = icp_ensure_state(h, plane);
    if (st != MRS_OK) return st;
    const IcpParams dp = icp_device_params(h, p);
    Estimator est;              // one kind of tick, one iteration each: search, sums, update.  No covariances, no voxel map.
    est.sp = icp_search_params(h, p);
    est.max_ticks = p->force_iterations > 0 ? p->force_iterations : p->max_iterations;
    est.tick = [h, plane, &dp](int* n_next, int, hipStream_t s) {
        launch_icp_sums(h, plane, s);
        launch_icp_update(h, plane, dp, n_next, s);
    };
    std::vector<LmState> init(h->n_pairs);
    init_states(init, h_guess, true, true);
    return run_alignment(h, est, init, AlignOut{h_final, h_converged, h_iterations, h_state, nullptr}, (hipStream_t)stream);
}

int icp_step(mrs_gicp_batch* h, const mrs_icp_params* p, bool plane, const double* h_poses, double* h_sums, double* h_delta, int32_t* h_state,
             int32_t* d_corr, mrs_stream stream)
{
    int st;
    MRS_HIP_TRY(hipSetDevice(h->ctx->device));
    hipStream_t s = (hipStream_t)stream;
    const int terms = plane ? kIcpPlaneTerms : kIcpTerms;
    if ((st = icp_ensure_state(h, plane)) != MRS_OK) return st;
    IcpParams dp = icp_device_params(h, p);
    dp.crit.max_iter = 1;           // one iteration, then the pair stops whatever the criteria say
    dp.crit.force_iters = 0;
    const GicpParams sp = icp_search_params(h, p);
    std::vector<LmState> init(h->n_pairs);
    init_states(init, h_poses, false, true);
    if ((st = step_prelude(h, init, &sp, s)) != MRS_OK) return st;
    launch_icp_sums(h, plane, s);
    launch_icp_update(h, plane, dp, h->lm.nactive.get(), s);
    if ((st = step_epilogue(h, d_corr, &init, s)) != MRS_OK) return st;
    MRS_HIP_TRY(hipStreamSynchronize(s));
    for (int q = 0; q < h->n_pairs; ++q) {
        memcpy(h_sums + (size_t)q * terms, init[q].H, terms * sizeof(double));
        memcpy(h_delta + (size_t)q * 16, init[q].delta, 16 * sizeof(double));
        if (h_state) h_state[q] = init[q].inner;
    }
    return MRS_OK;
}

}  // namespace

int mrs_gicp_batch_align_icp(mrs_gicp_batch* h, const mrs_icp_params* p, const double* h_guess, double* h_final, int32_t* h_converged,
                             int32_t* h_iterations, int32_t* h_state, mrs_stream stream)
{
    MRS_REQUIRE(h && p && h_final, "null pointer");
    MRS_REQUIRE(h->clouds_set(), "set source and target clouds first");
    MRS_REQUIRE(!h->no_cov, "a covariance-free container holds no correspondence buffers");
    const int st = icp_check_params(p);
    if (st != MRS_OK) return st;
    return icp_align(h, p, false, h_guess, h_final, h_converged, h_iterations, h_state, stream);
}

int mrs_gicp_batch_icp_step(mrs_gicp_batch* h, const mrs_icp_params* p, const double* h_poses, double* h_sums, double* h_delta,
                            int32_t* d_corr, mrs_stream stream)
{
    MRS_REQUIRE(h && p && h_poses && h_sums && h_delta, "null pointer");
    MRS_REQUIRE(h->clouds_set(), "set source and target clouds first");
    MRS_REQUIRE(!h->no_cov, "a covariance-free container holds no correspondence buffers");
    const int st = icp_check_params(p);
    if (st != MRS_OK) return st;
    return icp_step(h, p, false, h_poses, h_sums, h_delta, nullptr, d_corr, stream);
}

/* ---- point-to-plane ICP (row G12; kernels: icp_plane_device.hpp): ICP's tick loop with the plane estimator behind the target normals ---- */

void mrs_icp_plane_default_params(mrs_icp_plane_params* p)
{
    if (!p) return;
    mrs_icp_params q;
    mrs_icp_default_params(&q);
    p->max_iterations = q.max_iterations;
    p->force_iterations = q.force_iterations;
    p->max_correspondence_distance = q.max_correspondence_distance;
    p->transformation_epsilon = q.transformation_epsilon;
    p->rotation_epsilon = q.rotation_epsilon;
    p->euclidean_fitness_epsilon = q.euclidean_fitness_epsilon;
    p->normal_k = 15;                                   // setKSearch(15): global_manager.cpp:2689
    p->viewpoint[0] = p->viewpoint[1] = p->viewpoint[2] = 0.0;
}

int mrs_gicp_batch_align_icp_plane(mrs_gicp_batch* h, const mrs_icp_plane_params* p, const double* h_guess, double* h_final,
                                   int32_t* h_converged, int32_t* h_iterations, int32_t* h_state, mrs_stream stream)
{
    MRS_REQUIRE(h && p && h_final, "null pointer");
    MRS_REQUIRE(h->clouds_set(), "set source and target clouds first");
    MRS_REQUIRE(!h->no_cov, "a covariance-free container holds no correspondence buffers");
    const mrs_icp_params q = icp_params_of(p);
    int st = icp_check_params(&q);
    if (st != MRS_OK) return st;
    if ((st = icp_plane_normals(h, p, stream)) != MRS_OK) return st;
    return icp_align(h, &q, true, h_guess, h_final, h_converged, h_iterations, h_state, stream);
}

int mrs_gicp_batch_icp_plane_step(mrs_gicp_batch* h, const mrs_icp_plane_params* p, const double* h_poses, double* h_sums, double* h_delta,
                                  int32_t* h_state, int32_t* d_corr, mrs_stream stream)
{
    MRS_REQUIRE(h && p && h_poses && h_sums && h_delta, "null pointer");
    MRS_REQUIRE(h->clouds_set(), "set source and target clouds first");
    MRS_REQUIRE(!h->no_cov, "a covariance-free container holds no correspondence buffers");
    const mrs_icp_params q = icp_params_of(p);
    int st = icp_check_params(&q);
    if (st != MRS_OK) return st;
    if ((st = icp_plane_normals(h, p, stream)) != MRS_OK) return st;
    return icp_step(h, &q, true, h_poses, h_sums, h_delta, h_state, d_corr, stream);
}

/* ---- PCL-style GICP (row G11; kernels: pclgicp_device.hpp) ---- */

void mrs_pclgicp_default_params(mrs_pclgicp_params* p)
{
    if (!p) return;
    p->max_iterations = 200;                    // pcl::GeneralizedIterativeClosestPoint; Mapping sets icp_iters (global_manager.cpp:2423)
    p->max_inner_iterations = 20;               // setMaximumOptimizerIterations
    p->force_iterations = 0;
    p->max_correspondence_distance = 5.0;       // Mapping: 100 (:2422)
    p->rotation_epsilon = 2e-3;
    p->transformation_epsilon = 5e-4;           // Mapping: 1e-3 (:2424)
    p->gradient_tolerance = 1e-2;
}

namespace {

int pcl_check_params(const mrs_pclgicp_params* p)
{
    MRS_REQUIRE(p->max_iterations > 0, "max_iterations must be positive");
    MRS_REQUIRE(p->max_inner_iterations > 0, "max_inner_iterations must be positive");
    MRS_REQUIRE(p->force_iterations >= 0, "force_iterations must be >= 0");
    MRS_REQUIRE(p->max_correspondence_distance > 0, "max_correspondence_distance must be positive");
    MRS_REQUIRE(p->rotation_epsilon > 0, "rotation_epsilon must be positive");
    MRS_REQUIRE(p->transformation_epsilon > 0, "transformation_epsilon must be positive");
    MRS_REQUIRE(p->gradient_tolerance > 0, "gradient_tolerance must be positive");
    return MRS_OK;
}

PclGicpParams pcl_device_params(const mrs_gicp_batch* h, const mrs_pclgicp_params* p)
{
    PclGicpParams d;
    d.crit.rot_eps = p->rotation_epsilon;
    d.crit.trans_eps = p->transformation_epsilon;
    d.crit.grad_tol = p->gradient_tolerance;
    d.crit.max_iter = p->max_iterations;
    d.crit.max_inner = p->max_inner_iterations;
    d.crit.force_iters = p->force_iterations;
    d.crit.pad = 0;
    d.motion_switch = h->prm.motion_switch;
    d.pad = 0;
    return d;
}

// The searches' parameters of a PCL-GICP call: the handle's (search margins, motion switch) with the call's own correspondence distance.
GicpParams pcl_search_params(const mrs_gicp_batch* h, const mrs_pclgicp_params* p)
{
    GicpParams sp = h->prm;
    sp.max_corr2 = p->max_correspondence_distance >= 1e150 ? INFINITY : p->max_correspondence_distance * p->max_correspondence_distance;
    sp.voxel_res = 0.0;
    return sp;
}

// state, block counts and a partial buffer of 74 terms per workgroup plus the totals' row per pair
int pcl_ensure_state(mrs_gicp_batch* h)
{
    int st = ensure_state(h);
    if (st != MRS_OK) return st;
    const size_t need = (size_t)h->n_pairs * (h->lm.max_blocks + 1) * kPclTerms;
    return h->lm.partial.reserve(need, need);
}

}  // namespace

/* ICP's kind of tick (search, sums, update: one iteration each) behind the covariances of mrs_gicp_batch_align. */
int mrs_gicp_batch_align_pcl(mrs_gicp_batch* h, const mrs_pclgicp_params* p, const double* h_guess, double* h_final, int32_t* h_converged,
                             int32_t* h_iterations, int32_t* h_state, mrs_stream stream)
{
    MRS_REQUIRE(h && p && h_final, "null pointer");
    MRS_REQUIRE(h->clouds_set(), "set source and target clouds first");
    MRS_REQUIRE(!h->no_cov, "a covariance-free container holds no covariances");
    int st = pcl_check_params(p);
    if (st != MRS_OK) return st;
    MRS_HIP_TRY(hipSetDevice(h->ctx->device));
    if ((st = pcl_ensure_state(h)) != MRS_OK) return st;
    const PclGicpParams dp = pcl_device_params(h, p);
    Estimator est;
    est.sp = pcl_search_params(h, p);
    est.max_ticks = p->force_iterations > 0 ? p->force_iterations : p->max_iterations;
    est.covariances = true;
    est.tick = [h, &dp](int* n_next, int, hipStream_t s) {
        launch_pcl_sums(h, s);
        launch_pcl_update(h, dp, n_next, s);
    };
    std::vector<LmState> init(h->n_pairs);
    init_states(init, h_guess, true, false);
    return run_alignment(h, est, init, AlignOut{h_final, h_converged, h_iterations, h_state, nullptr}, (hipStream_t)stream);
}

int mrs_gicp_batch_pcl_step(mrs_gicp_batch* h, const mrs_pclgicp_params* p, const double* h_poses, double* h_sums, double* h_next,
                            int32_t* h_inner, int32_t* d_corr, mrs_stream stream)
{
    MRS_REQUIRE(h && p && h_poses && h_sums && h_next && h_inner, "null pointer");
    MRS_REQUIRE(h->clouds_set(), "set source and target clouds first");
    MRS_REQUIRE(!h->no_cov, "a covariance-free container holds no covariances");
    int st = pcl_check_params(p);
    if (st != MRS_OK) return st;
    MRS_HIP_TRY(hipSetDevice(h->ctx->device));
    hipStream_t s = (hipStream_t)stream;
    GicpLmBuffers& L = h->lm;
    if ((st = pcl_ensure_state(h)) != MRS_OK) return st;
    if ((st = covariances_first(h, nullptr, s)) != MRS_OK) return st;
    PclGicpParams dp = pcl_device_params(h, p);
    dp.crit.max_iter = 1;           // one iteration, then the pair stops whatever the rule says
    dp.crit.force_iters = 0;
    const GicpParams sp = pcl_search_params(h, p);
    const int P = h->n_pairs;
    std::vector<LmState> init(P);
    init_states(init, h_poses, false, false);
    if ((st = step_prelude(h, init, &sp, s)) != MRS_OK) return st;
    launch_pcl_sums(h, s);
    launch_pcl_update(h, dp, L.nactive.get(), s);
    if ((st = step_epilogue(h, d_corr, &init, s)) != MRS_OK) return st;
    for (int q = 0; q < P; ++q)
        MRS_HIP_TRY(hipMemcpyAsync(h_sums + (size_t)q * kPclTerms, L.partial.get() + ((size_t)q * (L.max_blocks + 1) + L.max_blocks) * kPclTerms,
                                   kPclTerms * sizeof(double), hipMemcpyDeviceToHost, s));
    MRS_HIP_TRY(hipStreamSynchronize(s));
    for (int q = 0; q < P; ++q) {
        memcpy(h_next + (size_t)q * 16, init[q].x, 16 * sizeof(double));
        h_inner[2 * q] = init[q].trials;
        h_inner[2 * q + 1] = init[q].failed;
    }
    return MRS_OK;
}

/* Measurement hook of tools/bench_pclgicp.py: the three stages of one iteration launched ALONE between HIP events on `stream`, at the given
 * poses, `reps` times each (the average goes to out_ms): [0] the search of every source point (the handle's search setting, warm),
 * [1] k_pclgicp_sums, [2] k_pclgicp_update.  out_counts: [0] source points, [1] correspondences at the poses.  Overwrites the batch's
 * correspondences and warm-start seeds. */
int mrs_gicp_batch_pcl_profile(mrs_gicp_batch* h, const mrs_pclgicp_params* p, const double* h_poses, int32_t reps, float* out_ms,
                               int64_t* out_counts, mrs_stream stream)
{
    MRS_REQUIRE(h && p && h_poses && out_ms && out_counts, "null pointer");
    MRS_REQUIRE(h->clouds_set(), "set source and target clouds first");
    MRS_REQUIRE(!h->no_cov, "a covariance-free container holds no covariances");
    MRS_REQUIRE(reps >= 1, "reps must be >= 1");
    int st = pcl_check_params(p);
    if (st != MRS_OK) return st;
    MRS_HIP_TRY(hipSetDevice(h->ctx->device));
    hipStream_t s = (hipStream_t)stream;
    GicpLmBuffers& L = h->lm;
    if ((st = pcl_ensure_state(h)) != MRS_OK) return st;
    if ((st = covariances_first(h, nullptr, s)) != MRS_OK) return st;
    PclGicpParams dp = pcl_device_params(h, p);
    dp.crit.max_iter = INT32_MAX;       // the update kernel is timed on pairs that stay active: no rule may end them
    dp.crit.force_iters = INT32_MAX;
    std::vector<LmState> init(h->n_pairs);
    init_states(init, h_poses, false, false);
    mrs::RepTimer timer;
    if ((st = profile_prelude(h, init, pcl_search_params(h, p), timer, reps, out_ms[0], s)) != MRS_OK) return st;
    if ((st = timer.timed(out_ms[1], reps, s, [&]() { launch_pcl_sums(h, s); })) != MRS_OK) return st;
    if ((st = count_correspondences(h, out_counts)) != MRS_OK) return st;
    MRS_HIP_TRY(hipMemsetAsync(L.nactive.get(), 0, 4 * sizeof(int), s));
    // every launch starts from the given poses (a device-to-device copy of the states, part of the time): the inner minimisation timed is
    // that of the sums at hand, not of a pose already at their minimum
    mrs::Scratch start;
    if ((st = start.alloc(init.size() * sizeof(LmState), s)) != MRS_OK) return st;
    MRS_HIP_TRY(hipMemcpyAsync(start.p, init.data(), init.size() * sizeof(LmState), hipMemcpyHostToDevice, s));
    MRS_HIP_TRY(hipStreamSynchronize(s));
    if ((st = timer.timed(out_ms[2], reps, s, [&]() {
             (void)hipMemcpyAsync(L.state.get(), start.p, init.size() * sizeof(LmState), hipMemcpyDeviceToDevice, s);
             launch_pcl_update(h, dp, L.nactive.get(), s);
         })) != MRS_OK) return st;
    return MRS_OK;
}

int mrs_gicp_batch_linearize(mrs_gicp_batch* h, const double* h_poses, double* h_H, double* h_b, double* h_err,
                             int32_t* d_corr, mrs_stream stream)
{
    MRS_REQUIRE(h && h_poses && h_H && h_b && h_err, "null pointer");
    MRS_REQUIRE(h->clouds_set(), "set source and target clouds first");
    MRS_HIP_TRY(hipSetDevice(h->ctx->device));
    hipStream_t s = (hipStream_t)stream;
    const GicpCloud& S = h->side[0];
    GicpLmBuffers& L = h->lm;
    const bool voxel = h->prm.voxel_res > 0.0;
    int st;
    if ((st = covariances_first(h, nullptr, s)) != MRS_OK) return st;
    if ((st = ensure_state(h)) != MRS_OK) return st;
    std::vector<LmState> init(h->n_pairs);
    init_states(init, h_poses, false, false);       // y0 stays 0: k_linearize does not read it
    if ((st = step_prelude(h, init, voxel ? nullptr : &h->prm, s)) != MRS_OK) return st;
    if (voxel) {
        if ((st = build_voxel_map(h, s)) != MRS_OK) return st;
        MRS_REQUIRE(d_corr == nullptr, "per-point correspondences are not defined for the voxelised variant");
        launch_linearize_voxel(h, s);
    } else {
        launch_linearize(h, 0, s);
    }
    if ((st = step_epilogue(h, d_corr, nullptr, s)) != MRS_OK) return st;
    std::vector<double> part((size_t)h->n_pairs * L.max_blocks * kTerms);
    MRS_HIP_TRY(hipMemcpyAsync(part.data(), L.partial.get(), part.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    MRS_HIP_TRY(hipStreamSynchronize(s));
    for (int p = 0; p < h->n_pairs; ++p) {
        double sum[kTerms] = {0};
        const int nb = std::min(blocks_for_points((int)(S.offs[p + 1] - S.offs[p])), L.max_blocks);
        for (int b = 0; b < nb; ++b)
            for (int t = 0; t < kTerms; ++t) sum[t] += part[((size_t)p * L.max_blocks + b) * kTerms + t];
        int t = 0;
        for (int r = 0; r < 6; ++r)
            for (int c = r; c < 6; ++c) { h_H[(size_t)p * 36 + 6 * r + c] = sum[t]; h_H[(size_t)p * 36 + 6 * c + r] = sum[t]; ++t; }
        for (int r = 0; r < 6; ++r) h_b[(size_t)p * 6 + r] = sum[21 + r];
        h_err[p] = sum[27];
    }
    return MRS_OK;
}

/* Measurement hook of tools/bench_icp.py: the three stages of one ICP iteration launched ALONE between HIP events on `stream`, at the given
 * poses, `reps` times each (the average goes to out_ms): [0] the search of every source point (the handle's search setting, warm),
 * [1] k_icp_sums, [2] k_icp_update.  out_counts: [0] source points, [1] correspondences at the poses.  Overwrites the batch's correspondences
 * and warm-start seeds.  plane (optional): the parameters of a point-to-plane call (tools/bench_icp_plane.py) -- its sums and update kernels
 * instead, and the targets' normals (selection + k_normals_from_knn) timed into ms_normals. */
static int icp_profile(mrs_gicp_batch* h, const mrs_icp_params* p, const mrs_icp_plane_params* plane, const double* h_poses, int32_t reps,
                       float* ms_search, float* ms_normals, float* ms_sums, float* ms_update, int64_t* out_counts, mrs_stream stream)
{
    MRS_REQUIRE(h->clouds_set(), "set source and target clouds first");
    MRS_REQUIRE(!h->no_cov, "a covariance-free container holds no correspondence buffers");
    MRS_REQUIRE(reps >= 1, "reps must be >= 1");
    int st = icp_check_params(p);
    if (st != MRS_OK) return st;
    MRS_HIP_TRY(hipSetDevice(h->ctx->device));
    hipStream_t s = (hipStream_t)stream;
    if ((st = icp_ensure_state(h, plane != nullptr)) != MRS_OK) return st;
    IcpParams dp = icp_device_params(h, p);
    dp.crit.max_iter = INT32_MAX;       // the update kernel is timed on pairs that stay active: no rule may end them
    dp.crit.force_iters = INT32_MAX;
    std::vector<LmState> init(h->n_pairs);
    init_states(init, h_poses, false, true);
    mrs::RepTimer timer;
    if ((st = profile_prelude(h, init, icp_search_params(h, p), timer, reps, *ms_search, s)) != MRS_OK) return st;
    if (plane) {
        MRS_REQUIRE(plane->normal_k >= 3 && plane->normal_k <= 32, "normal_k must be in [3, 32]");
        int nn_st = MRS_OK;
        if ((st = timer.timed(*ms_normals, reps, s, [&]() {
                 h->side[1].nrm_key = 0;            // computed again, whatever the handle holds
                 const int r = mrs_gicp_batch_compute_normals(h, 1, plane->normal_k, plane->viewpoint, stream);
                 if (r != MRS_OK) nn_st = r;
             })) != MRS_OK) return st;
        if (nn_st != MRS_OK) return nn_st;
    }
    if ((st = timer.timed(*ms_sums, reps, s, [&]() { launch_icp_sums(h, plane != nullptr, s); })) != MRS_OK) return st;
    if ((st = count_correspondences(h, out_counts)) != MRS_OK) return st;
    MRS_HIP_TRY(hipMemsetAsync(h->lm.nactive.get(), 0, 4 * sizeof(int), s));
    return timer.timed(*ms_update, reps, s, [&]() { launch_icp_update(h, plane != nullptr, dp, h->lm.nactive.get(), s); });
}

int mrs_gicp_batch_icp_profile(mrs_gicp_batch* h, const mrs_icp_params* p, const double* h_poses, int32_t reps, float* out_ms, int64_t* out_counts,
                               mrs_stream stream)
{
    MRS_REQUIRE(h && p && h_poses && out_ms && out_counts, "null pointer");
    return icp_profile(h, p, nullptr, h_poses, reps, out_ms, nullptr, out_ms + 1, out_ms + 2, out_counts, stream);
}

int mrs_gicp_batch_icp_plane_profile(mrs_gicp_batch* h, const mrs_icp_plane_params* p, const double* h_poses, int32_t reps, float* out_ms,
                                     int64_t* out_counts, mrs_stream stream)
{
    MRS_REQUIRE(h && p && h_poses && out_ms && out_counts, "null pointer");
    const mrs_icp_params q = icp_params_of(p);
    return icp_profile(h, &q, p, h_poses, reps, out_ms, out_ms + 1, out_ms + 2, out_ms + 3, out_counts, stream);
}

/* Measurement hook (bench.py's GICP rooflines): every kernel of one outer iteration launched ALONE between HIP events on `stream`, at
 * the given poses and with the batch's clouds / covariances, `reps` times each (the average goes to out_ms):
 *   [0] k_linearize, all 28 sums (phase 0)            [1] k_linearize, error only (an LM trial)
 *   [2] round-3 search of every point, warm           [3] k_nn_certify at an unchanged pose (everything certified)
 *   [4] round-4 search of every point, warm           [5] k-NN selection of the sources (k_knn_cov)
 *   [6] k_cov_from_knn of the sources                 [7] k_nn_certify + work-list search at a pose moved by 1 mm along x
 * out_counts: [0] source points, [1] correspondences (d^2 < max_corr^2) at the poses, [2] queries on the work lists of [7]. */
int mrs_gicp_batch_profile(mrs_gicp_batch* h, const double* h_poses, int32_t reps, float* out_ms, int64_t* out_counts, mrs_stream stream)
{
    MRS_REQUIRE(h && h_poses && out_ms && out_counts, "null pointer");
    MRS_REQUIRE(h->clouds_set(), "set source and target clouds first");
    MRS_REQUIRE(h->prm.voxel_res <= 0.0, "GICP only");
    MRS_REQUIRE(reps >= 1, "reps must be >= 1");
    MRS_HIP_TRY(hipSetDevice(h->ctx->device));
    hipStream_t s = (hipStream_t)stream;
    const GicpCloud& S = h->side[0];
    GicpLmBuffers& L = h->lm;
    int st;
    if ((st = covariances_first(h, nullptr, s)) != MRS_OK) return st;
    if ((st = ensure_state(h)) != MRS_OK) return st;
    const int P = h->n_pairs;
    std::vector<LmState> init(P);
    auto upload = [&](int phase, double dx) -> int {
        init_states(init, h_poses, false, false);
        for (LmState& S : init) {
            for (int i = 0; i < 16; ++i) S.delta[i] = (i % 5 == 0) ? 1.0 : 0.0;      // last step: none
            S.x[3] += dx; S.xi[3] += dx;
            S.phase = phase;
        }
        MRS_HIP_TRY(hipMemcpyAsync(L.state.get(), init.data(), init.size() * sizeof(LmState), hipMemcpyHostToDevice, s));
        MRS_HIP_TRY(hipStreamSynchronize(s));
        return MRS_OK;
    };
    // the search settings this function changes go back on EVERY way out (the MRS_HIP_TRY returns included)
    struct Guard {
        mrs_gicp_batch* h; int core, cold; bool cert;
        ~Guard() { h->search_core = core; h->cold_core = cold; h->use_certificates = cert; }
    } guard{h, h->search_core, h->cold_core, h->use_certificates};
    mrs::RepTimer timer;
    MRS_TRY(timer.create());
    const hipEvent_t e0 = timer.e0, e1 = timer.e1;
    h->search_core = 1; h->cold_core = 0; h->use_certificates = true;      // restored by `guard`
    auto round3 = [&]() { launch_nn_scan(h, h->prm, nullptr, 0, s); };
    auto linearize = [&]() { launch_linearize(h, 0, s); };
    if ((st = upload(0, 0.0)) != MRS_OK) return st;
    round3();                                         // seeds + correspondences at the poses
    if ((st = knn_dev_switches(s)) != MRS_OK) return st;
    if ((st = timer.timed(out_ms[2], reps, s, round3)) != MRS_OK) return st;
    if ((st = timer.timed(out_ms[0], reps, s, linearize)) != MRS_OK) return st;
    if ((st = count_correspondences(h, out_counts)) != MRS_OK) return st;       // at the poses
    if ((st = timer.timed(out_ms[4], reps, s, [&]() { launch_nn_scan_g(h, h->prm, false, s); })) != MRS_OK) return st;      // leaves certificates at the poses
    launch_nn_store_pose(h, 0, s);
    if ((st = timer.timed(out_ms[3], reps, s, [&]() { launch_nn_certify(h, h->prm, s); })) != MRS_OK) return st;
    if ((st = upload(1, 0.0)) != MRS_OK) return st;
    if ((st = timer.timed(out_ms[1], reps, s, linearize)) != MRS_OK) return st;
    // a pass after a 1 mm step: certify + search the work lists (the certificates are those of the unmoved poses: t_prev stays)
    if ((st = upload(0, 1e-3)) != MRS_OK) return st;
    {
        mrs::Scratch lb_save;
        if ((st = lb_save.alloc(L.n_seed * sizeof(float), s)) != MRS_OK) return st;
        MRS_HIP_TRY(hipMemcpyAsync(lb_save.p, h->cert.lb.get(), L.n_seed * sizeof(float), hipMemcpyDeviceToDevice, s));
        float acc = 0.0f;
        for (int r = 0; r < reps + 1; ++r) {
            MRS_HIP_TRY(hipMemcpyAsync(h->cert.lb.get(), lb_save.p, L.n_seed * sizeof(float), hipMemcpyDeviceToDevice, s));
            MRS_HIP_TRY(hipEventRecord(e0, s));
            launch_nn_certify(h, h->prm, s);
            launch_nn_scan_g(h, h->prm, true, s);
            MRS_HIP_TRY(hipEventRecord(e1, s));
            MRS_HIP_TRY(hipEventSynchronize(e1));
            float ms = 0.0f;
            MRS_HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
            if (r > 0) acc += ms;
        }
        out_ms[7] = acc / (float)reps;
        std::vector<int> bc((size_t)P * h->cert.nb);
        MRS_HIP_TRY(hipMemcpy(bc.data(), h->cert.bcount.get(), bc.size() * sizeof(int), hipMemcpyDeviceToHost));
        int64_t q = 0;
        for (int p = 0; p < P; ++p) {
            const int64_t n = S.offs[p + 1] - S.offs[p];
            for (int b = 0; b * (int64_t)kCertBlock < n; ++b) {
                const int64_t members = std::min<int64_t>(kCertBlock, n - b * (int64_t)kCertBlock), c = bc[(size_t)p * h->cert.nb + b];
                q += 2 * c > members ? members : c;
            }
        }
        out_counts[2] = q;
    }
    {   // k-NN selection + covariances of the sources
        const int k = h->prm.k;
        mrs::Scratch knn;
        if ((st = knn.alloc(knn_ints(L.n_seed, P, k) * sizeof(int), s)) != MRS_OK) return st;
        if ((st = timer.timed(out_ms[5], reps, s, [&]() { launch_knn_cov(h, 0, 0, P, k, knn.as<int>(), s); })) != MRS_OK) return st;
        if ((st = timer.timed(out_ms[6], reps, s, [&]() {
                 hipLaunchKernelGGL(k_cov_from_knn, dim3((unsigned)((S.longest + 255) / 256), P), dim3(256), 0, s, (const float4*)S.pts.get(),
                                    (const int64_t*)S.d_offs.get(), k, (const int*)knn.as<int>(), S.cov.get(), (int*)nullptr);
             })) != MRS_OK) return st;
        MRS_HIP_TRY(hipStreamSynchronize(s));
    }
    return MRS_OK;       // `guard` restores the search settings and destroys the events
}

int mrs_gicp_batch_fitness(mrs_gicp_batch* h, const double* h_poses, double max_range, double* h_scores,
                           mrs_stream stream)
{
    MRS_REQUIRE(h && h_poses && h_scores, "null pointer");
    MRS_REQUIRE(h->clouds_set(), "set source and target clouds first");
    MRS_HIP_TRY(hipSetDevice(h->ctx->device));
    hipStream_t s = (hipStream_t)stream;
    const GicpCloud &S = h->side[0], &T = h->side[1];
    int st = ensure_state(h);
    if (st != MRS_OK) return st;
    mrs::Scratch poses, part;
    st = poses.alloc((size_t)h->n_pairs * 16 * sizeof(double), s);
    if (st != MRS_OK) return st;
    // one round of the search (512 source points) per workgroup: the reduction kernels' grid (max_blocks: up to 4096 points per workgroup) left one
    // pair of 39 k points to 10 workgroups, 337 us for a search that takes 90
    const int fb = std::max(1, ((int)S.longest + 2 * kNNThreads - 1) / (2 * kNNThreads));
    st = part.alloc((size_t)h->n_pairs * fb * 2 * sizeof(double), s);
    if (st != MRS_OK) return st;
    // pageable host memory: a blocking copy (hipMemcpyAsync from a caller's stack array may be deferred past the launch)
    MRS_HIP_TRY(hipStreamSynchronize(s));
    MRS_HIP_TRY(hipMemcpy(poses.p, h_poses, (size_t)h->n_pairs * 16 * sizeof(double), hipMemcpyHostToDevice));
    MRS_HIP_TRY(hipMemsetAsync(part.p, 0, (size_t)h->n_pairs * fb * 2 * sizeof(double), s));
    hipLaunchKernelGGL(k_fitness, dim3(fb, h->n_pairs), dim3(kNNThreads), 0, s, S.pts.get(), S.d_offs.get(),
                       T.pts.get(), T.d_offs.get(), T.tile_base.get(), T.tlo.get(), T.thi.get(), T.mlo.get(), T.mhi.get(), poses.as<double>(), max_range,
                       part.as<double>(), fb, (const int*)h->lm.seed.get());
    MRS_HIP_TRY(hipGetLastError());
    std::vector<double> hp((size_t)h->n_pairs * fb * 2);
    MRS_HIP_TRY(hipMemcpyAsync(hp.data(), part.p, hp.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    MRS_HIP_TRY(hipStreamSynchronize(s));
    for (int p = 0; p < h->n_pairs; ++p) {
        double sum = 0, cnt = 0;
        for (int b = 0; b < fb; ++b) { sum += hp[((size_t)p * fb + b) * 2]; cnt += hp[((size_t)p * fb + b) * 2 + 1]; }
        h_scores[p] = cnt > 0 ? sum / cnt : DBL_MAX;  // pcl: std::numeric_limits<double>::max() when empty
    }
    return MRS_OK;
}


/* ---- RING++ point-feature front-end (row N1) ---- */
int mrs_pointfeat_from_neighbors(mrs_ctx* ctx, const float* d_points, int32_t n, int32_t k, const int32_t* d_knn,
                                 const float* d_eigens, float* d_features, mrs_stream stream)
{
    MRS_REQUIRE(ctx && d_points && d_knn && d_eigens && d_features, "null pointer");
    MRS_REQUIRE(n >= 0, "n must be >= 0");
    MRS_REQUIRE(k >= 1 && k <= 32, "k must be in [1, 32]");
    MRS_HIP_TRY(hipSetDevice(ctx->device));
    if (n == 0) return MRS_OK;
    hipLaunchKernelGGL(k_features_from_neighbors, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, d_points, n, k,
                       d_knn, d_eigens, d_features);
    MRS_HIP_TRY(hipGetLastError());
    return MRS_OK;
}

int mrs_pointfeat_from_neighbors_host(mrs_ctx* ctx, const float* h_points, int32_t n, int32_t k, const int32_t* h_knn,
                                      const float* h_eigens, float* h_features)
{
    MRS_REQUIRE(ctx && h_points && h_knn && h_eigens && h_features, "null pointer");
    MRS_REQUIRE(n > 0, "n must be positive");
    MRS_HIP_TRY(hipSetDevice(ctx->device));
    const size_t N = (size_t)n;
    DeviceBuffer<float> dp, de, df;
    DeviceBuffer<int> dk;
    int st;
    if ((st = dp.reserve(N * 3, N * 3)) != MRS_OK || (st = dk.reserve(N * k, N * k)) != MRS_OK || (st = de.reserve(N * 5, N * 5)) != MRS_OK ||
        (st = df.reserve(N * 13, N * 13)) != MRS_OK)
        return st;
    MRS_HIP_TRY(hipMemcpy(dp.get(), h_points, N * 3 * 4, hipMemcpyHostToDevice));
    MRS_HIP_TRY(hipMemcpy(dk.get(), h_knn, N * k * 4, hipMemcpyHostToDevice));
    MRS_HIP_TRY(hipMemcpy(de.get(), h_eigens, N * 5 * 4, hipMemcpyHostToDevice));
    if ((st = mrs_pointfeat_from_neighbors(ctx, dp.get(), n, k, dk.get(), de.get(), df.get(), nullptr)) != MRS_OK) return st;
    MRS_HIP_TRY(hipMemcpy(h_features, df.get(), N * 13 * 4, hipMemcpyDeviceToHost));
    return MRS_OK;
}

int mrs_pointfeat_batch(mrs_ctx* ctx, const float* d_points, int32_t stride_floats, const int64_t* h_offsets,
                        int32_t batch, int32_t k, int32_t* d_knn, float* d_eigens, float* d_features,
                        float* d_feat_planes, mrs_stream stream)
{
    MRS_REQUIRE(ctx && d_points && h_offsets, "null pointer");
    MRS_REQUIRE(batch > 0, "batch must be positive");
    MRS_REQUIRE(k >= 2 && k <= 32, "k must be in [2, 32]");
    MRS_REQUIRE(d_knn || d_eigens || d_features || d_feat_planes, "no output requested");
    // the Morton-ordered cloud container of the GICP front end, kept per context and batch size between calls (see mrs_ctx::pointfeat_cache)
    mrs_gicp_batch* h = nullptr;
    bool cached = false;
    int st = MRS_OK;
    std::unique_lock<std::mutex> lk(ctx->pointfeat_mu, std::try_to_lock);
    if (lk.owns_lock()) {
        auto it = ctx->pointfeat_cache.find(batch);
        if (it != ctx->pointfeat_cache.end()) { h = static_cast<mrs_gicp_batch*>(it->second.get()); cached = true; }
    }
    if (!h) {
        st = mrs_gicp_batch_create(ctx, batch, &h);
        if (st != MRS_OK) return st;
        h->no_cov = true;          // no covariance buffer (48 B per point) for the feature front end
        if (lk.owns_lock() && ctx->pointfeat_cache.size() < 4) {
            ctx->pointfeat_cache[batch] = std::shared_ptr<void>(h, [](void* p) { (void)mrs_gicp_batch_destroy(static_cast<mrs_gicp_batch*>(p)); });
            cached = true;
        }
    }
    st = mrs_gicp_batch_set_clouds(h, 0, d_points, stride_floats, h_offsets, stream);
    if (st == MRS_OK) {
        hipStream_t s = (hipStream_t)stream;
        const GicpCloud& S = h->side[0];
        const int64_t longest = S.longest;
        // the selection (k_knn_cov<30>: 5 waves per SIMD, no fp64 state) hands the neighbour indices to k_feat_from_knn through a scratch buffer
        // in blocks of 64 points, slot-major (knn_at); clouds go through in chunks that keep the buffer below 1 GiB (64 scans of 120 k points
        // at k = 30 are 0.92 GB: one chunk)
        const int64_t per_cloud = (int64_t)(knn_ints(longest, 1, k) * sizeof(int));
        const char* const lim_s = mrs::dev_env("MRS_FEAT_CHUNK_MB");        // development aid (the tests): a small limit forces several chunks
        const int64_t limit = lim_s ? std::max<int64_t>(1, atoll(lim_s)) << 20 : (1ll << 30);
        const int chunk = (int)std::max<int64_t>(1, std::min<int64_t>(batch, limit / per_cloud));
        mrs::Scratch knn;
        st = knn.alloc((size_t)chunk * per_cloud, s);
        if (st == MRS_OK) st = knn_dev_switches(s);
        for (int c0 = 0; st == MRS_OK && c0 < batch; c0 += chunk) {
            const int nc = std::min(chunk, batch - c0);
            int* const kn = knn.as<int>() - (size_t)h_offsets[c0] * k;       // the kernels index by global point number (see compute_covariances)
            launch_knn_cov(h, 0, c0, nc, k, kn, s);
            hipLaunchKernelGGL(k_feat_from_knn, dim3((unsigned)((longest + 255) / 256), nc), dim3(256), 0, s, (const float4*)S.pts.get(),
                               (const int64_t*)S.d_offs.get() + c0, k, (const int*)kn, d_knn, d_eigens, d_features, d_feat_planes);
        }
        if (st == MRS_OK && (hipGetLastError() != hipSuccess || hipStreamSynchronize(s) != hipSuccess)) {
            mrs::set_error("point-feature kernels failed: %s", hipGetErrorString(hipGetLastError()));
            st = MRS_ERR_HIP;
        }
    }
    if (!cached) mrs_gicp_batch_destroy(h);
    return st;
}

double mrs_gicp_batch_last_nn_passes(const mrs_gicp_batch* h) { return h ? h->last_nn_passes : 0.0; }

}  // extern "C"
