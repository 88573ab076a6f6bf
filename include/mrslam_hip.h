/*
 * mrslam_hip.h -- C ABI of libmrslam_hip.so: the MI355X (gfx950) implementation of
 * MR_SLAM's loop-closure hot path (BEV rasterisers, Radon sinogram, FFT correlation,
 * GICP refinement).  Plain pointers and sizes only; no torch / Eigen / PCL types.
 *
 * Conventions
 *   - every entry point returns an int status (MRS_OK == 0); nothing here ever calls
 *     exit() (the reference's torch-radon does: include/utils.h:38-48) or throws;
 *   - `d_` arguments are DEVICE pointers, `h_` arguments are HOST pointers;
 *   - `stream` is a hipStream_t passed as void* (NULL = the legacy default stream);
 *     device-pointer entry points only ENQUEUE work on it, they do not synchronise;
 *   - a context (mrs_ctx) is bound to one device; entry points are re-entrant and may
 *     be called concurrently from several host threads (the reference modules are
 *     entered concurrently by rospy callback threads: main_RING.py:241-390);
 *   - batches are "ragged": scan b owns points [offsets[b], offsets[b+1]) of the packed
 *     cloud; each scan keeps the reference's own SoA layout [x0..xn-1,y0..,z0..]
 *     starting at float 3*offsets[b] (util.py:177 `pc.transpose().flatten()`).
 *
 * Each function names the reference interface it replaces (file:line under
 * /root/reference).  INTEGRATION.md shows the reference-side bindings.
 */
#ifndef MRSLAM_HIP_H
#define MRSLAM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MRS_ABI_VERSION 1

enum mrs_status {
    MRS_OK = 0,
    MRS_ERR_ARG = 1,         /* bad argument (null pointer, non-positive size ...)      */
    MRS_ERR_HIP = 2,         /* a HIP runtime call failed; see mrs_last_error()          */
    MRS_ERR_UNSUPPORTED = 3, /* configuration outside what this build implements         */
    MRS_ERR_NO_DEVICE = 4,   /* no gfx950-class device visible                           */
    MRS_ERR_NOT_CONVERGED = 5
};

typedef struct mrs_ctx mrs_ctx;
typedef void* mrs_stream;

int mrs_abi_version(void);
const char* mrs_status_str(int status);
/* thread-local text of the last failure in the calling thread ("" if none) */
const char* mrs_last_error(void);

/* Bind a context to HIP device `device`.  Fails with MRS_ERR_NO_DEVICE when no GPU is
 * visible: there is NO CPU fallback anywhere behind this ABI. */
int mrs_ctx_create(int device, mrs_ctx** out_ctx);
int mrs_ctx_destroy(mrs_ctx* ctx);
int mrs_ctx_device(const mrs_ctx* ctx);

/* ------------------------------------------------------------------------------------
 * BEV rasterisers
 * ---------------------------------------------------------------------------------- */

/* Grid description shared by the three rasterisers.  Field meaning follows the reference
 * constructors: GPUTransformer(point, size, max_length, max_height, num_ring|num_x,
 * num_sector|num_y, num_height, enough_large|featsize)
 *   polar : disco_ros/tools/multi-layer-polar-cpu/cython/gputransform.pyx:19-30
 *   cart  : generate_bev_cython_binary/wrapper.pyx:18-29
 *   feat  : generate_bev_pointfeat_cython/wrapper.pyx:22-33 */
typedef struct mrs_bev_cfg {
    int32_t max_length;   /* half extent in x/y (cart) or max range (polar); reference int  */
    int32_t max_height;   /* half extent in z                                               */
    int32_t n0;           /* polar: num_ring    cart/feat: num_x                            */
    int32_t n1;           /* polar: num_sector  cart/feat: num_y                            */
    int32_t num_height;   /* height layers                                                  */
    int32_t enough_large; /* polar/cart: points kept per cell (cart ignores it, like the
                             reference); feat: featsize F                                   */
} mrs_bev_cfg;

/* output layouts */
enum mrs_bev_out {
    /* the reference `retreive()` array, bit for bit:
     *   polar/cart: float[3 * n0*n1*num_height * enough_large]  (x, y, value) triplets
     *   feat      : float[n0*n1*num_height * F]                 F interleaved channels  */
    MRS_BEV_OUT_REFERENCE = 0,
    /* only what the callers consume (util.py:186-187, disco_ros/main.py:121-123):
     *   polar/cart: float[n0*n1*num_height]   channel 2 (occupancy / max z), slab 0
     *   feat      : float[(F-3) * n0*n1*num_height] planar, channels 3..F-1 (util.py:231-240) */
    MRS_BEV_OUT_COMPACT = 1
};

/* Value written for a point the reference would mishandle (NaN, int overflow). */
#define MRS_BEV_DROPPED INT32_MIN

/* A1 -- per-point ring / sector / height of ONE scan.
 * Replaces GPUTransformer::transform() -> point2gridmap,
 * multi-layer-polar-cpu/cython/src/kernel.cpp:40-77 (GPU twin ...-gpu/.../kernel.cu:41-80).
 * Bit-exact with the CPU reference on every point it handles without UB. */
int mrs_bev_polar_indices(mrs_ctx* ctx, const float* d_xyz_soa, int32_t n, const mrs_bev_cfg* cfg,
                          int32_t* d_ring, int32_t* d_sector, int32_t* d_height, mrs_stream stream);

/* A3 -- per-point x / y / height cell of ONE scan.
 * Replaces point2gridmap, generate_bev_cython_binary/src/kernel.cu:14-61. */
int mrs_bev_cart_indices(mrs_ctx* ctx, const float* d_xyz_soa, int32_t n, const mrs_bev_cfg* cfg,
                         int32_t* d_ix, int32_t* d_iy, int32_t* d_ih, mrs_stream stream);

/* A1+A2 fused, batched: polar multi-layer occupancy BEV of `batch` scans.
 * Replaces transform()+retreive(), multi-layer-polar-cpu/cython/src/manager.cpp:36-58.
 * d_offsets: int64[batch+1] (device).  d_out: batch * (layout size) floats; the kernel
 * writes every element (no pre-zeroing needed). */
int mrs_bev_polar_batch(mrs_ctx* ctx, const float* d_xyz, const int64_t* d_offsets, int32_t batch,
                        const mrs_bev_cfg* cfg, int32_t out_layout, float* d_out, mrs_stream stream);

/* A3+A4 fused, batched: Cartesian max-z BEV.
 * Replaces transform()+retreive(), generate_bev_cython_binary/src/manager.cu:45-91. */
int mrs_bev_cart_batch(mrs_ctx* ctx, const float* d_xyz, const int64_t* d_offsets, int32_t batch,
                       const mrs_bev_cfg* cfg, int32_t out_layout, float* d_out, mrs_stream stream);

/* A5, batched: per-cell per-channel maximum of F channel-major planes [F*n] per scan
 * (planes 0..2 are x,y,z); scan b starts at float F*offsets[b].
 * Replaces point2gridmap + retreive, generate_bev_pointfeat_cython/src/kernel.cu:106-164,
 * src/manager.cu:54-63.  Deterministic true maximum (the reference races). */
int mrs_bev_feat_batch(mrs_ctx* ctx, const float* d_pts, const int64_t* d_offsets, int32_t batch,
                       const mrs_bev_cfg* cfg, int32_t out_layout, float* d_out, mrs_stream stream);

/* Host-buffer forms with the reference's calling convention (caller-owned numpy buffers in,
 * zero-initialised float array out; gputransform.pyx:32-39, wrapper.pyx:31-39).  They copy
 * H2D, run the kernels above, copy D2H and synchronise.  Layout MRS_BEV_OUT_REFERENCE. */
int mrs_bev_polar_host(mrs_ctx* ctx, const float* h_xyz_soa, int32_t n, const mrs_bev_cfg* cfg, float* h_out);
int mrs_bev_cart_host(mrs_ctx* ctx, const float* h_xyz_soa, int32_t n, const mrs_bev_cfg* cfg, float* h_out);
int mrs_bev_feat_host(mrs_ctx* ctx, const float* h_pts_cm, int32_t n, const mrs_bev_cfg* cfg, float* h_out);

/* ------------------------------------------------------------------------------------
 * Radon sinogram (rows R1, R2)
 * ---------------------------------------------------------------------------------- */
typedef struct mrs_radon_plan mrs_radon_plan;

/* Replaces the constructor torch_radon.ParallelBeam(det_count, angles, det_spacing, volume=None)
 * (torch_radon/radon.py:139-167) for a fixed image size; volume centre 0, voxel size 1
 * (torch_radon/volumes.py:13-21), which is how every MR_SLAM call site uses it
 * (RING_ros/util.py:192-195,241-245).  h_angles: n_angles floats on the HOST (radians);
 * their cos/sin are evaluated once, in double, when the plan is built, together with the per-ray
 * geometry table.  Images whose zero-bordered copy fits the LDS (up to ~190 x 190) take the LDS-resident
 * kernel; larger ones run the same sample loop against a padded copy in global memory. */
int mrs_radon_plan_create(mrs_ctx* ctx, const float* h_angles, int32_t n_angles, int32_t det_count,
                          float det_spacing, int32_t height, int32_t width, mrs_radon_plan** out_plan);
int mrs_radon_plan_destroy(mrs_radon_plan* plan);

/* R1 (+R2a): d_img float[batch][H][W] -> d_sino float[batch][n_angles][det_count].
 * Replaces torch_radon_cuda.forward / radon_forward_cuda<float>, parallel beam
 * (torch-radon/src/pytorch.cpp:42-81, src/forward.cu:12-178).
 * d_sino_norm (optional, may be NULL; d_sino may be NULL when it is given) receives
 * (S - mean(S)) / std(S) per image with the unbiased std: the fn.normalize(...) step of
 * generate_RING (RING_ros/util.py:197), fused so the sinogram never makes a second trip. */
int mrs_radon_forward(mrs_radon_plan* plan, const float* d_img, int32_t batch, float* d_sino,
                      float* d_sino_norm, mrs_stream stream);

/* Sinograms whose fused normalisation met a zero or non-finite standard deviation since the plan was created (or since
 * the last call with reset != 0): a blank / constant image.  The reference raises there (torchvision fn.normalize:
 * ValueError, RING_ros/util.py:197); the kernels write an all-zero normalised sinogram (finite, correlates with nothing:
 * dist = 1) and count the event so that the host mirror can raise the same error.  Synchronises the device. */
int mrs_radon_plan_degenerate_count(mrs_radon_plan* plan, int32_t reset, int32_t* out_count);

/* Read-only: the ray each lane slot of the two-image kernels marches (slot s = k * 1024 + lane, -1 = idle; every ray once), as the plan
 * dealt them when it was built.  Host memory, no GPU work.  *n_slots = number of slots (0: the plan has no slot tables); at most
 * `capacity` entries are written to h_slot_rays. */
int mrs_radon_plan_slot_rays(mrs_radon_plan* plan, int32_t* h_slot_rays, int32_t capacity, int32_t* n_slots);

/* A3/A4 + R1 + R2a in one launch: the front half of generate_RING (RING_ros/util.py:174-197: voxelocc.GPUTransformer
 * transform() + retreive(), channel 2 -> ParallelBeam.forward -> fn.normalize) for a batch of scans.  One persistent workgroup
 * per compute unit rasterises two scans straight into the Radon kernel's LDS tile and marches the rays; the BEV image goes to
 * HBM only when d_bev is given.  Results are bit-identical to mrs_bev_cart_batch(MRS_BEV_OUT_COMPACT) followed by
 * mrs_radon_forward.  d_xyz / d_offsets as for mrs_bev_cart_batch; cfg: num_height == 1 and n0 x n1 == the plan's image
 * (H x W).  Each of d_bev float[batch][n0][n1], d_sino, d_sino_norm float[batch][n_angles][det_count] may be NULL (not
 * all).  MRS_ERR_UNSUPPORTED when the configuration needs the two-call path (num_height > 1, a tile that does not fit the
 * LDS twice, more than 16 384 rays). */
int mrs_ring_descriptors_batch(mrs_radon_plan* plan, const float* d_xyz, const int64_t* d_offsets, int32_t batch,
                               const mrs_bev_cfg* cfg, float* d_bev, float* d_sino, float* d_sino_norm, mrs_stream stream);

/* Tuning knobs of mrs_ring_descriptors_batch (results do not depend on them). */
enum mrs_radon_option {
    MRS_RADON_OPT_FUSED_STAGGER_US = 1, /* odd workgroups start this many microseconds late (default 70, 0 = off) */
    MRS_RADON_OPT_FUSED_PREFETCH = 2,   /* 16-byte load triplets in flight per lane while rasterising: 2, 4 or 6 */
    MRS_RADON_OPT_FUSED_GRID = 3,       /* persistent workgroups (0 = one per compute unit)                      */
    MRS_RADON_OPT_FUSED_SKIP = 5,       /* measurement aid, outputs meaningless: 1 = leave out the rasteriser, 2 = the ray march (phase floors) */
    MRS_RADON_OPT_FUSED_VARIANT = 4     /* 2 (default): rays dealt to lanes by length (slot tables), raw sums in registers, the sinogram written
                                           once; 1: the same with the raw sums parked in the output buffer; 0: (angle, detector) order */
};
int mrs_radon_plan_set_option(mrs_radon_plan* plan, int32_t option, int32_t value);
/* The value an option has now (what the plan was created with, or the last value set).  Defaults: stagger 70, prefetch 2, grid 0,
 * variant 2, skip 0. */
int mrs_radon_plan_get_option(mrs_radon_plan* plan, int32_t option, int32_t* value);

/* (x - mean) / std over n_groups consecutive groups of group_len floats (unbiased std):
 * torchvision fn.normalize(t, mean=t.mean(), std=t.std()) as RING_ros/util.py:197,339-340,429-430
 * use it (RING++ normalises a whole [C,H,W] descriptor with ONE mean/std -> group_len=C*H*W).
 * In-place allowed (d_out == d_in).  A constant group (std == 0; torchvision raises) is written as zeros. */
int mrs_normalize_groups(mrs_ctx* ctx, const float* d_in, float* d_out, int32_t n_groups,
                         int32_t group_len, mrs_stream stream);

/* ------------------------------------------------------------------------------------
 * RING / RING++ descriptors and rotation correlation (rows R2, C1, C2, C3)
 * ---------------------------------------------------------------------------------- */

/* R2: TIRING = ortho FFT over the ANGLE axis of (already normalised) sinograms.
 * Replaces torch.fft.fft2(x, dim=-2, norm="ortho") at RING_ros/util.py:198.
 * d_x float[n_img][n_angles][det] -> d_out interleaved complex64 [n_img][n_angles][det]. */
int mrs_fft_angle_r2c(mrs_ctx* ctx, const float* d_x, int32_t n_img, int32_t n_angles, int32_t det,
                      float* d_out, mrs_stream stream);

/* R2 (RING++): |ortho FFT over the DETECTOR axis|.  Replaces forward_row_fft,
 * RING_ros/util.py:295-300 (first return value).  float[n_img][n_angles][det] both ways. */
int mrs_fft_row_magnitude(mrs_ctx* ctx, const float* d_x, int32_t n_img, int32_t n_angles, int32_t det,
                          float* d_out, mrs_stream stream);

/* C1/C2 database sweep: every query against every database entry.
 * Replaces the Python loop `for idx in range(len(pc_candidates)): fast_corr(...)`
 * (RING_ros/main_RING.py:133-140 -> util.py:362-374; RING++: util.py:337-358 after its two
 * fn.normalize calls, i.e. feed mrs_normalize_groups output).
 * d_query float[n_query][channels][n_angles][det], d_db float[n_db][...]: NORMALISED REAL
 * sinograms (RING) / normalised row-FFT magnitudes (RING++), the inverse transform of the
 * spectra the reference stores.  d_dist float[n_query][n_db] = 1 - max / (0.15*C*A*D),
 * d_angle int32[n_query][n_db] = A/2 - argmax(fftshift(corr)); d_corr (optional, may be NULL)
 * float[n_query][n_db][n_angles] = the shifted correlation vector. */
int mrs_ring_corr_sweep(mrs_ctx* ctx, const float* d_query, int32_t n_query, const float* d_db, int32_t n_db,
                        int32_t channels, int32_t n_angles, int32_t det, float* d_dist, int32_t* d_angle,
                        float* d_corr, mrs_stream stream);

/* Pairwise form of the sweep: pair i = (d_a[i], d_b[i]); outputs have n_pairs entries
 * (d_corr: float[n_pairs][n_angles]). */
int mrs_ring_corr_pairs(mrs_ctx* ctx, const float* d_a, const float* d_b, int32_t n_pairs, int32_t channels,
                        int32_t n_angles, int32_t det, float* d_dist, int32_t* d_angle, float* d_corr,
                        mrs_stream stream);

/* C1 literal: fast_corr(a, b) on complex spectra, pair by pair (RING_ros/util.py:362-374).
 * d_a, d_b interleaved complex64 [n_pairs][channels][n_angles][det]; outputs per pair.
 * dist = 1 - max / (0.15 * n_angles * det): like the reference, NO channel factor (util.py:369). */
int mrs_ring_corr_spectra(mrs_ctx* ctx, const float* d_a, const float* d_b, int32_t n_pairs, int32_t channels,
                          int32_t n_angles, int32_t det, float* d_dist, int32_t* d_angle, float* d_corr,
                          mrs_stream stream);

/* C3: solve_translation(query, positive, rot_angle) (RING_ros/util.py:388-423,488-506).
 * d_query/d_positive float[n_pairs][channels][height][width] (RING sinograms, `positive`
 * already row-rolled by the caller as main_RING.py:172-178 does); d_angles float[height]
 * (linspace(0, 2*pi, height)); d_rot float[n_pairs].  d_xy_err float[n_pairs][3] = x, y,
 * residual norm; d_shifts (optional) float[n_pairs][height] = the per-row integer shifts. */
int mrs_ring_solve_translation(mrs_ctx* ctx, const float* d_query, const float* d_positive, int32_t n_pairs,
                               int32_t channels, int32_t height, int32_t width, const float* d_angles,
                               const float* d_rot, float* d_xy_err, float* d_shifts, mrs_stream stream);

/* ------------------------------------------------------------------------------------
 * GICP refinement (rows G2-G6), batched over independent submap pairs
 * ---------------------------------------------------------------------------------- */
typedef struct mrs_gicp_batch mrs_gicp_batch;

/* Parameters with fast_gicp's names and defaults (upstream include/fast_gicp/gicp/
 * {fast_gicp.hpp,lsq_registration.hpp}).  Setters they replace:
 * setCorrespondenceRandomness, setMaxCorrespondenceDistance, setMaximumIterations,
 * setRotationEpsilon, setTransformationEpsilon (global_manager.cpp:2437-2442,
 * main_RING.py:93-94).  setNumThreads has no meaning on the GPU and is accepted and ignored
 * by the host-side mirrors. */
typedef struct mrs_gicp_params {
    int32_t k_correspondences;          /* neighbours for the covariances (20; Mapping: 15)   */
    int32_t max_iterations;             /* outer LM iterations (64; Mapping: icp_iters = 50)  */
    int32_t lm_max_iterations;          /* inner LM trials per iteration (10)                  */
    int32_t force_iterations;           /* > 0: run exactly this many outer iterations with the
                                           convergence test disabled (benchmark timing only)   */
    double max_correspondence_distance; /* DBL_MAX = unbounded (RING: 5.0, Mapping: 100)       */
    double rotation_epsilon;            /* 2e-3                                                */
    double transformation_epsilon;      /* 5e-4 (Mapping: 1e-3)                                */
    double lm_init_lambda_factor;       /* 1e-9                                                */
    double voxel_resolution;            /* 0 = GICP (FastGICP); > 0 = voxelised GICP, row G7
                                           (FastVGICP / FastVGICPCuda::setResolution; Mapping: 0.5,
                                           global_manager.cpp:2450)                            */
    int32_t voxel_neighbors;            /* 1 / 7 / 27 = DIRECT1 / DIRECT7 / DIRECT27
                                           (setNeighborSearchMethod, global_manager.cpp:2452)  */
    int32_t reserved;
    double convergence_factor;          /* LsqRegistration::is_converged: max(f |R - I| / rotation_epsilon,
                                           f |t| / transformation_epsilon) < 1 with upstream's f = 10
                                           (0 selects 10)                                      */
} mrs_gicp_params;

void mrs_gicp_default_params(mrs_gicp_params* p);

/* One handle aligns n_pairs independent (source, target) pairs together.
 * Replaces n_pairs instances of fast_gicp::FastGICP<PointXYZI,PointXYZI> / pygicp.FastGICP
 * (factory at global_manager.cpp:2416-2461; pygicp use at main_RING.py:81-104). */
int mrs_gicp_batch_create(mrs_ctx* ctx, int32_t n_pairs, mrs_gicp_batch** out);
int mrs_gicp_batch_destroy(mrs_gicp_batch* h);
int mrs_gicp_batch_set_params(mrs_gicp_batch* h, const mrs_gicp_params* p);

/* setInputSource (which = 0) / setInputTarget (which = 1) for every pair at once.
 * d_points: packed DEVICE array of points, x y z in the first three of every `stride_floats`
 * floats (3 = pygicp's Nx3, 4 = pcl::PointXYZ, 8 = pcl::PointXYZI); h_offsets: HOST
 * int64[n_pairs+1] point offsets of the pairs.  Copies into the library's float4 layout. */
int mrs_gicp_batch_set_clouds(mrs_gicp_batch* h, int32_t which, const float* d_points, int32_t stride_floats,
                              const int64_t* h_offsets, mrs_stream stream);

/* The same with the points in HOST memory (the form a pcl::PointCloud / numpy caller has: setInputSource / setInputTarget of
 * the C++ adapter, pygicp.FastGICP.set_input_*): staged through the library's scratch cache, synchronous. */
int mrs_gicp_batch_set_clouds_host(mrs_gicp_batch* h, int32_t which, const float* h_points, int32_t stride_floats,
                                   const int64_t* h_offsets);
/* Submap store: a second batch used as a container of UNIQUE clouds (mrs_gicp_batch_create(ctx, n_clouds), set_clouds(which = 1, ...),
 * compute_covariances(1)).  Pair i's cloud of side `which` := cloud h_ids[i] of side `store_which` of `store`: the sorted points, the
 * covariances, the boxes and the octree-cell hierarchy are copied on the device, nothing is rebuilt -- a submap that takes part in several
 * pairs (a new scan checked against several stored candidates: main_RING.py:81-104, global_manager.cpp:2016-2021, where fast_gicp itself
 * recomputes both clouds' covariances for every pair) is sorted and gets its covariances once.  Same results as set_clouds with the same
 * points (tests/test_gicp_gpu.py).  Both batches must use the same k_correspondences. */
int mrs_gicp_batch_set_clouds_from(mrs_gicp_batch* h, int32_t which, mrs_gicp_batch* store, int32_t store_which, const int32_t* h_ids,
                                   mrs_stream stream);

/* G2: FastGICP::calculate_covariances (brute-force kNN, PLANE regularisation).  Called lazily
 * by align; exposed so that it can be timed / cached per submap.  d_knn_out (optional, may be
 * NULL): int32[total_points][k] neighbour indices (cloud-local, ascending distance). */
int mrs_gicp_batch_compute_covariances(mrs_gicp_batch* h, int32_t which, int32_t* d_knn_out, mrs_stream stream);
/* h_cov6: double[total_points][6] = xx xy xz yy yz zz of the regularised 3x3 block */
int mrs_gicp_batch_get_covariances(mrs_gicp_batch* h, int32_t which, double* h_cov6);
/* Read-out of the voxel map that the voxelised variant (voxel_resolution > 0) registers against: upstream's GaussianVoxelMap of the targets
 * (fast_gicp's CUDA voxel map: voxel coordinate floor(x / resolution - 0.5) in float arithmetic, mean of the points, mean of
 * their regularised covariances).  Builds the map if it is not current (and the covariances it needs, like linearize does); needs both
 * sides' clouds.  h_n_voxels: int32[1], the number of voxels of all pairs together.  The arrays (each optional; all NULL: the count only)
 * hold one entry per voxel in ascending (pair, x, y, z): h_pair int32[n], h_coord int32[n][3] signed voxel coordinate, h_mean float[n][3],
 * h_count int32[n] points in the voxel, h_cov6 double[n][6] = xx xy xz yy yz zz.  Synchronises `stream`. */
int mrs_gicp_batch_get_voxel_map(mrs_gicp_batch* h, int32_t* h_n_voxels, int32_t* h_pair, int32_t* h_coord, float* h_mean, int32_t* h_count,
                                 double* h_cov6, mrs_stream stream);

/* align(output, guess): h_guess double[n_pairs][16] row-major 4x4 (NULL = identity; narrowed to
 * float like the reference's Eigen::Matrix4f guess), h_final double[n_pairs][16] =
 * getFinalTransformation() (float precision), h_converged = hasConverged(), h_iterations =
 * outer iterations used, h_hessian double[n_pairs][36] (each optional).  Synchronises `stream`. */
int mrs_gicp_batch_align(mrs_gicp_batch* h, const double* h_guess, double* h_final, int32_t* h_converged,
                         int32_t* h_iterations, double* h_hessian, mrs_stream stream);

/* G3+G4 once at given poses (kernel-level parity hook): H double[n_pairs][36], b [n_pairs][6],
 * err [n_pairs]; d_corr (optional) int32[total source points] correspondences or -1. */
int mrs_gicp_batch_linearize(mrs_gicp_batch* h, const double* h_poses, double* h_H, double* h_b, double* h_err,
                             int32_t* d_corr, mrs_stream stream);

/* G6: pcl::Registration::getFitnessScore(max_range) at the given poses
 * (global_manager.cpp:2058-2071, main_RING.py:100). */
int mrs_gicp_batch_fitness(mrs_gicp_batch* h, const double* h_poses, double max_range, double* h_scores,
                           mrs_stream stream);

/* number of brute-force NN passes the last align() issued (for iterations/s accounting) */
double mrs_gicp_batch_last_nn_passes(const mrs_gicp_batch* h);

/* Measurement hook of bench.py (no reference counterpart): every kernel of one outer iteration launched alone between HIP events on
 * `stream`, `reps` times, at the given poses (double[n_pairs][16]).  out_ms float[8]: 0 k_linearize (28 sums), 1 k_linearize (error only:
 * an LM trial), 2 round-3 search of every point (warm), 3 k_nn_certify at an unchanged pose, 4 round-4 search of every point (warm),
 * 5 k-NN selection of the sources, 6 k_cov_from_knn of the sources, 7 certify + work-list search after a 1 mm step.  out_counts int64[3]:
 * source points, correspondences at the poses, queries on the work lists of [7].  The batch's search settings are restored on every way out
 * (errors included); its correspondences, warm-start seeds and certificates are OVERWRITTEN (they are those of the profiled poses afterwards). */
int mrs_gicp_batch_profile(mrs_gicp_batch* h, const double* h_poses, int32_t reps, float* out_ms, int64_t* out_counts, mrs_stream stream);

/* Which exact nearest-neighbour searches the batch uses for G2 / G3 (no reference counterpart: upstream fast_gicp searches a
 * kd-tree; every setting returns the exact neighbours, ties aside -- identical transforms, tests/test_gicp_gpu.py):
 *   1 (default) align(): the first pass and every pair whose last step moved it by more than 2 cm are searched by the round-3 kernel
 *               (1024-point tiles / 16-point minis, candidates shared by a wave: best for broad searches); the other pairs first
 *               CERTIFY the neighbours of the previous pass (triangle inequality: a query that moved by delta keeps its neighbour
 *               if that neighbour's new distance is below [the old lower bound of every other point's distance] - delta) and search
 *               only what could not be certified, on octree-cell leaves with per-query culling (csrc/nn_core.hpp).  k-NN for the
 *               covariances: round-3 kernel;
 *   2           like 1 without certificates (every pass searches every point);
 *   3           round-4 kernels everywhere (first pass and k-NN too; slower on lidar scans, kept for comparison);
 *   0           the round-3 kernels everywhere, no certificates (A/B measurements, cross-check in the tests).
 * Invalidates cached covariances when the k-NN kernel changes. */
int mrs_gicp_batch_set_search(mrs_gicp_batch* h, int32_t core);
/* share of (source point, nearest-neighbour pass) of the last align() that needed a search (1.0 without certificates) */
double mrs_gicp_batch_last_searched_fraction(const mrs_gicp_batch* h);

/* Point-to-point ICP (row G9): pcl::IterativeClosestPoint<PointXYZI, PointXYZI> as GlobalManager::performLoopClosure
 * (global_manager.cpp:890-906) and the PCL_ICP branch of select_registration_method (:2427-2434) drive it, batched over the pairs of a
 * mrs_gicp_batch: same handle, same clouds (set_clouds / set_clouds_host / set_clouds_from), same exact searches; no covariances are
 * computed.  PCL is not part of the reference tree: DESIGN.md section 4.13 is the definition (TransformationEstimationSVD + DefaultConvergenceCriteria
 * with max_iterations_similar_transforms = 0; the pose accumulates in fp64), parity with PCL is unpinned.  Names and defaults are PCL's. */
typedef struct mrs_icp_params {
    int32_t max_iterations;             /* setMaximumIterations (10; Mapping: icp_iters)                        */
    int32_t force_iterations;           /* > 0: exactly this many iterations, stopping rules disabled (timing,
                                           fixed-length parity); converged = 0, state NOT_CONVERGED             */
    double max_correspondence_distance; /* setMaxCorrespondenceDistance (sqrt(DBL_MAX); Mapping: 2.0 and 100)   */
    double transformation_epsilon;      /* setTransformationEpsilon (0; Mapping: 1e-3): bound on the SQUARED
                                           translation of an increment, and 1 - it on the cosine of its angle  */
    double rotation_epsilon;            /* setTransformationRotationEpsilon (0 = derive from the above)         */
    double euclidean_fitness_epsilon;   /* setEuclideanFitnessEpsilon (-DBL_MAX = never; Mapping: 1e-3):
                                           relative change of the mean squared correspondence distance         */
} mrs_icp_params;

void mrs_icp_default_params(mrs_icp_params* p);

/* align(output, guess) of every pair.  h_guess / h_final as in mrs_gicp_batch_align; h_converged, h_iterations and h_state
 * (int32[n_pairs], each optional): hasConverged(), iterations run, and the ConvergenceState that ended the pair: 0 NOT_CONVERGED,
 * 1 ITERATIONS, 2 TRANSFORM, 3 ABS_MSE, 4 REL_MSE, 5 NO_CORRESPONDENCES (fewer than 3 correspondences: converged = 0, the pose stays).
 * getFitnessScore is mrs_gicp_batch_fitness.  Synchronises `stream`.  The handle's GICP parameters are not used: in particular a
 * voxel_resolution > 0 is ignored (ICP always searches the target points; the voxelised mode has no ICP counterpart).  An alignment leaves nothing behind that a later
 * mrs_gicp_batch_align or mrs_gicp_batch_align_icp on the same handle depends on. */
int mrs_gicp_batch_align_icp(mrs_gicp_batch* h, const mrs_icp_params* p, const double* h_guess, double* h_final, int32_t* h_converged,
                             int32_t* h_iterations, int32_t* h_state, mrs_stream stream);

/* One iteration's correspondences, sums and rigid fit at given poses (kernel-level parity hook, the twin of mrs_gicp_batch_linearize):
 * h_sums double[n_pairs][17] = n, sum a (3), sum b (3), sum a b^T (9, row-major), sum |b - a|^2 with a = pose * source point and b its
 * nearest target point; h_delta double[n_pairs][16] the fitted increment (identity below 3 correspondences); d_corr (optional)
 * int32[total source points] correspondences or -1. */
int mrs_gicp_batch_icp_step(mrs_gicp_batch* h, const mrs_icp_params* p, const double* h_poses, double* h_sums, double* h_delta,
                            int32_t* d_corr, mrs_stream stream);

/* Measurement hook of tools/bench_icp.py (no reference counterpart): the three stages of one ICP iteration launched alone between HIP
 * events on `stream`, `reps` times each, at the given poses (double[n_pairs][16]).  out_ms float[3]: 0 the search of every source point
 * (the handle's search setting, warm), 1 k_icp_sums, 2 k_icp_update.  out_counts int64[2]: source points, correspondences at the poses.
 * The batch's correspondences and warm-start seeds are overwritten, and the repeated launches of k_icp_update keep composing the same
 * increment into the poses: the alignment state the call leaves behind is meaningless (the next align / align_icp starts over anyway). */
int mrs_gicp_batch_icp_profile(mrs_gicp_batch* h, const mrs_icp_params* p, const double* h_poses, int32_t reps, float* out_ms,
                               int64_t* out_counts, mrs_stream stream);

/* Point-to-plane ICP (row G12): pcl::NormalEstimation with setKSearch as GlobalManager::addNormal drives it (global_manager.cpp:2679-2693)
 * and pcl::IterativeClosestPointWithNormals (TransformationEstimationPointToPlaneLLS + DefaultConvergenceCriteria), the class that helper
 * feeds; batched over the pairs of a mrs_gicp_batch: same handle, same clouds, same exact searches and k-NN selection.  PCL is not part of
 * the reference tree: DESIGN.md section 4.16 is the definition, parity with PCL is unpinned.  Names and defaults are PCL's. */
typedef struct mrs_icp_plane_params {
    int32_t max_iterations;             /* the six fields of mrs_icp_params, same meaning and defaults               */
    int32_t force_iterations;
    double max_correspondence_distance;
    double transformation_epsilon;
    double rotation_epsilon;
    double euclidean_fitness_epsilon;
    int32_t normal_k;                   /* setKSearch of the target normals computed on demand (15: :2689); 3 .. 32   */
    double viewpoint[3];               /* setViewPoint of those normals (0, 0, 0)                                    */
} mrs_icp_plane_params;

void mrs_icp_plane_default_params(mrs_icp_plane_params* p);

/* Normals of every point of side `which` (0 sources, 1 targets) from its min(k, n) nearest neighbours, itself included: unit eigenvector of
 * the smallest eigenvalue of the neighbours' covariance (fp64), turned towards h_viewpoint (double[3]; NULL = origin), and the curvature
 * lambda0 / (lambda0 + lambda1 + lambda2); NaN where a cloud has fewer than 3 points.  Kept on the handle, one float4 per point, until the
 * side's clouds are set again; a call with the k and viewpoint of the normals at hand does nothing.  Asynchronous on `stream`. */
int mrs_gicp_batch_compute_normals(mrs_gicp_batch* h, int32_t which, int32_t k, const double* h_viewpoint, mrs_stream stream);
/* (nx, ny, nz, curvature) of every point in INPUT order: float[total points][4].  Refuses when the side holds no normals. */
int mrs_gicp_batch_get_normals(mrs_gicp_batch* h, int32_t which, float* h_normals4);
/* Normals the caller already has (pcl::PointXYZINormal's normal_x / normal_y / normal_z), in the order of the points given to set_clouds:
 * point i's normal at normals[i * stride_floats + 0 .. 2], stride_floats >= 3; with stride_floats >= 4 the fourth float is kept as the
 * curvature, else 0.  They stay until the side's clouds are set again or mrs_gicp_batch_compute_normals replaces them. */
int mrs_gicp_batch_set_normals(mrs_gicp_batch* h, int32_t which, const float* d_normals, int32_t stride_floats, mrs_stream stream);
int mrs_gicp_batch_set_normals_host(mrs_gicp_batch* h, int32_t which, const float* h_normals, int32_t stride_floats);

/* align(output, guess) of every pair; arguments and results as mrs_gicp_batch_align_icp, with one more state: 6 DEGENERATE (the 6 x 6
 * system of an iteration is rank-deficient, e.g. all target normals parallel: converged = 0, the pose stays).  Target normals: those the
 * handle holds (given or computed, whatever their k), else computed with p->normal_k and p->viewpoint.  Source normals are not used. */
int mrs_gicp_batch_align_icp_plane(mrs_gicp_batch* h, const mrs_icp_plane_params* p, const double* h_guess, double* h_final,
                                   int32_t* h_converged, int32_t* h_iterations, int32_t* h_state, mrs_stream stream);

/* One iteration at given poses (kernel-level parity hook, the twin of mrs_gicp_batch_icp_step): h_sums double[n_pairs][29] = n, the upper
 * triangle of sum a a^T (21, row-major), sum a r (6), sum |d - s|^2 with s = pose * source point, d its nearest target point, nrm that
 * point's normal, a = [s x nrm, nrm], r = nrm . (d - s); h_delta double[n_pairs][16] the fitted increment (identity below 3 correspondences
 * or when degenerate); h_state (optional) int32[n_pairs]: 5, 6, or what one iteration with max_iterations = 1 ends in; d_corr (optional)
 * int32[total source points] correspondences or -1. */
int mrs_gicp_batch_icp_plane_step(mrs_gicp_batch* h, const mrs_icp_plane_params* p, const double* h_poses, double* h_sums, double* h_delta,
                                  int32_t* h_state, int32_t* d_corr, mrs_stream stream);

/* Measurement hook of tools/bench_icp_plane.py (no reference counterpart), as mrs_gicp_batch_icp_profile.  out_ms float[4]: 0 the search
 * of every source point, 1 the normals of the targets (selection + k_normals_from_knn, p->normal_k), 2 k_icp_plane_sums,
 * 3 k_icp_plane_update.  out_counts int64[2]: source points, correspondences at the poses.  Leaves computed target normals behind. */
int mrs_gicp_batch_icp_plane_profile(mrs_gicp_batch* h, const mrs_icp_plane_params* p, const double* h_poses, int32_t reps, float* out_ms,
                                     int64_t* out_counts, mrs_stream stream);

/* PCL-style GICP (row G11): pcl::GeneralizedIterativeClosestPoint<PointXYZI, PointXYZI> as the PCL_GICP branch of
 * GlobalManager::select_registration_method drives it (global_manager.cpp:2419-2426), batched over the pairs of a mrs_gicp_batch: same handle,
 * same clouds, same exact searches, and the handle's own k-NN covariances (k_correspondences of mrs_gicp_params; computed lazily, cached, shared
 * with mrs_gicp_batch_align).  PCL's optimiser: per outer iteration the Mahalanobis matrices are frozen and a BFGS over (t, roll, pitch, yaw)
 * minimises the mean Mahalanobis error -- here on 74 sums over the correspondences, of which the error is an exact quadratic form, so the
 * points are read once per outer iteration.  PCL is not part of the reference tree: DESIGN.md section 4.15 is the definition (line search,
 * pivot and the six named deviations included), parity with PCL is unpinned.  Names and defaults are PCL's. */
typedef struct mrs_pclgicp_params {
    int32_t max_iterations;             /* setMaximumIterations (200; Mapping: icp_iters)                                     */
    int32_t max_inner_iterations;       /* setMaximumOptimizerIterations (20): iterations of the inner BFGS                    */
    int32_t force_iterations;           /* > 0: exactly this many outer iterations, stopping rule disabled (timing,
                                           fixed-length parity); converged = 0, state NOT_CONVERGED                            */
    double max_correspondence_distance; /* setMaxCorrespondenceDistance (5.0; Mapping: 100)                                    */
    double rotation_epsilon;            /* setRotationEpsilon (2e-3): scale of the rotation entries of the pose change         */
    double transformation_epsilon;      /* setTransformationEpsilon (5e-4; Mapping: 1e-3): scale of its translation entries    */
    double gradient_tolerance;          /* the inner BFGS stops below this gradient norm (1e-2)                                */
} mrs_pclgicp_params;

void mrs_pclgicp_default_params(mrs_pclgicp_params* p);

/* align(output, guess) of every pair.  h_guess / h_final as in mrs_gicp_batch_align; h_converged, h_iterations and h_state (int32[n_pairs],
 * each optional): hasConverged(), outer iterations run, and the state that ended the pair in mrs_gicp_batch_align_icp's numbering: 0
 * NOT_CONVERGED, 1 ITERATIONS, 2 TRANSFORM (the largest entry of |X_new - X|, rotation entries over rotation_epsilon and translation
 * entries over transformation_epsilon, fell below 1), 5 NO_CORRESPONDENCES (fewer than 4: converged = 0, the pose stays).  getFitnessScore is
 * mrs_gicp_batch_fitness.  Synchronises `stream`.  The handle's GICP parameters are not touched and, k_correspondences apart, not used: a
 * voxel_resolution > 0 is ignored.  An alignment leaves nothing behind that a later mrs_gicp_batch_align, _align_icp or _align_pcl on the
 * same handle depends on, apart from the valid covariance cache. */
int mrs_gicp_batch_align_pcl(mrs_gicp_batch* h, const mrs_pclgicp_params* p, const double* h_guess, double* h_final, int32_t* h_converged,
                             int32_t* h_iterations, int32_t* h_state, mrs_stream stream);

/* One outer iteration at given poses (kernel-level parity hook, the twin of mrs_gicp_batch_icp_step): h_sums double[n_pairs][74] in the
 * layout of DESIGN.md section 4.15 (n, sum M, sum M q, sum q'Mq, sum p_a M, sum p_a M q, sum p_a p_b M; zeros below 4 correspondences);
 * h_next double[n_pairs][16] the next pose (the given one below 4 correspondences); h_inner int32[n_pairs][2] the inner minimisation's
 * iterations and ending (0 GRADIENT, 1 LIMIT, 2 NO_PROGRESS); d_corr (optional) int32[total source points] correspondences or -1. */
int mrs_gicp_batch_pcl_step(mrs_gicp_batch* h, const mrs_pclgicp_params* p, const double* h_poses, double* h_sums, double* h_next,
                            int32_t* h_inner, int32_t* d_corr, mrs_stream stream);

/* Measurement hook of tools/bench_pclgicp.py (no reference counterpart): the three stages of one outer iteration launched alone between HIP
 * events on `stream`, `reps` times each, at the given poses (double[n_pairs][16]).  out_ms float[3]: 0 the search of every source point
 * (the handle's search setting, warm), 1 k_pclgicp_sums, 2 k_pclgicp_update (every launch from the given poses: a device-to-device copy of the states is part of the time).  out_counts int64[2]:
 * source points, correspondences at the poses.  The batch's correspondences and warm-start seeds are overwritten: the alignment state the
 * call leaves behind is meaningless (the next alignment starts over anyway). */
int mrs_gicp_batch_pcl_profile(mrs_gicp_batch* h, const mrs_pclgicp_params* p, const double* h_poses, int32_t reps, float* out_ms,
                               int64_t* out_counts, mrs_stream stream);

/* ------------------------------------------------------------------------------------
 * rocFFT-backed 2-D correlations: DiSCO (rows D1, D2) and RING++ BEV translation (row C4)
 * ---------------------------------------------------------------------------------- */

/* D1: DiSCO.forward with the UNet bypassed, as the ROS node runs it
 * (disco_ros/models/DiSCO.py:315-334, fftshift2d :280-294).
 * d_bev float[batch][num_height][num_ring][num_sector] (polar occupancy, mrs_bev_polar_batch COMPACT)
 * -> d_signature float[batch][4*col*col] (shifted magnitude, centre crop; col = 16 -> 1024-d) and
 *    d_spectrum interleaved complex64 [batch][num_ring][num_sector] (ortho fft2 of the height sum). */
int mrs_disco_descriptor(mrs_ctx* ctx, const float* d_bev, int32_t batch, int32_t num_height, int32_t num_ring,
                         int32_t num_sector, int32_t col, float* d_signature, float* d_spectrum, mrs_stream stream);

/* D2: phase_corr(a, b) (disco_ros/main.py:260-272) for n_pairs spectra pairs.
 * d_flat_argmax int32[n_pairs] = flat argmax of the shifted magnitude map (the reference then takes
 * `% num_sector`; the host mirror does that); d_corr (optional) float[n_pairs][num_ring][num_sector]. */
int mrs_disco_phase_corr(mrs_ctx* ctx, const float* d_a, const float* d_b, int32_t n_pairs, int32_t num_ring,
                         int32_t num_sector, int32_t* d_flat_argmax, float* d_corr, mrs_stream stream);

/* C4: solve_translation_bev(a, b) (RING_ros/util.py:427-450): d_a, d_b float[n_pairs][channels][H][W];
 * d_arg int32[n_pairs] = flat (row-major) index of the first maximum of the shifted correlation map,
 * d_max (optional) float[n_pairs] its value, d_corr (optional) float[n_pairs][H][W] the map. */
int mrs_bev_translation(mrs_ctx* ctx, const float* d_a, const float* d_b, int32_t n_pairs, int32_t channels,
                        int32_t height, int32_t width, int32_t* d_arg, float* d_max, float* d_corr, mrs_stream stream);

/* rotate_bev (RING_ros/util.py:67-70 -> torchvision rotate: nearest, about the centre, zero fill).
 * d_img float[n_images][H][W]; image i uses d_angle_deg[i / images_per_angle] (degrees, counter-clockwise). */
int mrs_rotate_nearest(mrs_ctx* ctx, const float* d_img, int32_t n_images, int32_t images_per_angle, int32_t height,
                       int32_t width, const float* d_angle_deg, float* d_out, mrs_stream stream);

/* ------------------------------------------------------------------------------------
 * RING++ point-feature front-end
 * ---------------------------------------------------------------------------------- */

/* Replaces voxelfeat.GPUFeatureExtractor(point, size, 13, k, neighbors_indices, eigens).get_features()
 * (generate_bev_pointfeat_cython/wrapper.pyx:43-59, src/kernel.cu:16-104): d_points float[n][3]
 * row-major, d_knn int32[n][k], d_eigens float[n][5] (3-D then 2-D eigenvalues, descending),
 * d_features float[n][13] = C,O,L,E,P,S,A,X,D,S2,L2,dZ,vZ.  k <= 32. */
int mrs_pointfeat_from_neighbors(mrs_ctx* ctx, const float* d_points, int32_t n, int32_t k, const int32_t* d_knn,
                                 const float* d_eigens, float* d_features, mrs_stream stream);
int mrs_pointfeat_from_neighbors_host(mrs_ctx* ctx, const float* h_points, int32_t n, int32_t k, const int32_t* h_knn,
                                      const float* h_eigens, float* h_features);

/* The whole front-end of generate_RINGplusplus on the GPU (RING_ros/util.py:163-170 build_neighbors_NN
 * [sklearn kd-tree kNN, k = 30], :123-160 covariation_eigenvalue [CPU eigvalsh], :218-228 features):
 * exact kNN (self included), covariance / (k-1), eigenvalues, 13 features, for `batch` clouds.
 * d_points: packed device points, xyz in the first 3 of every stride_floats floats; h_offsets HOST
 * int64[batch+1].  Outputs (each optional) in the caller's point order: d_knn int32[N][k],
 * d_eigens float[N][5], d_features float[N][13], d_feat_planes float[9*N]: per scan the channel-major
 * planes x,y,z,C,O,E,L2,dZ,vZ, i.e. exactly the input of mrs_bev_feat_batch with featsize 9.
 * A cloud with 2 <= n < k points gives, for every output, exactly what the same call gives with k = n (the covariance, the neighbour z
 * statistics and D_ are taken over its n points); its d_knn slots past n stay -1.  (The reference's sklearn call raises for n < k.)
 * Synchronises `stream`.  The Morton-ordered working copy of the clouds (~60 B per point) stays in the context between calls, per value of
 * `batch` (at most four) and grow-only, and is released by mrs_ctx_destroy; calls from several threads are safe (one of them uses the kept
 * buffers, the others temporary ones). */
int mrs_pointfeat_batch(mrs_ctx* ctx, const float* d_points, int32_t stride_floats, const int64_t* h_offsets,
                        int32_t batch, int32_t k, int32_t* d_knn, float* d_eigens, float* d_features,
                        float* d_feat_planes, mrs_stream stream);

/* ------------------------------------------------------------------------------------
 * FFT-domain RING correlation (rows R2, C1), specialised for num_ring = num_sector = 120
 * ---------------------------------------------------------------------------------- */

/* Half TIRING: the first n_angles/2+1 = 61 angle-frequency rows of torch.fft.fft2(x, dim=-2, norm="ortho")
 * (RING_ros/util.py:198) for real input; the remaining rows are their conjugates.
 * d_norm_sino float[n_img][120][120] -> d_half_spec interleaved complex64 [n_img][61][120].
 * This is the database format of the FFT-domain sweep (58 560 B per entry). */
int mrs_ring_half_spectrum(mrs_ctx* ctx, const float* d_norm_sino, int32_t n_img, int32_t n_angles, int32_t det,
                           float* d_half_spec, mrs_stream stream);

/* C1 sweep / pairs on half spectra: same outputs as mrs_ring_corr_sweep / mrs_ring_corr_pairs
 * (fast_corr, RING_ros/util.py:362-374; single channel). */
int mrs_ring_corr_fft_sweep(mrs_ctx* ctx, const float* d_query_spec, int32_t n_query, const float* d_db_spec,
                            int32_t n_db, float* d_dist, int32_t* d_angle, float* d_corr, mrs_stream stream);
int mrs_ring_corr_fft_pairs(mrs_ctx* ctx, const float* d_a_spec, const float* d_b_spec, int32_t n_pairs,
                            float* d_dist, int32_t* d_angle, float* d_corr, mrs_stream stream);
/* Several sweeps in one launch (the loop of main_RING.py:133-140 for a batch of new scans, each against ITS OWN slice of one descriptor
 * pool): query q is entry d_query_row[q] of d_spec ([entries][61][120] complex64) and sweeps the n_db entries that start at entry
 * d_db_first[q] (device int64 arrays, n_query <= 65535); d_dist / d_angle [n_query][n_db] as in mrs_ring_corr_fft_sweep.
 * PRECONDITION (not checked: the indices live on the device): every d_query_row[q] and every d_db_first[q] + n_db - 1 is an entry of d_spec. */
int mrs_ring_corr_fft_sweep_blocks(mrs_ctx* ctx, const float* d_spec, const int64_t* d_query_row, int32_t n_query, const int64_t* d_db_first,
                                   int32_t n_db, float* d_dist, int32_t* d_angle, mrs_stream stream);

/* DMA-tiled database entries: the 7 320 complex values of a half spectrum permuted so that every 1-KiB LDS-DMA wave-instruction of the
 * one-query sweep (gfx950 `global_load_lds_dwordx4`) reads ONE contiguous, 128-byte aligned block (csrc/ringfft.hip: kTiledEntryBytes):
 * 58 624 bytes per entry (58 560 + 64 of padding).  The array must be followed by at least 1 KiB of readable memory (row 30 is a half block).
 * mrs_ring_spec_to_tiled: d_half_spec [n][61][120] complex64 -> d_tiled [n][58 624 B].
 * mrs_ring_corr_fft_sweep_tiled: ONE query (row layout, [channels][61][120] complex64) against n_db entries of `channels` tiled planes each
 * (channels = 1: RING; 6: RING++); outputs as mrs_ring_corr_fft_sweep / _mc, bit-identical to them.  This is the sweep behind mrs_loopdb_query (the node's loop, main_RING.py:133-140). */
#define MRS_RING_TILED_ENTRY_BYTES 58624
int mrs_ring_spec_to_tiled(mrs_ctx* ctx, const float* d_half_spec, int32_t n, float* d_tiled, mrs_stream stream);
int mrs_ring_corr_fft_sweep_tiled(mrs_ctx* ctx, const float* d_query_spec, const float* d_db_tiled, int32_t n_db, int32_t channels, float* d_dist,
                                  int32_t* d_angle, mrs_stream stream);
/* The same for n_query queries at once ([n_query][channels][61][120] complex64, row layout; d_dist / d_angle [n_query][n_db]): one robot's scan
 * against the other robots' lists, or the three callbacks' scans against one list (main_RING.py:241-390; BASELINE configs[3]).  Every
 * (query, entry) goes through the one-query pipeline unchanged (bit-identical results); the workgroups that sweep the same entries for
 * different queries share an XCD, so an entry is fetched from HBM once per launch and served to the others by that XCD's L2.  Launches of at
 * most 32 (channels = 1) / 8 (channels > 1) queries; more are split. */
int mrs_ring_corr_fft_sweep_tiled_q(mrs_ctx* ctx, const float* d_query_spec, int32_t n_query, const float* d_db_tiled, int32_t n_db, int32_t channels,
                                    float* d_dist, int32_t* d_angle, mrs_stream stream);

/* One launch for the new-descriptor side of a batch of loop checks: half spectra of n_pairs freshly normalised
 * sinograms (d_half_spec and/or its fp16 replica, either may be null) and their correlation with one candidate
 * spectrum each (d_cand_spec [n_pairs][61][120] complex64).  Results are bitwise those of mrs_ring_half_spectrum
 * followed by mrs_ring_corr_fft_pairs. */
int mrs_ring_spectrum_corr_pairs(mrs_ctx* ctx, const float* d_norm_sino, const float* d_cand_spec, int32_t n_pairs,
                                 int32_t n_angles, int32_t det, float* d_half_spec, void* d_half_spec_f16, float* d_dist,
                                 int32_t* d_angle, mrs_stream stream);
/* Same launch with the candidates picked out of a database: candidate of pair i = row d_cand_index[i] of d_db_spec,
 * a [n_db][61][120] array of complex64 half spectra (db_is_f16 = 0) or of their fp16 replicas (db_is_f16 = 1:
 * IEEE binary16 pairs, the multi-GPU exchange format; arithmetic stays fp32).  This is the per-query step after a
 * candidate pre-selection over the replicated database (RING_ros/main_RING.py:133-140 scores every candidate).
 * An index outside [0, n_db) means "no candidate": dist = +inf, angle = 0 (the new spectrum is still written). */
int mrs_ring_spectrum_corr_pairs_db(mrs_ctx* ctx, const float* d_norm_sino, const void* d_db_spec, int32_t db_is_f16, int32_t n_db,
                                    const int32_t* d_cand_index, int32_t n_pairs, int32_t n_angles, int32_t det, float* d_half_spec,
                                    void* d_half_spec_f16, float* d_dist, int32_t* d_angle, mrs_stream stream);

/* Multi-channel forms (RING++, fast_corr_RINGplusplus, RING_ros/util.py:337-358): descriptors are
 * [channels][61][120] complex64 half spectra of the jointly normalised channels (mrs_normalize_groups over
 * channels*120*120, then mrs_ring_half_spectrum with n_img = n * channels); |corr| is summed over channels and
 * detectors, dist = 1 - max / (0.15 * channels * 120 * 120). */
int mrs_ring_corr_fft_sweep_mc(mrs_ctx* ctx, const float* d_query_spec, int32_t n_query, const float* d_db_spec, int32_t n_db,
                               int32_t channels, float* d_dist, int32_t* d_angle, float* d_corr, mrs_stream stream);
int mrs_ring_corr_fft_pairs_mc(mrs_ctx* ctx, const float* d_a_spec, const float* d_b_spec, int32_t n_pairs, int32_t channels,
                               float* d_dist, int32_t* d_angle, float* d_corr, mrs_stream stream);

/* fp16 replica format (multi-GPU exchange): every descriptor has to reach every GPU, and at
 * >1 M descriptors/s/GPU the fp32 half spectrum (58 560 B) exceeds what the xGMI links carry.  A rank keeps its
 * own descriptors in fp32 (exact scoring) and ships round-to-nearest fp16 copies (29 280 B) to the others, which
 * sweep them with the same kernel (fp32 arithmetic; |dist - fp32 dist| < 2e-3).  The reference has no multi-GPU
 * path; this is the RCCL all-gather format, not a change of the single-GPU results.
 * mrs_ring_half_spectrum_f16: like mrs_ring_half_spectrum, with either output optional (not both null);
 * d_half_spec_f16 = IEEE binary16 pairs [n_img][61][120][2]. */
int mrs_ring_half_spectrum_f16(mrs_ctx* ctx, const float* d_norm_sino, int32_t n_img, int32_t n_angles, int32_t det,
                               float* d_half_spec, void* d_half_spec_f16, mrs_stream stream);
int mrs_ring_corr_fft_sweep_f16(mrs_ctx* ctx, const float* d_query_spec, int32_t n_query, const void* d_db_spec_f16,
                                int32_t n_db, float* d_dist, int32_t* d_angle, float* d_corr, mrs_stream stream);

/* ------------------------------------------------------------------------------------
 * Scan pre-processing
 * ---------------------------------------------------------------------------------- */

/* open3d PointCloud.voxel_down_sample(voxel_size) as the RING / RING++ / SC nodes call it
 * (RING_ros/main_RING.py:257-259): d_points [n][stride] float (is_double = 0) or double (1), xyz first;
 * d_out double[<= n][3] = voxel centroids sorted by voxel index; *h_count = number of voxels.
 * Synchronises `stream`. */
int mrs_voxel_downsample(mrs_ctx* ctx, const void* d_points, int32_t is_double, int32_t stride, int32_t n,
                         double voxel_size, double* d_out, int32_t* h_count, mrs_stream stream);

/* The same filter for a batch of scans in one set of launches (hash grid instead of a sort, one host synchronisation per call instead of per
 * scan): d_points [total][stride], d_raw_offsets / h_raw_offsets int64[batch + 1] (device and host copies of the same offsets, starting at 0).
 * d_out double[<= total][3] receives the centroids scan after scan, each scan's voxels in order of FIRST OCCURRENCE (open3d's own order is
 * unspecified), d_out_offsets int64[batch + 1] (device) their extents.  Centroids are within 1e-13 m of mrs_voxel_downsample's. */
int mrs_voxel_downsample_batch(mrs_ctx* ctx, const void* d_points, int32_t is_double, int32_t stride, const int64_t* d_raw_offsets,
                               const int64_t* h_raw_offsets, int32_t batch, double voxel_size, double* d_out, int64_t* d_out_offsets,
                               mrs_stream stream);

/* G1: pygicp.downsample(points, resolution) (RING_ros/main_RING.py:84-85, disco_ros/main.py:177-178, main_SC.py:111-112)
 * = pcl::ApproximateVoxelGrid<pcl::PointXYZ> with leaf (r, r, r): points narrowed to float, a 512-entry direct-mapped
 * history streamed in input order (a voxel evicted by a colliding one and met again yields another output point),
 * centroids in float, output in flush order.  Same arguments as mrs_voxel_downsample; the result equals the sequential
 * filter bit for bit, order included.  Synchronises `stream`. */
int mrs_voxel_downsample_approx(mrs_ctx* ctx, const void* d_points, int32_t is_double, int32_t stride, int32_t n,
                                double leaf_size, double* d_out, int32_t* h_count, mrs_stream stream);
/* host arrays in and out (pygicp.downsample's calling convention); h_out: room for n x 3 doubles */
int mrs_voxel_downsample_approx_host(mrs_ctx* ctx, const void* h_points, int32_t is_double, int32_t stride, int32_t n,
                                     double leaf_size, double* h_out, int32_t* h_count);

/* load_pc_infer (RING_ros/util.py:91-112, disco_ros/main.py:94-113) for a batch of raw clouds: float32
 * cast, keep |x|,|y| < 70 and 0 < z < 30, divide by 70/70/30.  Raw cloud b = points
 * [raw_offsets[b], raw_offsets[b+1]) (the offsets are needed on both sides: d_ device, h_ host).
 * d_xyz_soa: float[3 * total_raw] (upper bound); d_out_offsets: int64[batch+1], written on the device.
 * (d_xyz_soa, d_out_offsets) is exactly the input of mrs_bev_*_batch: no host round trip. */
int mrs_crop_scale_batch(mrs_ctx* ctx, const void* d_points, int32_t is_double, int32_t stride,
                         const int64_t* d_raw_offsets, const int64_t* h_raw_offsets, int32_t batch,
                         float* d_xyz_soa, int64_t* d_out_offsets, mrs_stream stream);

/* ------------------------------------------------------------------------------------
 * GICP submap assembly from a resident keyframe store
 * ---------------------------------------------------------------------------------- */

/* GlobalManager::mergeNearestKeyframes (Mapping/src/global_manager/src/global_manager.cpp:1894-1939; called twice per loop candidate by
 * ICPCheck, :1968-1969) concatenates the 2 * submap_size + 1 keyframes around the loop keyframe, each moved into the loop keyframe's frame
 * by currPose.inverse() * nearPose, keeps x and y in [-60, 60] (pcl::PassThrough) and runs pcl::VoxelGrid with leaf icp_filter_size -- on the
 * host, on whole clouds, once per candidate.  A mrs_keyframes keeps one robot's keyframes on the device (an arena of float4 x, y, z,
 * intensity; poses on the host) and builds the submaps of a whole batch of candidates in one chain of launches, in the layout
 * mrs_gicp_batch_set_clouds takes (stride_floats = 4).  DESIGN.md section 4.11 states the arithmetic (float32, one rounding per operation,
 * no fused multiply-add; exact pcl::VoxelGrid cells and output order, 64-bit keys) and the deviations from the reference.  Thread-safe (one
 * lock per handle); the device work of a handle runs on the handle's own stream, `stream` is the stream that produced a DEVICE argument or
 * uses d_out (the handle waits for it).  "Bad argument" below is MRS_ERR_ARG, checked before any launch. */
typedef struct mrs_keyframes mrs_keyframes;
/* capacity_hint_points: points to allocate up front (the arena doubles when it runs out; earlier keyframes keep their ids and bits) */
int mrs_keyframes_create(mrs_ctx* ctx, int64_t capacity_hint_points, mrs_keyframes** out);
int mrs_keyframes_destroy(mrs_keyframes* kf);
/* *out_n = keyframes stored, *out_points (optional) = their points */
int mrs_keyframes_size(mrs_keyframes* kf, int32_t* out_n, int64_t* out_points);
/* `keyframes.push_back(cloud)` + `trajectory.push_back(pose)`: points [n][stride] float (is_double = 0) or double (1), xyz first, stride 3, 4
 * or 8 (pygicp's Nx3, pcl::PointXYZ, pcl::PointXYZI), in HOST (on_device = 0; staged through pinned memory, blocking) or DEVICE memory;
 * intensity_col = the column that holds the intensity (4 in a pcl::PointXYZI, 3 in a packed x y z i row) or -1 for none (stored as 0).
 * h_pose16: row-major float32 4x4 rigid transform.  *out_id = the new keyframe's id (0, 1, 2 ...).  One copy (float [n][4] with the
 * intensity in column 3) or one conversion kernel. */
int mrs_keyframes_append(mrs_keyframes* kf, const void* points, int32_t on_device, int32_t is_double, int32_t stride, int32_t intensity_col,
                         int64_t n, const float* h_pose16, int32_t* out_id, mrs_stream stream);
/* the pose graph re-optimises trajectories (global_manager.cpp:636-664): the pose of keyframe `id` replaced, its points untouched */
int mrs_keyframes_set_pose(mrs_keyframes* kf, int32_t id, const float* h_pose16);
/* h_pose16 <- the pose of keyframe `id`, *out_points (optional) <- its point count */
int mrs_keyframes_get_pose(mrs_keyframes* kf, int32_t id, float* h_pose16, int64_t* out_points);

/* n_submaps submaps from explicit segments: segment i puts keyframe h_seg_keyframe[i], moved by the row-major float32 4x4 h_seg_T16 + 16 i,
 * into submap h_seg_submap[i]; segments are listed in ascending submap order (a submap may have none).  Every point is transformed
 * (x' = ((T00 x + T01 y) + T02 z) + T03 ...), dropped unless x', y', z' are finite and -crop <= x', y' <= crop, and the survivors of a
 * submap go through the voxel grid: cell = floorf(v * (1.0f / leaf)), key = (i - min.x) + (j - min.y) div.x + (k - min.z) div.x div.y in 64
 * bits, one output point per occupied voxel in ascending key order = the mean of x', y', z', intensity over the voxel's points.
 * d_out float[capacity_points][4] (device) receives the submaps one after the other, h_offsets int64[n_submaps + 1] (host) their extents.
 * capacity_points must be at least the sum of the segments' point counts (otherwise: bad argument, nothing written).  Bad argument too:
 * leaf <= 0 or not finite, crop < 0 or not finite, a keyframe id out of range, and (after the launches) a grid whose keys need more than
 * 63 bits.  Results are the same bits from run to run and do not depend on the batch a submap is in.  One host synchronisation, at the end. */
int mrs_submap_assemble(mrs_keyframes* kf, int32_t n_submaps, int32_t n_segments, const int32_t* h_seg_submap, const int32_t* h_seg_keyframe,
                        const float* h_seg_T16, float crop, float leaf, float* d_out, int64_t capacity_points, int64_t* h_offsets,
                        mrs_stream stream);
/* mergeNearestKeyframes for n_submaps loop keyframes at once: submap b = the keyframes h_loop_ids[b] + i, i = -submap_size .. submap_size,
 * with 0 < id < size (the reference's `keyNear <= 0` skip is kept: keyframe 0 is never merged; its `keyNear == size()` read past the vector
 * is not), each moved by inverse(pose[loop id]) * pose[id], computed on the host in float32 term by term.  Then as mrs_submap_assemble. */
int mrs_submap_merge_nearest(mrs_keyframes* kf, int32_t n_submaps, const int32_t* h_loop_ids, int32_t submap_size, float crop, float leaf,
                             float* d_out, int64_t capacity_points, int64_t* h_offsets, mrs_stream stream);

/* ------------------------------------------------------------------------------------
 * Keyframe intake: raw clouds filtered on the device and registered in the store
 * ---------------------------------------------------------------------------------- */

/* The front of GlobalManager::mapUpdate (Mapping/src/global_manager/src/global_manager.cpp:1684-1709, :1735, :1797): pcl::fromROSMsg, an
 * exact pcl::VoxelGrid with leaf submap_voxel_leaf_size_, pcl::PassThrough on z in [-1, 30], intensity = robotid * 30, emplace_back -- for
 * n_clouds >= 0 raw clouds in one chain of launches.  DESIGN.md section 4.14 is the contract; the cells, keys, output order and means are
 * section 4.11's.
 * `data` is one byte blob in HOST (on_device = 0; staged through the handle's pinned buffer) or DEVICE memory (4-byte aligned).  Cloud c is
 * the points h_offsets[c] .. h_offsets[c + 1] (int64 [n_clouds + 1], ascending, h_offsets[0] = 0); point i starts at byte i * point_step;
 * off_x, off_y, off_z are the byte offsets of three float32 fields and off_intensity that of a fourth, or -1 for none (taken as 0): what a
 * sensor_msgs/PointCloud2 describes.  pcl::toROSMsg of a pcl::PointXYZI cloud is point_step 32 with offsets 0, 4, 8, 16; the store's own
 * float[n][4] is 16 with 0, 4, 8, 12.
 * Per cloud, independently of the others: a point is dropped unless x, y, z are finite; the rest go through the voxel grid (cell =
 * floorf(v * (1.0f / leaf)), 64-bit keys, one point per occupied voxel in ascending key order = the mean of x, y, z, intensity, summed in
 * float64 in input order and rounded to float32 once); a voxel is kept iff z_lo <= mean z <= z_hi (both ends inclusive, +-inf switches a
 * side off); if set_intensity is 1 every survivor's intensity becomes `intensity` (the caller passes robotid * 30).  The survivors become
 * keyframe out_ids[c] (int32 [n_clouds], consecutive, in input order) with the row-major float32 4x4 pose h_pose16s + 16 c; out_counts[c]
 * (int64 [n_clouds]) is their number.  A cloud with no point or no survivor is a keyframe with 0 points and gets its id.  Only the
 * survivors are stored: mrs_keyframes_size's point total grows by the sum of out_counts.  Results are the same bits from run to run and
 * do not depend on the other clouds of the call.
 * Bad argument (MRS_ERR_ARG), checked before any launch, store unchanged: a null pointer where one is needed; point_step < 12 or not a
 * multiple of 4; an offset that is negative (other than off_intensity = -1), not a multiple of 4 or beyond point_step - 4; off_x, off_y,
 * off_z not ascending; leaf <= 0 or not finite; z_lo or z_hi NaN, or z_lo > z_hi; set_intensity other than 0 / 1; intensity not finite
 * when set_intensity is 1; a pose that is not finite; h_offsets not ascending from 0; more than 2^31 - 1 points in the call.  MRS_ERR_ARG
 * too, after the first launches and with the store still unchanged: a cloud whose grid needs keys of more than 63 bits, and a call whose
 * (cloud, key) pairs do not fit 64 bits together (bits of the widest grid + bits of n_clouds: split the call; one cloud always fits).
 * Thread-safe (the handle's lock); the device work runs on the handle's stream, which waits for `stream` (the stream that produced a
 * device blob).  Two host synchronisations: one for the key widths, one for the counts. */
int mrs_keyframes_ingest(mrs_keyframes* kf, int32_t n_clouds, const void* data, int32_t on_device, const int64_t* h_offsets, int32_t point_step,
                         int32_t off_x, int32_t off_y, int32_t off_z, int32_t off_intensity, float leaf, float z_lo, float z_hi,
                         int32_t set_intensity, float intensity, const float* h_pose16s, int32_t* out_ids, int64_t* out_counts,
                         mrs_stream stream);
/* `keyframe_pub.publish(*keyframe)` (global_manager.cpp:1800-1802) and savingKeyframes (:218-272): the points of keyframe `id` copied as
 * float[n][4] (x, y, z, intensity) into `out`, in HOST (on_device = 0; blocking) or DEVICE memory (ordered after and before the work of
 * `stream`); *out_points = n.  Bad argument: id out of range, capacity_points (the room in `out`, in points) below n. */
int mrs_keyframes_get_points(mrs_keyframes* kf, int32_t id, float* out, int32_t on_device, int64_t capacity_points, int64_t* out_points,
                             mrs_stream stream);

/* ------------------------------------------------------------------------------------
 * The merged multi-robot map composed from the keyframe stores
 * ---------------------------------------------------------------------------------- */

/* GlobalManager::composeGlobalMap (Mapping/src/global_manager/src/global_manager.cpp:2090-2210) / savingGlobalMap (:143-170): every robot's
 * keyframes moved by their optimised poses, concatenated, one pcl::VoxelGrid with leaf globalmap_voxel_leaf_size_ over the whole thing.
 * ONE voxel grid for the whole call (the point arithmetic, cells, keys and output order are section 4.11's).  The
 * input is, in this order: the optional previous map d_prev, float[n_prev][4] on the device, taken as it is (the incremental branch,
 * :2170-2189: an old centroid counts as one point), then segment 0, 1, ...: keyframe h_seg_keyframe[i] of stores[h_seg_store[i]] moved by
 * the row-major float32 4x4 h_seg_T16 + 16 i; segments of different stores may interleave, and a store may be listed more than once.  A
 * point is dropped only if x', y' or z' is not finite; there is no crop.  d_out float[capacity_points][4] (device) receives one point per
 * occupied voxel in ascending key order, the mean of x', y', z', intensity, summed in float64 in an order fixed by the input alone and
 * rounded to float32 once: the same bits from call to call.  *out_points = the number of voxels.
 * Bad argument (MRS_ERR_ARG), checked before any launch, nothing written: a null pointer where one is needed, n_stores outside
 * 1 .. MRS_MAP_MAX_STORES, stores on different devices, a store index or keyframe id out of range, a transform or leaf that is not finite,
 * leaf <= 0, capacity_points < n_prev + the segments' point counts, more than 2^31 - 1 input points, d_prev overlapping d_out.  MRS_ERR_ARG
 * too, after the first launches, when the grid's keys need more than 63 bits.
 * Thread-safe: every distinct store is locked once, in address order.  The device work runs on the first store's stream, which waits for
 * the other stores' streams and for `stream` (the stream that produced d_prev and uses d_out).  Two host synchronisations: one for the
 * key width, one at the end. */
#define MRS_MAP_MAX_STORES 16
int mrs_map_compose(int32_t n_stores, mrs_keyframes* const* stores, int32_t n_segments, const int32_t* h_seg_store,
                    const int32_t* h_seg_keyframe, const float* h_seg_T16, const float* d_prev, int64_t n_prev, float leaf, float* d_out,
                    int64_t capacity_points, int64_t* out_points, mrs_stream stream);

/* ------------------------------------------------------------------------------------
 * Multi-GPU exchange of the descriptor database over RCCL / xGMI
 * ---------------------------------------------------------------------------------- */

/* The reference has no collective at all (its three robots share one process and one GPU).  One process per GPU here; every rank builds the
 * descriptors of its share of the scans, then either every rank receives everybody's (mrs_exchange_allgather: ONE ncclAllGather per launch;
 * the per-robot lists of main_RING.py:284-288, replicated) or only the candidate rows a rank asks for travel (mrs_exchange_fetch_rows).
 * A C++ host (the Mapping node) calls these directly; mr_slam_amd/shard.py calls the same entry points.  RCCL is looked up at run time
 * (symbols already in the process first, then librccl.so.1); mrs_exchange_available() says whether it was found. */
typedef struct mrs_exchange mrs_exchange;
int mrs_exchange_available(void);
/* ncclGetUniqueId: 128 bytes made by ONE rank and handed to the others by the host (file, socket, torch.distributed broadcast ...) */
int mrs_exchange_unique_id(uint8_t* out128);
/* ncclCommInitRank on the context's device; collective over all n_ranks */
int mrs_exchange_create(mrs_ctx* ctx, int32_t n_ranks, int32_t rank, const uint8_t* id128, mrs_exchange** out);
/* borrow a communicator the host already has (ncclComm_t as void*); it is not destroyed with the handle */
int mrs_exchange_create_from_comm(mrs_ctx* ctx, void* nccl_comm, int32_t n_ranks, int32_t rank, mrs_exchange** out);
int mrs_exchange_destroy(mrs_exchange* x);
int mrs_exchange_world(const mrs_exchange* x, int32_t* n_ranks, int32_t* rank);
/* d_all [n_ranks][n_local] entries of entry_bytes <- every rank's d_local [n_local], in rank order.  Enqueued on `stream`. */
int mrs_exchange_allgather(mrs_exchange* x, const void* d_local, int64_t n_local, int64_t entry_bytes, void* d_all, mrs_stream stream);
/* Rank r owns global rows [r * rows_per_rank, (r + 1) * rows_per_rank) (d_local_db).  d_out [n_rows] <- the entries of d_global_rows (device
 * int64 [n_rows], any owner, repeats allowed; the same n_rows on every rank), in request order: the requests are all-gathered, every owner
 * packs what it was asked for, one grouped send / receive per peer pair moves exactly those rows.  entry_bytes % 16 == 0.  Collective; blocking. */
int mrs_exchange_fetch_rows(mrs_exchange* x, const void* d_local_db, int64_t rows_per_rank, int64_t entry_bytes, const int64_t* d_global_rows,
                            int32_t n_rows, void* d_out, mrs_stream stream);
/* The same with the request phase done ahead of time (candidate rows are known long before the entries are needed: they come out of a coarse
 * search).  mrs_exchange_fetch_plan_create is a COLLECTIVE (every rank calls it, with its own d_global_rows [n_rows]; one all-gather of the
 * requests + one host synchronisation); mrs_exchange_fetch_planned then only enqueues work on `stream` (gather -> one grouped send / receive
 * per remote peer -> scatter to request order into d_out [n_rows][entry_bytes]): no host synchronisation, so it can be issued launches ahead
 * on a communication stream.  Fetches of ONE plan share the plan's staging buffers and must follow each other in stream order. */
typedef struct mrs_fetch_plan mrs_fetch_plan;
int mrs_exchange_fetch_plan_create(mrs_exchange* x, int64_t rows_per_rank, const int64_t* d_global_rows, int32_t n_rows, mrs_stream stream,
                                   mrs_fetch_plan** out);
int mrs_exchange_fetch_planned(mrs_fetch_plan* plan, const void* d_local_db, int64_t entry_bytes, void* d_out, mrs_stream stream);
int mrs_exchange_fetch_plan_counts(const mrs_fetch_plan* plan, int64_t* rows_sent_to_peers, int64_t* rows_received_from_peers);
int mrs_exchange_fetch_plan_destroy(mrs_fetch_plan* plan);

/* ------------------------------------------------------------------------------------
 * Loop database: the per-robot descriptor lists of the LoopDetection nodes, resident on the device
 * ---------------------------------------------------------------------------------- */

/* The reference keeps one Python list of descriptors per robot, appends one entry per callback and scores every new scan
 * against every entry of the other robots' lists in a Python loop:
 *   RING   : TIRING<k>.append(pc_TIRING) / `for idx in range(len(pc_candidates)): fast_corr(TIRING_current, TIRING_candidates[idx])`
 *            (RING_ros/main_RING.py:284-288, 126-140)
 *   RING++ : the same with fast_corr_RINGplusplus (RING_ros/main_RINGplusplus.py:126-134)
 *   DiSCO  : DiSCO<k>.append / FFT<k>.append, `KDTree(np.array(DiSCO_candidates)).query(DiSCO_current, k=1)` + phase_corr of the winner
 *            (disco_ros/main.py:276-291, 356-360)
 * A mrs_loopdb is that list on the device: entries are stored in the format the sweep kernels stream (RING: DMA-tiled half spectra,
 * RING++: [C][61][120] half spectra of the jointly normalised channels, DiSCO: 1024-d signatures + 40 x 120 spectra), an append writes
 * ONE slot (amortised doubling, nothing is re-uploaded), a query is ONE sweep over all entries.  Thread-safe (one lock per handle; the
 * reference's callbacks run on concurrent rospy threads); all device work of a handle runs on the handle's own stream, `stream` is the
 * stream that produced a DEVICE argument (the handle waits for it; for appends it is made to wait until the argument has been consumed). */
typedef struct mrs_loopdb mrs_loopdb;
enum mrs_loopdb_kind { MRS_LOOPDB_RING = 0, MRS_LOOPDB_RINGPP = 1, MRS_LOOPDB_DISCO = 2, MRS_LOOPDB_SC = 3, MRS_LOOPDB_M2DP = 4, MRS_LOOPDB_FH = 5 };
/* where / what a RING or RING++ descriptor argument is:
 *   HOST / DEVICE : the reference's own object -- RING: pc_TIRING, complex64 [1][120][120] (util.py:198; its first 61 rows are what is
 *                   kept); RING++: pc_TIRING, float32 [C][120][120] magnitudes (util.py:247-250; normalised jointly + transformed along the
 *                   angle axis here, once, instead of at every comparison as util.py:339-343 does)
 *   DEVICE_SPEC   : half spectra in the product's row layout, complex64 [C][61][120] (mrs_ring_half_spectrum / mrs_ring_spectrum_corr_pairs) */
enum mrs_loopdb_form { MRS_LOOPDB_FORM_HOST = 0, MRS_LOOPDB_FORM_DEVICE = 1, MRS_LOOPDB_FORM_DEVICE_SPEC = 2 };

/* channels: 1 for RING, C (6 in the reference) for RING++, ignored for DiSCO, SC and M2DP; for FH it carries the number of buckets
 * (1 .. MRS_FH_MAX_BINS); capacity_hint: entries to allocate up front (>= 1) */
int mrs_loopdb_create(mrs_ctx* ctx, int32_t kind, int32_t channels, int32_t capacity_hint, mrs_loopdb** out);
int mrs_loopdb_destroy(mrs_loopdb* db);
int mrs_loopdb_size(mrs_loopdb* db, int32_t* out_n);
int mrs_loopdb_reserve(mrs_loopdb* db, int32_t capacity);
int mrs_loopdb_clear(mrs_loopdb* db);
/* `TIRING<k>.append(descriptor)`.  count > 1 only with DEVICE_SPEC (a batch producer appending `count` consecutive half spectra). */
int mrs_loopdb_append(mrs_loopdb* db, const void* descriptor, int32_t form, int32_t count, mrs_stream stream);
/* The candidate loop of detect_loop_icp (main_RING.py:133-140): scores `descriptor` against every entry with one sweep and returns, in
 * index order, the entries with dist < dist_threshold (float32 comparison): h_index / h_dist / h_angle [max_out] and *h_count (the number
 * that qualified; when it exceeds max_out only the first max_out were written).  h_all_dist / h_all_angle (optional, [all_capacity]) receive
 * the scores of the first min(n, all_capacity) entries, *h_n (optional) the number of entries n this call scored -- another thread may append
 * between the caller's mrs_loopdb_size and this call, so arrays are never written past all_capacity.  Blocking; an empty database returns
 * *h_count = 0 without device work. */
int mrs_loopdb_query(mrs_loopdb* db, const void* descriptor, int32_t form, float dist_threshold, int32_t max_out, int32_t* h_index,
                     float* h_dist, int32_t* h_angle, int32_t* h_count, int32_t all_capacity, float* h_all_dist, int32_t* h_all_angle, int32_t* h_n,
                     mrs_stream stream);
/* `count` descriptors (consecutive in memory, all in the same form; 1 .. 1024) against every entry in ONE sweep
 * (mrs_ring_corr_fft_sweep_tiled_q): the shape of one robot's scan against several lists, of the three callbacks' scans against one list
 * (main_RING.py:241-390), and of BASELINE configs[3].  h_all_dist / h_all_angle [count][all_capacity]: row q = the scores of query q over
 * the first min(n, all_capacity) entries; *h_n = n.  Same bits as `count` calls of mrs_loopdb_query.  Blocking. */
int mrs_loopdb_query_multi(mrs_loopdb* db, const void* descriptors, int32_t form, int32_t count, int32_t all_capacity, float* h_all_dist,
                           int32_t* h_all_angle, int32_t* h_n, mrs_stream stream);
/* DiSCO: signature float32 [1024], spectrum complex64 [40][120] (DiSCO.forward's two outputs, disco_ros/models/DiSCO.py:315-334). */
int mrs_loopdb_append_disco(mrs_loopdb* db, const float* signature, const float* spectrum, int32_t on_device, mrs_stream stream);
/* disco_ros/main.py:284-291 in two launches: nearest signature (squared L2, ties to the lower index) and phase_corr(FFT_candidates[idx],
 * fft_current): *h_index (-1 for an empty database), *h_dist2, *h_flat_argmax = flat index of the first maximum of the shifted magnitude
 * map (the reference takes it `% num_sector`).  Blocking. */
int mrs_loopdb_query_disco(mrs_loopdb* db, const float* signature, const float* spectrum, int32_t on_device, int32_t* h_index, float* h_dist2,
                           int32_t* h_flat_argmax, mrs_stream stream);
/* Scan Context: SC<k>.append(SC_current) / RingkeyPC<k>.append(make_ringkey(SC_current)) of the SC node (RING_ros/main_SC.py; descriptor
 * = generate_scan_context, main_SC.py:57-69: the Cartesian max-z BEV, float32 [120][120], axis -2 "ring", axis -1 "sector").  The handle
 * stores the descriptor with its sector keys and column norms, and its ring key (make_ringkey, pr_methods/ScanContext.py:13-21). */
int mrs_loopdb_append_sc(mrs_loopdb* db, const float* sc, int32_t on_device, mrs_stream stream);
/* detect_loop_icp_SC's candidate step (main_SC.py:159-167) with num_candidates = k (1 .. 64; the node uses 1, config.py:15 has 10):
 * the k nearest ring keys (Euclidean, fp64, ascending, ties to the lower index: KDTree(Ringkey_candidates).query(k)), then
 * dist_align_sc(SC_candidate, SC_current, search_ratio) (pr_methods/ScanContext.py:128-142) for each.  h_index / h_key_dist / h_dist /
 * h_shift [num_candidates]; *h_count = min(k, n).  The shift is the reference's: in [-S, S), the roll applied to SC_current.  Blocking;
 * an empty database returns *h_count = 0 and index -1 without device work. */
int mrs_loopdb_query_sc(mrs_loopdb* db, const float* sc, int32_t on_device, int32_t num_candidates, double search_ratio, int32_t* h_index,
                        float* h_key_dist, float* h_dist, int32_t* h_shift, int32_t* h_count, mrs_stream stream);
/* dist_align_sc(entry, sc, search_ratio) against EVERY entry in one launch: h_all_dist / h_all_shift receive the first min(n, all_capacity)
 * results, *h_best the index of the first smallest dist over all n (-1 when empty), *h_n = n.  Blocking. */
int mrs_loopdb_query_sc_all(mrs_loopdb* db, const float* sc, int32_t on_device, double search_ratio, int32_t all_capacity, float* h_all_dist,
                            int32_t* h_all_shift, int32_t* h_best, int32_t* h_n, mrs_stream stream);
/* M2DP (MRS_LOOPDB_M2DP): the list of 192-d descriptors a node would keep per robot and search by Euclidean distance (the M2DP paper's
 * matching rule; the reference ships the descriptor, RING_ros/pr_methods/M2DP.py, without a node of its own).  desc = double [192] as
 * mrs_m2dp_batch writes it, host (on_device = 0) or device; entries are stored as float32 [192]. */
int mrs_loopdb_append_m2dp(mrs_loopdb* db, const double* desc, int32_t on_device, mrs_stream stream);
/* The k nearest entries by squared L2 distance over the float32-rounded descriptors (mrs_signature_knn with dim = 192: ascending, ties to
 * the lower index), 1 <= k <= 32: h_index / h_dist2 [k], *h_count = min(k, n); the slots past it hold -1 / +inf.  Blocking; an empty
 * database returns *h_count = 0 and index -1 without device work. */
int mrs_loopdb_query_m2dp(mrs_loopdb* db, const double* desc, int32_t on_device, int32_t k, int32_t* h_index, float* h_dist2, int32_t* h_count,
                          mrs_stream stream);
/* Fast Histogram (MRS_LOOPDB_FH): the list of range histograms a node would keep per robot and compare with getEMD / calculateW
 * (RING_ros/pr_methods/FastHistogram.py:66-84; the reference ships the descriptor without a node of its own).  hist = double [bins] as
 * mrs_fh_batch writes it, host (on_device = 0) or device; entries are stored as they come, in fp64, one row of `bins` doubles each. */
int mrs_loopdb_append_fh(mrs_loopdb* db, const double* hist, int32_t on_device, mrs_stream stream);
/* getEMD(hist, entry) = calculateW (FastHistogram.py:66-84) against every entry in one launch: the sum over i, in index order, of
 * |hist_i - entry_i| in fp64, divided by bins -- the reference's bits, not an approximation (one lane per entry walks the buckets in
 * order).  The k nearest, 1 <= k <= 32, ascending, ties to the lower index: h_index / h_dist [k], *h_count = min(k, n); the slots past it
 * hold -1 / +inf.  Blocking; an empty database returns *h_count = 0 and index -1 without device work. */
int mrs_loopdb_query_fh(mrs_loopdb* db, const double* hist, int32_t on_device, int32_t k, int32_t* h_index, double* h_dist, int32_t* h_count,
                        mrs_stream stream);
/* The same distances to all n entries, left on the device: d_dist double [n], n = mrs_loopdb_size at the time of the call (the caller
 * keeps other threads from appending between sizing the array and this call).  The work runs on the handle's stream; `stream` is made to
 * wait for it, so the caller's later work on `stream` sees the distances.  Not blocking. */
int mrs_loopdb_distances_fh(mrs_loopdb* db, const double* hist, int32_t on_device, double* d_dist, mrs_stream stream);
/* the entries as they lie on the device (tests, exchange): valid until the next append that grows the capacity.  SC: d_entries = packed
 * entries (entry_floats apart: sector keys [128], column norms [128], then the [120][120] descriptor), d_signatures = ring keys [n][120] */
int mrs_loopdb_device_entries(mrs_loopdb* db, const float** d_entries, const float** d_signatures, int32_t* out_n, int64_t* entry_floats);

/* ------------------------------------------------------------------------------------
 * Scan Context on device arrays (RING_ros/pr_methods/ScanContext.py).  d_sc* are float32 [n][num_ring][num_sector], row-major like the
 * reference's descriptors; num_ring, num_sector <= 128 (the node's 120 x 120 Cartesian descriptor, or the paper's 20 x 60 polar one from
 * mrs_bev_polar_batch); larger geometries return MRS_ERR_UNSUPPORTED.
 * ---------------------------------------------------------------------------------- */

/* make_ringkey (row means, [n][num_ring]) and make_sectorkey (column means, [n][num_sector]) (ScanContext.py:13-31); either output may be
 * NULL.  float32 values (the reference stores the float32 means in float64 arrays). */
int mrs_sc_keys(mrs_ctx* ctx, const float* d_sc, int32_t n, int32_t num_ring, int32_t num_sector, float* d_ring_key, float* d_sector_key,
                mrs_stream stream);
/* fast_align_with_sectorkey(key1, key2) (ScanContext.py:86-101) for pairs of float32 keys [n_pairs][len]: min over s of
 * ||key1 - roll(key2, s)|| (fp64) and the first s attaining it. */
int mrs_sc_key_align_pairs(mrs_ctx* ctx, const float* d_key1, const float* d_key2, int32_t n_pairs, int32_t len, double* d_norm, int32_t* d_shift,
                           mrs_stream stream);
/* dist_direct_sc(sc1, sc2) (ScanContext.py:105-126): 1 - mean column cosine over the columns where both norms are > 0 (1.0 if none). */
int mrs_sc_dist_direct_pairs(mrs_ctx* ctx, const float* d_sc1, const float* d_sc2, int32_t n_pairs, int32_t num_ring, int32_t num_sector,
                             float* d_dist, mrs_stream stream);
/* dist_align_sc(sc1, sc2, search_ratio) (ScanContext.py:128-142): sector-key pre-alignment s*, then the window
 * [max(-S, s* - r), min(S, s* + r + 1)) with r = round(0.5 search_ratio S), first minimum; d_shift may be negative. */
int mrs_sc_dist_align_pairs(mrs_ctx* ctx, const float* d_sc1, const float* d_sc2, int32_t n_pairs, int32_t num_ring, int32_t num_sector,
                            double search_ratio, float* d_dist, int32_t* d_shift, mrs_stream stream);
/* distance_sc(sc1, sc2) (ScanContext.py:34-69): all num_sector shifts of sc1, mean cosine over the engaged columns (0 if none);
 * d_dist = 1 - max, d_yaw = argmax + 1 (the reference's convention). */
int mrs_sc_distance_pairs(mrs_ctx* ctx, const float* d_sc1, const float* d_sc2, int32_t n_pairs, int32_t num_ring, int32_t num_sector, float* d_dist,
                          int32_t* d_yaw, mrs_stream stream);

/* ------------------------------------------------------------------------------------
 * M2DP on device arrays (RING_ros/pr_methods/M2DP.py:43-124)
 * ---------------------------------------------------------------------------------- */

/* points per workgroup of the signature-matrix kernel (tests probe both sides of it) */
#define MRS_M2DP_TILE_POINTS 1024

/* M2DP(cloud) for a batch of clouds in one set of launches, replacing the reference's Python loop over 64 planes with np.histogram2d
 * inside (GetSignatureMatrix, M2DP.py:43-82) and its sklearn PCA / np.linalg.svd calls (M2DP.py:99-123).  d_points [total][stride] float
 * (is_double = 0; widened to double first) or double (1), xyz first; d_offsets / h_offsets int64 [batch + 1], device and host copies of the
 * same offsets (the convention of mrs_voxel_downsample_batch).  d_desc double [batch][192] = concat(u0 [64], v0 [128]) of the signature
 * matrix, with the sign that makes sum(u0) >= 0 (both vectors non-negative; LAPACK's sign is arbitrary); d_A double [batch][64][128]
 * (optional) = the signature matrix, row 16 * azimuth_index + elevation_index, column 16 * rho_bin + theta_bin, counts / n.  Clouds of
 * fewer than 3 points give zeros (M2DP.py:100-109).  All arithmetic is fp64 and the counts are integers: the result does not depend on
 * the batch a cloud is in.  Enqueued on `stream`. */
int mrs_m2dp_batch(mrs_ctx* ctx, const void* d_points, int32_t is_double, int32_t stride, const int64_t* d_offsets, const int64_t* h_offsets,
                   int32_t batch, double* d_desc, double* d_A, mrs_stream stream);
/* The PCA stage of mrs_m2dp_batch alone (PCA().fit_transform, M2DP.py:105, and maxRho, M2DP.py:117-118): d_pca double [batch][16] =
 * mean [3], components [3][3] (rows, descending eigenvalue, largest-magnitude coefficient positive), maxRho, covariance eigenvalues [3];
 * zeros for clouds of fewer than 3 points. */
int mrs_m2dp_pca_batch(mrs_ctx* ctx, const void* d_points, int32_t is_double, int32_t stride, const int64_t* d_offsets,
                       const int64_t* h_offsets, int32_t batch, double* d_pca, mrs_stream stream);
/* One cloud, host arrays in and out (the reference's calling convention): h_points [n][stride], n >= 0; h_desc double [192],
 * h_A double [64][128] (optional).  Blocking. */
int mrs_m2dp_host(mrs_ctx* ctx, const void* h_points, int32_t is_double, int32_t stride, int32_t n, double* h_desc, double* h_A);

/* ------------------------------------------------------------------------------------
 * Fast Histogram on device arrays (RING_ros/pr_methods/FastHistogram.py:10-63)
 * ---------------------------------------------------------------------------------- */

/* points per workgroup of the range and bin kernels (tests probe both sides of it) */
#define MRS_FH_TILE_POINTS 2048
/* largest number of buckets */
#define MRS_FH_MAX_BINS 256

/* statisticsOnRange(cloud, bins) for a batch of clouds in one set of launches, replacing calculateRange's Python loop over the points
 * (FastHistogram.py:10-21) and statisticsOnRange's per-point distanceJudge call with its loop over all buckets (FastHistogram.py:24-63).
 * d_points [total][stride] float (is_double = 0; widened to double first) or double (1), xyz first; d_offsets / h_offsets int64
 * [batch + 1], device and host copies of the same offsets (the convention of mrs_m2dp_batch).  bins in 1 .. MRS_FH_MAX_BINS (the reference's
 * default is 100).  d_hist double [batch][bins] = counts / n; optional: d_counts int32 [batch][bins], d_range double [batch] = the largest
 * finite range M of each cloud (0 for an empty one), d_unbound int32 [batch] = the points with 0 < d < M above the last edge fl(bins w),
 * where the reference raises UnboundLocalError (they are counted in bucket bins - 1).  A point at range d = sqrt((x x + y y) + z z) falls
 * into the largest i < bins with fl(i w) <= d, w = fl(M / bins), when 0 < d < M, and into bucket bins - 1 otherwise (d == 0, d == M, d not
 * finite; such points do not take part in M).  An empty cloud gives zeros.  All arithmetic is correctly rounded fp64 and the counts are
 * integers: the result does not depend on the batch a cloud is in.  Enqueued on `stream`. */
int mrs_fh_batch(mrs_ctx* ctx, const void* d_points, int32_t is_double, int32_t stride, const int64_t* d_offsets, const int64_t* h_offsets,
                 int32_t batch, int32_t bins, double* d_hist, int32_t* d_counts, double* d_range, int32_t* d_unbound, mrs_stream stream);
/* One cloud, host arrays in and out (the reference's calling convention, FastHistogram.py:40): h_points [n][stride], n >= 0; h_hist double
 * [bins]; optional: h_counts int32 [bins], h_range double [1], h_unbound int32 [1].  Blocking. */
int mrs_fh_host(mrs_ctx* ctx, const void* h_points, int32_t is_double, int32_t stride, int32_t n, int32_t bins, double* h_hist, int32_t* h_counts,
                double* h_range, int32_t* h_unbound);

/* ------------------------------------------------------------------------------------
 * Pairwise consistency of the inter-robot loops of one robot pair: what
 * global_map::GlobalMap::pairwiseConsistencyMaximization computes for DistributedPCM::solveCentralized
 * (Mapping/src/global_manager/src/global_manager.cpp:1301-1310): the consistency matrix of
 * pairwise_consistency.cpp:40-137 and the clique of FMC::maxCliqueHeu (findCliqueHeu.cpp:120-243).  DESIGN.md 4.18.
 * Host arrays in and out; every call is blocking and works on the legacy default stream.  One caller at a time per handle.
 * ---------------------------------------------------------------------------------- */
typedef struct mrs_pcm mrs_pcm;

/* most loops one handle holds */
#define MRS_PCM_MAX_LOOPS 4096

/* capacity in 1 .. MRS_PCM_MAX_LOOPS (more: MRS_ERR_UNSUPPORTED); threshold > 0 and finite: loops u, v are consistent iff
 * |Logmap(Z_u^-1 (XA_i^-1 XA_j) Z_v (XB_l^-1 XB_k))| < threshold (getChiSquaredThreshold: 0.872 for the launch default p = 0.01) */
int mrs_pcm_create(mrs_ctx* ctx, int32_t capacity, double threshold, mrs_pcm** out);
int mrs_pcm_destroy(mrs_pcm* pcm);
/* The two trajectories as row-major 4x4 poses, double [na][4][4] and [nb][4][4] (buildTrajectory's chain from the identity).  Clears the
 * loops. */
int mrs_pcm_set_trajectories(mrs_pcm* pcm, const double* h_XA, int32_t na, const double* h_XB, int32_t nb);
/* Appends n loops (h_ia[u], h_kb[u], h_Z[u]): h_Z double [n][4][4] is the measured pose of B_k in the frame of A_i.  Vertex numbers follow
 * the order of addition.  Computes the new rows and columns of the consistency matrix; the bits do not depend on how the loops were split
 * over calls.  An index outside its trajectory: MRS_ERR_ARG; more loops than the capacity: MRS_ERR_UNSUPPORTED; nothing is added then.  A
 * loop whose pose is not finite is consistent with no other. */
int mrs_pcm_add_loops(mrs_pcm* pcm, const int32_t* h_ia, const int32_t* h_kb, const double* h_Z, int32_t n);
int mrs_pcm_clear_loops(mrs_pcm* pcm);
int mrs_pcm_count(mrs_pcm* pcm, int32_t* h_count);
/* FMC::maxCliqueHeu of the current matrix: h_clique int32 [count] receives the member list in the reference's order (the start vertex,
 * then the vertices in the order the greedy chain took them), h_n_clique its length (0 without loops, where the reference returns -1);
 * optional h_n_rounds: the speculative rounds it took (at most length + 1). */
int mrs_pcm_solve(mrs_pcm* pcm, int32_t* h_clique, int32_t* h_n_clique, int32_t* h_n_rounds);
/* The exact search expands at most MRS_PCM_EXACT_LAUNCH_NODES nodes per wave and launch in at most MRS_PCM_EXACT_MAX_WAVES waves, so a call
 * may count up to MRS_PCM_EXACT_OVERSHOOT nodes more than its budget.  The default budget is about one second of search on an MI355X at
 * the node rate measured on long searches, 27 000 to 74 000 nodes per second (profiles/pcm_exact_notes.md). */
#define MRS_PCM_EXACT_LAUNCH_NODES 4096
#define MRS_PCM_EXACT_MAX_WAVES 1024
#define MRS_PCM_EXACT_OVERSHOOT 4194304
#define MRS_PCM_EXACT_DEFAULT_NODES 50000
/* A MAXIMUM clique of the current matrix, what FMC::maxClique(gio, 0, data) returns (findClique.cpp:29-154): h_clique
 * int32 [count] receives, in ASCENDING order, the maximum clique whose members sorted descending form the lexicographically largest
 * sequence; h_n_clique its size (0 without loops; [count - 1] without edges).  The search is a branch and bound with a budget of
 * max_nodes nodes (a node: one vertex taken into the current clique).  h_proof: 2 = size proven and list canonical (bit-stable from run to
 * run and over any split of the loops); 1 = size proven, the list is a clique of that size; 0 = the budget ran out first: the list is the
 * best clique found, never smaller than mrs_pcm_solve's.  h_nodes: the nodes counted, at most max_nodes + MRS_PCM_EXACT_OVERSHOOT.
 * max_nodes = 0: the heuristic's clique, ascending, proof 0, nodes 0.  max_nodes < 0 or a null pointer: MRS_ERR_ARG.  Unlike the
 * reference, a call never returns a size with an empty list.  mrs_pcm_solve is not affected. */
int mrs_pcm_solve_exact(mrs_pcm* pcm, int64_t max_nodes, int32_t* h_clique, int32_t* h_n_clique, int32_t* h_proof, int64_t* h_nodes);
/* the search launches the last mrs_pcm_solve_exact of this handle made (for measurements) */
int mrs_pcm_exact_launches(mrs_pcm* pcm, int64_t* h_launches);
/* the consistency matrix, uint8 [count][count] of 0 / 1: symmetric, zero diagonal */
int mrs_pcm_get_matrix(mrs_pcm* pcm, uint8_t* h_dense);
/* Replaces the loops by `count` vertices with the given adjacency (uint8 [count][count], non-zero = edge), so that the clique stage can be
 * used without the geometry.  Asymmetric input or a set diagonal: MRS_ERR_ARG.  Such vertices have no distances, and loops cannot be
 * appended to them: both are MRS_ERR_ARG until the loops are cleared. */
int mrs_pcm_set_matrix(mrs_pcm* pcm, int32_t count, const uint8_t* h_dense);
/* the consistency distances, double [count][count], recomputed by this call (they are never stored): symmetric, zero diagonal.  They are
 * the quantity compared with the threshold: |Logmap| without covariances, the squared Mahalanobis distance with them (NaN where that is
 * not finite or the cycle covariance has no Cholesky factor). */
int mrs_pcm_get_distances(mrs_pcm* pcm, double* h_d);

/* Consistency under covariances: loops u < v are consistent iff xi^T Sigma_E^-1 xi < threshold, xi = Logmap of the cycle
 * pose and Sigma_E the covariance computeConsistencyError propagates around the cycle (pairwise_consistency.cpp:99-128) from the odometry
 * and loop covariances; the threshold is then an upper chi-squared quantile with 6 degrees of freedom.  Every covariance is a row-major
 * double [6][6] in gtsam's Pose3 tangent order (rotation xyz, translation xyz) of which the lower triangle is read.
 *   MRS_PCM_COV_SPAN      : the trajectory part is the odometry between the two poses alone, S_i,i = 0,
 *                           S_i,m+1 = Ad(o_m^-1) S_i,m Ad(o_m^-1)^T + Q_m (the test of the PCM paper; recommended);
 *   MRS_PCM_COV_REFERENCE : the reference's lines: marginals from the chain start (buildTrajectory, M_0 = first), and
 *                           Ad(r^-1) M_i Ad(r^-1)^T + M_j for the pose between i and j, which treats two correlated marginals as
 *                           independent and grows with the distance from the start;
 *   MRS_PCM_COV_NONE      : back to the plain test. */
#define MRS_PCM_COV_NONE 0
#define MRS_PCM_COV_SPAN 1
#define MRS_PCM_COV_REFERENCE 2
/* After mrs_pcm_set_trajectories (which resets the mode to NONE); clears the loops.  h_QA double [na - 1][6][6] and h_QB [nb - 1][6][6]: the
 * covariance of each odometry step X_m^-1 X_m+1; NULL: FIXED_COVARIANCE (graph_types.h:79-85) per step, and NULL is required for a
 * trajectory of one pose.  h_first double [6][6]: the covariance of the first pose of either trajectory (REFERENCE only); NULL:
 * FIXED_COVARIANCE.  A bad mode, an entry that is not finite or a matrix that is not positive definite: MRS_ERR_ARG, nothing changes. */
int mrs_pcm_set_covariances(mrs_pcm* pcm, int32_t mode, const double* h_QA, const double* h_QB, const double* h_first);
/* mrs_pcm_add_loops with a covariance per loop, h_C double [n][6][6]; NULL (or plain mrs_pcm_add_loops on a handle with covariances):
 * FIXED_COVARIANCE each.  h_C on a handle in mode NONE, an entry that is not finite or a matrix that is not positive definite:
 * MRS_ERR_ARG, nothing is added. */
int mrs_pcm_add_loops_cov(mrs_pcm* pcm, const int32_t* h_ia, const int32_t* h_kb, const double* h_Z, const double* h_C, int32_t n);
/* One pair recomputed in one host thread: h_xi double [6] = Logmap of the cycle pose of (min, max), h_cov double [6][6] = Sigma_E (the
 * identity in mode NONE), h_d = the compared quantity.  u == v or a loop that does not exist: MRS_ERR_ARG. */
int mrs_pcm_get_pair(mrs_pcm* pcm, int32_t u, int32_t v, double* h_xi, double* h_cov, double* h_d);

/* ------------------------------------------------------------------------------------
 * Mapping-side DiSCO matcher
 * ---------------------------------------------------------------------------------- */

/* GlobalManager::calcRelOri(newDiSCO, oldDiSCO) (Mapping/src/global_manager/src/global_manager.cpp:2719-2762),
 * literal including its quirks (non-conjugate cross term, no normalisation, unshifted argmax):
 * d_a, d_b interleaved complex64 [n_pairs][height][width] -> d_rel_angle_deg float[n_pairs]
 * = (argmax(real(IFFT2_double(cross))) % width) * 3.0. */
int mrs_disco_rel_ori_literal(mrs_ctx* ctx, const float* d_a, const float* d_b, int32_t n_pairs, int32_t height,
                              int32_t width, float* d_rel_angle_deg, mrs_stream stream);

/* Nearest DiSCO signature by squared L2 distance: replaces the kd-tree query over the 1024-d signatures
 * (global_manager.cpp:993-1188, src/kdtree.cpp; LoopDetection twin: sklearn KDTree k=1 at
 * disco_ros/main.py:284-285).  d_query float[n_query][dim], d_db float[n_db][dim]. */
int mrs_signature_search(mrs_ctx* ctx, const float* d_query, int32_t n_query, const float* d_db, int32_t n_db, int32_t dim,
                         int32_t* d_index, float* d_dist2, mrs_stream stream);

/* The k nearest signatures per query, ascending by squared distance (ties: lower index first): what
 * kdtree_knn_search(kdtree, query, NUM_CANDIDATES_FROM_TREE) + kdtree_knn_result return (global_manager.cpp:1002-1007,
 * src/kdtree.cpp:535-586; the reference reports sqrt of these distances and walks the list from entry 1, entry 0 being
 * the query's own descriptor, global_manager.cpp:1136-1139).  1 <= k <= 32; d_index / d_dist2 are [n_query][k], rows past
 * the database size hold -1 / +inf. */
int mrs_signature_knn(mrs_ctx* ctx, const float* d_query, int32_t n_query, const float* d_db, int32_t n_db, int32_t dim, int32_t k,
                      int32_t* d_index, float* d_dist2, mrs_stream stream);

/* ------------------------------------------------------------------------------------
 * Elevation mapping: the nine functions of the reference's libgpu.so
 * (Mapping/src/elevation_mapping_periodical/elevation_mapping/cuda/gpu_process.cu:938-1312; declared by hand
 * in elevation_mapping/src/ElevationMapping.cpp:44-50 and src/sensor_processors/SensorProcessorBase.cpp:34).
 * Same argument meaning, host arrays in/out like the reference; Eigen arguments become plain floats
 * (row-major 4x4 / 3x3, 3-vectors); the map state lives in a handle instead of __device__ globals.
 * ---------------------------------------------------------------------------------- */
typedef struct mrs_elev_map mrs_elev_map;

/* Init_GPU_elevationmap(length, resolution, mahalanobisDistanceThreshold, obstacle_threshold) */
int mrs_elev_create(mrs_ctx* ctx, int32_t length, float resolution, float mahalanobis_threshold, float obstacle_threshold,
                    mrs_elev_map** out);
int mrs_elev_destroy(mrs_elev_map* m);
/* Move(current_Position[3], resolution, length, Central_coordinate[2], Start_indice[2], alignedPositionShift[2]).
 * A shift of a whole map length or more clears the map, in either direction (the reference is undefined for -length and
 * below).  Move, Map_optmove and Map_closeloop return MRS_ERR_ARG and change nothing when a position is not finite or lies
 * 2^30 cells or more from the map centre. */
int mrs_elev_move(mrs_elev_map* m, const float* h_position3, float* h_central2, int32_t* h_start2, float* h_aligned_shift2);
/* Process_points(map_index, point_x/y/z (read only: the reference never copies its device copy back), point_var, point_x/y/z_ts, transform, point_num, thresholds,
 * sensor model, sensorJacobian, rotationVariance, C_SB_transpose, P_mul_C_BM_transpose, B_r_BS_skew) */
int mrs_elev_process_points(mrs_elev_map* m, int32_t n, const float* h_x, const float* h_y, const float* h_z, const float* h_transform16,
                            double relative_lower_threshold, double relative_upper_threshold, float min_r, float beam_a,
                            float beam_c, const float* h_sensorJacobian3, const float* h_rotationVariance9,
                            const float* h_C_SB_transpose9, const float* h_P_mul_C_BM_transpose3, const float* h_B_r_BS_skew9,
                            int32_t* h_map_index, float* h_var, float* h_x_ts, float* h_y_ts, float* h_z_ts);
/* Fuse(length, point_num, point_index, colorR/G/B, intensity, height, var) */
int mrs_elev_fuse(mrs_elev_map* m, int32_t n, const int32_t* h_index, const int32_t* h_colorR, const int32_t* h_colorG,
                  const int32_t* h_colorB, const float* h_intensity, const float* h_height, const float* h_var);
/* Mapvar_update(length, var_update) */
int mrs_elev_mapvar_update(mrs_elev_map* m, float var_update);
/* Map_feature(length, elevation, var, colorR/G/B, rough, slope, traver, intensity): float/int32 [length*length] each */
int mrs_elev_map_feature(mrs_elev_map* m, float* h_elevation, float* h_var, int32_t* h_colorR, int32_t* h_colorG,
                         int32_t* h_colorB, float* h_rough, float* h_slope, float* h_traver, float* h_intensity);
/* Raytracing(length) */
int mrs_elev_raytracing(mrs_elev_map* m);
/* Map_optmove(opt_p[2], height_update, resolution, length, opt_alignedPosition[2]) */
int mrs_elev_map_optmove(mrs_elev_map* m, const float* h_opt_p2, float height_update, float* h_aligned2);
/* Map_closeloop(update_position[2], height_update, length, resolution) */
int mrs_elev_map_closeloop(mrs_elev_map* m, const float* h_update_position2, float height_update);
/* state readback for tests / debugging: which = 0 lowest, 1 elevation, 2 variance, 3 intensity, 4 traversability */
int mrs_elev_get_layer(mrs_elev_map* m, int32_t which, float* h_out);
int mrs_elev_get_frame(mrs_elev_map* m, float* h_central2, int32_t* h_start2);

/* ------------------------------------------------------------------------------------
 * Globally consistent elevation map: the submap stack of
 * ElevationMapping::updateLocalMap (elevation_mapping/src/ElevationMapping.cpp:653-815), its correction in updateGlobalMap
 * (:821-962), the elevation branch of GlobalManager::composeGlobalMap (global_manager.cpp:2133-2152) and
 * PointMapLayer::updateBounds (pointMap_layer.cpp:100-135).
 * A cell record is ten 32-bit values: float x, y, z (the elevation), var; int32 r, g, b, frontier; float intensity, travers.
 * Records go in and come out as [n][10] words, from host memory (h_*) or device memory (d_*): pass exactly one of the two.
 * Every call is blocking and works on the legacy default stream.  One caller at a time per handle.
 * ---------------------------------------------------------------------------------- */
typedef struct mrs_gem mrs_gem;

#define MRS_GEM_WEIGHTED 0     /* z = (vn^2 zo + vo^2 zn) / (vo^2 + vn^2), var = vo^2 vn^2 / (vo^2 + vn^2): the default, a named fix */
#define MRS_GEM_AS_WRITTEN 1   /* the reference's expressions with C precedence (ElevationMapping.cpp:913-914) */
#define MRS_GEM_MAX_SUBMAPS 4096

/* resolution > 0: the cell size of the key k = ceil((double)v / resolution); radius (the reference's 15) and min_neighbours (its 3: a
 * centre submap fuses only when its radius search returns at least that many submaps, itself included) steer mrs_gem_update_global. */
int mrs_gem_create(mrs_ctx* ctx, double resolution, int32_t rule, float radius, int32_t min_neighbours, mrs_gem** out);
int mrs_gem_destroy(mrs_gem* gem);
/* Inserts n records into the open submap, keyed by the bit patterns of (x, y) (so -0.0 and 0.0 are different keys): a key met again
 * replaces the stored record, within a call and across calls, and keeps its place in the order of first insertion. */
int mrs_gem_append_cells(mrs_gem* gem, const void* h_cells, const void* d_cells, int64_t n);
/* The same for the records that pass the window predicate of ElevationMapping.cpp:770-779, evaluated in float: elevation != -10 and
 * the eight clauses on the signs of h_shift2 and the position against h_current2 -+ length * resolution / 2. */
int mrs_gem_append_leaving(mrs_gem* gem, const void* h_cells, const void* d_cells, int64_t n, const float* h_current2, const float* h_shift2,
                           int32_t length, float resolution);
/* The open submap's records with elevation != -10 become the next submap, in ascending order of first insertion, with pose float
 * [4][4] row-major and centre (cx, cy); the open submap is empty afterwards.  More than MRS_GEM_MAX_SUBMAPS: MRS_ERR_UNSUPPORTED. */
int mrs_gem_close_submap(mrs_gem* gem, const float* h_pose16, const float* h_centre2);
/* any of the three may be NULL: closed submaps, records in them, records appended to the open submap (before de-duplication) */
int mrs_gem_count(mrs_gem* gem, int32_t* h_submaps, int64_t* h_cells, int64_t* h_open);
/* Submap `index`: its record count in h_n, optionally its records (capacity in records), its pose [16] and its centre [2]. */
int mrs_gem_get_submap(mrs_gem* gem, int32_t index, void* h_cells, void* d_cells, int64_t capacity, int64_t* h_n, float* h_pose16,
                       float* h_centre2);
/* updateGlobalMap with h_opt_poses float [n_poses][4][4]: K = min(n_poses, submaps); submaps 1 .. K - 1 are moved by
 * opt[i] * inverse(pose[i]) and take opt[i] as their pose; then, for every centre submap in index order, each neighbour within the
 * radius is fused into it cell by cell (DESIGN.md 4.19 has the exact order and arithmetic).  All device memory the call needs is
 * allocated before the first record or pose is changed: a failed allocation leaves the store as it was.  A runtime error after that
 * point (a failed launch or copy) leaves the store undefined: destroy it. */
int mrs_gem_update_global(mrs_gem* gem, const float* h_opt_poses, int32_t n_poses);
/* of the last mrs_gem_update_global: records dropped for a non-finite position or a key outside |k| < 2^23, and cells fused (one count
 * per matched key and pair) */
int mrs_gem_stats(mrs_gem* gem, int64_t* h_dropped, int64_t* h_matched);
/* all submaps concatenated in index order (composingGlobalMap, ElevationMapping.cpp:501-509); h_n alone when both outputs are NULL */
int mrs_gem_compose(mrs_gem* gem, void* h_cells, void* d_cells, int64_t capacity, int64_t* h_n);
/* The elevation branch of GlobalManager::composeGlobalMap: submap j of robot r moved by h_poses (float [sum of submaps][4][4], in (robot,
 * submap) order), then the robots' local maps (h_local_cells or d_local_cells, at most one of the two; records h_local_offsets[r] ..
 * h_local_offsets[r + 1]; all three may be NULL) moved by h_refs float [n_robots][4][4].  merge_cells != 0 places one grid of `resolution` over the concatenation and folds records of equal
 * key left to right with `rule`: one record per cell, in key order.  h_n: the record count (with both outputs NULL: an upper bound to
 * size them by); h_dropped (optional): records without a key, which merge_cells leaves out.  The stores are only read: an error leaves
 * them as they were (the caller's output may be partly written). */
int mrs_gem_compose_robots(mrs_ctx* ctx, mrs_gem* const* stores, int32_t n_robots, const float* h_poses, const void* h_local_cells,
                           const void* d_local_cells, const int64_t* h_local_offsets, const float* h_refs, int32_t merge_cells, int32_t rule,
                           double resolution, void* h_cells, void* d_cells, int64_t capacity, int64_t* h_n, int64_t* h_dropped);
/* PointMapLayer::updateBounds: uint8 grid [size_y][size_x], 255 where no point fell; a point sets its cell to 254 if z != -10, z != 10,
 * travers != -10 and (thresh_type 0: travers < thresh; 1: z > thresh), else to 0; the last point in input order wins. */
int mrs_gem_costmap(mrs_ctx* ctx, const void* h_cloud, const void* d_cloud, int64_t n, double origin_x, double origin_y, int32_t size_x, int32_t size_y,
                    double resolution, int32_t thresh_type, double thresh, uint8_t* h_grid, uint8_t* d_grid);

/* ------------------------------------------------------------------------------------
 * FPFH: all neighbours within a radius as CSR rows, SPFH of every point, FPFH of
 * keypoints (RING_ros/FPFH.py:33-105) and ISS keypoints.  Everywhere: d_points float [N][stride_floats], xyz first, the clouds of a
 * ragged batch packed one after the other; d_offsets / h_offsets int64 [batch + 1], device and host copies of the same offsets,
 * offsets[0] = 0 and N = offsets[batch] < 2^31 - 1; batch in 1 .. 65535.  Rows are CSR in the caller's point order: d_row_start int64
 * [N + 1], d_index int32 [total] of CLOUD-LOCAL indices.  Every kernel that reads rows skips an entry outside its cloud and clamps the
 * row bounds to [0, total]: rows from anywhere cannot make it read out of bounds.
 * ---------------------------------------------------------------------------------- */
#define MRS_FPFH_MAX_BINS 32

/* Step 1 of the radius search: d_row_start [N + 1] and *h_total = row_start[N].  Row i holds every j != i of the same cloud with
 * ((dx dx + dy dy) + dz dz) <= radius radius, all in fp64 on the float32 coordinates widened (exact differences); coincident points
 * are members, a point with a NaN coordinate is nobody's neighbour.  radius > 0 and finite.  MRS_ERR_UNSUPPORTED when the total
 * exceeds 2^31 - 1.  Blocking (one host synchronisation for the total). */
int mrs_radius_count(mrs_ctx* ctx, const float* d_points, int32_t stride_floats, const int64_t* d_offsets, const int64_t* h_offsets,
                     int32_t batch, double radius, int64_t* d_row_start, int64_t* h_total, mrs_stream stream);
/* Step 2: d_index [total], every row ascending, for the d_row_start of step 1 with the same points, offsets and radius.  Enqueued. */
int mrs_radius_fill(mrs_ctx* ctx, const float* d_points, int32_t stride_floats, const int64_t* d_offsets, const int64_t* h_offsets,
                    int32_t batch, double radius, const int64_t* d_row_start, int64_t total, int32_t* d_index, mrs_stream stream);

/* SPFH of every point: d_normals float [N][3]; bins in 1 .. MRS_FPFH_MAX_BINS; d_counts int32 [N][3 bins] (optional), d_spfh double
 * [N][3 bins]: the alpha, phi and theta histograms over [-1, 1], [-1, 1], [-pi, pi] (np.histogram's rule), each divided by its own sum
 * (zeros when that is 0).  Entry i of row i and a neighbour at distance 0 are skipped.  Enqueued. */
int mrs_fpfh_spfh(mrs_ctx* ctx, const float* d_points, int32_t stride_floats, const float* d_normals, const int64_t* d_offsets,
                  int32_t batch, int64_t n, const int64_t* d_row_start, const int32_t* d_index, int64_t total, int32_t bins,
                  int32_t* d_counts, double* d_spfh, mrs_stream stream);
/* The same on rows the caller made (sklearn's lists: the point itself may be in its row, order is free).  Blocking: an entry outside
 * its cloud or row bounds outside [0, total] are MRS_ERR_ARG (the outputs are then computed without those entries). */
int mrs_fpfh_spfh_from_neighbors(mrs_ctx* ctx, const float* d_points, int32_t stride_floats, const float* d_normals,
                                 const int64_t* d_offsets, int32_t batch, int64_t n, const int64_t* d_row_start, const int32_t* d_index,
                                 int64_t total, int32_t bins, int32_t* d_counts, double* d_spfh, mrs_stream stream);
/* FPFH of K keypoints (d_keypoints int64 [K], packed point indices; NULL: K = n, every point): d_fpfh double [K][3 bins] =
 * f / |f|, f = spfh_i + (1 / k) sum_j spfh_j / |p_j - p_i| over the k kept entries of row i IN ROW ORDER (ascending for rows of
 * mrs_radius_fill); zeros when k = 0 or |f| = 0 or the keypoint index is outside [0, n).  Enqueued. */
int mrs_fpfh_describe(mrs_ctx* ctx, const float* d_points, int32_t stride_floats, const int64_t* d_offsets, int32_t batch, int64_t n,
                      const int64_t* d_row_start, const int32_t* d_index, int64_t total, int32_t bins, const double* d_spfh,
                      const int64_t* d_keypoints, int64_t n_keypoints, double* d_fpfh, mrs_stream stream);

/* ISS saliency of every point from its rows at the salient radius plus the point itself: 0 with fewer than min_neighbors members,
 * else the smallest eigenvalue l3 of the members' fp64 covariance (about their mean, divided by their number) when
 * l2 < gamma21 l1 and l3 < gamma32 l2, else 0.  d_saliency double [N].  Enqueued. */
int mrs_iss_saliency(mrs_ctx* ctx, const float* d_points, int32_t stride_floats, const int64_t* d_offsets, int32_t batch, int64_t n,
                     const int64_t* d_row_start, const int32_t* d_index, int64_t total, int32_t min_neighbors, double gamma21,
                     double gamma32, double* d_saliency, mrs_stream stream);
/* d_keep uint8 [N] = 1 iff saliency_i > 0 and, for every j of row i (rows at the non-maximum radius), saliency_i > saliency_j, or
 * they are equal and i < j.  Enqueued. */
int mrs_iss_nonmax(mrs_ctx* ctx, const int64_t* d_offsets, int32_t batch, int64_t n, const int64_t* d_row_start, const int32_t* d_index,
                   int64_t total, const double* d_saliency, uint8_t* d_keep, mrs_stream stream);

/* ------------------------------------------------------------------------------------
 * RANSAC pose from point correspondences: per pair of a ragged batch, `hypotheses`
 * seeded triples, pre-rejected by edge length and collinearity, fitted (Kabsch), scored by their integer inlier count over all
 * correspondences of the pair, the best one (ties to the lowest hypothesis) refitted on its inliers.  All arithmetic in fp64 on the
 * widened float32 coordinates; results do not depend on the batch a pair is in or on the call.
 * ---------------------------------------------------------------------------------- */
#define MRS_RANSAC_MAX_HYPOTHESES 65536
#define MRS_RANSAC_MAX_REFINE 16

typedef struct mrs_ransac_params {
    int32_t hypotheses;       /* 1 .. MRS_RANSAC_MAX_HYPOTHESES triples per pair */
    int32_t refine_iters;     /* 0 .. MRS_RANSAC_MAX_REFINE refits on the inlier set */
    double max_distance;      /* inlier iff |R p + t - q|^2 <= max_distance^2; finite, > 0 */
    double edge_similarity;   /* in [0, 1]: a triple needs dp >= s^2 dq and dq >= s^2 dp on every edge; 0 leaves only dp, dq > 0 */
    double min_sin2;          /* in [0, 1): a triple needs |e1 x e2|^2 > min_sin2 |e1|^2 |e2|^2 on both sides */
} mrs_ransac_params;

/* d_src / d_dst float [total][stride_floats], xyz first: row m of d_src corresponds to row m of d_dst; d_offsets / h_offsets int64
 * [n_pairs + 1], device and host copies of the same offsets, offsets[0] = 0, ascending, a pair's size below 2^31 - 1; n_pairs in
 * 0 .. 65535; h_seeds one seed per pair.  d_T double [n_pairs][16] row-major; d_info int32 [n_pairs][4] = {inliers, best hypothesis,
 * valid hypotheses, refits done}; d_mask uint8 [total] (may be NULL): 1 for the inliers of the returned pose.  A pair with fewer than 3
 * correspondences or without a valid hypothesis gets the identity, {0, -1, valid, 0} and a zero mask.  A correspondence with a
 * non-finite coordinate is never an inlier and rejects every triple that holds it.  MRS_ERR_ARG before any launch, nothing written,
 * for a null pointer or a parameter outside its range.  Enqueued: one chain on `stream`, no host synchronisation. */
int mrs_ransac_pose_batch(mrs_ctx* ctx, const float* d_src, const float* d_dst, int32_t stride_floats, const int64_t* d_offsets,
                          const int64_t* h_offsets, int32_t n_pairs, const uint64_t* h_seeds, const mrs_ransac_params* params,
                          double* d_T, int32_t* d_info, uint8_t* d_mask, mrs_stream stream);
/* The same call with the times of its three stages between events (for measurements): h_stage_ms float [3] = milliseconds of the models
 * (draw, pre-rejection, fit, compaction), the scoring and the refit.  Blocking. */
int mrs_ransac_pose_batch_profile(mrs_ctx* ctx, const float* d_src, const float* d_dst, int32_t stride_floats, const int64_t* d_offsets,
                                  const int64_t* h_offsets, int32_t n_pairs, const uint64_t* h_seeds, const mrs_ransac_params* params,
                                  double* d_T, int32_t* d_info, uint8_t* d_mask, float* h_stage_ms, mrs_stream stream);

/* ------------------------------------------------------------------------------------
 * Pose-graph optimisation: what evaluation_utils::centralizedGNEstimation computes
 * (Mapping/src/global_manager/src/distributed_mapper/evaluation_utils.cpp:273-329, called at global_manager.cpp:1354): the rotations by
 * chordal relaxation, then Gauss-Newton on BetweenChordalFactor errors (between_chordal_factor.h:97-144) with unit weights and pose 0
 * held at its initial value.  All arithmetic is fp64.  The graph is `nr` odometry chains, poses numbered chain after chain, plus loop
 * factors between any two poses.  Host arrays in and out; every call is blocking and works on the legacy default stream.  One caller
 * at a time per handle.  Results are the same bits from run to run and do not depend on how the loops were split over calls.
 * ---------------------------------------------------------------------------------- */
typedef struct mrs_pgo mrs_pgo;

#define MRS_PGO_MAX_CHAINS 16
#define MRS_PGO_MAX_POSES 65536
#define MRS_PGO_MAX_LOOPS 8192
/* most separators of the Gauss-Newton system: the poses a loop touches (pose 0 apart) and the cut poses that bound a segment's length */
#define MRS_PGO_MAX_SEPARATORS 1024
/* longest run of poses one segment walk eliminates unless mrs_pgo_set_segment_length says otherwise (0: unbounded) */
#define MRS_PGO_DEFAULT_SEGMENT_LENGTH 64
/* panel width of the dense Cholesky of the reduced system (the tests place their reduced orders around its multiples) */
#define MRS_PGO_PANEL_WIDTH 24
#define MRS_PGO_DEFAULT_MAX_ITERATIONS 200
/* doubles of mrs_pgo_optimize's h_info: iterations done, converged (0 / 1), the last max|delta|, 0.5 sum |e|^2 at the stage-1 values and
 * at the result, the separator count */
#define MRS_PGO_INFO_DOUBLES 6

/* nr in 1 .. MRS_PGO_MAX_CHAINS chains of h_chain_lengths[r] >= 1 poses, MRS_PGO_MAX_POSES in all at most (more: MRS_ERR_UNSUPPORTED) */
int mrs_pgo_create(mrs_ctx* ctx, int32_t nr, const int32_t* h_chain_lengths, mrs_pgo** out);
int mrs_pgo_destroy(mrs_pgo* pgo);
/* The odometry factors, chain after chain: h_Z double [n][4][4] row-major, the measured pose of pose p + 1 in the frame of pose p.
 * n must be (poses - nr), and every entry finite: MRS_ERR_ARG otherwise, the handle unchanged. */
int mrs_pgo_set_odometry(mrs_pgo* pgo, const double* h_Z, int32_t n);
/* Appends n loop factors (h_i[u], h_j[u], h_Z[u]): h_Z double [n][4][4] is the measured pose of j in the frame of i.  Any two different
 * poses, in either order; repeated pairs, consecutive poses and pose 0 are allowed.  i == j, an index outside the graph or a pose that is
 * not finite: MRS_ERR_ARG.  More than MRS_PGO_MAX_LOOPS loops or MRS_PGO_MAX_SEPARATORS separators: MRS_ERR_UNSUPPORTED.  Nothing is
 * added then. */
int mrs_pgo_add_loops(mrs_pgo* pgo, const int32_t* h_i, const int32_t* h_j, const double* h_Z, int32_t n);
int mrs_pgo_clear_loops(mrs_pgo* pgo);
/* the number of loop factors */
int mrs_pgo_count(mrs_pgo* pgo, int32_t* h_count);
/* The prior on pose 0, double [4][4] (the identity until set): stage 1 ties pose 0's rotation to its rotation; the translation of
 * pose 0 is zero whatever it says, as pose3WithZeroTranslation leaves it. */
int mrs_pgo_set_prior(mrs_pgo* pgo, const double* h_T);
/* No run of poses between two separators is longer than `length` (0: unbounded).  Negative: MRS_ERR_ARG; a length that needs more than
 * MRS_PGO_MAX_SEPARATORS separators: MRS_ERR_UNSUPPORTED, the setting unchanged.  A setting's results do not depend on earlier ones. */
int mrs_pgo_set_segment_length(mrs_pgo* pgo, int32_t length);
/* Stage 1 alone: h_T double [poses][4][4] receives the relaxed rotations projected to SO(3), with zero translations.  A chain that no
 * loop factors connect to chain 0, or odometry not set: MRS_ERR_ARG.  A pivot block that is not positive definite:
 * MRS_ERR_NOT_CONVERGED with the pose in mrs_last_error(). */
int mrs_pgo_initialize(mrs_pgo* pgo, double* h_T);
/* Both stages: Gauss-Newton from the stage-1 values until max|delta| < eps or max_iterations steps are done (eps = 0: exactly
 * max_iterations, what the reference does with 200; max_iterations = 1: centralizedEstimation).  eps >= 0, max_iterations >= 1.
 * h_T double [poses][4][4]; h_info double [MRS_PGO_INFO_DOUBLES].  Errors as mrs_pgo_initialize; the handle's graph is never changed. */
int mrs_pgo_optimize(mrs_pgo* pgo, double eps, int32_t max_iterations, double* h_T, double* h_info);
/* The last mrs_pgo_optimize between events (for measurements): h_ms float [6] = milliseconds of stage 1, and of the linearisation with
 * the gather, the segment walks (both directions), the assembly, the dense factorisation with its solves, and the retraction, each
 * summed over the iterations.  Zeros unless MRS_DEV=1 and MRS_PGO_TIMING=1 were set when the call ran. */
int mrs_pgo_last_stage_ms(mrs_pgo* pgo, float* h_ms);

/* ---- per-factor noise, Levenberg-Marquardt step control and robust kernels on the loop factors ----
 * A covariance is double [6][6] in gtsam's Pose3 order, rotation xyz then translation xyz, and is converted as
 * evaluation_utils::convertToChordalNoise converts it (evaluation_utils.cpp:333-366, the reference's use_between_noise = true): weight
 * 1 / max(C00, C11, C22) on the nine rotation rows, information Rhat (C[3:6][3:6] + 0.01 I)^-1 Rhat^T on the translation rows, Rhat the
 * stage-1 rotation of the factor's first pose (i as given), fixed for a call; the rotation-translation blocks are ignored.  Stage 1 is
 * not weighted.  A factor without a covariance keeps the unit model.  Refused with MRS_ERR_ARG, the handle unchanged: an entry that is
 * not finite, max(C00, C11, C22) <= 0, a C[3:6][3:6] + 0.01 I that is not positive definite.  Both optimisers honour the noise. */
int mrs_pgo_set_odometry_noise(mrs_pgo* pgo, const double* h_C, int32_t n);     /* n = the number of odometry factors; NULL, 0 clears */
/* mrs_pgo_add_loops with a covariance per loop, h_C double [n][6][6] */
int mrs_pgo_add_loops_noise(mrs_pgo* pgo, const int32_t* h_i, const int32_t* h_j, const double* h_Z, const double* h_C, int32_t n);

#define MRS_PGO_KERNEL_NONE 0
#define MRS_PGO_KERNEL_HUBER 1
#define MRS_PGO_KERNEL_CAUCHY 2
#define MRS_PGO_KERNEL_GEMAN_MCCLURE 3
/* A robust kernel on every loop factor, with r = sqrt(e^T L e) over the factor's 12 rows: Huber w = 1 (r <= k) or k / r; Cauchy
 * w = k^2 / (k^2 + r^2); Geman-McClure w = (k^2 / (k^2 + r^2))^2.  k must be positive and finite.  A kernel works only under
 * mrs_pgo_optimize_lm; mrs_pgo_optimize on a handle with one returns MRS_ERR_ARG.  Not pinned to the reference: its chordal conversion
 * cannot carry a Robust model. */
int mrs_pgo_set_loop_kernel(mrs_pgo* pgo, int32_t kernel, double k);

/* Levenberg-Marquardt's constants: lambda starts at gtsam's lambdaInitial and stays within [MIN, MAX]; a step whose predicted decrease
 * is at most PRED_FLOOR times the cost is below what an fp64 cost resolves: it is accepted and its gain counts as 1 */
#define MRS_PGO_LM_LAMBDA_INITIAL 1e-5
#define MRS_PGO_LM_LAMBDA_MIN 1e-12
#define MRS_PGO_LM_LAMBDA_MAX 1e12
#define MRS_PGO_LM_PRED_FLOOR 1e-10
/* doubles of mrs_pgo_optimize_lm's h_info: solves done, steps accepted, converged (0 / 1), the last accepted max|delta|, the cost at the
 * stage-1 values and at the result (sum 0.5 r^2 over the odometry factors + sum rho(r) over the loops), the separator count, the final
 * lambda */
#define MRS_PGO_LM_INFO_DOUBLES 8
/* Both stages with step control.  Solve 1 is the Gauss-Newton step (lambda = 0, kernel weights 1), accepted whatever it does to the
 * cost: the linear solve for the translations from t = 0.  Later solves: (H + lambda diag H) delta = g, the loops' blocks scaled by the
 * kernel's weight at the current poses; pred = 0.5 delta^T (lambda diag(H) delta + g), rho = (c - c_new) / pred (1 for a step below
 * the floor); accepted iff
 * c_new <= c or pred <= PRED_FLOOR c; then lambda *= max(1/3, 1 - (2 rho - 1)^3) and nu = 2, else lambda *= nu, nu *= 2 and the poses
 * are restored.  Stops at an accepted step with max|delta| < eps or after max_solves solves (rejected ones count).  Errors as
 * mrs_pgo_optimize. */
int mrs_pgo_optimize_lm(mrs_pgo* pgo, double eps, int32_t max_solves, double* h_T, double* h_info);
/* The kernel's weight and e^T L e of every loop at the last result of either optimiser (weights 1 without a kernel): h_w, h_r2 double
 * [capacity], capacity >= the number of loops.  MRS_ERR_ARG when the graph changed since, or nothing was optimised. */
int mrs_pgo_get_loop_state(mrs_pgo* pgo, double* h_w, double* h_r2, int32_t capacity);

/* ---- a sparse elimination tier in front of the dense Cholesky of the reduced system ----
 * DENSE (the default) factors all separators densely and holds MRS_PGO_MAX_SEPARATORS of them.  SPARSE first eliminates separators of
 * low degree in the block graph of the reduced system, level after level of pairwise non-adjacent ones, until at most `dense_limit` are
 * left for the dense Cholesky; its size limit is a budget of blocks (a column's diagonal block and its blocks below it). */
#define MRS_PGO_SOLVER_DENSE 0
#define MRS_PGO_SOLVER_SPARSE 1
/* a level takes the separators whose degree is at most the smallest degree plus this slack */
#define MRS_PGO_SPARSE_DEGREE_SLACK 1
/* the default budget of blocks of the sparse columns, per stage */
#define MRS_PGO_MAX_SPARSE_BLOCKS 1048576
/* entries of mrs_pgo_get_solver_stats' h_stats: separators, eliminated, core, levels, blocks = sum (d + 1),
 * block updates = sum d (d + 1) / 2, the largest degree d, the solver in force */
#define MRS_PGO_SOLVER_STATS 8
/* solver: MRS_PGO_SOLVER_*.  dense_limit in [0, MRS_PGO_MAX_SEPARATORS], -1: MRS_PGO_MAX_SEPARATORS; max_blocks > 0, 0:
 * MRS_PGO_MAX_SPARSE_BLOCKS; both are ignored under DENSE.  Anything else: MRS_ERR_ARG.  A graph that needs more blocks than max_blocks
 * under SPARSE, or has more than MRS_PGO_MAX_SEPARATORS separators under DENSE: MRS_ERR_UNSUPPORTED.  The handle is unchanged on
 * refusal.  Under SPARSE mrs_pgo_add_loops, mrs_pgo_add_loops_noise and mrs_pgo_set_segment_length check the block budget instead of the
 * separator count.  With no more than dense_limit separators nothing is eliminated and the results are DENSE's bit for bit. */
int mrs_pgo_set_solver(mrs_pgo* pgo, int32_t solver, int32_t dense_limit, int32_t max_blocks);
/* The symbolic phase of a stage (1: rotations, 2: Gauss-Newton) for the graph as it stands: h_stats int64 [MRS_PGO_SOLVER_STATS].
 * Host work only.  Under DENSE: eliminated, levels, blocks, updates and the degree are 0 and core is the separator count. */
int mrs_pgo_get_solver_stats(mrs_pgo* pgo, int32_t stage, int64_t* h_stats);
/* The sparse tier's share of the last optimisation's `dense factorisation` time (mrs_pgo_last_stage_ms), between events and summed over
 * the solves: h_ms float [2] = milliseconds of the sparse columns with the core's update, and of the columns' way back.  Zeros unless
 * MRS_DEV=1 and MRS_PGO_TIMING=1 were set when the call ran, and when nothing is eliminated. */
int mrs_pgo_last_tier_ms(mrs_pgo* pgo, float* h_ms);

/* ---- marginal covariances of the last result by selected inversion ----
 * H = sum_f w_f J_f^T L_f J_f is the Gauss-Newton information matrix at the poses the last mrs_pgo_optimize / mrs_pgo_optimize_lm left:
 * L_f the factor's information (the unit model without noise), w_f = 1 for odometry factors and the kernel's weight at the result for
 * the loops (what mrs_pgo_get_loop_state returns), lambda = 0 also after Levenberg-Marquardt, pose 0 held.  The marginal of pose p is the
 * 6 x 6 diagonal block of H^-1 (zero for pose 0); the joint marginal of (i, j) is [[S_ii, S_ij], [S_ji, S_jj]].  Everything is fp64 with a
 * fixed order of sums: the same bits from call to call and from a fresh handle. */
#define MRS_PGO_FRAME_CHORDAL 0          /* the optimiser's own tangent: R <- R Exp(d[0:3]), t <- t + d[3:6] */
#define MRS_PGO_FRAME_POSE3 1            /* M S M^T with M = blockdiag(I, R^T) per pose: gtsam's Pose3 local coordinates to first order */
/* the tile of the triangular inverse and of the symmetric product of the reduced system */
#define MRS_PGO_MARGINAL_TILE 32
/* entries of mrs_pgo_compute_marginals' h_info: separators, order of the reduced system, bytes held by the handle for the marginals, 0 */
#define MRS_PGO_MARGINAL_INFO 4
/* Replaces the set of poses that stage 2 treats as separators whether or not a loop touches them (joint marginals are answered between
 * separators); NULL, 0 clears it, which is the default.  Stage 1 never sees the set.  A pose outside the graph or named twice:
 * MRS_ERR_ARG.  More than MRS_PGO_MAX_SEPARATORS separators (under SPARSE: blocks past the budget): MRS_ERR_UNSUPPORTED.  The handle is
 * unchanged on refusal; otherwise the last result is gone, as after mrs_pgo_set_segment_length.  Marking pose 0 changes nothing. */
int mrs_pgo_mark_poses(mrs_pgo* pgo, const int32_t* h_poses, int32_t n);
/* Factors H at the last result again and inverts it on the factor's pattern: the inverse of the reduced system of the separators
 * (8 (6 E)^2 bytes) and two 6 x 6 per pose, owned by the handle until the graph, the marks, the segment length, the solver or the result
 * change.  h_info int64 [MRS_PGO_MARGINAL_INFO] (may be NULL).  Reads the result and does not change it.  MRS_ERR_ARG without a result
 * of the graph as it stands; MRS_ERR_UNSUPPORTED when stage 2's sparse tier eliminated something; MRS_ERR_NOT_CONVERGED with the pose
 * named when a pivot is not positive and finite. */
int mrs_pgo_compute_marginals(mrs_pgo* pgo, int64_t* h_info);
/* h_cov double [n][6][6], symmetric to the bit, of the poses h_poses [n] (NULL: all poses in order, n = the number of poses) in `frame`
 * (MRS_PGO_FRAME_*).  Needs mrs_pgo_compute_marginals of the result as it stands: MRS_ERR_ARG otherwise. */
int mrs_pgo_get_marginals(mrs_pgo* pgo, const int32_t* h_poses, int32_t n, int32_t frame, double* h_cov);
/* h_cov double [n][12][12] of the pairs (h_i[u], h_j[u]).  Answered when both poses are separators of stage 2 or pose 0, or consecutive
 * poses of one chain; any other pair is MRS_ERR_ARG and names the pose to mark, as is i == j.  Nothing is written on refusal. */
int mrs_pgo_get_joint_marginals(mrs_pgo* pgo, const int32_t* h_i, const int32_t* h_j, int32_t n, int32_t frame, double* h_cov);
/* The last mrs_pgo_compute_marginals between events: h_ms float [4] = milliseconds of the factorisation at the result, the triangular
 * inverse, the symmetric product and the segment walk.  Zeros unless MRS_DEV=1 and MRS_PGO_TIMING=1 were set when the call ran. */
int mrs_pgo_last_marginal_ms(mrs_pgo* pgo, float* h_ms);

#ifdef __cplusplus
}
#endif
#endif /* MRSLAM_HIP_H */
