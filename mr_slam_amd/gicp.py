"""Batched GICP over the C ABI (rows G2-G6).  Host logic only; the kernels live in csrc/gicp_device.hpp, their host side in csrc/gicp.hip."""
import ctypes as C

import numpy as np
import torch

from . import _lib


class GicpParams(C.Structure):
    _fields_ = [("k_correspondences", C.c_int32), ("max_iterations", C.c_int32),
                ("lm_max_iterations", C.c_int32), ("force_iterations", C.c_int32),
                ("max_correspondence_distance", C.c_double), ("rotation_epsilon", C.c_double),
                ("transformation_epsilon", C.c_double), ("lm_init_lambda_factor", C.c_double),
                ("voxel_resolution", C.c_double), ("voxel_neighbors", C.c_int32), ("reserved", C.c_int32),
                ("convergence_factor", C.c_double)]


def default_params():
    p = GicpParams()
    _lib.load().mrs_gicp_default_params(C.byref(p))
    return p


class IcpParams(C.Structure):
    _fields_ = [("max_iterations", C.c_int32), ("force_iterations", C.c_int32),
                ("max_correspondence_distance", C.c_double), ("transformation_epsilon", C.c_double),
                ("rotation_epsilon", C.c_double), ("euclidean_fitness_epsilon", C.c_double)]


ICP_STATES = ("NOT_CONVERGED", "ITERATIONS", "TRANSFORM", "ABS_MSE", "REL_MSE", "NO_CORRESPONDENCES")    # PCL's ConvergenceState


def default_icp_params(**kw):
    """pcl::IterativeClosestPoint's defaults, with the given fields replaced"""
    p = IcpParams()
    _lib.load().mrs_icp_default_params(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


class IcpPlaneParams(C.Structure):
    _fields_ = IcpParams._fields_ + [("normal_k", C.c_int32), ("viewpoint", C.c_double * 3)]


ICP_PLANE_STATES = ICP_STATES + ("DEGENERATE",)     # 6: an iteration's 6 x 6 system was rank-deficient


def default_icp_plane_params(**kw):
    """pcl::IterativeClosestPointWithNormals' defaults (normal_k = 15, viewpoint at the origin), with the given fields replaced"""
    p = IcpPlaneParams()
    _lib.load().mrs_icp_plane_default_params(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, (C.c_double * 3)(*v) if k == "viewpoint" else v)
    return p


class PclGicpParams(C.Structure):
    _fields_ = [("max_iterations", C.c_int32), ("max_inner_iterations", C.c_int32), ("force_iterations", C.c_int32),
                ("max_correspondence_distance", C.c_double), ("rotation_epsilon", C.c_double),
                ("transformation_epsilon", C.c_double), ("gradient_tolerance", C.c_double)]


PCL_INNER_ENDS = ("GRADIENT", "LIMIT", "NO_PROGRESS")    # how the inner BFGS of a PCL-style GICP iteration ended


def default_pclgicp_params(**kw):
    """pcl::GeneralizedIterativeClosestPoint's defaults, with the given fields replaced"""
    p = PclGicpParams()
    _lib.load().mrs_pclgicp_default_params(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


_tls = __import__("threading").local()


def _staging(points):
    """thread-local pinned float32 [>= points, 3] staging tensor, grown geometrically"""
    buf = getattr(_tls, "buf", None)
    if buf is None or buf.shape[0] < points:
        cap = max(1 << 16, 1 << int(points - 1).bit_length())
        buf = torch.empty((cap, 3), dtype=torch.float32).pin_memory()
        _tls.buf = buf
    return buf


class GicpBatch(_lib.Handle):
    """n_pairs independent (source, target) registrations advanced together on one GPU."""
    _destroy = "mrs_gicp_batch_destroy"

    def __init__(self, n_pairs, device=0):
        self.n_pairs = int(n_pairs)
        self.device = device
        self._create("mrs_gicp_batch_create", _lib.ctx(device), self.n_pairs)
        self.params = default_params()
        self._n = [None, None]

    def set_params(self, **kw):
        for k, v in kw.items():
            if not hasattr(self.params, k):
                raise AttributeError(k)
            setattr(self.params, k, v)
        _lib.load().mrs_gicp_batch_set_params(self._h, C.byref(self.params))

    def set_search(self, core):
        """1 (default): octree-cell leaves, per-query culling, certified neighbours; 2: without certificates; 3: round-4 kernel for the cold
        pass too; 0: the round-3 wave-shared traversal (A/B, cross-check)."""
        _lib.load().mrs_gicp_batch_set_search(self._h, int(core))

    def _set(self, which, clouds):
        """clouds: list of [n_i, >=3] arrays (host) or a (device tensor [N, s], offsets) tuple."""
        if isinstance(clouds, tuple):
            pts, offs = clouds
            offs = np.ascontiguousarray(offs, dtype=np.int64)
        else:
            # host clouds (what the nodes hand over, float64 [n, 3] from pygicp.downsample): converted to float32 straight INTO a pinned staging
            # buffer (one pass instead of convert + concatenate + a pageable copy) and sent with one asynchronous copy; mrs_gicp_batch_set_clouds
            # synchronises the stream before it returns, so the buffer (one per thread: the callbacks run concurrently) is free again by then
            srcs = [np.asarray(c) for c in clouds]
            offs = np.zeros(len(srcs) + 1, np.int64)
            offs[1:] = np.cumsum([a.shape[0] for a in srcs])
            total = int(offs[-1])
            stage = _staging(total)
            view = stage.numpy()
            for a, lo, hi in zip(srcs, offs[:-1], offs[1:]):
                np.copyto(view[lo:hi], a[:, :3], casting="same_kind")
            pts = torch.empty((total, 3), dtype=torch.float32, device=f"cuda:{self.device}")
            pts.copy_(stage[:total], non_blocking=True)
        assert offs.size == self.n_pairs + 1
        pts = pts.contiguous()
        _lib.load().mrs_gicp_batch_set_clouds(self._h, which, pts, pts.shape[1], offs, _lib.current_stream(self.device))
        self._n[which] = offs

    def set_sources(self, clouds):
        self._set(0, clouds)

    def set_targets(self, clouds):
        self._set(1, clouds)

    def set_sources_from(self, store, ids, store_which=1):
        """Pair i's source := cloud ids[i] of `store` (a GicpBatch used as a submap store: set_targets(unique clouds) +
        compute_covariances(1)).  Sorted points, covariances and boxes are copied on the device, nothing is rebuilt."""
        self._set_from(0, store, ids, store_which)

    def set_targets_from(self, store, ids, store_which=1):
        self._set_from(1, store, ids, store_which)

    def _set_from(self, which, store, ids, store_which):
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        assert ids.size == self.n_pairs
        _lib.load().mrs_gicp_batch_set_clouds_from(self._h, which, store._h, int(store_which), ids, _lib.current_stream(self.device))
        so = store._n[store_which]
        offs = np.zeros(self.n_pairs + 1, np.int64)
        offs[1:] = np.cumsum([so[i + 1] - so[i] for i in ids])
        self._n[which] = offs

    def compute_covariances(self, which, want_knn=False):
        knn = None
        if want_knn:
            knn = torch.empty((int(self._n[which][-1]), self.params.k_correspondences), dtype=torch.int32,
                              device=f"cuda:{self.device}")
        _lib.load().mrs_gicp_batch_compute_covariances(self._h, which, knn, _lib.current_stream(self.device))
        return knn

    def covariances(self, which):
        """[N,3,3] float64 regularised covariances (host)."""
        n = int(self._n[which][-1])
        c6 = np.empty((n, 6), np.float64)
        _lib.load().mrs_gicp_batch_get_covariances(self._h, which, c6)
        out = np.empty((n, 3, 3), np.float64)
        out[:, 0, 0], out[:, 0, 1], out[:, 0, 2] = c6[:, 0], c6[:, 1], c6[:, 2]
        out[:, 1, 0], out[:, 1, 1], out[:, 1, 2] = c6[:, 1], c6[:, 3], c6[:, 4]
        out[:, 2, 0], out[:, 2, 1], out[:, 2, 2] = c6[:, 2], c6[:, 4], c6[:, 5]
        return out

    def voxel_map(self):
        """The targets' voxel map of the voxelised variant (voxel_resolution > 0), built if need be: (pair [V] int32, coord [V,3] int32,
        mean [V,3] float32, count [V] int32, cov [V,3,3] float64), voxels in ascending (pair, x, y, z)."""
        lib, stream = _lib.load(), _lib.current_stream(self.device)
        n = np.zeros(1, np.int32)
        lib.mrs_gicp_batch_get_voxel_map(self._h, n, None, None, None, None, None, stream)
        V = int(n[0])
        pair = np.empty(V, np.int32); coord = np.empty((V, 3), np.int32); mean = np.empty((V, 3), np.float32)
        count = np.empty(V, np.int32); c6 = np.empty((V, 6), np.float64)
        lib.mrs_gicp_batch_get_voxel_map(self._h, n, pair, coord, mean, count, c6, stream)
        return pair, coord, mean, count, c6[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(V, 3, 3)

    def _poses(self, poses):
        return np.ascontiguousarray(np.asarray(poses, dtype=np.float64).reshape(self.n_pairs, 16))

    def _corr_out(self, want_corr):
        """one int32 per source point on the device, for a step's correspondences"""
        return torch.empty(int(self._n[0][-1]), dtype=torch.int32, device=f"cuda:{self.device}") if want_corr else None

    def _align(self, entry, params_ref, guesses, want_state, want_hessian):
        """One of the four mrs_gicp_batch_align* entry points: (handle, [params,] guesses, T, converged, iterations, state or Hessian, stream)."""
        P = self.n_pairs
        T = np.empty((P, 16), np.float64)
        conv = np.empty(P, np.int32)
        its = np.empty(P, np.int32)
        state = np.empty(P, np.int32) if want_state else None
        if want_hessian:
            self.hessian = np.empty((P, 36), np.float64)
        lib = _lib.load()
        args = (self._h,) + (() if params_ref is None else (params_ref,)) + (None if guesses is None else self._poses(guesses), T, conv, its)
        getattr(lib, entry)(*args, self.hessian if want_hessian else state, _lib.current_stream(self.device))
        self.nn_passes = lib.mrs_gicp_batch_last_nn_passes(self._h)
        self.searched_fraction = lib.mrs_gicp_batch_last_searched_fraction(self._h)
        out = (T.reshape(P, 4, 4), conv.astype(bool), its)
        return out + (state,) if want_state else out

    def align(self, guesses=None):
        """Returns (T [P,4,4] float64, converged [P] bool, iterations [P] int32)."""
        return self._align("mrs_gicp_batch_align", None, guesses, False, True)

    def linearize(self, poses, want_corr=False):
        P, poses = self.n_pairs, self._poses(poses)
        H = np.empty((P, 36), np.float64); b = np.empty((P, 6), np.float64); e = np.empty(P, np.float64)
        corr = self._corr_out(want_corr)
        _lib.load().mrs_gicp_batch_linearize(self._h, poses, H, b, e, corr, _lib.current_stream(self.device))
        return e, H.reshape(P, 6, 6), b, (corr.cpu().numpy() if want_corr else None)

    def align_icp(self, guesses=None, **params):
        """Point-to-point ICP (row G9, pcl::IterativeClosestPoint) on the batch's clouds; params: the fields of IcpParams (PCL's defaults
        otherwise).  Returns (T [P,4,4] float64, converged [P] bool, iterations [P] int32, state [P] int32: index into ICP_STATES)."""
        return self._align("mrs_gicp_batch_align_icp", C.byref(default_icp_params(**params)), guesses, True, False)

    def icp_step(self, poses, want_corr=False, **params):
        """One ICP iteration's correspondences, 17 sums and fitted increment at `poses` (mrs_gicp_batch_icp_step).
        Returns (sums [P,17], delta [P,4,4], corr or None)."""
        P, poses = self.n_pairs, self._poses(poses)
        sums = np.empty((P, 17), np.float64); delta = np.empty((P, 16), np.float64)
        corr = self._corr_out(want_corr)
        _lib.load().mrs_gicp_batch_icp_step(self._h, C.byref(default_icp_params(**params)), poses, sums, delta, corr,
                                            _lib.current_stream(self.device))
        return sums, delta.reshape(P, 4, 4), (corr.cpu().numpy() if want_corr else None)

    def icp_profile(self, poses, reps=3, **params):
        """HIP-event duration of the three stages of one ICP iteration, each launched alone at `poses` (mrs_gicp_batch_icp_profile).
        Returns (dict of ms, dict of counts)."""
        poses = self._poses(poses)
        ms = np.zeros(3, np.float32); cnt = np.zeros(2, np.int64)
        _lib.load().mrs_gicp_batch_icp_profile(self._h, C.byref(default_icp_params(**params)), poses, int(reps), ms, cnt,
                                               _lib.current_stream(self.device))
        return ({n: float(v) for n, v in zip(("search", "icp_sums", "icp_update"), ms)},
                {"source_points": int(cnt[0]), "correspondences": int(cnt[1])})

    def compute_normals(self, which, k=15, viewpoint=(0.0, 0.0, 0.0)):
        """Surface normals of side `which` (row G12: pcl::NormalEstimation with setKSearch(k), setViewPoint), kept on the handle."""
        v = np.ascontiguousarray(viewpoint, dtype=np.float64).reshape(3)
        _lib.load().mrs_gicp_batch_compute_normals(self._h, int(which), int(k), v, _lib.current_stream(self.device))

    def normals(self, which):
        """[N,4] float32 (nx, ny, nz, curvature) of the side's points, in the order they were given (host)."""
        out = np.empty((int(self._n[which][-1]), 4), np.float32)
        _lib.load().mrs_gicp_batch_get_normals(self._h, int(which), out)
        return out

    def set_normals(self, which, normals):
        """Normals the caller already has: [N, 3 or more] float32 (host array or device tensor), rows in the order of the side's points;
        a fourth column is kept as the curvature."""
        lib = _lib.load()
        if isinstance(normals, torch.Tensor) and normals.is_cuda:
            nrm = normals.to(torch.float32).contiguous()
            assert nrm.dim() == 2 and nrm.shape[0] == int(self._n[which][-1])
            lib.mrs_gicp_batch_set_normals(self._h, int(which), nrm, nrm.shape[1], _lib.current_stream(self.device))
        else:
            nrm = np.ascontiguousarray(normals, dtype=np.float32)
            assert nrm.ndim == 2 and nrm.shape[0] == int(self._n[which][-1])
            lib.mrs_gicp_batch_set_normals_host(self._h, int(which), nrm, nrm.shape[1])

    def align_icp_plane(self, guesses=None, **params):
        """Point-to-plane ICP (row G12, pcl::IterativeClosestPointWithNormals) on the batch's clouds and the targets' normals (those the
        handle holds, else computed with normal_k and viewpoint); params: the fields of IcpPlaneParams (PCL's defaults otherwise).
        Returns (T [P,4,4] float64, converged [P] bool, iterations [P] int32, state [P] int32: index into ICP_PLANE_STATES)."""
        return self._align("mrs_gicp_batch_align_icp_plane", C.byref(default_icp_plane_params(**params)), guesses, True, False)

    def icp_plane_step(self, poses, want_corr=False, **params):
        """One point-to-plane iteration's correspondences, 29 sums and fitted increment at `poses` (mrs_gicp_batch_icp_plane_step).
        Returns (sums [P,29], delta [P,4,4], state [P] int32, corr or None)."""
        P, poses = self.n_pairs, self._poses(poses)
        sums = np.empty((P, 29), np.float64); delta = np.empty((P, 16), np.float64); state = np.empty(P, np.int32)
        corr = self._corr_out(want_corr)
        _lib.load().mrs_gicp_batch_icp_plane_step(self._h, C.byref(default_icp_plane_params(**params)), poses, sums, delta, state, corr,
                                                  _lib.current_stream(self.device))
        return sums, delta.reshape(P, 4, 4), state, (corr.cpu().numpy() if want_corr else None)

    def icp_plane_profile(self, poses, reps=3, **params):
        """HIP-event duration of the stages of one point-to-plane iteration and of the targets' normals, each launched alone at `poses`
        (mrs_gicp_batch_icp_plane_profile).  Returns (dict of ms, dict of counts)."""
        poses = self._poses(poses)
        ms = np.zeros(4, np.float32); cnt = np.zeros(2, np.int64)
        _lib.load().mrs_gicp_batch_icp_plane_profile(self._h, C.byref(default_icp_plane_params(**params)), poses, int(reps), ms, cnt,
                                                     _lib.current_stream(self.device))
        return ({n: float(v) for n, v in zip(("search", "normals", "icp_plane_sums", "icp_plane_update"), ms)},
                {"source_points": int(cnt[0]), "correspondences": int(cnt[1])})

    def align_pcl(self, guesses=None, **params):
        """PCL-style GICP (row G11, pcl::GeneralizedIterativeClosestPoint) on the batch's clouds and covariances; params: the fields of
        PclGicpParams (PCL's defaults otherwise).  Returns (T [P,4,4] float64, converged [P] bool, iterations [P] int32, state [P] int32:
        index into ICP_STATES)."""
        return self._align("mrs_gicp_batch_align_pcl", C.byref(default_pclgicp_params(**params)), guesses, True, False)

    def pcl_step(self, poses, want_corr=False, **params):
        """One outer iteration of PCL-style GICP at `poses` (mrs_gicp_batch_pcl_step): correspondences, the 74 sums, the inner BFGS.
        Returns (sums [P,74], next pose [P,4,4], inner [P,2] int32: iterations and index into PCL_INNER_ENDS, corr or None)."""
        P, poses = self.n_pairs, self._poses(poses)
        sums = np.empty((P, 74), np.float64); nxt = np.empty((P, 16), np.float64); inner = np.empty((P, 2), np.int32)
        corr = self._corr_out(want_corr)
        _lib.load().mrs_gicp_batch_pcl_step(self._h, C.byref(default_pclgicp_params(**params)), poses, sums, nxt, inner, corr,
                                            _lib.current_stream(self.device))
        return sums, nxt.reshape(P, 4, 4), inner, (corr.cpu().numpy() if want_corr else None)

    def pcl_profile(self, poses, reps=3, **params):
        """HIP-event duration of the three stages of one PCL-style GICP iteration, each launched alone at `poses`
        (mrs_gicp_batch_pcl_profile).  Returns (dict of ms, dict of counts)."""
        poses = self._poses(poses)
        ms = np.zeros(3, np.float32); cnt = np.zeros(2, np.int64)
        _lib.load().mrs_gicp_batch_pcl_profile(self._h, C.byref(default_pclgicp_params(**params)), poses, int(reps), ms, cnt,
                                               _lib.current_stream(self.device))
        return ({n: float(v) for n, v in zip(("search", "pclgicp_sums", "pclgicp_update"), ms)},
                {"source_points": int(cnt[0]), "correspondences": int(cnt[1])})

    def profile(self, poses, reps=3):
        """HIP-event duration of every kernel of one outer iteration, launched alone at `poses` (mrs_gicp_batch_profile).
        Returns (dict of ms, dict of counts)."""
        poses = self._poses(poses)
        ms = np.zeros(8, np.float32); cnt = np.zeros(3, np.int64)
        _lib.load().mrs_gicp_batch_profile(self._h, poses, int(reps), ms, cnt, _lib.current_stream(self.device))
        names = ("linearize", "linearize_error_only", "search_round3_all", "certify", "search_round4_all", "knn_select", "cov_from_knn",
                 "certify_plus_worklist_1mm")
        return {n: float(v) for n, v in zip(names, ms)}, {"source_points": int(cnt[0]), "correspondences": int(cnt[1]), "worklist_queries_1mm": int(cnt[2])}

    def fitness(self, poses, max_range):
        P, poses = self.n_pairs, self._poses(poses)
        out = np.empty(P, np.float64)
        _lib.load().mrs_gicp_batch_fitness(self._h, poses, max_range, out, _lib.current_stream(self.device))
        return out
