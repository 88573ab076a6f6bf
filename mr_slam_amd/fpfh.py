"""FPFH on device tensors (RING_ros/FPFH.py): all neighbours within a radius as CSR rows, the SPFH of every point, the FPFH of keypoints,
ISS keypoints, a nearest-descriptor match, the correspondences it gives and the RANSAC pose from correspondences.

Thin host logic over the C ABI (mrs_radius_*, mrs_fpfh_*, mrs_iss_*, mrs_signature_knn); there is no CPU fallback.  Points are a packed
[N, stride >= 3] float32 device tensor, the clouds of a ragged batch one after the other, with int64 offsets [batch + 1] starting at 0;
normals are [N, 3] float32.  Float32 inputs are widened to float64 before anything is computed.  Rows are (row_start int64 [N + 1], index
int32 [total]) in the caller's point order, every row ascending, CLOUD-LOCAL indices.  The contract, the summation orders and the named
deviations from the reference (a neighbour at distance 0, an empty histogram, a keypoint without neighbours) are in DESIGN.md 4.20; the
RANSAC contract (draw, pre-rejection, scoring, refit) is in DESIGN.md 4.22.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib

DEFAULT_BINS = 5
MAX_BINS = _lib.header_int("MRS_FPFH_MAX_BINS")
MATCH_MAX_K = 32
RANSAC_MAX_HYPOTHESES = _lib.header_int("MRS_RANSAC_MAX_HYPOTHESES")


class RansacParams(C.Structure):
    """mrs_ransac_params"""
    _fields_ = [("hypotheses", C.c_int32), ("refine_iters", C.c_int32), ("max_distance", C.c_double), ("edge_similarity", C.c_double),
                ("min_sin2", C.c_double)]


def _check_bins(bins):
    return _lib.in_range("bins", bins, MAX_BINS)


def _ragged(points, offsets):
    """float32 points and offsets that start at 0 and end at N (a (host, device) pair of offsets costs no copy)"""
    return _lib.ragged(points, offsets, dtype=torch.float32, exact=True)


def _rows(rows, p):
    row_start, index = rows
    row_start = row_start.detach().to(p.device, torch.int64).contiguous()
    index = index.detach().to(p.device, torch.int32).contiguous()
    assert row_start.numel() == p.shape[0] + 1, (row_start.numel(), p.shape[0])
    return row_start, index


def radius_neighbors(points, offsets, radius):
    """every j != i of the same cloud with d2(i, j) <= radius^2 (fp64 on the widened coordinates; coincident points included) ->
    (row_start int64 [N + 1], index int32 [total]) device tensors.  Two calls: counts and total, then the fill.  Blocking."""
    d, p, (h_off, d_off, B) = _ragged(points, offsets)
    n = p.shape[0]
    row_start = torch.empty(n + 1, dtype=torch.int64, device=p.device)
    total = np.zeros(1, np.int64)
    lib, ctx, stream = _lib.load(), _lib.ctx(d), _lib.current_stream(d)
    lib.mrs_radius_count(ctx, p, p.shape[1], d_off, h_off, B, float(radius), row_start, total, stream)
    index = torch.empty(int(total[0]), dtype=torch.int32, device=p.device)
    lib.mrs_radius_fill(ctx, p, p.shape[1], d_off, h_off, B, float(radius), row_start, int(total[0]), index, stream)
    return row_start, index


def rows_from_lists(neighbors, offsets=None, device="cuda:0"):
    """CSR rows from per-point index lists (sklearn's query_radius output): each list is made ascending and free of repeats, as the
    reference's set() does; the point itself may stay in its row.  Lists of a batch hold cloud-local indices."""
    rows = [np.unique(np.asarray(r, np.int64)) for r in neighbors]
    lens = np.fromiter((r.size for r in rows), np.int64, len(rows))
    row_start = np.zeros(len(rows) + 1, np.int64)
    np.cumsum(lens, out=row_start[1:])
    index = np.concatenate(rows).astype(np.int32) if len(rows) and row_start[-1] else np.zeros(0, np.int32)
    return torch.from_numpy(row_start).to(device), torch.from_numpy(index).to(device)


def spfh(points, normals, offsets, rows, bins=DEFAULT_BINS, from_neighbors=False):
    """-> (counts int32 [N, 3 bins], spfh float64 [N, 3 bins]): the alpha, phi and theta histograms of every point over its row, each third
    divided by its own sum.  from_neighbors=True is for rows the caller made: they are checked (an entry outside its cloud raises)."""
    bins = _check_bins(bins)
    d, p, (h_off, d_off, B) = _ragged(points, offsets)
    nrm = normals.detach().to(p.device, torch.float32).contiguous()
    assert nrm.shape == (p.shape[0], 3), tuple(nrm.shape)
    row_start, index = _rows(rows, p)
    n = p.shape[0]
    counts = torch.empty((n, 3 * bins), dtype=torch.int32, device=p.device)
    out = torch.empty((n, 3 * bins), dtype=torch.float64, device=p.device)
    lib = _lib.load()
    fn = lib.mrs_fpfh_spfh_from_neighbors if from_neighbors else lib.mrs_fpfh_spfh
    fn(_lib.ctx(d), p, p.shape[1], nrm, d_off, B, n, row_start, index, index.numel(), bins, counts, out, _lib.current_stream(d))
    return counts, out


def _keypoints(keypoints, h_off, device):
    """packed int64 indices from a tensor / array of packed indices, or from a list of per-cloud tensors of cloud-local indices (what
    iss_keypoints returns)"""
    if isinstance(keypoints, (list, tuple)) and len(keypoints) == h_off.numel() - 1 and all(hasattr(k, "__len__") for k in keypoints):
        parts = [torch.as_tensor(k).to(device, torch.int64).reshape(-1) + int(h_off[c]) for c, k in enumerate(keypoints)]
        return torch.cat(parts) if parts else torch.zeros(0, dtype=torch.int64, device=device)
    return torch.as_tensor(keypoints).detach().to(device, torch.int64).reshape(-1).contiguous()


def describe(points, offsets, rows, spfh_all, bins=DEFAULT_BINS, keypoints=None):
    """FPFH [K, 3 bins] float64 of the keypoints (every point when None) from the SPFH of all points: f = spfh_i + (1 / k) sum_j spfh_j /
    |p_j - p_i| over row i in row order, then f / |f|"""
    bins = _check_bins(bins)
    d, p, (h_off, d_off, B) = _ragged(points, offsets)
    row_start, index = _rows(rows, p)
    n = p.shape[0]
    assert spfh_all.shape == (n, 3 * bins) and spfh_all.dtype == torch.float64 and spfh_all.is_contiguous(), tuple(spfh_all.shape)
    kp = None if keypoints is None else _keypoints(keypoints, h_off, p.device)
    K = n if kp is None else kp.numel()
    out = torch.empty((K, 3 * bins), dtype=torch.float64, device=p.device)
    _lib.load().mrs_fpfh_describe(_lib.ctx(d), p, p.shape[1], d_off, B, n, row_start, index, index.numel(), bins, spfh_all, kp, K,
                                  out, _lib.current_stream(d))
    return out


def fpfh(points, normals, offsets, radius, bins=DEFAULT_BINS, keypoints=None, return_parts=False):
    """radius rows -> SPFH of every point -> FPFH [K, 3 bins] float64 of the keypoints (packed indices, or the per-cloud lists of
    iss_keypoints; every point when None).  return_parts=True: (fpfh, spfh, counts, (row_start, index))."""
    rows = radius_neighbors(points, offsets, radius)
    counts, s = spfh(points, normals, offsets, rows, bins)
    f = describe(points, offsets, rows, s, bins, keypoints)
    return (f, s, counts, rows) if return_parts else f


def iss_keypoints(points, offsets, salient_radius, non_max_radius, gamma21=0.975, gamma32=0.975, min_neighbors=5):
    """ISS keypoints (parity unpinned: the reference imports an ISS module it does not ship; this is the published method)
    -> (list of ascending cloud-local int64 index tensors, one per cloud; saliency float64 [N])"""
    d, p, (h_off, d_off, B) = _ragged(points, offsets)
    n = p.shape[0]
    lib, ctx, stream = _lib.load(), _lib.ctx(d), _lib.current_stream(d)
    rs, idx = radius_neighbors(p, (h_off, d_off), salient_radius)
    sal = torch.empty(n, dtype=torch.float64, device=p.device)
    lib.mrs_iss_saliency(ctx, p, p.shape[1], d_off, B, n, rs, idx, idx.numel(), int(min_neighbors), float(gamma21), float(gamma32), sal, stream)
    if float(non_max_radius) != float(salient_radius):
        rs, idx = radius_neighbors(p, (h_off, d_off), non_max_radius)
    keep = torch.empty(n, dtype=torch.uint8, device=p.device)
    lib.mrs_iss_nonmax(ctx, d_off, B, n, rs, idx, idx.numel(), sal, keep, stream)
    picked = torch.nonzero(keep).reshape(-1)
    bounds = torch.searchsorted(picked, d_off).tolist()
    return [picked[bounds[c]:bounds[c + 1]] - int(h_off[c]) for c in range(B)], sal


def match(a, b, k=1):
    """the k nearest rows of b for every row of a by squared L2 distance over the float32-rounded descriptors (mrs_signature_knn: ascending,
    ties to the lower index) -> (index int32 [len(a), k], dist2 float32 [len(a), k]); slots past len(b) hold -1 / +inf"""
    k = _lib.in_range("k", k, MATCH_MAX_K)
    d = _lib.device_of(a)
    qa = a.detach().to(torch.float32).contiguous()
    qb = b.detach().to(a.device, torch.float32).contiguous()
    assert qa.dim() == 2 and qb.dim() == 2 and qa.shape[1] == qb.shape[1], (tuple(qa.shape), tuple(qb.shape))
    index = torch.full((qa.shape[0], k), -1, dtype=torch.int32, device=a.device)
    dist2 = torch.full((qa.shape[0], k), float("inf"), dtype=torch.float32, device=a.device)
    if qa.shape[0] and qb.shape[0]:
        _lib.load().mrs_signature_knn(_lib.ctx(d), qa, qa.shape[0], qb, qb.shape[0], qa.shape[1], k, index, dist2, _lib.current_stream(d))
    return index, dist2


def correspondences(fa, fb, k=1, mutual=False):
    """index pairs (ia, ib int64 device tensors) from the descriptors of two keypoint sets: every row i of fa with each of its k nearest
    rows j of fb (match: ascending distance, ties to the lower index), i ascending.  mutual=True keeps i -> j only if the nearest row
    of fa for j is i.  Plain torch over match(); gather the points with them for ransac_pose."""
    index, _ = match(fa, fb, k)
    ia = torch.arange(index.shape[0], device=index.device, dtype=torch.int64).repeat_interleave(index.shape[1])
    ib = index.reshape(-1).to(torch.int64)
    keep = ib >= 0
    if mutual and fa.shape[0] and fb.shape[0]:
        back, _ = match(fb, fa, 1)
        keep &= back[:, 0].to(torch.int64)[ib.clamp(min=0)] == ia
    return ia[keep], ib[keep]


def ransac_pose(src, dst, offsets, max_distance, seeds=None, hypotheses=4096, edge_similarity=0.9, min_sin2=1e-6, refine_iters=3,
                return_mask=False, profile=False):
    """RANSAC pose of every pair of a ragged batch from point correspondences: src / dst packed [total, stride >= 3]
    float32, row m of src corresponds to row m of dst; offsets int64 [P + 1]; seeds one uint64 per pair (0 .. P - 1 when None).
    -> (T float64 [P, 4, 4] with dst ~ T src, info int32 [P, 4] = inliers, best hypothesis, valid hypotheses, refits done[, mask uint8
    [total]]) on the device.  A pair without a pose (fewer than 3 correspondences, every triple rejected) gets the identity and
    info = (0, -1, valid, 0).  Enqueued on the current stream; a pair's result does not depend on the batch it is in.
    profile=True (measurements; blocking) appends the milliseconds of the three stages (models, score, refit) to the result."""
    d, p, (h_off, d_off, P) = _ragged(src, offsets)
    q = dst.detach().to(p.device, torch.float32).contiguous()
    assert q.shape == p.shape, (tuple(p.shape), tuple(q.shape))
    h_seeds = np.arange(P, dtype=np.uint64) if seeds is None else np.ascontiguousarray(np.asarray(seeds).astype(np.uint64)).reshape(-1)
    assert h_seeds.size == P, (h_seeds.size, P)
    par = RansacParams(int(hypotheses), int(refine_iters), float(max_distance), float(edge_similarity), float(min_sin2))
    T = torch.empty((P, 4, 4), dtype=torch.float64, device=p.device)
    info = torch.empty((P, 4), dtype=torch.int32, device=p.device)
    mask = torch.empty(p.shape[0], dtype=torch.uint8, device=p.device) if return_mask else None
    out = (T, info, mask) if return_mask else (T, info)
    if profile:
        ms = np.zeros(3, np.float32)
        _lib.load().mrs_ransac_pose_batch_profile(_lib.ctx(d), p, q, p.shape[1], d_off, h_off, P, h_seeds, C.byref(par), T, info, mask, ms,
                                                  _lib.current_stream(d))
        return out + (ms,)
    _lib.load().mrs_ransac_pose_batch(_lib.ctx(d), p, q, p.shape[1], d_off, h_off, P, h_seeds, C.byref(par), T, info, mask,
                                      _lib.current_stream(d))
    return out
