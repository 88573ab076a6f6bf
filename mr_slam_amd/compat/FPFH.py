"""Drop-in for the two functions of the reference module `FPFH` that carry its arithmetic (LoopDetection/src/RING_ros/FPFH.py:33-105).

`mr_slam_amd.compat.install(fpfh=True)` registers it as `FPFH`.  Same calls: `get_spfh(point_cloud, nearest_idx, keypoint_id, radius, B)`
and `describe(...)` take a host cloud [n, >= 3], the per-point neighbour lists of sklearn's `KDTree.query_radius` and one point's index, and
return a float64 [3 B] NumPy vector; the normals come from the module global `point_cloud_normals`, which the caller sets as the
reference's __main__ does.  The SPFH of ALL points is computed once per (point_cloud, nearest_idx, point_cloud_normals, B) identity by the
HIP kernels of fpfh.hip and the per-keypoint calls are served from it (the reference recomputes a neighbour's SPFH for every keypoint that
has it in its list).  `radius` is not used, as in the reference: the lists say who the neighbours are.

Differences: points and normals are rounded to float32 and widened again; a list is taken as a set in ascending order; a
neighbour at distance 0 is skipped; an empty histogram and a keypoint without neighbours give zeros where the reference gives NaN or raises.
"""
import numpy as np
import torch

from .. import fpfh as _fpfh
from .util import upload

_DEVICE = "cuda:0"
point_cloud_normals = None
_cache = None          # (point_cloud, nearest_idx, normals, B, state): the identities are compared with `is`, the objects kept alive


def _state(point_cloud, nearest_idx, B):
    global _cache
    if point_cloud_normals is None:
        raise NameError("name 'point_cloud_normals' is not defined (set FPFH.point_cloud_normals, as the reference's __main__ does)")
    c = _cache
    if c is not None and c[0] is point_cloud and c[1] is nearest_idx and c[2] is point_cloud_normals and c[3] == int(B):
        return c[4]
    pts, nrm = upload(point_cloud, np.float32, 3, _DEVICE), upload(point_cloud_normals, np.float32, 3, _DEVICE)
    offsets = torch.tensor([0, pts.shape[0]], dtype=torch.int64)
    rows = _fpfh.rows_from_lists(nearest_idx, device=_DEVICE)
    _, s = _fpfh.spfh(pts, nrm, offsets, rows, int(B), from_neighbors=True)
    state = (pts, offsets, rows, s, s.cpu().numpy())
    _cache = (point_cloud, nearest_idx, point_cloud_normals, int(B), state)
    return state


def get_spfh(point_cloud, nearest_idx, keypoint_id, radius, B):
    return _state(point_cloud, nearest_idx, B)[4][int(keypoint_id)].copy()


def describe(point_cloud, nearest_idx, keypoint_id, radius, B):
    pts, offsets, rows, s, _ = _state(point_cloud, nearest_idx, B)
    return _fpfh.describe(pts, offsets, rows, s, int(B), torch.tensor([int(keypoint_id)], dtype=torch.int64))[0].cpu().numpy()
