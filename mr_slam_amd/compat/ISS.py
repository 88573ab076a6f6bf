"""Stand-in for the `ISS` module that the reference's FPFH.py imports (`from ISS import *`, then `iss(point_cloud_raw)`) and does not ship.

`mr_slam_amd.compat.install(fpfh=True)` registers it as `ISS`.  Parity is unpinned: there is no reference text to compare with; this is
the published ISS detector as DESIGN.md 4.20 states it, on the HIP kernels of fpfh.hip.  The two radii have no universal default: pass them,
or set the module globals `salient_radius` / `non_max_radius` before a bare `iss(points)` call.
"""
import numpy as np
import torch

from .. import fpfh as _fpfh
from .util import upload

_DEVICE = "cuda:0"
salient_radius = None
non_max_radius = None


def iss(points, salient_radius=None, non_max_radius=None, gamma21=0.975, gamma32=0.975, min_neighbors=5):
    """host cloud [n, >= 3] -> ascending int64 NumPy array of keypoint indices"""
    sr = salient_radius if salient_radius is not None else globals()["salient_radius"]
    nr = non_max_radius if non_max_radius is not None else globals()["non_max_radius"]
    if sr is None or nr is None:
        raise ValueError("iss needs salient_radius and non_max_radius (arguments, or the globals ISS.salient_radius / ISS.non_max_radius)")
    pts = upload(points, np.float32, 3, _DEVICE)
    keypoints, _ = _fpfh.iss_keypoints(pts, torch.tensor([0, pts.shape[0]], dtype=torch.int64), sr, nr, gamma21, gamma32, min_neighbors)
    return keypoints[0].cpu().numpy()
