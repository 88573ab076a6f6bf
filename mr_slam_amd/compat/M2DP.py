"""Drop-in for the reference module `pr_methods.M2DP` (LoopDetection/src/RING_ros/pr_methods/M2DP.py).

`mr_slam_amd.compat.install(m2dp=True)` registers it, so that `from pr_methods.M2DP import M2DP` resolves here.  Same call: a host cloud
[n, 3] in, (descriptor float64 [192], signature matrix float64 [64, 128]) out as NumPy arrays, zeros for a cloud of fewer than 3 points.
The PCA, the 64-plane signature matrix and the leading singular pair run in the HIP kernels of m2dp.hip (mrs_m2dp_host).  The descriptor's
sign is fixed (sum(u0) >= 0) where LAPACK's is arbitrary, and a float32 cloud is widened to float64 first.
"""
import numpy as np

from .. import _lib

_DEVICE = 0


def M2DP(cloud):
    pts = np.asarray(cloud)
    if pts.dtype not in (np.float32, np.float64):
        pts = pts.astype(np.float64)
    pts = np.ascontiguousarray(pts.reshape(-1, pts.shape[-1] if pts.ndim == 2 else 3))
    desc, A = np.zeros(192, np.float64), np.zeros((64, 128), np.float64)
    if pts.shape[0] >= 3:
        _lib.load().mrs_m2dp_host(_lib.ctx(_DEVICE), pts, pts.dtype == np.float64, pts.shape[1], pts.shape[0], desc, A)
    return desc, A
