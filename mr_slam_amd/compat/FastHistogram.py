"""Drop-in for the reference module `pr_methods.FastHistogram` (LoopDetection/src/RING_ros/pr_methods/FastHistogram.py).

`mr_slam_amd.compat.install(fasthistogram=True)` registers it, so that `from pr_methods.FastHistogram import statisticsOnRange, getEMD`
resolves here.  Same calls: a host cloud [n, >= 3] in, a float64 [b] NumPy vector out.  The range pass, the bucket of every point and the
normalisation run in the HIP kernels of fasthist.hip (mrs_fh_host); a float32 cloud is widened to float64 first, and where the reference
raises (a point in the one-ulp gap above the last edge, an empty cloud, an infinite coordinate) a defined result comes back instead
(DESIGN.md 4.17).  The two-vector distances stay on the host: 2 b numbers, added in index order so that they carry the reference's bits.
"""
import numpy as np

from .. import _lib

_DEVICE = 0


def _cloud(xyzs):
    pts = np.asarray(xyzs)
    if pts.dtype not in (np.float32, np.float64):
        pts = pts.astype(np.float64)
    return np.ascontiguousarray(pts.reshape(-1, pts.shape[-1] if pts.ndim == 2 else 3))


def _host(xyzs, b):
    pts = _cloud(xyzs)
    b = int(b)
    hist, rng = np.zeros(max(b, 0), np.float64), np.zeros(1, np.float64)
    _lib.load().mrs_fh_host(_lib.ctx(_DEVICE), pts, pts.dtype == np.float64, pts.shape[1], pts.shape[0], b, hist, None, rng, None)
    return hist, float(rng[0])


def calculateRange(xyzs):
    """(minDist, maxDist): the minimum starts at 0 and no range is below it, so it is always 0.0"""
    return 0.0, _host(xyzs, 1)[1]


def distanceJudge(distance, minDist, maxDist, b):
    """bucket of one range: the last i < b with minDist + i w <= distance <= minDist + (i + 1) w when minDist < distance < maxDist,
    b - 1 otherwise (and for a range in the one-ulp gap above the last edge, where the reference raises)"""
    w = (maxDist - minDist) / b
    if not (distance > minDist and distance < maxDist):
        return b - 1
    edges = minDist + np.arange(b + 1, dtype=np.float64) * w
    hit = np.nonzero((distance >= edges[:-1]) & (distance <= edges[1:]))[0]
    return int(hit[-1]) if hit.size else b - 1


def statisticsOnRange(xyzs, b=100):
    return _host(xyzs, b)[0]


def getEMD(vector1, vector2):
    """sum of |vector1[i] - vector2[i]| in index order, divided by the length"""
    v1, v2 = np.asarray(vector1, np.float64).reshape(-1), np.asarray(vector2, np.float64).reshape(-1)[:np.size(vector1)]
    if v1.size == 0:
        raise ZeroDivisionError("float division by zero")
    return float(np.add.accumulate(np.abs(v1 - v2))[-1] / v1.size)


calculateW = getEMD
