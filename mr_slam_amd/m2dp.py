"""M2DP on device tensors (RING_ros/pr_methods/M2DP.py): the 192-d descriptor of a raw 3-D cloud, its 64 x 128 signature matrix, and a
device-resident descriptor list searched by Euclidean distance.

Thin host logic over the C ABI (mrs_m2dp_*, mrs_loopdb_*_m2dp); there is no CPU fallback.  Two things differ from the reference on purpose
(DESIGN.md 4.10): the descriptor's sign is fixed (sum(u0) >= 0, which makes both singular vectors non-negative; LAPACK's is arbitrary), and a
float32 cloud is widened to float64 before anything is computed, so the contract is `M2DP(cloud.astype(np.float64))`.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .loopdb import VectorLoopDb

NUM_PLANES, NUM_BINS, DESC_DIM = 64, 128, 192
KIND_M2DP = 4
MAX_K = 32
# points per workgroup of the signature-matrix kernel (MRS_M2DP_TILE_POINTS of the C ABI header)
TILE_POINTS = _lib.header_int("MRS_M2DP_TILE_POINTS")


def _args(points, offsets):
    """([total, stride >= 3] float32 / float64 device tensor, offsets [B + 1] in any form _lib.ragged takes) -> the C ABI's leading arguments"""
    d, p, (h_off, d_off, B) = _lib.ragged(points, offsets)
    return d, p, (_lib.ctx(d), p, p.dtype == torch.float64, p.shape[1], d_off, h_off, B)


def m2dp_batch(points, offsets):
    """M2DP of a ragged batch: cloud b = points[offsets[b]:offsets[b + 1], :3] -> (desc [B, 192], A [B, 64, 128]) float64 device tensors;
    clouds of fewer than 3 points give zeros"""
    d, p, a = _args(points, offsets)
    B = a[-1]
    desc = torch.empty((B, DESC_DIM), dtype=torch.float64, device=p.device)
    A = torch.empty((B, NUM_PLANES, NUM_BINS), dtype=torch.float64, device=p.device)
    _lib.load().mrs_m2dp_batch(*a, desc, A, _lib.current_stream(d))
    return desc, A


def pca_batch(points, offsets):
    """the PCA stage alone -> float64 [B, 16] device tensor: mean [3], components [3, 3] (rows), maxRho, covariance eigenvalues [3]"""
    d, p, a = _args(points, offsets)
    out = torch.empty((a[-1], 16), dtype=torch.float64, device=p.device)
    _lib.load().mrs_m2dp_pca_batch(*a, out, _lib.current_stream(d))
    return out


def m2dp(cloud, device="cuda:0"):
    """one cloud [n, >= 3] (device tensor, host tensor or array) -> (desc [192], A [64, 128]) float64 device tensors"""
    desc, A = m2dp_batch(*_lib.one_cloud(cloud, device))
    return desc[0], A[0]


class M2DPDatabase(VectorLoopDb):
    """Device-resident list of M2DP descriptors of one robot (mrs_loopdb, kind M2DP; entries are kept as float32 [192]): `append(desc)`;
    `query(desc, k)` = the k nearest entries by squared L2 distance, ascending, ties to the lower index."""
    _elem = (torch.float64, np.float64, DESC_DIM)

    def __init__(self, device=0, capacity=1024):
        super().__init__(KIND_M2DP, 1, device, capacity)

    def append(self, desc):
        _lib.load().mrs_loopdb_append_m2dp(self._h, *self._arg(desc))

    def query(self, desc, k=1):
        """-> (indices, squared distances) as numpy arrays of length min(k, len(self)), nearest first"""
        k = _lib.in_range("k", k, MAX_K)
        t, dev, stream = self._arg(desc)
        idx, d2 = np.full(k, -1, np.int32), np.full(k, np.inf, np.float32)
        cnt = C.c_int32(0)
        _lib.load().mrs_loopdb_query_m2dp(self._h, t, dev, k, idx, d2, C.byref(cnt), stream)
        return idx[:cnt.value], d2[:cnt.value]
