"""M2DP on device tensors (RING_ros/pr_methods/M2DP.py): the 192-d descriptor of a raw 3-D cloud, its 64 x 128 signature matrix, and a
device-resident descriptor list searched by Euclidean distance.

Thin host logic over the C ABI (mrs_m2dp_*, mrs_loopdb_*_m2dp); there is no CPU fallback.  Two things differ from the reference on purpose
(DESIGN.md 4.10): the descriptor's sign is fixed (sum(u0) >= 0, which makes both singular vectors non-negative; LAPACK's is arbitrary), and a
float32 cloud is widened to float64 before anything is computed, so the contract is `M2DP(cloud.astype(np.float64))`.
"""
import ctypes as C
import re

import numpy as np
import torch

from . import _lib

NUM_PLANES, NUM_BINS, DESC_DIM = 64, 128, 192
KIND_M2DP = 4
MAX_K = 32
# points per workgroup of the signature-matrix kernel (MRS_M2DP_TILE_POINTS of the C ABI header)
TILE_POINTS = int(re.search(r"#define\s+MRS_M2DP_TILE_POINTS\s+(\d+)", open(_lib.HEADER).read())[1])


def _args(points, offsets):
    """([total, stride >= 3] float32 / float64 device tensor, int64 offsets [B + 1] on either side) -> the C ABI's leading arguments"""
    d = _lib.device_of(points)
    p = points.detach()
    if p.dtype not in (torch.float32, torch.float64):
        p = p.to(torch.float64)
    assert p.dim() == 2 and p.shape[1] >= 3, tuple(p.shape)
    p = p.contiguous()
    h_off = offsets.detach().to("cpu", torch.int64).contiguous()
    d_off = offsets.detach().to(p.device, torch.int64).contiguous()
    B = h_off.numel() - 1
    assert B >= 1 and int(h_off[-1]) <= p.shape[0], (B, int(h_off[-1]), p.shape[0])
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
    if not isinstance(cloud, torch.Tensor):
        cloud = torch.from_numpy(np.ascontiguousarray(cloud))
    if not cloud.is_cuda:
        cloud = cloud.to(device)
    cloud = cloud.reshape(-1, cloud.shape[-1] if cloud.dim() == 2 else 3)
    desc, A = m2dp_batch(cloud, torch.tensor([0, cloud.shape[0]], dtype=torch.int64))
    return desc[0], A[0]


class M2DPDatabase:
    """Device-resident list of M2DP descriptors of one robot (mrs_loopdb, kind M2DP; entries are kept as float32 [192]): `append(desc)`;
    `query(desc, k)` = the k nearest entries by squared L2 distance, ascending, ties to the lower index."""

    def __init__(self, device=0, capacity=1024):
        self.device = int(device)
        self._h = C.c_void_p()
        _lib.load().mrs_loopdb_create(_lib.ctx(self.device), KIND_M2DP, 1, int(capacity), C.byref(self._h))

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                _lib.load().mrs_loopdb_destroy(self._h)
        except Exception:
            pass

    def __len__(self):
        n = C.c_int32(0)
        _lib.load().mrs_loopdb_size(self._h, C.byref(n))
        return n.value

    def _arg(self, desc):
        """(descriptor, on_device, stream) of one [192] descriptor (torch host / device tensor or numpy array)"""
        if isinstance(desc, torch.Tensor):
            t = desc.detach().to(torch.float64).contiguous()
            assert t.numel() == DESC_DIM, tuple(t.shape)
            if t.is_cuda:
                return t, 1, _lib.current_stream(t.device.index or 0)
            return t, 0, None
        a = np.ascontiguousarray(desc, dtype=np.float64)
        assert a.size == DESC_DIM, a.shape
        return a, 0, None

    def append(self, desc):
        _lib.load().mrs_loopdb_append_m2dp(self._h, *self._arg(desc))

    def query(self, desc, k=1):
        """-> (indices, squared distances) as numpy arrays of length min(k, len(self)), nearest first"""
        k = int(k)
        if not 1 <= k <= MAX_K:
            raise ValueError("k in 1..%d" % MAX_K)
        t, dev, stream = self._arg(desc)
        idx, d2 = np.full(k, -1, np.int32), np.full(k, np.inf, np.float32)
        cnt = C.c_int32(0)
        _lib.load().mrs_loopdb_query_m2dp(self._h, t, dev, k, idx, d2, C.byref(cnt), stream)
        return idx[:cnt.value], d2[:cnt.value]
