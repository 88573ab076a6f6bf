"""Fast Histogram on device tensors (RING_ros/pr_methods/FastHistogram.py): the range histogram of a raw 3-D cloud and a device-resident
list of histograms compared by getEMD / calculateW.

Thin host logic over the C ABI (mrs_fh_*, mrs_loopdb_*_fh); there is no CPU fallback.  A float32 cloud is widened to float64 before anything
is computed, so the contract is `statisticsOnRange(cloud.astype(np.float64), bins)`; the three named deviations (a point in the one-ulp gap
above the last edge, an empty cloud, non-finite points) are in DESIGN.md 4.17.
"""
import ctypes as C
import re

import numpy as np
import torch

from . import _lib

DEFAULT_BINS = 100
KIND_FH = 5
MAX_K = 32
_HEADER = open(_lib.HEADER).read()
# points per workgroup of the range and bin kernels, and the largest bucket count (MRS_FH_TILE_POINTS / MRS_FH_MAX_BINS of the C ABI header)
TILE_POINTS = int(re.search(r"#define\s+MRS_FH_TILE_POINTS\s+(\d+)", _HEADER)[1])
MAX_BINS = int(re.search(r"#define\s+MRS_FH_MAX_BINS\s+(\d+)", _HEADER)[1])


def _check_bins(bins):
    bins = int(bins)
    if not 1 <= bins <= MAX_BINS:
        raise ValueError("bins in 1..%d" % MAX_BINS)
    return bins


def range_histogram_batch(points, offsets, bins=DEFAULT_BINS):
    """range histograms of a ragged batch: cloud b = points[offsets[b]:offsets[b + 1], :3] of a [total, stride >= 3] float32 / float64
    device tensor -> (hist float64 [B, bins], counts int32 [B, bins], max_range float64 [B], unbound int32 [B]) device tensors; an empty
    cloud gives zeros.  offsets: an int64 [B + 1] tensor on either side (it is copied to the other), or a (host, device) pair of the same
    offsets, which costs no copy"""
    bins = _check_bins(bins)
    d = _lib.device_of(points)
    p = points.detach()
    if p.dtype not in (torch.float32, torch.float64):
        p = p.to(torch.float64)
    assert p.dim() == 2 and p.shape[1] >= 3, tuple(p.shape)
    p = p.contiguous()
    h_off, d_off = offsets if isinstance(offsets, (tuple, list)) else (offsets, offsets)
    h_off = h_off.detach().to("cpu", torch.int64).contiguous()
    d_off = d_off.detach().to(p.device, torch.int64).contiguous()
    B = h_off.numel() - 1
    assert B >= 1 and int(h_off[-1]) <= p.shape[0], (B, int(h_off[-1]), p.shape[0])
    hist = torch.empty((B, bins), dtype=torch.float64, device=p.device)
    counts = torch.empty((B, bins), dtype=torch.int32, device=p.device)
    max_range = torch.empty(B, dtype=torch.float64, device=p.device)
    unbound = torch.empty(B, dtype=torch.int32, device=p.device)
    _lib.load().mrs_fh_batch(_lib.ctx(d), p, p.dtype == torch.float64, p.shape[1], d_off, h_off, B, bins, hist, counts, max_range, unbound,
                             _lib.current_stream(d))
    return hist, counts, max_range, unbound


def range_histogram(cloud, bins=DEFAULT_BINS, device="cuda:0"):
    """one cloud [n, >= 3] (device tensor, host tensor or array) -> (hist [bins], counts [bins], max_range, unbound) device tensors"""
    if not isinstance(cloud, torch.Tensor):
        cloud = torch.from_numpy(np.ascontiguousarray(cloud))
    if not cloud.is_cuda:
        cloud = cloud.to(device)
    cloud = cloud.reshape(-1, cloud.shape[-1] if cloud.dim() == 2 else 3)
    hist, counts, max_range, unbound = range_histogram_batch(cloud, torch.tensor([0, cloud.shape[0]], dtype=torch.int64), bins)
    return hist[0], counts[0], max_range[0], unbound[0]


class FastHistogramDatabase:
    """Device-resident list of range histograms of one robot (mrs_loopdb, kind FH; entries are kept in float64 as they come): `append(hist)`;
    `query(hist, k)` = the k nearest entries by getEMD, ascending, ties to the lower index; `distances(hist)` = getEMD to every entry.  The
    distances carry the reference's bits: |G_i - H_i| added in index order in float64, divided by bins."""

    def __init__(self, device=0, capacity=1024, bins=DEFAULT_BINS):
        self.device = int(device)
        self.bins = _check_bins(bins)
        self._h = C.c_void_p()
        _lib.load().mrs_loopdb_create(_lib.ctx(self.device), KIND_FH, self.bins, int(capacity), C.byref(self._h))

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

    def _arg(self, hist):
        """(histogram, on_device, stream) of one [bins] histogram (torch host / device tensor or numpy array)"""
        if isinstance(hist, torch.Tensor):
            t = hist.detach().to(torch.float64).contiguous()
            assert t.numel() == self.bins, tuple(t.shape)
            if t.is_cuda:
                return t, 1, _lib.current_stream(t.device.index or 0)
            return t, 0, None
        a = np.ascontiguousarray(hist, dtype=np.float64)
        assert a.size == self.bins, a.shape
        return a, 0, None

    def append(self, hist):
        _lib.load().mrs_loopdb_append_fh(self._h, *self._arg(hist))

    def query(self, hist, k=1):
        """-> (indices int32, distances float64) as numpy arrays of length min(k, len(self)), nearest first"""
        k = int(k)
        if not 1 <= k <= MAX_K:
            raise ValueError("k in 1..%d" % MAX_K)
        t, dev, stream = self._arg(hist)
        idx, dist = np.full(k, -1, np.int32), np.full(k, np.inf, np.float64)
        cnt = C.c_int32(0)
        _lib.load().mrs_loopdb_query_fh(self._h, t, dev, k, idx, dist, C.byref(cnt), stream)
        return idx[:cnt.value], dist[:cnt.value]

    def distances(self, hist):
        """-> float64 [len(self)] device tensor (ordered after the current stream of the database's device).  Appends from another thread
        between sizing the result and the sweep are the caller's to exclude."""
        t, dev, _ = self._arg(hist)
        out = torch.empty(len(self), dtype=torch.float64, device="cuda:%d" % self.device)
        _lib.load().mrs_loopdb_distances_fh(self._h, t, dev, out, _lib.current_stream(self.device))
        return out
