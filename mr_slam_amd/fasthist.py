"""Fast Histogram on device tensors (RING_ros/pr_methods/FastHistogram.py): the range histogram of a raw 3-D cloud and a device-resident
list of histograms compared by getEMD / calculateW.

Thin host logic over the C ABI (mrs_fh_*, mrs_loopdb_*_fh); there is no CPU fallback.  A float32 cloud is widened to float64 before anything
is computed, so the contract is `statisticsOnRange(cloud.astype(np.float64), bins)`; the three named deviations (a point in the one-ulp gap
above the last edge, an empty cloud, non-finite points) are in DESIGN.md 4.17.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .loopdb import VectorLoopDb

DEFAULT_BINS = 100
KIND_FH = 5
MAX_K = 32
# points per workgroup of the range and bin kernels, and the largest bucket count (MRS_FH_TILE_POINTS / MRS_FH_MAX_BINS of the C ABI header)
TILE_POINTS = _lib.header_int("MRS_FH_TILE_POINTS")
MAX_BINS = _lib.header_int("MRS_FH_MAX_BINS")


def _check_bins(bins):
    return _lib.in_range("bins", bins, MAX_BINS)


def range_histogram_batch(points, offsets, bins=DEFAULT_BINS):
    """range histograms of a ragged batch: cloud b = points[offsets[b]:offsets[b + 1], :3] of a [total, stride >= 3] float32 / float64
    device tensor -> (hist float64 [B, bins], counts int32 [B, bins], max_range float64 [B], unbound int32 [B]) device tensors; an empty
    cloud gives zeros.  offsets: an int64 [B + 1] tensor on either side (it is copied to the other), or a (host, device) pair of the same
    offsets, which costs no copy"""
    bins = _check_bins(bins)
    d, p, (h_off, d_off, B) = _lib.ragged(points, offsets)
    hist = torch.empty((B, bins), dtype=torch.float64, device=p.device)
    counts = torch.empty((B, bins), dtype=torch.int32, device=p.device)
    max_range = torch.empty(B, dtype=torch.float64, device=p.device)
    unbound = torch.empty(B, dtype=torch.int32, device=p.device)
    _lib.load().mrs_fh_batch(_lib.ctx(d), p, p.dtype == torch.float64, p.shape[1], d_off, h_off, B, bins, hist, counts, max_range, unbound,
                             _lib.current_stream(d))
    return hist, counts, max_range, unbound


def range_histogram(cloud, bins=DEFAULT_BINS, device="cuda:0"):
    """one cloud [n, >= 3] (device tensor, host tensor or array) -> (hist [bins], counts [bins], max_range, unbound) device tensors"""
    hist, counts, max_range, unbound = range_histogram_batch(*_lib.one_cloud(cloud, device), bins)
    return hist[0], counts[0], max_range[0], unbound[0]


class FastHistogramDatabase(VectorLoopDb):
    """Device-resident list of range histograms of one robot (mrs_loopdb, kind FH; entries are kept in float64 as they come): `append(hist)`;
    `query(hist, k)` = the k nearest entries by getEMD, ascending, ties to the lower index; `distances(hist)` = getEMD to every entry.  The
    distances carry the reference's bits: |G_i - H_i| added in index order in float64, divided by bins."""

    def __init__(self, device=0, capacity=1024, bins=DEFAULT_BINS):
        self.bins = _check_bins(bins)
        self._elem = (torch.float64, np.float64, self.bins)
        super().__init__(KIND_FH, self.bins, device, capacity)

    def append(self, hist):
        _lib.load().mrs_loopdb_append_fh(self._h, *self._arg(hist))

    def query(self, hist, k=1):
        """-> (indices int32, distances float64) as numpy arrays of length min(k, len(self)), nearest first"""
        k = _lib.in_range("k", k, MAX_K)
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
