"""Scan Context on device tensors (RING_ros/pr_methods/ScanContext.py and the candidate step of RING_ros/main_SC.py).

The descriptor is the SC node's own (main_SC.py:57-69): the CARTESIAN max-z BEV of voxelocc, 120 x 120 over [-1, 1)^2, not the polar grid
of the Scan Context paper.  Axis -2 is called "ring", axis -1 "sector"; a sector shift is a roll along the y bins.  The pairwise functions
also take any num_ring, num_sector <= 128 (for example the paper's 20 x 60 polar descriptor from `bev.polar_bev`).

Thin host logic over the C ABI (mrs_sc_*, mrs_loopdb_*_sc*); there is no CPU fallback.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib, bev
from .loopdb import VectorLoopDb, query_grown

NUM_RING = NUM_SECTOR = 120
KIND_SC = 3
MAX_CANDIDATES = 64


def _batch(sc):
    """[R, S] / [1, R, S] (one descriptor) or [n, R, S] / [n, 1, R, S] float32 device tensor -> ([n, R, S] contiguous, one descriptor?)"""
    _lib.device_of(sc)
    t = sc.detach().to(torch.float32)
    R, S = t.shape[-2:]
    return t.reshape(-1, R, S).contiguous(), t.dim() <= 3 and t.numel() == R * S


def sc_descriptors(xyz, offsets):
    """generate_scan_context for a ragged batch (bev.pack_scans layout) -> float32 [B, 120, 120]: channel 2 (max z) of voxelocc's
    GPUTransformer(pc, size, 1, 1, 120, 120, 1, 1), the COMPACT output of the Cartesian rasteriser."""
    return bev.cart_bev(xyz, offsets, 1, 1, NUM_RING, NUM_SECTOR, 1).view(-1, NUM_RING, NUM_SECTOR)


def generate_scan_context(pc, device="cuda:0"):
    """main_SC.py:57-69 on one cloud: float32 [n, 3] (host or device) -> [1, 120, 120] device tensor"""
    if isinstance(pc, torch.Tensor):
        pc = pc.detach().cpu().numpy()
    xyz, offs = bev.pack_scans([np.asarray(pc, np.float32)], device)
    return sc_descriptors(xyz, offs).view(1, NUM_RING, NUM_SECTOR)


def keys(sc):
    """(ring keys [n, R], sector keys [n, S]) float32 of a batch of descriptors (make_ringkey / make_sectorkey)"""
    t, _ = _batch(sc)
    n, R, S = t.shape
    d = _lib.device_of(t)
    ring = torch.empty((n, R), dtype=torch.float32, device=t.device)
    sector = torch.empty((n, S), dtype=torch.float32, device=t.device)
    _lib.load().mrs_sc_keys(_lib.ctx(d), t, n, R, S, ring, sector, _lib.current_stream(d))
    return ring, sector


def make_ringkey(sc):
    """ScanContext.py:13-21: the mean of each row -> [R] ([n, R] for a batch)"""
    t, single = _batch(sc)
    r = keys(t)[0]
    return r[0] if single else r


def make_sectorkey(sc):
    """ScanContext.py:23-31: the mean of each column -> [S] ([n, S] for a batch)"""
    t, single = _batch(sc)
    s = keys(t)[1]
    return s[0] if single else s


def fast_align_with_sectorkey(key1, key2):
    """ScanContext.py:86-101 for device keys [len] or [n, len]: (min ||key1 - roll(key2, s)|| (fp64), first s) over s < len"""
    _lib.device_of(key1)
    a = key1.detach().to(torch.float32).reshape(-1, key1.shape[-1]).contiguous()
    b = key2.detach().to(torch.float32).reshape(-1, key2.shape[-1]).contiguous()
    assert a.shape == b.shape, (a.shape, b.shape)
    n, L = a.shape
    d = _lib.device_of(a)
    norm = torch.empty(n, dtype=torch.float64, device=a.device)
    shift = torch.empty(n, dtype=torch.int32, device=a.device)
    _lib.load().mrs_sc_key_align_pairs(_lib.ctx(d), a, b, n, L, norm, shift, _lib.current_stream(d))
    return (norm[0], shift[0]) if key1.dim() == 1 else (norm, shift)


def _pairs(fn, sc1, sc2, *extra, with_shift=True):
    a, single = _batch(sc1)
    b, _ = _batch(sc2)
    if a.shape[0] != b.shape[0] and min(a.shape[0], b.shape[0]) == 1:
        a, b = a.expand(b.shape[0], -1, -1).contiguous() if a.shape[0] == 1 else a, b.expand(a.shape[0], -1, -1).contiguous() if b.shape[0] == 1 else b
        single = False
    assert a.shape == b.shape, (a.shape, b.shape)
    n, R, S = a.shape
    d = _lib.device_of(a)
    dist = torch.empty(n, dtype=torch.float32, device=a.device)
    shift = torch.empty(n, dtype=torch.int32, device=a.device) if with_shift else None
    outs = (dist, shift) if with_shift else (dist,)
    getattr(_lib.load(), fn)(_lib.ctx(d), a, b, n, R, S, *extra, *outs, _lib.current_stream(d))
    if single:
        return (dist[0], shift[0]) if with_shift else dist[0]
    return (dist, shift) if with_shift else dist


def dist_direct_sc(sc1, sc2):
    """ScanContext.py:105-126: 1 - mean column cosine over the columns where both norms are > 0 (1.0 if none)"""
    return _pairs("mrs_sc_dist_direct_pairs", sc1, sc2, with_shift=False)


def dist_align_sc(sc1, sc2, search_ratio=0.1):
    """ScanContext.py:128-142: (dist, shift); the shift rolls sc2 and may be negative.  Batched over a leading axis."""
    return _pairs("mrs_sc_dist_align_pairs", sc1, sc2, float(search_ratio))


def distance_sc(sc1, sc2):
    """ScanContext.py:34-69: all num_sector shifts of sc1 -> (1 - best mean cosine, argmax + 1)"""
    return _pairs("mrs_sc_distance_pairs", sc1, sc2)


class ScanContextDatabase(VectorLoopDb):
    """Device-resident SC<k> + RingkeyPC<k> of one robot (mrs_loopdb, kind SC): `append(sc)` stores a [120, 120] descriptor with its keys;
    `query(sc, num_candidates, search_ratio)` = main_SC.py:159-167 (the nearest ring keys, then dist_align_sc(candidate, current));
    `query_all(sc, search_ratio)` aligns the query against every entry; `device_entries()` = (packed entries [n, entry_floats], ring
    keys [n, 120], n, entry_floats)."""
    _elem = (torch.float32, np.float32, NUM_RING * NUM_SECTOR)

    def __init__(self, device=0, capacity=1024):
        super().__init__(KIND_SC, 1, device, capacity)

    def append(self, sc):
        _lib.load().mrs_loopdb_append_sc(self._h, *self._arg(sc))

    def query(self, sc, num_candidates=1, search_ratio=0.1):
        """-> (indices, ring-key distances, dists, shifts) as numpy arrays of length min(num_candidates, len(self)), nearest key first"""
        k = _lib.in_range("num_candidates", num_candidates, MAX_CANDIDATES)
        t, dev, stream = self._arg(sc)
        idx, kd = np.full(k, -1, np.int32), np.zeros(k, np.float32)
        dist, shift = np.zeros(k, np.float32), np.zeros(k, np.int32)
        cnt = C.c_int32(0)
        _lib.load().mrs_loopdb_query_sc(self._h, t, dev, k, float(search_ratio), idx, kd, dist, shift, C.byref(cnt), stream)
        c = cnt.value
        return idx[:c], kd[:c], dist[:c], shift[:c]

    def query_all(self, sc, search_ratio=0.1):
        """-> (dists [n], shifts [n], index of the first smallest dist or -1): dist_align_sc(entry, sc) for every entry"""
        t, dev, stream = self._arg(sc)
        lib = _lib.load()

        def sweep(cap):
            dist, shift = np.zeros(max(cap, 1), np.float32), np.zeros(max(cap, 1), np.int32)
            best, n = C.c_int32(-1), C.c_int32(0)
            lib.mrs_loopdb_query_sc_all(self._h, t, dev, float(search_ratio), cap, dist, shift, C.byref(best), C.byref(n), stream)
            return n.value, (dist[:n.value], shift[:n.value], best.value)
        return query_grown(sweep, len(self))          # exact: another thread may have appended since len()
