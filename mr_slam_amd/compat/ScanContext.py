"""Drop-in for the reference module `pr_methods.ScanContext` (LoopDetection/src/RING_ros/pr_methods/ScanContext.py).

`mr_slam_amd.compat.install(scancontext=True)` registers it, so that `import pr_methods.ScanContext as SC` in main_SC.py resolves here.
Same public functions and signatures, NumPy in and out, the reference's return types (a float dist, an int shift, float64 keys).  The
keys, the sector-key alignment and the column-cosine distances run in the HIP kernels of scancontext.hip (mr_slam_amd.scancontext);
fast_align and dist_align_cc (off the node's path) are device-side torch glue around them.  num_ring / num_sector come from the
descriptor's shape (120 x 120 for the node's descriptors, what config.py sets).
"""
import numpy as np
import torch

from .. import scancontext as _sc
from .util import upload

_DEVICE = "cuda:0"


def _t(x):
    return upload(x, np.float32, None, _DEVICE)


def make_ringkey(sc):
    return _sc.make_ringkey(_t(sc)).cpu().numpy().astype(np.float64)


def make_sectorkey(sc):
    return _sc.make_sectorkey(_t(sc)).cpu().numpy().astype(np.float64)


def distance_sc(sc1, sc2):
    d, yaw = _sc.distance_sc(_t(sc1), _t(sc2))
    return float(d), int(yaw)


def fast_align(sc1, sc2):
    """min over shift of ||sc1 - roll(sc2, shift, axis=-1)|| (first minimum), all shifts in one batched device expression"""
    a, b = _t(sc1), _t(sc2)
    S = b.shape[-1]
    rolled = torch.stack([torch.roll(b, s, dims=-1) for s in range(S)])
    norms = torch.linalg.vector_norm((a.unsqueeze(0) - rolled).reshape(S, -1).to(torch.float64), dim=1)
    s = int(torch.argmin(norms))
    return float(np.float32(norms[s].item())), s


def fast_align_with_sectorkey(sector_key1, sector_key2):
    n, s = _sc.fast_align_with_sectorkey(_t(sector_key1).reshape(-1), _t(sector_key2).reshape(-1))
    return float(n), int(s)


def dist_direct_sc(sc1, sc2):
    return float(_sc.dist_direct_sc(_t(sc1), _t(sc2)))


def dist_align_sc(sc1, sc2, search_ratio=0.1):
    d, s = _sc.dist_align_sc(_t(sc1), _t(sc2), search_ratio)
    return float(d), int(s)


def dist_align_cc(sc1, sc2, search_ratio=0.1):
    """the ring-key twin of dist_align_sc: pre-alignment on the ring keys, window of rolls along axis -2 (ScanContext.py:144-158)"""
    a, b = _t(sc1), _t(sc2)
    R = b.shape[-2]
    _, s = _sc.fast_align_with_sectorkey(_sc.make_ringkey(a), _sc.make_ringkey(b))
    r = round(0.5 * search_ratio * R)
    shifts = list(range(max(-R, int(s) - r), min(R, int(s) + r + 1)))
    rolled = torch.stack([torch.roll(b.reshape(R, -1), k, dims=0) for k in shifts])
    d = _sc.dist_direct_sc(a.reshape(1, R, -1).expand(len(shifts), -1, -1), rolled)
    i = int(torch.argmin(d))
    return float(d[i]), shifts[i]
