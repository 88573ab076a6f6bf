"""The globally consistent elevation map (GEM) of the Mapping side on the device: the submap stack that
ElevationMapping::updateLocalMap fills (elevation_mapping/src/ElevationMapping.cpp:653-815), its correction after a pose-graph
optimisation (updateGlobalMap, :821-962), the elevation branch of GlobalManager::composeGlobalMap (global_manager.cpp:2133-2152) and
the costmap layer that consumes it (pointMap_layer.cpp:100-135).

Thin host logic over the C ABI (mrs_gem_*); there is no CPU fallback.  Cell records are numpy arrays of dtype CELL (or anything that
reshapes to [n, 10] 32-bit words) or device tensors of int32 / float32 [n, 10] holding the same words.  The contract, the two quirks it
reproduces and its two fixes are in DESIGN.md 4.19.
"""
import ctypes as C

import numpy as np

from . import _lib

CELL = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("var", "<f4"), ("r", "<i4"), ("g", "<i4"), ("b", "<i4"), ("frontier", "<i4"),
                 ("intensity", "<f4"), ("travers", "<f4")])
WEIGHTED, AS_WRITTEN = 0, 1
THRESH_TRAVERS, THRESH_Z = 0, 1


def _cells(cells):
    """-> (h_cells, d_cells, n): a host array of CELL records or a device tensor [n, 10] of 32-bit words"""
    if hasattr(cells, "is_cuda"):
        if not cells.is_cuda:
            cells = cells.numpy()
        else:
            if cells.dim() != 2 or cells.shape[1] != 10 or cells.element_size() != 4 or not cells.is_contiguous():
                raise ValueError("device cells: expected a contiguous [n, 10] tensor of 32-bit words")
            return None, cells, cells.shape[0]
    a = np.asarray(cells)
    if a.dtype != CELL:
        if a.dtype.itemsize != 4 or a.ndim != 2 or a.shape[1] != 10:
            raise ValueError("cells: expected records of dtype gem.CELL or an [n, 10] array of 32-bit words")
        a = np.ascontiguousarray(a).view(CELL)
    a = np.ascontiguousarray(a.reshape(-1))
    return (a if a.size else None), None, a.size


def _poses(p, what):
    p = np.ascontiguousarray(p, np.float32)
    if p.ndim == 2:
        p = p[None]
    if p.ndim != 3 or p.shape[1:] != (4, 4):
        raise ValueError("%s: expected [n, 4, 4] poses, got %s" % (what, p.shape))
    return p


class ElevationSubmaps(_lib.Handle):
    """The submap store of one robot.  `append_cells` / `append_leaving` fill the open submap, `close_submap(pose, centre)` makes it
    submap K, `update_global(opt_poses)` moves and fuses the closed ones, `submap(i)` / `compose()` read them back; `dropped` and
    `matched` are the counts of the last `update_global`."""
    _destroy = "mrs_gem_destroy"

    def __init__(self, resolution=0.2, rule=WEIGHTED, radius=15.0, min_neighbours=3, device=0):
        self.device = int(device)
        self.resolution = float(resolution)
        self.rule = int(rule)
        self._create("mrs_gem_create", _lib.ctx(self.device), self.resolution, self.rule, float(radius), int(min_neighbours))

    def _counts(self):
        k, n, o = C.c_int32(0), C.c_int64(0), C.c_int64(0)
        _lib.load().mrs_gem_count(self._h, C.byref(k), C.byref(n), C.byref(o))
        return k.value, n.value, o.value

    def __len__(self):
        return self._counts()[0]

    @property
    def n_cells(self):
        return self._counts()[1]

    @property
    def n_open(self):
        """records appended to the open submap so far (replaced ones included)"""
        return self._counts()[2]

    def append_cells(self, cells):
        h, d, n = _cells(cells)
        if n:
            _lib.load().mrs_gem_append_cells(self._h, h, d, n)

    def append_leaving(self, cells, current_xy, shift_xy, length, resolution):
        """the cells of the previous window (positions supplied by the caller) that the window predicate lets into the open submap"""
        h, d, n = _cells(cells)
        if n:
            _lib.load().mrs_gem_append_leaving(self._h, h, d, n, np.ascontiguousarray(current_xy, np.float32).reshape(2),
                                               np.ascontiguousarray(shift_xy, np.float32).reshape(2), int(length), float(resolution))

    def close_submap(self, pose, centre):
        _lib.load().mrs_gem_close_submap(self._h, _poses(pose, "pose")[0], np.ascontiguousarray(centre, np.float32).reshape(2))

    def update_global(self, opt_poses):
        """-> number of cells fused"""
        p = _poses(opt_poses, "opt_poses") if len(opt_poses) else np.zeros((0, 4, 4), np.float32)
        _lib.load().mrs_gem_update_global(self._h, p if p.size else None, p.shape[0])
        return self.matched

    def _stats(self):
        d, m = C.c_int64(0), C.c_int64(0)
        _lib.load().mrs_gem_stats(self._h, C.byref(d), C.byref(m))
        return d.value, m.value

    @property
    def dropped(self):
        return self._stats()[0]

    @property
    def matched(self):
        return self._stats()[1]

    def submap(self, i, device=False):
        """-> (cells, pose [4, 4], centre [2]); cells as CELL records, or with device=True as an int32 tensor [n, 10]"""
        lib, n = _lib.load(), C.c_int64(0)
        pose, centre = np.zeros((4, 4), np.float32), np.zeros(2, np.float32)
        lib.mrs_gem_get_submap(self._h, int(i), None, None, 0, C.byref(n), pose, centre)
        out = self._out(n.value, device)
        if n.value:
            lib.mrs_gem_get_submap(self._h, int(i), None if device else out, out if device else None, n.value, C.byref(n), None, None)
        return out, pose, centre

    def compose(self, device=False):
        """all submaps concatenated in index order"""
        lib, n = _lib.load(), C.c_int64(0)
        lib.mrs_gem_compose(self._h, None, None, 0, C.byref(n))
        out = self._out(n.value, device)
        if n.value:
            lib.mrs_gem_compose(self._h, None if device else out, out if device else None, n.value, C.byref(n))
        return out

    def costmap(self, origin_xy, size_xy, resolution, cloud=None, **thresh):
        """the module-level `costmap` over `cloud`, by default over compose(), which then never leaves the device"""
        return costmap(self.compose(device=True) if cloud is None else cloud, origin_xy, size_xy, resolution, **thresh)

    def _out(self, n, device):
        if device:
            import torch
            return torch.empty((n, 10), dtype=torch.int32, device="cuda:%d" % self.device)
        return np.zeros(n, CELL)


def compose_robots(stores, poses, local_maps=None, refs=None, merge_cells=False, rule=WEIGHTED, resolution=None, device=False):
    """The elevation branch of GlobalManager::composeGlobalMap: poses[r] [len(stores[r]), 4, 4] moves robot r's submaps, refs[r] [4, 4]
    its current local map local_maps[r] (host CELL records, or device tensors [n, 10] of 32-bit words for all robots, which then never
    leave the device); everything concatenated in (robot, submap) order, the local maps last.
    merge_cells=True folds records of equal cell key left to right into one record per cell, in key order.  With device=True the result
    is an int32 tensor [n, 10]."""
    lib = _lib.load()
    if not stores:
        raise ValueError("compose_robots needs at least one store")
    dev = stores[0].device
    P = [_poses(p, "poses[%d]" % r) if len(p) else np.zeros((0, 4, 4), np.float32) for r, p in enumerate(poses)]
    if len(P) != len(stores) or any(p.shape[0] != len(s) for p, s in zip(P, stores)):
        raise ValueError("poses: one [4, 4] pose per submap of every robot")
    P = np.ascontiguousarray(np.concatenate(P, 0)) if P else np.zeros((0, 4, 4), np.float32)
    h_local = d_local = h_off = h_refs = None
    if local_maps is not None:
        if refs is None or len(local_maps) != len(stores):
            raise ValueError("local_maps: one per robot, with refs")
        on_device = [bool(getattr(m, "is_cuda", False)) for m in local_maps]
        h_off = np.zeros(len(stores) + 1, np.int64)
        if any(on_device):
            import torch
            if not all(on_device):
                raise ValueError("local_maps: all on the host or all on the device")
            L = [_cells(m)[1] for m in local_maps]
            h_off[1:] = np.cumsum([m.shape[0] for m in L])
            d_local = torch.cat([m.view(torch.int32) for m in L]).contiguous() if h_off[-1] else None
        else:
            L = [np.ascontiguousarray(np.asarray(m, CELL).reshape(-1)) for m in local_maps]
            h_off[1:] = np.cumsum([m.size for m in L])
            h_local = np.ascontiguousarray(np.concatenate(L)) if h_off[-1] else None
        h_refs = _poses(refs, "refs")
        if h_refs.shape[0] != len(stores):
            raise ValueError("refs: one [4, 4] pose per robot")
    res = float(stores[0].resolution if resolution is None else resolution)
    handles = (C.c_void_p * len(stores))(*[s._h for s in stores])
    n, dropped = C.c_int64(0), C.c_int64(0)
    args = (_lib.ctx(dev), handles, len(stores), P if P.size else None, h_local, d_local, h_off, h_refs, int(bool(merge_cells)), int(rule), res)
    lib.mrs_gem_compose_robots(*args, None, None, 0, C.byref(n), C.byref(dropped))
    cap = n.value
    if device:
        import torch
        out = torch.empty((cap, 10), dtype=torch.int32, device="cuda:%d" % dev)
    else:
        out = np.zeros(cap, CELL)
    if cap:
        lib.mrs_gem_compose_robots(*args, None if device else out, out if device else None, cap, C.byref(n), C.byref(dropped))
    return out[:n.value]


def costmap(cloud, origin_xy, size_xy, resolution, travers_thresh=None, z_thresh=None, device=False):
    """PointMapLayer::updateBounds over `cloud` (CELL records or a device tensor [n, 10]): uint8 [size_y, size_x], 255 = no information,
    254 = lethal, 0 = free; exactly one of travers_thresh / z_thresh selects the threshold type."""
    if (travers_thresh is None) == (z_thresh is None):
        raise ValueError("give exactly one of travers_thresh and z_thresh")
    h, d, n = _cells(cloud)
    dev = _lib.device_of(d) if d is not None else 0
    sx, sy = int(size_xy[0]), int(size_xy[1])
    kind, thresh = (THRESH_TRAVERS, travers_thresh) if z_thresh is None else (THRESH_Z, z_thresh)
    if device:
        import torch
        grid = torch.empty((sy, sx), dtype=torch.uint8, device="cuda:%d" % dev)
    else:
        grid = np.zeros((sy, sx), np.uint8)
    _lib.load().mrs_gem_costmap(_lib.ctx(dev), h, d, n, float(origin_xy[0]), float(origin_xy[1]), sx, sy, float(resolution), kind, float(thresh),
                                None if device else grid, grid if device else None)
    return grid
