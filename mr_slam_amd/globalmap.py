"""The merged multi-robot point-cloud map composed on the GPU from the robots' keyframe stores (row G8).  Host logic only; the kernels
live in csrc/mapcompose.hip.

Replaces GlobalManager::composeGlobalMap (Mapping/src/global_manager/src/global_manager.cpp:2090-2210) and savingGlobalMap (:143-170):
every robot's keyframes moved by optMapTF * originMapTF, concatenated, one voxel grid over the whole thing.  DESIGN.md section 4.12 is
the contract.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .submap import KeyframeStore

F = np.float32


def compose_keyframe_ids(n_keyframes, skip=3):
    """The (keyframe id, transform index) pairs composeGlobalMap merges for one robot when the map is rebuilt (global_manager.cpp:2161-2164):
    transform k = 1, 1 + skip, 1 + 2 skip ... < n_keyframes moves keyframe k - 1.  The reference's off-by-one (keyframe k - 1 under transform
    k, so the newest keyframe is never merged by this branch) is kept on purpose."""
    return [(k - 1, k) for k in range(1, n_keyframes, skip)]


def pose_product(A, B):
    """A * B for row-major 4x4 float32 matrices (optMapTF[r][k] * originMapTF[r][k]), every product and sum rounded once in float32 in the
    written order: C[i,j] = ((A[i,0] B[0,j] + A[i,1] B[1,j]) + A[i,2] B[2,j]) + A[i,3] B[3,j].  -> float32 [4, 4]"""
    A, B = np.asarray(A, F).reshape(4, 4), np.asarray(B, F).reshape(4, 4)
    out = np.empty((4, 4), F)
    for i in range(4):
        out[i] = ((A[i, 0] * B[0] + A[i, 1] * B[1]) + A[i, 2] * B[2]) + A[i, 3] * B[3]
    return out


class GlobalMap:
    """merged_pointcloud of the Mapping node, resident on the GPU.  stores: the robots' KeyframeStore objects, all on one device."""

    def __init__(self, stores, leaf=0.5):
        self.stores = list(stores)
        if not self.stores:
            raise ValueError("at least one keyframe store is needed")
        self.device = self.stores[0].device
        self.leaf = float(leaf)
        self._handles = (C.c_void_p * len(self.stores))(*[s._h.value for s in self.stores])
        self.points = torch.empty((0, 4), dtype=torch.float32, device=f"cuda:{self.device}")

    def _compose(self, segments, prev):
        segments = list(segments)
        n = len(segments)
        idx = np.array([r for r, _, _ in segments], np.int32)
        kfs = np.array([k for _, k, _ in segments], np.int32)
        Ts = np.ascontiguousarray(np.array([np.asarray(T, F).reshape(16) for _, _, T in segments], F).reshape(-1, 16))
        counts = [self.stores[r]._counts[k] for r, k in zip(idx, kfs) if 0 <= r < len(self.stores) and 0 <= k < len(self.stores[r])]
        n_prev = 0 if prev is None else int(prev.shape[0])
        capacity = n_prev + sum(counts)
        out = self.stores[0]._out(capacity)
        m = C.c_int64(-1)
        _lib.load().mrs_map_compose(len(self.stores), self._handles, n, idx if n else None, kfs if n else None, Ts if n else None,
                                    prev if n_prev else None, n_prev, self.leaf, out, capacity, C.byref(m),
                                    _lib.current_stream(self.device))
        self.points = KeyframeStore._trim(out, m.value)
        return self.points

    def rebuild(self, segments):
        """The mapNeedsToBeCorrected branch (:2142-2168) and savingGlobalMap: the map from nothing.  segments: (store index, keyframe id,
        T 4x4) triples in the order the reference concatenates them.  -> points float32 device [M, 4]"""
        return self._compose(segments, None)

    def add(self, segments):
        """The incremental branch (:2170-2189): VoxelGrid(the map so far + the new keyframes); an old centroid counts as one point."""
        return self._compose(segments, self.points.contiguous())
