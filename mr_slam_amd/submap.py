"""GICP submaps assembled on the GPU from a resident keyframe store (row G0).  Host logic only; the kernels live in csrc/submap.hip.

Replaces GlobalManager::mergeNearestKeyframes (Mapping/src/global_manager/src/global_manager.cpp:1894-1939): the keyframes around a loop
keyframe moved into its frame, pass-through on x and y, exact voxel grid.  What assemble / merge_nearest return is the (points, offsets)
tuple GicpBatch.set_sources / set_targets take, so a submap goes from the store to the registration without leaving the device.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib

F = np.float32
# (point_step, off_x, off_y, off_z, off_intensity) in bytes of a float32 [n, columns] cloud: xyz, the store's x y z i, pcl::PointXYZI
LAYOUTS = {3: (12, 0, 4, 8, -1), 4: (16, 0, 4, 8, 12), 8: (32, 0, 4, 8, 16)}


def nearest_keyframe_ids(loop_id, submap_size, n_keyframes):
    """The keyframes mergeNearestKeyframes merges around loop_id (global_manager.cpp:1901-1905): loop_id + i for i = -submap_size ..
    submap_size, in that order, kept where 0 < id < n_keyframes.  The reference's `keyNear <= 0` skip is kept on purpose (keyframe 0 is
    never merged, a centre of 0 yields only its later neighbours); its `keyNear > size()` test lets id == size() through and reads past
    the vector: that id is dropped here."""
    return [loop_id + i for i in range(-submap_size, submap_size + 1) if 0 < loop_id + i < n_keyframes]


def relative_transform(center_pose, near_pose):
    """currPose.inverse() * nearPose (global_manager.cpp:1908-1911) for rigid row-major 4x4 poses, in float32, every product and sum
    rounded once in the written order (what mrs_submap_merge_nearest computes on the host): Ri = Rc^T,
    ti[i] = -((Ri[i,0] tc[0] + Ri[i,1] tc[1]) + Ri[i,2] tc[2]), T[i,j] = (Ri[i,0] Pk[0,j] + Ri[i,1] Pk[1,j]) + Ri[i,2] Pk[2,j],
    T[i,3] = ((Ri[i,0] Pk[0,3] + Ri[i,1] Pk[1,3]) + Ri[i,2] Pk[2,3]) + ti[i].  -> float32 [4, 4]"""
    Pc, Pk = np.asarray(center_pose, F).reshape(4, 4), np.asarray(near_pose, F).reshape(4, 4)
    Ri, tc = Pc[:3, :3].T, Pc[:3, 3]
    T = np.zeros((4, 4), F)
    T[3, 3] = 1
    for i in range(3):
        ti = -((Ri[i, 0] * tc[0] + Ri[i, 1] * tc[1]) + Ri[i, 2] * tc[2])
        T[i, :3] = (Ri[i, 0] * Pk[0, :3] + Ri[i, 1] * Pk[1, :3]) + Ri[i, 2] * Pk[2, :3]
        T[i, 3] = ((Ri[i, 0] * Pk[0, 3] + Ri[i, 1] * Pk[1, 3]) + Ri[i, 2] * Pk[2, 3]) + ti
    return T


class KeyframeStore(_lib.Handle):
    """One robot's keyframes (thisRobotHandle->keyframes / ->trajectory) resident on one GPU."""
    _destroy = "mrs_keyframes_destroy"

    def __init__(self, device=0, capacity_hint=1 << 20):
        self.device = device
        self._counts = []
        self._create("mrs_keyframes_create", _lib.ctx(device), int(capacity_hint))

    def __len__(self):
        return len(self._counts)

    def append(self, points, pose, intensity_col=None):
        """points: [n, 3 | 4 | 8] float32 or float64, a host array or a device tensor; the intensity is column 3 of a 4-column cloud and
        column 4 of an 8-column one (pcl::PointXYZI) unless intensity_col says otherwise, and 0 for 3 columns.  pose: 4x4.  -> the id"""
        on_device = isinstance(points, torch.Tensor) and points.is_cuda
        if on_device:
            if points.dtype not in (torch.float32, torch.float64):
                points = points.to(torch.float32)
            points = points.contiguous()
            is_double = points.dtype == torch.float64
        else:
            points = np.asarray(points)
            if points.dtype not in (np.float32, np.float64):
                points = points.astype(F)
            points = np.ascontiguousarray(points)
            is_double = points.dtype == np.float64
        if points.ndim != 2 or points.shape[1] not in (3, 4, 8):
            raise ValueError("points must be [n, 3], [n, 4] or [n, 8]")
        n, stride = int(points.shape[0]), int(points.shape[1])
        if intensity_col is None:
            intensity_col = {3: -1, 4: 3, 8: 4}[stride]
        pose = np.ascontiguousarray(np.asarray(pose, F).reshape(16))
        kid = C.c_int32(-1)
        _lib.load().mrs_keyframes_append(self._h, points if n else None, int(on_device), int(is_double), stride, int(intensity_col), n, pose,
                                         C.byref(kid), _lib.current_stream(self.device))
        self._counts.append(n)
        return kid.value

    @staticmethod
    def _blob(cloud, layout):
        """-> (contiguous host array or device tensor, on_device, points, (point_step, off_x, off_y, off_z, off_intensity))"""
        on_device = isinstance(cloud, torch.Tensor) and cloud.is_cuda
        if isinstance(cloud, (bytes, bytearray, memoryview)):
            cloud = np.frombuffer(cloud, np.uint8)
        if layout is None:
            if not on_device:
                cloud = np.asarray(cloud)
            if cloud.ndim != 2 or cloud.shape[1] not in LAYOUTS or str(cloud.dtype).replace("torch.", "") != "float32":
                raise ValueError("a cloud without a layout must be float32 [n, 3], [n, 4] or [n, 8]")
            layout = LAYOUTS[int(cloud.shape[1])]
        elif len(layout) != 5:
            raise ValueError("layout is (point_step, off_x, off_y, off_z, off_intensity)")
        cloud = cloud.contiguous() if on_device else np.ascontiguousarray(cloud)
        nbytes = cloud.numel() * cloud.element_size() if on_device else cloud.nbytes
        step = int(layout[0])
        if step <= 0 or nbytes % step:
            raise ValueError("the blob's size is not a multiple of point_step")
        return cloud, on_device, nbytes // step, tuple(int(v) for v in layout)

    def ingest_batch(self, clouds, poses, leaf=0.3, z_limits=(-1.0, 30.0), intensity=None, layout=None, offsets=None):
        """GlobalManager::mapUpdate's intake (global_manager.cpp:1684-1709) for several raw clouds in one chain of launches: exact voxel grid
        with `leaf`, pass-through on z in z_limits (inclusive), every survivor's intensity set to `intensity` (robotid * 30; None keeps the
        voxel means), the result registered as a keyframe with its pose.  clouds: a list of float32 [n, 3 | 4 | 8] host arrays or device
        tensors of one shape (as append takes them), or of bytes / uint8 blobs with layout = (point_step, off_x, off_y, off_z,
        off_intensity) in bytes (off_intensity -1: none); with `offsets` (int64 [len(poses) + 1], in points) `clouds` is ONE such array or
        blob that holds all of them.  poses: 4x4 each.  -> (ids list, counts int64 [n]: the points each keyframe kept)"""
        poses = np.ascontiguousarray(np.asarray(poses, F).reshape(-1, 16))
        n = int(poses.shape[0])
        if offsets is None:
            parts = [self._blob(c, layout) for c in clouds]
            if len(parts) != n:
                raise ValueError("one pose per cloud")
            if len({(p[1], p[3]) for p in parts}) > 1:
                raise ValueError("the clouds of one call share one layout and one placement")
            offsets = np.concatenate([[0], np.cumsum([p[2] for p in parts])]).astype(np.int64)
            on_device, lay = (parts[0][1], parts[0][3]) if parts else (False, LAYOUTS[4])
            if n == 1:
                data = parts[0][0]
            elif on_device:
                data = torch.cat([p[0].reshape(-1).view(torch.uint8) for p in parts])
            else:
                data = np.concatenate([p[0].reshape(-1).view(np.uint8) for p in parts]) if parts else np.zeros(0, np.uint8)
        else:
            data, on_device, total, lay = self._blob(clouds, layout)
            offsets = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
            if offsets.size != n + 1 or (n and int(offsets[-1]) != total):
                raise ValueError("offsets must be [len(poses) + 1] and end at the blob's point count")
        ids, counts = np.full(n, -1, np.int32), np.zeros(n, np.int64)
        lo, hi = z_limits
        _lib.load().mrs_keyframes_ingest(self._h, n, data if int(offsets[-1]) else None, int(on_device), offsets, lay[0], lay[1], lay[2], lay[3],
                                         lay[4], float(leaf), float(lo), float(hi), int(intensity is not None),
                                         float(0.0 if intensity is None else intensity), poses if n else None, ids if n else None,
                                         counts if n else None, _lib.current_stream(self.device))
        self._counts.extend(int(c) for c in counts)
        return ids.tolist(), counts

    def ingest(self, cloud, pose, leaf=0.3, z_limits=(-1.0, 30.0), intensity=None, layout=None):
        """One raw cloud filtered and registered (see ingest_batch).  -> the id"""
        return self.ingest_batch([cloud], [pose], leaf, z_limits, intensity, layout)[0][0]

    def points(self, kid):
        """A copy of keyframe kid's points -> float32 device tensor [n, 4] (x, y, z, intensity)"""
        kid = int(kid)
        if not 0 <= kid < len(self._counts):
            raise IndexError("keyframe id out of range")
        n = self._counts[kid]
        out = torch.empty((n, 4), dtype=torch.float32, device=f"cuda:{self.device}")
        got = C.c_int64(-1)
        _lib.load().mrs_keyframes_get_points(self._h, kid, out if n else None, 1, n, C.byref(got), _lib.current_stream(self.device))
        assert got.value == n
        return out

    def set_pose(self, kid, pose):
        _lib.load().mrs_keyframes_set_pose(self._h, int(kid), np.ascontiguousarray(np.asarray(pose, F).reshape(16)))

    def pose(self, kid):
        out = np.empty(16, F)
        _lib.load().mrs_keyframes_get_pose(self._h, int(kid), out, None)
        return out.reshape(4, 4)

    def _out(self, capacity):
        return torch.empty((max(int(capacity), 1), 4), dtype=torch.float32, device=f"cuda:{self.device}")

    @staticmethod
    def _trim(out, m):
        """The first m rows of the capacity-sized output buffer.  The buffer holds one row per SEGMENT point (about three times the
        voxels at leaf 0.2), and a view would keep all of it alive for as long as the caller holds the result, so when less than half
        of it is used the rows are copied out (16 B per voxel, on the device) and the buffer is released."""
        return out[:m].clone() if 2 * m < out.shape[0] else out[:m]

    def assemble(self, segments, crop=60.0, leaf=0.2):
        """segments: one list per submap of (keyframe id, T 4x4) pairs.  -> (points float32 device [M, 4], offsets int64 host [B + 1])"""
        sub = np.array([b for b, segs in enumerate(segments) for _ in segs], np.int32)
        kfs = np.array([k for segs in segments for k, _ in segs], np.int32)
        Ts = np.ascontiguousarray(np.array([np.asarray(T, F).reshape(16) for segs in segments for _, T in segs], F).reshape(-1, 16))
        capacity = sum(self._counts[k] for k in kfs if 0 <= k < len(self._counts))
        out, offs = self._out(capacity), np.zeros(len(segments) + 1, np.int64)
        _lib.load().mrs_submap_assemble(self._h, len(segments), int(sub.size), sub if sub.size else None, kfs if sub.size else None,
                                        Ts if sub.size else None, float(crop), float(leaf), out, capacity, offs,
                                        _lib.current_stream(self.device))
        return self._trim(out, int(offs[-1])), offs

    def merge_nearest(self, loop_ids, submap_size, crop=60.0, leaf=0.2):
        """mergeNearestKeyframes for every loop keyframe of loop_ids in one set of launches.  -> (points float32 device [M, 4], offsets
        int64 host [B + 1])"""
        ids = np.ascontiguousarray(loop_ids, dtype=np.int32).reshape(-1)
        n = len(self._counts)
        capacity = sum(self._counts[k] for c in ids for k in nearest_keyframe_ids(int(c), int(submap_size), n))
        out, offs = self._out(capacity), np.zeros(ids.size + 1, np.int64)
        _lib.load().mrs_submap_merge_nearest(self._h, int(ids.size), ids if ids.size else None, int(submap_size), float(crop), float(leaf),
                                             out, capacity, offs, _lib.current_stream(self.device))
        return self._trim(out, int(offs[-1])), offs
