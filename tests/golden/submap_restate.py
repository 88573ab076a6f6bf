"""NumPy restatement of the GICP submap assembly: keyframes moved into the loop keyframe's frame,
pass-through on x and y, exact voxel grid.

Written from the definition in DESIGN.md section 4.11, not from any reference text.  Every operation on a point is one float32
operation, in the written order (NumPy rounds each float32 operation once and fuses nothing), so the cells and keys are the bits any
conforming implementation must produce; only the per-voxel sums are kept wider (float64), as the yardstick the float32 summation bound
is measured against.  NumPy only: the CPU and the GPU suites both import it.
"""
import collections

import numpy as np

F = np.float32

Result = collections.namedtuple("Result", "means counts keys vmax kept points")


def nearest_keyframe_ids(loop_id, submap_size, n_keyframes):
    """loop_id + i for i = -submap_size .. submap_size, kept where 0 < id < n_keyframes"""
    return [loop_id + i for i in range(-submap_size, submap_size + 1) if 0 < loop_id + i < n_keyframes]


def relative_transform(center_pose, near_pose):
    """inverse(center) * near for rigid float32 4x4 poses, term by term in float32 -> float32 [4, 4]"""
    Pc, Pk = np.asarray(center_pose, F).reshape(4, 4), np.asarray(near_pose, F).reshape(4, 4)
    Ri = Pc[:3, :3].T.copy()
    tc = Pc[:3, 3]
    T = np.zeros((4, 4), F)
    T[3, 3] = F(1)
    for i in range(3):
        ti = -((Ri[i, 0] * tc[0] + Ri[i, 1] * tc[1]) + Ri[i, 2] * tc[2])
        for j in range(3):
            T[i, j] = (Ri[i, 0] * Pk[0, j] + Ri[i, 1] * Pk[1, j]) + Ri[i, 2] * Pk[2, j]
        T[i, 3] = ((Ri[i, 0] * Pk[0, 3] + Ri[i, 1] * Pk[1, 3]) + Ri[i, 2] * Pk[2, 3]) + ti
    return T


def transform(points, T):
    """points float32 [n, 4] (x, y, z, intensity) moved by T (float32 [4, 4]); the intensity is carried through"""
    p, T = np.asarray(points, F), np.asarray(T, F)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    out = np.empty_like(p)
    with np.errstate(all="ignore"):
        for i in range(3):
            out[:, i] = ((T[i, 0] * x + T[i, 1] * y) + T[i, 2] * z) + T[i, 3]
    out[:, 3] = p[:, 3]
    return out


def passthrough(points, crop):
    """the rows with finite x, y, z and -crop <= x, y <= crop (both ends inclusive; z is not cropped)"""
    p, c = np.asarray(points, F), F(crop)
    with np.errstate(invalid="ignore"):
        keep = np.isfinite(p[:, :3]).all(axis=1) & (p[:, 0] >= -c) & (p[:, 0] <= c) & (p[:, 1] >= -c) & (p[:, 1] <= c)
    return p[keep]


def voxel_keys(points, leaf):
    """int64 key per (already cropped) point: cell = floor(v * (1 / leaf)) in float32, relative to the component-wise minimum cell"""
    inv = F(1) / F(leaf)
    cell = np.floor(np.asarray(points, F)[:, :3] * inv).astype(np.int64)
    mn = cell.min(axis=0)
    div = cell.max(axis=0) - mn + 1
    assert float(div[0]) * float(div[1]) * float(div[2]) < 2.0 ** 63, "key does not fit in 63 bits"
    c = cell - mn
    return c[:, 0] + c[:, 1] * div[0] + c[:, 2] * (div[0] * div[1])


def voxel_grid(points, leaf):
    """-> (means float64 [m, 4], counts int64 [m], keys int64 [m] ascending, vmax float64 [m, 4] = max |v| per voxel and channel)"""
    p = np.asarray(points, F)
    if p.shape[0] == 0:
        return np.zeros((0, 4)), np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros((0, 4))
    key = voxel_keys(p, leaf)
    order = np.argsort(key, kind="stable")
    keys, inverse, counts = np.unique(key[order], return_inverse=True, return_counts=True)
    p64 = p[order].astype(np.float64)
    sums = np.zeros((keys.size, 4))
    np.add.at(sums, inverse, p64)
    vmax = np.zeros((keys.size, 4))
    np.maximum.at(vmax, inverse, np.abs(p64))
    return sums / counts[:, None], counts.astype(np.int64), keys.astype(np.int64), vmax


def assemble(segments, crop=60.0, leaf=0.2):
    """One submap from segments [(points float32 [n, 4], T float32 [4, 4]), ...] -> Result(means, counts, keys, vmax, kept, points):
    `points` are the kept, transformed float32 points in segment order (what the voxel grid saw)."""
    parts = [passthrough(transform(p, T), crop) for p, T in segments]
    pts = np.concatenate(parts) if parts else np.zeros((0, 4), F)
    means, counts, keys, vmax = voxel_grid(pts, leaf)
    return Result(means, counts, keys, vmax, pts.shape[0], pts)


def merge_nearest(clouds, poses, loop_id, submap_size, crop=60.0, leaf=0.2):
    """The submap around keyframe loop_id of a store (clouds: float32 [n_k, 4] each, poses: float32 [4, 4] each)"""
    ids = nearest_keyframe_ids(loop_id, submap_size, len(clouds))
    return assemble([(clouds[k], relative_transform(poses[loop_id], poses[k])) for k in ids], crop, leaf)


def mean_bound(counts, vmax):
    """[m, 4]: (count + 1) * 2^-24 * max(max |v|, 1), the float32 summation bound in any order plus the final rounding"""
    return (np.asarray(counts, np.float64)[:, None] + 1.0) * 2.0 ** -24 * np.maximum(vmax, 1.0)


def pose(yaw, t):
    """float32 4x4: rotation by yaw about z, translation t"""
    c, s = np.cos(yaw), np.sin(yaw)
    P = np.eye(4, dtype=F)
    P[:3, :3] = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], F)
    P[:3, 3] = np.asarray(t, F)
    return P


def with_intensity(xyz, seed):
    """[n, 3] -> float32 [n, 4] with a seeded intensity column in [0, 255)"""
    xyz = np.asarray(xyz, F)
    i = np.random.default_rng(seed).uniform(0, 255, xyz.shape[0]).astype(F)
    return np.ascontiguousarray(np.concatenate([xyz[:, :3], i[:, None]], axis=1))
