"""NumPy restatement of the keyframe intake: a raw point blob decoded, exact voxel grid, pass-through on
the z of the float32 means, the intensity tag.

Written from the definition in DESIGN.md section 4.14, not from any reference text.  The voxel grid is section 4.11's and is not restated:
submap_restate.voxel_grid / mean_bound are imported.  NumPy only: the CPU and the GPU suites both import it.
"""
import collections

import numpy as np

import submap_restate as R

F = np.float32

# (point_step, off_x, off_y, off_z, off_intensity) in bytes: the store's own rows, pcl::PointXYZI, bare xyz, a layout with the intensity first
LAYOUTS = {"xyzi16": (16, 0, 4, 8, 12), "pcl32": (32, 0, 4, 8, 16), "xyz12": (12, 0, 4, 8, -1), "ixyz24": (24, 8, 12, 16, 4)}

Result = collections.namedtuple("Result", "points grid keep undecided sure_keep")


def encode(cloud, layout, fill=77.0):
    """float32 [n, 4] (x, y, z, intensity) -> uint8 blob in `layout`; the bytes no field covers hold the float32 `fill`"""
    step, ox, oy, oz, oi = layout
    c = np.asarray(cloud, F)
    rows = np.full((c.shape[0], step // 4), fill, F)
    for col, off in enumerate((ox, oy, oz, oi)):
        if off >= 0:
            rows[:, off // 4] = c[:, col]
    return np.ascontiguousarray(rows).reshape(-1).view(np.uint8)


def decode(blob, layout):
    """uint8 blob (or bytes) -> float32 [n, 4]: the float32 fields at their byte offsets, intensity 0 without a field"""
    step, ox, oy, oz, oi = layout
    b = np.frombuffer(bytes(blob), np.uint8) if isinstance(blob, (bytes, bytearray)) else np.asarray(blob).reshape(-1).view(np.uint8)
    assert step % 4 == 0 and b.size % step == 0
    rows = b.reshape(-1, step)
    out = np.zeros((rows.shape[0], 4), F)
    for col, off in enumerate((ox, oy, oz, oi)):
        if off >= 0:
            out[:, col] = np.ascontiguousarray(rows[:, off:off + 4]).view(F)[:, 0]
    return out


def ingest(cloud, leaf=0.3, z_limits=(-1.0, 30.0), intensity=None):
    """One cloud, float32 [n, 4] -> Result:
    points    float32 [m, 4]: the keyframe (float32 of the float64 means that pass the z test, tagged)
    grid      submap_restate.Result of the voxel grid (all voxels, before the z test)
    keep      bool [voxels]: the z test on the float32 of the restated mean
    undecided bool [voxels]: the mean z lies within the summation bound of a limit AND the voxel's points do not share one z; a conforming
              implementation may keep or drop such a voxel
    sure_keep = keep & ~undecided"""
    c = np.asarray(cloud, F)
    finite = np.isfinite(c[:, :3]).all(axis=1)
    kept = c[finite]
    means, counts, keys, vmax = R.voxel_grid(kept, leaf)
    grid = R.Result(means, counts, keys, vmax, kept.shape[0], kept)
    lo, hi = F(z_limits[0]), F(z_limits[1])
    m32 = means.astype(F)
    keep = (m32[:, 2] >= lo) & (m32[:, 2] <= hi) if keys.size else np.zeros(0, bool)
    undecided = np.zeros(keys.size, bool)
    if keys.size:
        bound = R.mean_bound(counts, vmax)[:, 2]
        near = (np.abs(means[:, 2] - float(lo)) <= bound) | (np.abs(means[:, 2] - float(hi)) <= bound)
        # one z value per voxel: the mean is that value, exactly
        key = R.voxel_keys(kept, leaf)
        order = np.argsort(key, kind="stable")
        inverse = np.unique(key[order], return_inverse=True)[1]
        zmin, zmax = np.full(keys.size, np.inf), np.full(keys.size, -np.inf)
        np.minimum.at(zmin, inverse, kept[order, 2].astype(np.float64))
        np.maximum.at(zmax, inverse, kept[order, 2].astype(np.float64))
        undecided = near & (zmin != zmax)
    pts = m32[keep].copy()
    if intensity is not None:
        pts[:, 3] = F(intensity)
    return Result(pts, grid, keep, undecided, keep & ~undecided)
