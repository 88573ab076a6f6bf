"""NumPy restatement of the merged multi-robot map: the previous map as it is, then every segment moved by
its transform, non-finite points dropped, ONE exact voxel grid over everything.

Written from the definition in DESIGN.md section 4.12; the point arithmetic, cells, keys and the mean bound are section 4.11's, taken from
submap_restate.py unchanged.  NumPy only: the CPU and the GPU suites both import it.
"""
import numpy as np

import submap_restate as R

F = np.float32


def compose_keyframe_ids(n_keyframes, skip=3):
    """(keyframe id, transform index): transform k = 1, 1 + skip, ... < n_keyframes moves keyframe k - 1"""
    out, k = [], 1
    while k < n_keyframes:
        out.append((k - 1, k))
        k += skip
    return out


def pose_product(A, B):
    """A * B, float32, C[i,j] = ((A[i,0] B[0,j] + A[i,1] B[1,j]) + A[i,2] B[2,j]) + A[i,3] B[3,j] -> float32 [4, 4]"""
    A, B = np.asarray(A, F).reshape(4, 4), np.asarray(B, F).reshape(4, 4)
    out = np.zeros((4, 4), F)
    for i in range(4):
        for j in range(4):
            out[i, j] = ((A[i, 0] * B[0, j] + A[i, 1] * B[1, j]) + A[i, 2] * B[2, j]) + A[i, 3] * B[3, j]
    return out


def compose(segments, leaf, prev=None):
    """segments [(points float32 [n, 4], T float32 [4, 4]), ...]; prev: float32 [n_prev, 4] put FIRST and not moved (an old centroid is one
    point).  -> submap_restate.Result(means, counts, keys, vmax, kept, points)"""
    inf = F(np.inf)
    parts = [] if prev is None else [R.passthrough(np.asarray(prev, F).reshape(-1, 4), inf)]
    parts += [R.passthrough(R.transform(p, T), inf) for p, T in segments]
    pts = np.concatenate(parts) if parts else np.zeros((0, 4), F)
    means, counts, keys, vmax = R.voxel_grid(pts, leaf)
    return R.Result(means, counts, keys, vmax, pts.shape[0], pts)


def key_bits(result, leaf):
    """the number of bits the grid's largest possible key needs (what the device-wide sort is narrowed to)"""
    inv = F(1) / F(leaf)
    cell = np.floor(result.points[:, :3] * inv).astype(np.int64)
    div = cell.max(axis=0) - cell.min(axis=0) + 1
    return max(1, int(int(div[0]) * int(div[1]) * int(div[2]) - 1).bit_length())
