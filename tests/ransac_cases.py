"""Inputs shared by tests/test_ransac_cpu.py (the margin condition, recovery) and tests/test_ransac_gpu.py (the exact comparisons): seeded
correspondence sets -- a planted pose plus Gaussian noise on the inliers, uniform outliers -- and the restatement's results, computed once
per process.  A fixture whose seed puts a residual within 1e-9 d^2 of d^2 is replaced here, never tolerated there."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import fpfh_restate as F  # noqa: E402
import ransac_restate as R  # noqa: E402

TILE = 512                       # kTile of mr_slam_amd/csrc/ransac.hip
MARGIN = 1e-9
ANGLE = 0.7
TRUE_R = np.array([[np.cos(ANGLE), -np.sin(ANGLE), 0.0], [np.sin(ANGLE), np.cos(ANGLE), 0.0], [0.0, 0.0, 1.0]])
TRUE_T = np.array([3.0, -2.0, 0.5])
D = 0.3                          # max_distance of every fixture


def make(seed, M, inl=0.5, noise=0.02, stride=3, mirror=False):
    """(src, dst float32 [M, stride], planted inlier flags): points in a flat 60 m box (within +-64 m after the pose)"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-30, 30, (M, 3)).astype(np.float32)
    p[:, 2] *= np.float32(0.1)
    q = p.astype(np.float64) @ TRUE_R.T + TRUE_T + rng.normal(0, noise, (M, 3))
    if mirror:
        q[:, 0] = -q[:, 0]
    out = rng.random(M) >= inl
    q[out] = rng.uniform(-30, 30, (int(out.sum()), 3))
    src = np.zeros((M, stride), np.float32)
    dst = np.zeros((M, stride), np.float32)
    src[:, :3], dst[:, :3] = p, q.astype(np.float32)
    src[:, 3:], dst[:, 3:] = 7.0, -7.0                          # padding columns must not be read
    return src, dst, ~out


def exact(seed, M):
    """all inliers, no noise, and a pose float32 holds exactly: a quarter turn about z and a dyadic translation on a 1/64 m lattice"""
    rng = np.random.default_rng(seed)
    p = (rng.integers(-30 * 64, 30 * 64, (M, 3)) / 64.0).astype(np.float32)
    T = np.eye(4)
    T[:3, :3] = [[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]
    T[:3, 3] = [3.0, -2.0, 0.5]
    q = p.astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    assert np.array_equal(q.astype(np.float32).astype(np.float64), q)
    return p, q.astype(np.float32), T


def _repeated(seed):
    src, dst, _ = make(seed, 200)
    src[:20], dst[:20] = src[0], dst[0]                          # coincident on both sides
    src[20:40] = src[1]                                          # coincident sources, different targets
    src[150:], dst[150:] = src[50:100], dst[50:100]              # repeated correspondences
    return src, dst


def _dead(seed):
    src, dst, _ = make(seed, 200)
    src[3, 0] = np.nan; dst[10, 2] = np.nan; src[17, 1] = np.inf; dst[40, 0] = -np.inf
    src[77] = np.nan; dst[77] = np.nan; dst[120, 1] = np.inf; src[199, 2] = np.nan
    return src, dst


def _all_rejected(seed):
    src, _, _ = make(seed, 100)
    return src, (2 * src).astype(np.float32)


# name -> (builder of (src, dst), seed of the draw, parameters).  Sizes around the wave (64), the chunk of hypotheses (256) and the LDS tile.
CASES = {}
for _M in (0, 1, 2, 3, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 5):
    CASES["M%d" % _M] = (functools.partial(lambda M: make(100 + M, M, inl=1.0 if M == 3 else 0.5)[:2], _M), 1000 + _M, dict(hypotheses=256))
for _H in (1, 63, 64, 65, 256, 1000):
    CASES["H%d" % _H] = (lambda: make(7, 200, inl=0.6)[:2], 5, dict(hypotheses=_H))
CASES["all_rejected"] = (lambda: _all_rejected(11), 3, dict(hypotheses=256))
CASES["repeated"] = (lambda: _repeated(12), 4, dict(hypotheses=256))
CASES["dead"] = (lambda: _dead(13), 6, dict(hypotheses=256))
CASES["exact"] = (lambda: exact(14, 300)[:2], 8, dict(hypotheses=64))
CASES["mirror"] = (lambda: make(15, 120, inl=1.0, noise=0.0, mirror=True)[:2], 9, dict(hypotheses=256))
CASES["no_refit"] = (lambda: make(16, 200)[:2], 10, dict(hypotheses=256, refine_iters=0))
CASES["stride5"] = (lambda: make(16, 200, stride=5)[:2], 10, dict(hypotheses=256))
CASES["no_edge_test"] = (lambda: make(17, 80, inl=0.7)[:2], 12, dict(hypotheses=128, edge_similarity=0.0, min_sin2=0.0))
# noisy inliers: the refit changes the count; in the first the count also goes DOWN again (70 -> 86 -> 87 -> 86: the result is iterate 2)
CASES["refit_changes"] = (lambda: make(2, 200, inl=0.5, noise=0.12)[:2], 2000003 + 7, dict(hypotheses=256))
CASES["refit_rises"] = (lambda: make(5, 200, inl=0.5, noise=0.12)[:2], 5000015 + 7, dict(hypotheses=256))
# few correspondences: several hypotheses share the best count
CASES["tie"] = (lambda: make(21, 12, inl=0.6)[:2], 13, dict(hypotheses=64))
# the ragged batch: nine pairs, an empty one in the middle, one with dead rows
BATCH = ["H256", "M65", "M%d" % (TILE + 1), "M3", "M0", "dead", "M64", "refit_changes", "tie"]
BATCH_H = 256


@functools.lru_cache(maxsize=None)
def inputs(name):
    src, dst = CASES[name][0]()
    src.setflags(write=False); dst.setflags(write=False)
    return src, dst


def params(name):
    p = dict(R.DEFAULTS)
    p.update(CASES[name][2])
    return p


@functools.lru_cache(maxsize=None)
def expected(name, hypotheses=None):
    """the restatement's result for a case (with another hypothesis count when given: the batch runs all its pairs at BATCH_H)"""
    src, dst = inputs(name)
    p = params(name)
    if hypotheses is not None:
        p["hypotheses"] = hypotheses
    return R.ransac(src, dst, CASES[name][1], D, **p)


def pack(names):
    """(src, dst [total, 3], offsets int64, seeds uint64) of several cases as one ragged batch (stride 3 cases only)"""
    parts = [inputs(n) for n in names]
    offsets = np.zeros(len(names) + 1, np.int64)
    np.cumsum([s.shape[0] for s, _ in parts], out=offsets[1:])
    return (np.concatenate([s[:, :3] for s, _ in parts]), np.concatenate([d[:, :3] for _, d in parts]), offsets,
            np.array([CASES[n][1] for n in names], np.uint64))


# ---- end to end: a cloud and its rigid copy ---------------------------------------------------------------------------------------------
E2E_D = 0.05                     # max_distance; the scene is a 1 m box with 2 mm noise
E2E_T = np.array([0.4, -0.3, 0.2])
E2E_ROTVEC = (0.1, -0.2, 0.5)


@functools.lru_cache(maxsize=None)
def e2e_scene(seed=31):
    """the FPFH scene (two planes and a sphere patch, perturbed normals) and its rigid copy: points and normals moved, the order permuted.
    -> (points, normals, points2, normals2, where: point i of the first cloud is point where[i] of the second, rotation)"""
    from scipy.spatial.transform import Rotation as Rot
    pts, nrm = F.scene(seed, perturb=0.05)
    perm = np.random.default_rng(seed + 1).permutation(len(pts))
    Rm = Rot.from_rotvec(E2E_ROTVEC).as_matrix()
    pts2 = (pts.astype(np.float64) @ Rm.T + E2E_T).astype(np.float32)[perm]
    nrm2 = (nrm.astype(np.float64) @ Rm.T).astype(np.float32)[perm]
    where = np.empty_like(perm)
    where[perm] = np.arange(len(perm))
    return pts, nrm, pts2, nrm2, where, Rm
