"""Inputs shared by tests/test_pclgicp_cpu.py (the margin conditions) and tests/test_pclgicp_gpu.py (the comparisons): the synthetic lidar
pairs of tests/icp_cases.py, PCL_GICP's settings at global_manager.cpp:2422-2425, and the restatement's results, computed once per process."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import icp_cases as K  # noqa: E402
import pclgicp_restate as G  # noqa: E402

MAPPING_2422 = dict(G.MAPPING_2422)
FIXTURES = (3, 4, 5, 6)         # icp_cases.CFGS: the pairs of the step, sums and forced-iteration comparisons
# Seeds of the natural-stopping comparisons: icp_cases.build(seed, 3000).  Seeds 3, 4, 5, 6 run as DESIGN.md 4.15 says (4 / 4 / 3 / 6 outer
# iterations) but fail the inner margin: near convergence their closest Armijo test has f(x + a d) within 9.8e-8 / 1.1e-7 / 4.0e-8 / 1.2e-8
# (relative) of f + 0.01 a g.d.  Of seeds 100-139 at 3000 points these four meet both margins (test_pclgicp_cpu.py).
NATURAL = (100, 109, 117, 132)
NATURAL_POINTS = 3000
MARGIN = K.MARGIN               # outer deltas: a factor 1.25 from 1
INNER_MARGIN = 1e-6             # inner decisions: relative distance from their thresholds
DECREASE_MARGIN = 0.01          # the Armijo tests as decrease against required decrease (a second, scale-free view)
SHIFT = np.array([55.0, -48.0, 3.0])
pose_err, build = K.pose_err, K.build


@functools.lru_cache(maxsize=None)
def pair(seed):
    """(source, target, true transform): icp_cases' pair for its seeds, else build(seed, NATURAL_POINTS)"""
    return K.pair(seed) if seed in K.CFGS else build(seed, NATURAL_POINTS)


@functools.lru_cache(maxsize=None)
def covs(seed):
    """the restatement's covariances of a pair's two clouds (read-only: shared between tests)"""
    src, tgt, _ = pair(seed)
    return G.covariances(src), G.covariances(tgt)


@functools.lru_cache(maxsize=None)
def natural(seed):
    """the restatement's run of a natural-stopping fixture under PCL_GICP's settings"""
    src, tgt, _ = pair(seed)
    return G.gicp(src, tgt, covs=covs(seed), **MAPPING_2422)


@functools.lru_cache(maxsize=None)
def frozen(seed, shift=False):
    """(p, q, M6, pose, pivot) of a fixture's first outer iteration at a pose near the true one; shift: both clouds moved by SHIFT"""
    src, tgt, T = pair(seed)
    CA, CB = covs(seed)
    X = T.copy(); X[:3, 3] += [0.25, -0.1, 0.05]
    if shift:
        src = (src.astype(np.float64) + SHIFT).astype(np.float32)
        tgt = (tgt.astype(np.float64) + SHIFT).astype(np.float32)
        X[:3, 3] += SHIFT - X[:3, :3] @ SHIFT
    corr, _ = G.I.correspondences(src, G.I.Target(tgt), X, 5.0)
    c = G.pivot(tgt)
    return G.frozen_terms(src, tgt, X, corr, CA, CB, c) + (X, c)


def planar(n=3000, seed=0):
    """a planar cloud (z = 0, 40 m x 30 m) and its copy rotated by 3 degrees about z"""
    from scipy.spatial.transform import Rotation as Rot
    rng = np.random.default_rng(seed)
    A = np.zeros((n, 3)); A[:, :2] = rng.uniform(-1, 1, (n, 2)) * [20, 15]
    B = A @ Rot.from_rotvec([0, 0, np.deg2rad(3.0)]).as_matrix().T
    return A.astype(np.float32), B.astype(np.float32)
