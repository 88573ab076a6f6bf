"""Inputs shared by tests/test_icp_plane_cpu.py (the conditions on the fixtures) and tests/test_icp_plane_gpu.py (the comparisons): the
synthetic lidar pairs of tests/icp_cases.py plus one smaller pair, the parameter sets with natural stopping, the clouds of the normals
tests, and the restatement's results, computed once per process."""
import functools
import os
import sys

import numpy as np

import icp_cases as K

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import icp_plane_restate as PR  # noqa: E402

R = K.R
MARGIN = K.MARGIN
SETTINGS = K.SETTINGS
# seed 103: seed 3's motion on 3000 points
CFGS = dict(K.CFGS)
CFGS[103] = (3000, (0.02, -0.03, 0.08), (0.6, -0.4, 0.1))
# (settings name, seed) of every natural-stopping comparison of the GPU suite: the fixtures of tests/icp_cases.py whose point-to-plane
# traces keep every criterion a factor 1.25 from its threshold (test_icp_plane_cpu.py checks that)
NATURAL = [("MAPPING_890", 5), ("MAPPING_890", 6), ("MAPPING_890", 43), ("MAPPING_890", 103), ("REL_MSE", 3), ("REL_MSE", 4), ("REL_MSE", 6)]
NORMAL_K = (15, 5)
VIEWPOINTS = ((0.0, 0.0, 0.0), (5.0, -3.0, 2.0))
# largest deviation of lambda0 / (lambda0 + lambda1 + lambda2) from the host build of eig3.hpp against eigvalsh on the covariances of the
# clouds below (measured 2.85e-16; test_icp_plane_cpu.py keeps it true): the GPU suite allows 4 x this plus half a float32 ulp
EIG3_CURVATURE_DEV = 3e-16


@functools.lru_cache(maxsize=None)
def pair(seed):
    n, rotvec, t = CFGS[seed]
    return K.build(seed, n, rotvec, t)


@functools.lru_cache(maxsize=None)
def target_normals(seed, k=15, viewpoint=(0.0, 0.0, 0.0)):
    return PR.normals(pair(seed)[1], k, viewpoint)


@functools.lru_cache(maxsize=None)
def natural(name, seed):
    """the restatement's run of a natural-stopping fixture (read-only: shared between tests)"""
    src, tgt, _ = pair(seed)
    return PR.icp(src, tgt, target_normals(seed)["normals"], **SETTINGS[name])


@functools.lru_cache(maxsize=None)
def normal_clouds():
    """name -> cloud [n, 3] float32 of the normals tests: a synthetic scan, a cloud smaller than k, a cloud too small for a normal and a
    cloud on an exact plane (coordinates on a dyadic grid: every product and sum of the covariance is exact)"""
    from mr_slam_amd import synth
    rng = np.random.default_rng(11)
    scan = (synth.lidar_scan(31, 4000, metric=True).astype(np.float64) + rng.normal(0, 0.01, (4000, 3))).astype(np.float32)
    ten = rng.normal(size=(10, 3)).astype(np.float32)
    two = rng.normal(size=(2, 3)).astype(np.float32)
    uv = rng.permutation(64 * 64)[:1500]
    u, v = (uv // 64 - 32) / 8.0, (uv % 64 - 32) / 8.0
    plane = np.stack([u, v, 0.5 * u - 0.25 * v + 3.0], 1).astype(np.float32)
    return {"scan": scan, "ten": ten, "two": two, "plane": plane}


@functools.lru_cache(maxsize=None)
def cloud_normals(name, k, viewpoint):
    return PR.normals(normal_clouds()[name], k, viewpoint)


def unreliable(w, gap=1e-6, level=1e-6):
    """points whose normal direction or orientation a rounding error may change: eigen-gap (l1 - l0) / l2 below `gap`, or the viewpoint
    within `level` of the tangent plane"""
    lam = w["lam"]
    with np.errstate(invalid="ignore", divide="ignore"):
        return ~((lam[:, 1] - lam[:, 0]) / lam[:, 2] >= gap) | ~(w["toward"] > level)


pose_err = K.pose_err
