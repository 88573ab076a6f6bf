"""Inputs shared by tests/test_icp_cpu.py (the margin condition) and tests/test_icp_gpu.py (the comparisons): synthetic lidar pairs built
like tests/test_gicp_gpu.py::_pair, the two parameter sets with natural stopping, and the restatement's results, computed once per process."""
import functools
import os
import sys

import numpy as np
from scipy.spatial.transform import Rotation as Rot

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import icp_restate as R  # noqa: E402

# (seed, points, rotation vector, translation): the ragged three-pair batch of test_align_batch_within_north_star_tolerance plus a small pair
CFGS = {3: (9000, (0.02, -0.03, 0.08), (0.6, -0.4, 0.1)),
        4: (6001, (0.0, 0.0, -0.05), (-0.8, 0.3, 0.0)),
        5: (12000, (0.01, 0.01, 0.0), (0.1, 0.1, -0.05)),
        6: (1500, (0.02, -0.03, 0.08), (0.6, -0.4, 0.1)),
        # seed 3's trace under MAPPING_890 has an iteration with |t|^2 = 1.17e-3, inside the margin around 1e-3 (test_icp_cpu.py): seed 23 takes
        # its place there; seed 43 is a second pair that ends by REL_MSE (seed 4 ends by TRANSFORM in the iteration where both rules hold)
        23: (9000, (0.02, -0.03, 0.08), (0.6, -0.4, 0.1)),
        43: (9000, (0.02, -0.03, 0.08), (0.6, -0.4, 0.1))}
# global_manager.cpp:890-906 with icp_iters = 50 (launch/global_manager.launch:53)
MAPPING_890 = dict(R.MAPPING_890)
# settings under which the relative change of the mean squared error decides
REL_MSE = dict(max_correspondence_distance=2.0, max_iterations=50, transformation_epsilon=1e-10, rotation_epsilon=1.0 - 1e-12,
               euclidean_fitness_epsilon=1e-3)
# (settings name, seed) of every natural-stopping comparison of the GPU suite
NATURAL = [("MAPPING_890", 23), ("MAPPING_890", 4), ("MAPPING_890", 5), ("MAPPING_890", 6), ("REL_MSE", 3), ("REL_MSE", 4), ("REL_MSE", 43)]
SETTINGS = {"MAPPING_890": MAPPING_890, "REL_MSE": REL_MSE}
MARGIN = 1.25


def build(seed, n, rotvec=(0.02, -0.03, 0.08), t=(0.6, -0.4, 0.1), noise=0.01):
    """(source, target, true transform): a synthetic scan and its moved copy, both with noise (tests/test_gicp_gpu.py::_pair)"""
    from mr_slam_amd import synth
    rng = np.random.default_rng(seed)
    base = synth.lidar_scan(seed, n, metric=True).astype(np.float64)
    Rm = Rot.from_rotvec(rotvec).as_matrix()
    src = (base + rng.normal(0, noise, base.shape)).astype(np.float32)
    tgt = (base @ Rm.T + np.asarray(t) + rng.normal(0, noise, base.shape)).astype(np.float32)
    T = np.eye(4); T[:3, :3] = Rm; T[:3, 3] = t
    return src, tgt, T


@functools.lru_cache(maxsize=None)
def pair(seed):
    n, rotvec, t = CFGS[seed]
    return build(seed, n, rotvec, t)


@functools.lru_cache(maxsize=None)
def natural(name, seed):
    """the restatement's run of a natural-stopping fixture (read-only: shared between tests)"""
    src, tgt, _ = pair(seed)
    return R.icp(src, tgt, **SETTINGS[name])


def pose_err(A, B):
    dt = np.linalg.norm(A[:3, 3] - B[:3, 3])
    dr = np.linalg.norm(Rot.from_matrix(A[:3, :3] @ B[:3, :3].T).as_rotvec())
    return dt, dr
