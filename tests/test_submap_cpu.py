"""CPU suite of the GICP submap assembly (row G0): the host helpers of mr_slam_amd.submap, the NumPy restatement
tests/golden/submap_restate.py on a case worked by hand, and the C ABI's declarations.  No GPU."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import submap_restate as R  # noqa: E402

from mr_slam_amd import submap  # noqa: E402

F = np.float32

# identity transform, leaf 0.2, crop 60
HAND_POINTS = np.array([[0.1, 0.1, 0.1, 1], [0.15, 0.12, 0.05, 3], [59.99, 0, 0, 5], [60.0, 0, 0, 7], [60.00001, 0, 0, 9],
                        [np.nan, 0, 0, 1], [-0.05, -0.05, -0.05, 2]], F)


@pytest.mark.parametrize("args, want", [((5, 1, 10), [4, 5, 6]), ((0, 1, 10), [1]), ((1, 2, 10), [1, 2, 3]), ((9, 1, 10), [8, 9]),
                                        ((3, 0, 10), [3]), ((0, 0, 10), [])])
def test_nearest_keyframe_ids(args, want):
    assert submap.nearest_keyframe_ids(*args) == want
    assert R.nearest_keyframe_ids(*args) == want


def _random_pose(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    P = np.eye(4)
    P[:3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                 [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                 [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
    P[:3, 3] = rng.uniform(-200, 200, 3)
    return P.astype(F)


def test_relative_transform():
    rng = np.random.default_rng(7)
    poses = [_random_pose(rng) for _ in range(101)]
    for a, b in zip(poses[:-1], poses[1:]):
        same = submap.relative_transform(a, a)
        assert same.dtype == F and np.abs(same - np.eye(4, dtype=F)).max() <= 2.0 ** -22
        got, want = submap.relative_transform(a, b), R.relative_transform(a, b)
        assert got.dtype == F and got.tobytes() == want.tobytes()
        # and it is the inverse times the other pose, to float32 accuracy
        exact = np.linalg.inv(a.astype(np.float64)) @ b.astype(np.float64)
        assert np.abs(got - exact).max() <= 1e-3


def test_restatement_on_the_hand_case():
    r = R.assemble([(HAND_POINTS, np.eye(4, dtype=F))], crop=60.0, leaf=0.2)
    assert r.kept == 5
    assert r.counts.tolist() == [1, 2, 1, 1]
    assert r.keys.tolist() == [0, 907, 1206, 1207]
    assert np.array_equal(r.means[0], np.array([-0.05, -0.05, -0.05, 2], F).astype(np.float64))
    want = (HAND_POINTS[0].astype(np.float64) + HAND_POINTS[1].astype(np.float64)) / 2
    assert np.array_equal(r.means[1], want) and np.abs(want - [0.125, 0.11, 0.075, 2]).max() < 1e-7
    assert r.means[2, 0] == np.float64(F(59.99)) and r.means[3, 0] == 60.0
    assert np.all(np.abs(r.means - r.means.astype(F)) <= R.mean_bound(r.counts, r.vmax))


def test_restatement_empty_and_cropped():
    empty = R.assemble([], 60.0, 0.2)
    assert empty.kept == 0 and empty.means.shape == (0, 4) and empty.keys.size == 0
    far = np.eye(4, dtype=F)
    far[0, 3] = 500
    assert R.assemble([(HAND_POINTS, far)], 60.0, 0.2).kept == 0


def test_header_declares_the_submap_functions():
    from mr_slam_amd import _lib
    protos = _lib.parse_header(_lib.HEADER)
    for name in ("mrs_keyframes_create", "mrs_keyframes_destroy", "mrs_keyframes_size", "mrs_keyframes_append", "mrs_keyframes_set_pose",
                 "mrs_keyframes_get_pose", "mrs_submap_assemble", "mrs_submap_merge_nearest"):
        assert name in protos and protos[name][0] == "int", name
    assert [p[2] for p in protos["mrs_submap_merge_nearest"][1]] == ["kf", "n_submaps", "h_loop_ids", "submap_size", "crop", "leaf", "d_out",
                                                                    "capacity_points", "h_offsets", "stream"]


def test_null_handles_are_rejected_without_a_gpu():
    """the C side's argument checks come before any device work"""
    from mr_slam_amd import _lib
    lib = _lib.load()
    n = np.zeros(1, np.int32)
    for call in (lambda: lib.mrs_keyframes_size(None, n, None), lambda: lib.mrs_keyframes_set_pose(None, 0, np.eye(4, dtype=F).reshape(16)),
                 lambda: lib.mrs_submap_merge_nearest(None, 0, None, 1, 60.0, 0.2, None, 0, np.zeros(1, np.int64), None)):
        with pytest.raises(_lib.MrsError) as e:
            call()
        assert e.value.status == 1
