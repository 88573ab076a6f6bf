"""CPU suite of the merged global map (row G8): the NumPy restatement tests/golden/globalmap_restate.py against hand-computed cases, and
the host helpers of mr_slam_amd/globalmap.py against it.  No GPU."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import globalmap_restate as G  # noqa: E402
import submap_restate as R  # noqa: E402

from mr_slam_amd.globalmap import compose_keyframe_ids, pose_product  # noqa: E402

F = np.float32
EYE = np.eye(4, dtype=F)

STORE0 = np.array([[0.1, 0.1, 0.1, 1], [0.3, 0.2, 0.4, 3], [np.nan, 0, 0, 1], [-0.05, -0.05, -0.05, 2], [100.25, -200.25, 3.0, 8]], F)
STORE1 = np.array([[0.2, 0.2, 0.2, 5], [1, 1, 1, 6]], F)
SHIFT = EYE.copy()
SHIFT[:3, 3] = [100, -200.5, 2.75]


def test_compose_keyframe_ids():
    assert compose_keyframe_ids(8) == [(0, 1), (3, 4), (6, 7)]
    assert compose_keyframe_ids(0) == [] and compose_keyframe_ids(1) == []
    assert compose_keyframe_ids(2) == [(0, 1)] and compose_keyframe_ids(5, skip=1) == [(0, 1), (1, 2), (2, 3), (3, 4)]
    for n in range(12):
        for skip in (1, 2, 3, 5):
            assert compose_keyframe_ids(n, skip) == G.compose_keyframe_ids(n, skip)


def test_pose_product():
    rng = np.random.default_rng(4)
    for _ in range(20):
        A = R.pose(rng.uniform(-3, 3), rng.uniform(-100, 100, 3))
        B = R.pose(rng.uniform(-3, 3), rng.uniform(-100, 100, 3))
        got = pose_product(A, B)
        assert got.dtype == F and got.shape == (4, 4) and got.tobytes() == G.pose_product(A, B).tobytes()
        exact = A.astype(np.float64) @ B.astype(np.float64)
        # four products and three sums per entry, each rounded once: 7 * 2^-24 of the sum of the terms' magnitudes
        bound = 7 * 2.0 ** -24 * (np.abs(A.astype(np.float64)) @ np.abs(B.astype(np.float64)))
        assert np.all(np.abs(got.astype(np.float64) - exact) <= bound)
        assert got[3].tolist() == [0, 0, 0, 1]
    assert pose_product(EYE, A).tobytes() == A.tobytes() and pose_product(A, EYE).tobytes() == A.tobytes()


def test_hand_case_two_stores():
    want = G.compose([(STORE0, EYE), (STORE1, SHIFT)], 0.5)
    assert want.kept == 6                                       # the NaN point is dropped, nothing is cropped
    assert want.keys.tolist() == [81600, 163813, 492249, 574257, 656675] and want.counts.tolist() == [1, 2, 1, 1, 1]
    assert want.means[0].tolist() == [float(F(-0.05))] * 3 + [2.0] and want.means[1, 3] == 2.0
    assert G.key_bits(want, 0.5) == 20
    # the incremental branch: the old centroids count as ONE point each
    prev = want.means.astype(F)
    again = G.compose([(STORE1, SHIFT)], 0.5, prev=prev)
    assert again.keys.tolist() == want.keys.tolist() and again.counts.tolist() == [1, 1, 2, 1, 2]
    assert again.points[:5].tobytes() == prev.tobytes()         # first, and not moved
    m = (prev[2].astype(np.float64) + R.transform(STORE1, SHIFT)[0].astype(np.float64)) / 2
    assert again.means[2].tolist() == m.tolist()


def test_hand_case_one_cell():
    pts = np.array([[0.25, 0.25, 0.25, 10], [0.75, 0.25, 0.25, 20], [0.3, 0.3, 0.3, 30], [np.inf, 0, 0, 1], [0, -np.inf, 0, 1]], F)
    want = G.compose([(pts, EYE)], 0.5)
    assert want.keys.tolist() == [0, 1] and want.counts.tolist() == [2, 1] and want.kept == 3
    assert np.allclose(want.means[0], [0.275, 0.275, 0.275, 20.0], atol=1e-7) and want.means[1].tolist() == [0.75, 0.25, 0.25, 20.0]
    assert G.key_bits(want, 0.5) == 1
    empty = G.compose([], 0.5)
    assert empty.keys.size == 0 and empty.kept == 0
    assert G.compose([(pts[3:], EYE)], 0.5).keys.size == 0


def test_no_previous_map_equals_the_submap_restatement():
    rng = np.random.default_rng(9)
    segs = [(R.with_intensity(rng.uniform(-40, 40, (3000, 3)), k), R.pose(0.3 * k, (2.0 * k, -k, 0.1 * k))) for k in range(4)]
    a, b = G.compose(segs, 0.3), R.assemble(segs, crop=np.inf, leaf=0.3)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert a.kept == 12000
