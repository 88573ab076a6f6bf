"""CPU suite of the keyframe intake (row G10): the NumPy restatement tests/golden/intake_restate.py on a case worked by hand and against the
submap restatement, the blob layouts, and the C ABI's declarations.  No GPU."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import intake_restate as K  # noqa: E402
import submap_restate as R  # noqa: E402

from mr_slam_amd import synth  # noqa: E402

F = np.float32
EYE = np.eye(4, dtype=F)

# leaf 0.3, z in [-1, 30], intensity 60; rows x, y, z, i
HAND = np.array([[0.1, 0.1, 0.1, 10], [0.2, 0.25, 0.05, 20], [0.1, 0.1, -1.0, 5], [5.0, 0.1, np.nextafter(F(-1), F(-np.inf)), 5],
                 [5.0, 5.0, 30.0, 7], [5.0, -5.0, np.nextafter(F(30), F(np.inf)), 9], [np.nan, 0, 0, 1], [0, 0, np.inf, 1],
                 [-0.05, -0.05, -0.05, 2]], F)


def test_restatement_on_the_hand_case():
    r = K.ingest(HAND, 0.3, (-1.0, 30.0), 60.0)
    assert r.grid.kept == 7
    assert r.grid.keys.tolist() == [307, 323, 2124, 2755, 63665, 64259]
    assert r.grid.counts.tolist() == [1, 1, 1, 2, 1, 1]
    assert r.keep.tolist() == [True, False, True, True, False, True] and not r.undecided.any()
    want = np.array([[0.1, 0.1, -1.0], [-0.05, -0.05, -0.05], [0.15, 0.175, 0.075], [5, 5, 30]])
    assert r.points.dtype == F and r.points.shape == (4, 4)
    assert np.abs(r.points[:, :3] - want).max() < 1e-7 and r.points[:, 3].tolist() == [60.0] * 4
    assert np.array_equal(r.points[0, :3], HAND[2, :3]) and np.array_equal(r.points[3, :3], HAND[4, :3])      # a voxel of one point is that point
    assert K.ingest(HAND, 0.3, (-1.0, 30.0), None).points[:, 3].tolist() == [5.0, 2.0, 15.0, 7.0]
    # a side switched off
    assert K.ingest(HAND, 0.3, (-np.inf, 30.0), 60.0).points.shape[0] == 5 and K.ingest(HAND, 0.3, (-1.0, np.inf), 60.0).points.shape[0] == 5


def test_restatement_equals_the_submap_restatement_plus_the_z_test():
    c = R.with_intensity(synth.lidar_scan(3, 9000, metric=True), 3)
    c[:, 2] -= F(1.7)
    c[::97, 0] = np.nan
    for leaf, (lo, hi), tag in ((0.3, (-1.0, 30.0), 60.0), (0.2, (0.5, 2.0), None)):
        got = K.ingest(c, leaf, (lo, hi), tag)
        sub = R.assemble([(c, EYE)], crop=3e38, leaf=leaf)
        assert np.array_equal(got.grid.keys, sub.keys) and np.array_equal(got.grid.means, sub.means) and got.grid.kept == sub.kept
        m = sub.means.astype(F)
        want = m[(m[:, 2] >= F(lo)) & (m[:, 2] <= F(hi))]
        if tag is not None:
            want[:, 3] = F(tag)
        assert 0 < want.shape[0] < sub.keys.size and got.points.tobytes() == want.tobytes()


def test_empty_and_emptied_clouds():
    assert K.ingest(np.zeros((0, 4), F)).points.shape == (0, 4)
    assert K.ingest(np.full((5, 4), np.nan, F)).points.shape == (0, 4)
    high = R.with_intensity(np.random.default_rng(1).uniform(40, 50, (100, 3)), 1)
    r = K.ingest(high)
    assert r.grid.keys.size > 0 and r.points.shape == (0, 4)


def test_blob_layouts_decode_to_the_same_points():
    c = R.with_intensity(synth.lidar_scan(1, 600, metric=True), 1)
    for name, layout in K.LAYOUTS.items():
        blob = K.encode(c, layout)
        assert blob.dtype == np.uint8 and blob.size == c.shape[0] * layout[0], name
        got = K.decode(blob, layout)
        assert got[:, :3].tobytes() == c[:, :3].tobytes(), name
        assert np.array_equal(got[:, 3], c[:, 3]) if layout[4] >= 0 else not got[:, 3].any(), name
        assert np.array_equal(K.decode(blob.tobytes(), layout), got)
    assert K.encode(c, K.LAYOUTS["xyzi16"]).tobytes() == c.tobytes()
    from mr_slam_amd import submap
    assert submap.LAYOUTS[4] == K.LAYOUTS["xyzi16"] and submap.LAYOUTS[8] == K.LAYOUTS["pcl32"] and submap.LAYOUTS[3] == K.LAYOUTS["xyz12"]


def test_header_declares_the_intake_functions():
    from mr_slam_amd import _lib
    protos = _lib.parse_header(_lib.HEADER)
    for name in ("mrs_keyframes_ingest", "mrs_keyframes_get_points"):
        assert name in protos and protos[name][0] == "int", name
    assert [p[2] for p in protos["mrs_keyframes_ingest"][1]] == [
        "kf", "n_clouds", "data", "on_device", "h_offsets", "point_step", "off_x", "off_y", "off_z", "off_intensity", "leaf", "z_lo", "z_hi",
        "set_intensity", "intensity", "h_pose16s", "out_ids", "out_counts", "stream"]
    assert [p[2] for p in protos["mrs_keyframes_get_points"][1]] == ["kf", "id", "out", "on_device", "capacity_points", "out_points", "stream"]
    # scalars and pointers only: the header-driven binding needs no new type
    for name in ("mrs_keyframes_ingest", "mrs_keyframes_get_points"):
        for base, depth, _ in protos[name][1]:
            assert depth > 0 or base in _lib._SCALARS or base == "mrs_stream", (name, base)


def test_null_handles_are_rejected_without_a_gpu():
    """the C side's argument checks come before any device work"""
    from mr_slam_amd import _lib
    lib = _lib.load()
    offs, ids, counts, got = np.zeros(1, np.int64), np.zeros(1, np.int32), np.zeros(1, np.int64), np.zeros(1, np.int64)
    for call in (lambda: lib.mrs_keyframes_ingest(None, 0, None, 0, offs, 16, 0, 4, 8, 12, 0.3, -1.0, 30.0, 1, 60.0, None, ids, counts, None),
                 lambda: lib.mrs_keyframes_get_points(None, 0, None, 0, 0, got, None)):
        with pytest.raises(_lib.MrsError) as e:
            call()
        assert e.value.status == 1
