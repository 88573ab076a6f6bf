"""GPU suite of the GICP submap assembly (row G0, csrc/submap.hip) against the NumPy restatement tests/golden/submap_restate.py.

For every comparison the voxel count and the output order are exact, and every mean lies within (m + 1) * 2^-24 * max(max |v|, 1) of the
restatement's float64 mean, per voxel and per channel (m = the voxel's point count, max |v| = the largest magnitude it averaged): the
float32 summation bound for any order plus the final rounding, the magnitude floored at 1.  The order is checked twice: position by
position against the restatement's means (ascending key), and by recomputing the key of every returned mean on the restatement's grid
wherever that mean is further than its bound from a cell boundary.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import submap_restate as R  # noqa: E402

from mr_slam_amd import _lib, synth  # noqa: E402
from mr_slam_amd.submap import KeyframeStore, relative_transform  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
EYE = np.eye(4, dtype=F)


@functools.lru_cache(maxsize=None)
def _cloud(seed, n):
    c = R.with_intensity(synth.lidar_scan(seed, n, metric=True), seed)
    c.setflags(write=False)
    return c


def _pose(k):
    return R.pose(0.1 * k, (3.0 * k, 0.5 * k, 0.02 * k))


def _submap(points, offs, b):
    return points[int(offs[b]):int(offs[b + 1])].cpu().numpy()


def _check(got, want, leaf, min_sure=0.5):
    """got: float32 [m, 4] from the device; want: the restatement's Result; min_sure: the least share of voxels whose mean must lie clear of
    every cell boundary (so that the key check is not vacuous; 0 for clouds built ON the boundaries)"""
    assert got.shape[0] == want.keys.size, (got.shape[0], want.keys.size)
    if want.keys.size == 0:
        return
    bound = R.mean_bound(want.counts, want.vmax)
    err = np.abs(got.astype(np.float64) - want.means)
    worst = (err / bound).max()
    print("voxels %d kept %d largest voxel %d worst error / bound %.3f" % (want.keys.size, want.kept, want.counts.max(), worst))
    assert np.all(err <= bound), worst
    # the key of every returned mean, on the restatement's grid
    inv = F(1) / F(leaf)
    cell = np.floor(want.points[:, :3] * inv).astype(np.int64)
    mn = cell.min(axis=0)
    div = cell.max(axis=0) - mn + 1
    scaled = got[:, :3].astype(np.float64) * float(inv)
    sure = (np.abs(scaled - np.round(scaled)) > 2 * bound[:, :3] * float(inv)).all(axis=1)
    c = np.floor(got[:, :3] * inv).astype(np.int64) - mn
    keys = c[:, 0] + c[:, 1] * div[0] + c[:, 2] * (div[0] * div[1])
    assert np.array_equal(keys[sure], want.keys[sure])
    print("share of voxels whose key is recomputed: %.3f" % sure.mean())
    assert sure.mean() >= min_sure or want.keys.size < 8
    assert np.all(np.diff(want.keys) > 0)


HAND = np.array([[0.1, 0.1, 0.1, 1], [0.15, 0.12, 0.05, 3], [59.99, 0, 0, 5], [60.0, 0, 0, 7], [60.00001, 0, 0, 9], [np.nan, 0, 0, 1],
                 [-0.05, -0.05, -0.05, 2]], F)


def test_hand_case():
    s = KeyframeStore()
    assert s.append(HAND, EYE) == 0 and len(s) == 1
    pts, offs = s.assemble([[(0, EYE)]])
    assert pts.dtype == torch.float32 and pts.is_cuda and pts.shape[1] == 4 and offs.dtype == np.int64 and offs.tolist() == [0, 4]
    got = pts.cpu().numpy()
    want = R.assemble([(HAND, EYE)])
    assert want.keys.tolist() == [0, 907, 1206, 1207]
    _check(got, want, 0.2)
    assert got[0].tolist() == [F(-0.05), F(-0.05), F(-0.05), 2.0] and got[3, 0] == 60.0 and got[1, 3] == 2.0


@functools.lru_cache(maxsize=None)
def _three():
    clouds = [_cloud(k, 20000) for k in range(3)]
    poses = [_pose(k) for k in range(3)]
    s = KeyframeStore()
    for c, p in zip(clouds, poses):
        s.append(c, p)
    return s, clouds, poses


@pytest.mark.parametrize("crop, leaf", [(60.0, 0.2), (10.0, 0.5), (60.0, 0.05)])
def test_three_keyframes(crop, leaf):
    s, clouds, poses = _three()
    pts, offs = s.merge_nearest([1], 1, crop=crop, leaf=leaf)
    want = R.merge_nearest(clouds, poses, 1, 1, crop, leaf)
    assert want.kept > 1000 and offs[0] == 0 and offs[1] == pts.shape[0]
    _check(pts.cpu().numpy(), want, leaf)
    # all three keyframes through explicit segments (merge_nearest never takes keyframe 0)
    segs = [(k, relative_transform(poses[0], poses[k])) for k in range(3)]
    pts, offs = s.assemble([segs], crop=crop, leaf=leaf)
    _check(pts.cpu().numpy(), R.assemble([(clouds[k], T) for k, T in segs], crop, leaf), leaf)


def test_batch_equals_single_calls():
    sizes = [5000, 20000, 7777, 12001, 1024, 9000]              # 1024 = exactly one tile, the others end in a partial one
    clouds = [_cloud(10 + k, n) for k, n in enumerate(sizes)]
    poses = [_pose(k) for k in range(6)]
    s = KeyframeStore()
    for c, p in zip(clouds, poses):
        s.append(c, p)
    centres = [1, 0, 5, 3, 3]
    far = EYE.copy()
    far[0, 3] = 500.0
    segments = [[(k, relative_transform(poses[c], poses[k])) for k in R.nearest_keyframe_ids(c, 2, 6)] for c in centres] + [[(2, far)], []]
    pts, offs = s.assemble(segments)
    assert np.all(np.diff(offs) >= 0) and offs[0] == 0 and offs[-1] == pts.shape[0]
    assert offs[5] == offs[6] == offs[7]                       # cropped away / no segment
    assert np.array_equal(_submap(pts, offs, 3), _submap(pts, offs, 4)) and offs[4] > offs[3]
    again, offs2 = s.assemble(segments)
    assert np.array_equal(offs, offs2) and torch.equal(pts.view(torch.int32), again.view(torch.int32))
    merged, moffs = s.merge_nearest(centres, 2)
    assert np.array_equal(moffs, offs[:6]) and torch.equal(merged.view(torch.int32), pts[:int(offs[5])].view(torch.int32))
    for b, c in enumerate(centres):
        one, o1 = s.merge_nearest([c], 2)
        got = _submap(pts, offs, b)
        assert o1.tolist() == [0, got.shape[0]] and one.cpu().numpy().tobytes() == got.tobytes()
        _check(got, R.merge_nearest(clouds, poses, c, 2), 0.2)
    assert s.assemble([[(2, far)]])[1].tolist() == [0, 0] and s.assemble([[]])[1].tolist() == [0, 0] and s.assemble([])[1].tolist() == [0]


def _adversarial():
    rng = np.random.default_rng(3)
    leaf = F(0.2)
    out = {}
    k = rng.integers(-250, 250, size=(1366, 3)).astype(F) * leaf                       # exact multiples of the leaf and their neighbours
    out["multiples"] = np.concatenate([k, np.nextafter(k, F(np.inf)), np.nextafter(k, F(-np.inf))])
    out["around_zero"] = rng.uniform(-0.3, 0.3, size=(4096, 3)).astype(F)
    out["one_point"] = np.tile(np.array([[12.3, -45.6, 1.7]], F), (25000, 1))
    edge = rng.uniform(-59, 59, size=(4096, 3)).astype(F)
    for i, v in enumerate([60.0, -60.0, np.nextafter(F(60), F(np.inf)), np.nextafter(F(-60), F(-np.inf))]):
        edge[i::16, 0] = v
        edge[i + 4::16, 1] = v
    out["crop_edge"] = edge
    tall = rng.uniform(-60, 60, size=(8000, 3)).astype(F)
    tall[:, 2] = rng.uniform(-1e4, 1e4, 8000).astype(F)
    out["tall"] = tall
    bad = rng.uniform(-30, 30, size=(4096, 3)).astype(F)
    for i, v in enumerate([np.nan, np.inf, -np.inf]):
        for axis in range(3):
            bad[3 * i + axis::40, axis] = v
    out["non_finite"] = bad
    return {name: R.with_intensity(c, 5) for name, c in out.items()}


def test_adversarial_clouds():
    clouds = _adversarial()
    s = KeyframeStore()
    for c in clouds.values():
        s.append(c, EYE)
    pts, offs = s.assemble([[(k, EYE)] for k in range(len(clouds))])
    for b, (name, c) in enumerate(clouds.items()):
        want = R.assemble([(c, EYE)])
        print(name, end=": ")
        _check(_submap(pts, offs, b), want, 0.2, min_sure=0.0 if name == "multiples" else 0.5)      # "multiples" sits ON the cell boundaries
        if name == "one_point":
            assert want.keys.size == 1 and want.counts[0] == 25000
        if name == "tall":
            assert want.keys.max() > 2 ** 31
        if name in ("crop_edge", "non_finite"):
            assert 0 < want.kept < c.shape[0]
    # and under a transform that is not the identity
    T = relative_transform(_pose(2), _pose(5))
    pts, offs = s.assemble([[(k, T)] for k in range(len(clouds))], crop=30.0, leaf=0.3)
    for b, c in enumerate(clouds.values()):
        _check(_submap(pts, offs, b), R.assemble([(c, T)], 30.0, 0.3), 0.3)


def test_input_forms():
    c = _cloud(1, 6000)
    xyz = np.ascontiguousarray(c[:, :3])
    wide = np.zeros((c.shape[0], 8), F)
    wide[:, :3], wide[:, 4] = xyz, c[:, 3]
    forms = [(xyz, False), (xyz.astype(np.float64), False), (c, True), (wide, True)]
    s = KeyframeStore()
    ids = []
    for a, _ in forms:
        ids.append(s.append(a, EYE))
        ids.append(s.append(torch.from_numpy(a.copy()).cuda(), EYE))
    assert ids == list(range(8))
    pts, offs = s.assemble([[(k, _pose(1))] for k in ids], leaf=0.3)
    want = R.assemble([(c, _pose(1))], leaf=0.3)
    ref = _submap(pts, offs, 4)                                 # float32 [n, 4] from the host
    _check(ref, want, 0.3)
    for j, k in enumerate(ids):
        got = _submap(pts, offs, k)
        assert got[:, :3].tobytes() == ref[:, :3].tobytes(), k
        assert np.array_equal(got[:, 3], ref[:, 3]) if forms[j // 2][1] else not got[:, 3].any(), k


def test_growth_and_poses():
    s = KeyframeStore(capacity_hint=1000)
    clouds = [_cloud(20 + k, 5000) for k in range(8)]
    poses = [_pose(k) for k in range(8)]
    for k in range(3):
        s.append(clouds[k], poses[k])
    before, boffs = s.merge_nearest([1], 1)
    before = before.clone()
    for k in range(3, 8):
        assert s.append(clouds[k], poses[k]) == k
    assert len(s) == 8
    after, aoffs = s.merge_nearest([1], 1)
    assert np.array_equal(boffs, aoffs) and torch.equal(before.view(torch.int32), after.view(torch.int32))
    _check(after.cpu().numpy(), R.merge_nearest(clouds, poses, 1, 1), 0.2)
    pts, offs = s.merge_nearest([6, 7], 1)
    _check(_submap(pts, offs, 0), R.merge_nearest(clouds, poses, 6, 1), 0.2)
    _check(_submap(pts, offs, 1), R.merge_nearest(clouds, poses, 7, 1), 0.2)
    poses[2] = R.pose(0.35, (5.0, -2.0, 0.3))
    s.set_pose(2, poses[2])
    assert np.array_equal(s.pose(2), poses[2])
    moved, moffs = s.merge_nearest([1, 2], 1)
    assert not np.array_equal(moffs[:2], aoffs) or not torch.equal(moved[:int(moffs[1])], after)
    _check(_submap(moved, moffs, 0), R.merge_nearest(clouds, poses, 1, 1), 0.2)
    _check(_submap(moved, moffs, 1), R.merge_nearest(clouds, poses, 2, 1), 0.2)


def test_hand_over_to_gicp():
    from mr_slam_amd.gicp import GicpBatch
    clouds = [_cloud(30 + k, 14000) for k in range(3)]
    poses = [_pose(k) for k in range(3)]
    a = np.deg2rad(2.0)
    M = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    rng = np.random.default_rng(11)
    src, tgt = KeyframeStore(), KeyframeStore()
    for c, p in zip(clouds, poses):
        src.append(c, p)
        moved = c.copy()
        moved[:, :3] = (c[:, :3].astype(np.float64) @ M.T + [0.3, 0.0, 0.0] + rng.normal(0, 0.01, (c.shape[0], 3))).astype(F)
        tgt.append(moved, p)
    # submap_size 0: a submap is one filtered keyframe, so the target submap is the source submap moved rigidly by the known offset
    s_dev, t_dev = src.merge_nearest([1, 2], 0), tgt.merge_nearest([1, 2], 0)
    print("submap sizes", np.diff(s_dev[1]), np.diff(t_dev[1]))
    assert 4000 < np.diff(s_dev[1]).min() and np.diff(s_dev[1]).max() < 14000
    b = GicpBatch(2)
    b.set_sources(s_dev)
    b.set_targets(t_dev)
    T1, c1, i1 = b.align()
    host = [[_submap(p, o, j) for j in range(2)] for p, o in (s_dev, t_dev)]
    b2 = GicpBatch(2)
    b2.set_sources(host[0])
    b2.set_targets(host[1])
    T2, c2, i2 = b2.align()
    assert np.array_equal(T1, T2) and np.array_equal(c1, c2) and np.array_equal(i1, i2)
    print("converged", c1, "iterations", i1)
    assert np.abs(T1[:, 0, 3] - 0.3).max() < 0.1 and np.abs(T1[:, 1, 0] - np.sin(a)).max() < 0.01


def test_errors_leave_the_store_usable():
    s = KeyframeStore()
    for k in range(3):
        s.append(_cloud(k, 20000)[:3000], _pose(k))
    good, goffs = s.merge_nearest([1], 1)
    good = good.clone()
    for kw in (dict(leaf=0.0), dict(leaf=-0.2), dict(leaf=float("nan")), dict(crop=-1.0), dict(crop=float("inf"))):
        with pytest.raises(_lib.MrsError) as e:
            s.merge_nearest([1], 1, **kw)
        assert e.value.status == 1
        with pytest.raises(_lib.MrsError):
            s.assemble([[(1, EYE)]], **kw)
    for k in (3, -1):
        with pytest.raises(_lib.MrsError):
            s.assemble([[(k, EYE)]])
    with pytest.raises(_lib.MrsError):
        s.merge_nearest([3], 1)
    with pytest.raises(_lib.MrsError):
        s.set_pose(3, EYE)
    for hint in (-1, 1 << 60):                                  # refused before any allocation
        with pytest.raises(_lib.MrsError) as e:
            KeyframeStore(capacity_hint=hint)
        assert e.value.status == 1
    # a capacity one point short, through the raw ABI: refused, nothing written
    out = torch.full((6000, 4), -7.0, dtype=torch.float32, device="cuda:0")
    offs = np.full(2, -1, np.int64)
    ids = np.array([1], np.int32)
    lib = _lib.load()
    with pytest.raises(_lib.MrsError) as e:
        lib.mrs_submap_merge_nearest(s._h, 1, ids, 1, 60.0, 0.2, out, 5999, offs, _lib.current_stream(0))
    assert e.value.status == 1 and "capacity" in str(e.value)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and offs.tolist() == [-1, -1]
    lib.mrs_submap_merge_nearest(s._h, 1, ids, 1, 60.0, 0.2, out, 6000, offs, _lib.current_stream(0))
    assert offs.tolist() == goffs.tolist() and torch.equal(out[:int(offs[1])], good)
    again, aoffs = s.merge_nearest([1], 1)
    assert np.array_equal(aoffs, goffs) and torch.equal(again, good)
