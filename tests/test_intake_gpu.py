"""GPU suite of the keyframe intake (row G10, csrc/intake.hip) against the NumPy restatement tests/golden/intake_restate.py.

Compared as tests/test_submap_gpu.py compares a submap: the voxel count and the output order are exact, every mean lies within
(m + 1) * 2^-24 * max(max |v|, 1) of the restatement's float64 mean (m = the voxel's point count), and the key of every returned mean is
recomputed on the restatement's grid wherever the mean is clear of a cell boundary.  The z test can be undecided only where a voxel's restated
mean z lies within that bound of a limit AND its points do not all share one z: such a voxel may be present or absent, every other voxel
must match, and at most 1 % of a cloud's voxels may be undecided.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import intake_restate as K  # noqa: E402
import submap_restate as R  # noqa: E402

from mr_slam_amd import _lib, synth  # noqa: E402
from mr_slam_amd.submap import KeyframeStore  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
EYE = np.eye(4, dtype=F)

HAND = np.array([[0.1, 0.1, 0.1, 10], [0.2, 0.25, 0.05, 20], [0.1, 0.1, -1.0, 5], [5.0, 0.1, np.nextafter(F(-1), F(-np.inf)), 5],
                 [5.0, 5.0, 30.0, 7], [5.0, -5.0, np.nextafter(F(30), F(np.inf)), 9], [np.nan, 0, 0, 1], [0, 0, np.inf, 1],
                 [-0.05, -0.05, -0.05, 2]], F)


@functools.lru_cache(maxsize=None)
def _cloud(seed, n):
    """a lidar scan in the sensor's frame (the generator's ground sits at z = 0, the sensor 1.7 m above it)"""
    c = R.with_intensity(synth.lidar_scan(seed, n, metric=True), seed)
    c[:, 2] -= F(1.7)
    c.setflags(write=False)
    return c


def _pose(k):
    return R.pose(0.1 * k, (3.0 * k, 0.5 * k, 0.02 * k))


def _size(s):
    n, pts = np.zeros(1, np.int32), np.zeros(1, np.int64)
    _lib.load().mrs_keyframes_size(s._h, n, pts)
    return int(n[0]), int(pts[0])


def _check(got, cloud, leaf, limits, tag, min_sure=0.5, may_be_undecided=False):
    """got: float32 [m, 4], a stored keyframe; cloud: the raw float32 [n, 4] it was ingested from"""
    want = K.ingest(cloud, leaf, limits, tag)
    g = want.grid
    n_und = int(want.undecided.sum())
    print("voxels %d kept by z %d undecided %d" % (g.keys.size, int(want.keep.sum()), n_und), end=" ")
    assert may_be_undecided or n_und == 0
    assert n_und <= 0.01 * max(g.keys.size, 1)
    bound = R.mean_bound(g.counts, g.vmax) if g.keys.size else np.zeros((0, 4))
    # the returned rows are the sure voxels, in order, with any of the undecided ones in between
    rows, j = [], 0
    for v in np.flatnonzero(want.sure_keep | want.undecided):
        if want.undecided[v] and (j >= got.shape[0] or np.any(np.abs(got[j, :3].astype(np.float64) - g.means[v, :3]) > bound[v, :3])):
            continue
        rows.append(v)
        j += 1
    rows = np.array(rows, np.int64)
    assert got.shape[0] == rows.size, (got.shape[0], rows.size, int(want.sure_keep.sum()))
    if rows.size == 0:
        return want
    err = np.abs(got.astype(np.float64) - g.means[rows])
    worst = (err[:, :3] / bound[rows, :3]).max()
    print("largest voxel %d worst error / bound %.3f" % (g.counts.max(), worst))
    assert np.all(err[:, :3] <= bound[rows, :3]), worst
    if tag is None:
        assert np.all((err[:, 3] <= bound[rows, 3]) | (np.isnan(got[:, 3]) & np.isnan(g.means[rows, 3])))
    else:
        assert np.all(got[:, 3] == F(tag))
    # a voxel of one z value has an exact mean z
    one_z = g.vmax[rows, 2] == np.abs(g.means[rows, 2])
    assert np.array_equal(got[one_z, 2].astype(np.float64), g.means[rows, 2][one_z])
    lo, hi = F(limits[0]), F(limits[1])
    assert np.all((got[:, 2] >= lo) & (got[:, 2] <= hi))
    # the key of every returned mean, on the restatement's grid
    inv = F(1) / F(leaf)
    cell = np.floor(g.points[:, :3] * inv).astype(np.int64)
    mn = cell.min(axis=0)
    div = cell.max(axis=0) - mn + 1
    scaled = got[:, :3].astype(np.float64) * float(inv)
    sure = (np.abs(scaled - np.round(scaled)) > 2 * bound[rows, :3] * float(inv)).all(axis=1)
    c = np.floor(got[:, :3] * inv).astype(np.int64) - mn
    keys = c[:, 0] + c[:, 1] * div[0] + c[:, 2] * (div[0] * div[1])
    assert np.array_equal(keys[sure], g.keys[rows][sure])
    assert sure.mean() >= min_sure or rows.size < 8
    assert np.all(np.diff(g.keys) > 0)
    return want


def _raw_ingest(s, blob, offsets, layout, poses, leaf=0.3, lo=-1.0, hi=30.0, set_intensity=1, intensity=60.0, on_device=0):
    n = len(offsets) - 1
    ids, counts = np.full(n, -1, np.int32), np.full(n, -1, np.int64)
    _lib.load().mrs_keyframes_ingest(s._h, n, blob, on_device, np.asarray(offsets, np.int64), layout[0], layout[1], layout[2], layout[3], layout[4],
                                     leaf, lo, hi, set_intensity, intensity, np.ascontiguousarray(np.asarray(poses, F).reshape(-1, 16)), ids,
                                     counts, _lib.current_stream(0))
    s._counts.extend(int(c) for c in counts)
    return ids, counts


def test_hand_case():
    s = KeyframeStore()
    assert s.ingest(HAND, EYE, leaf=0.3, z_limits=(-1.0, 30.0), intensity=60.0) == 0 and len(s) == 1
    pts = s.points(0)
    assert pts.dtype == torch.float32 and pts.is_cuda and tuple(pts.shape) == (4, 4)
    got = pts.cpu().numpy()
    want = np.array([[0.1, 0.1, -1.0], [-0.05, -0.05, -0.05], [0.15, 0.175, 0.075], [5, 5, 30]])
    assert np.abs(got[:, :3] - want).max() < 1e-7 and got[:, 3].tolist() == [60.0] * 4
    assert got.tobytes() == K.ingest(HAND, 0.3, (-1.0, 30.0), 60.0).points.tobytes()
    _check(got, HAND, 0.3, (-1.0, 30.0), 60.0)
    assert _size(s) == (1, 4)
    # the raw ABI: the pcl::PointXYZI layout from the host, untagged, and an empty cloud in the same call
    blob = K.encode(HAND, K.LAYOUTS["pcl32"])
    ids, counts = _raw_ingest(s, blob, [0, 9, 9], K.LAYOUTS["pcl32"], [_pose(1), _pose(2)], set_intensity=0)
    assert ids.tolist() == [1, 2] and counts.tolist() == [4, 0] and _size(s) == (3, 8)
    got2 = s.points(1).cpu().numpy()
    assert got2[:, :3].tobytes() == got[:, :3].tobytes() and got2[:, 3].tolist() == [5.0, 2.0, 15.0, 7.0]
    assert tuple(s.points(2).shape) == (0, 4) and np.array_equal(s.pose(2), _pose(2))
    # read back into host memory
    host, n = np.full((5, 4), -7.0, F), np.zeros(1, np.int64)
    _lib.load().mrs_keyframes_get_points(s._h, 1, host, 0, 5, n, _lib.current_stream(0))
    assert n[0] == 4 and host[:4].tobytes() == got2.tobytes() and np.all(host[4] == -7.0)


@pytest.mark.parametrize("seed, n", [(0, 1024), (1, 5000), (2, 20000), (3, 40000)])       # 1024 = exactly one tile
@pytest.mark.parametrize("leaf, limits, tag", [(0.3, (-1.0, 30.0), 60.0), (0.2, (0.5, 2.0), None)])
def test_lidar_clouds(seed, n, leaf, limits, tag):
    c = _cloud(seed, n)
    s = KeyframeStore()
    s.append(c[:100], EYE)
    before = _size(s)
    kid = s.ingest(c, _pose(1), leaf=leaf, z_limits=limits, intensity=tag)
    got = s.points(kid).cpu().numpy()
    want = _check(got, c, leaf, limits, tag)
    assert kid == 1 and 0 < got.shape[0] < want.grid.keys.size
    assert _size(s) == (2, before[1] + got.shape[0])           # the survivors only
    assert s.points(0).cpu().numpy().tobytes() == c[:100].tobytes()


def _adversarial():
    rng = np.random.default_rng(4)
    out = {}
    edge = rng.uniform(-20, 20, size=(4096, 3)).astype(F)
    edge[:, 2] = rng.uniform(-3, 33, 4096).astype(F)
    for i, v in enumerate([F(-1), F(30), np.nextafter(F(-1), F(-np.inf)), np.nextafter(F(-1), F(np.inf)), np.nextafter(F(30), F(-np.inf)),
                           np.nextafter(F(30), F(np.inf))]):
        edge[i::16, 2] = v
    out["limit_edge"] = edge
    rng = np.random.default_rng(3)
    leaf = F(0.3)
    k = rng.integers(-60, 60, size=(1366, 3)).astype(F) * leaf                         # exact multiples of the leaf and their neighbours
    out["multiples"] = np.concatenate([k, np.nextafter(k, F(np.inf)), np.nextafter(k, F(-np.inf))])
    out["around_zero"] = rng.uniform(-0.45, 0.45, size=(4096, 3)).astype(F)
    out["one_point"] = np.tile(np.array([[12.3, -45.6, 1.7]], F), (25000, 1))
    tall = rng.uniform(-60, 60, size=(8000, 3)).astype(F)
    tall[:, 2] = rng.uniform(-1e4, 1e4, 8000).astype(F)
    out["tall"] = tall
    bad = rng.uniform(-20, 20, size=(4096, 3)).astype(F)
    for i, v in enumerate([np.nan, np.inf, -np.inf]):
        for axis in range(3):
            bad[3 * i + axis::40, axis] = v
    out["non_finite"] = bad
    # voxels of 1 .. 130 points, shuffled: the sums are cut into chunks of 32 points (one point over, one short, exactly full)
    lengths = [1, 2, 31, 32, 33, 34, 63, 64, 65, 66, 95, 96, 97, 98, 129, 130]
    runs = np.concatenate([np.array([3.0 * i + 0.01, 0.01, 0.01]) + rng.uniform(0, 0.28, size=(m, 3)) for i, m in enumerate(lengths)]).astype(F)
    out["run_lengths"] = runs[rng.permutation(runs.shape[0])]
    out = {name: R.with_intensity(c, 5) for name, c in out.items()}
    out["non_finite"][20::40, 3] = np.nan                      # rows with finite x, y, z: a non-finite intensity is carried like any value
    assert np.isfinite(out["non_finite"][20::40, :3]).all()
    return out


def test_adversarial_clouds():
    clouds = _adversarial()
    s = KeyframeStore()
    for tag in (60.0, None):
        limits = (-1.0, 30.0) if tag is not None else (-np.inf, np.inf)
        ids, counts = s.ingest_batch(list(clouds.values()), [EYE] * len(clouds), leaf=0.3, z_limits=limits, intensity=tag)
        for kid, m, (name, c) in zip(ids, counts, clouds.items()):
            print(name, end=": ")
            got = s.points(kid).cpu().numpy()
            assert got.shape[0] == m
            want = _check(got, c, 0.3, limits, tag, min_sure=0.0 if name == "multiples" else 0.5, may_be_undecided=name == "limit_edge")
            if name == "limit_edge" and tag is not None:
                assert want.undecided.any() and want.sure_keep.sum() > 1000
            if name == "one_point":
                assert want.grid.keys.size == 1 and want.grid.counts[0] == 25000 and got.shape[0] == 1
            if name == "run_lengths":
                assert sorted(want.grid.counts.tolist()) == [1, 2, 31, 32, 33, 34, 63, 64, 65, 66, 95, 96, 97, 98, 129, 130]
            if name == "tall":
                assert want.grid.keys.max() > 2 ** 31
            if name == "non_finite":
                assert 0 < want.grid.kept < c.shape[0]
                assert tag is not None or np.isnan(got[:, 3]).any()


def test_layouts_from_host_and_device():
    c = _cloud(1, 6000)
    s = KeyframeStore()
    ids = []
    for name, layout in K.LAYOUTS.items():
        blob = K.encode(c, layout)
        ids.append(s.ingest(blob.tobytes(), EYE, intensity=None, layout=layout))
        ids.append(s.ingest(torch.from_numpy(blob.copy()).cuda(), EYE, intensity=None, layout=layout))
    # the array forms append takes: [n, 3], [n, 4], [n, 8]
    wide = np.zeros((c.shape[0], 8), F)
    wide[:, :3], wide[:, 4] = c[:, :3], c[:, 3]
    forms = [(np.ascontiguousarray(c[:, :3]), False), (c, True), (wide, True)]
    for a, _ in forms:
        ids.append(s.ingest(a, EYE))
        ids.append(s.ingest(torch.from_numpy(a.copy()).cuda(), EYE))
    # a device blob at an address that is 4-byte but not 16-byte aligned, point_step 16: the 4-byte loads
    shifted = torch.zeros(c.size + 1, dtype=torch.float32, device="cuda:0")
    shifted[1:] = torch.from_numpy(c.copy()).cuda().reshape(-1)
    ids.append(s.ingest(shifted[1:].view(torch.uint8), EYE, layout=K.LAYOUTS["xyzi16"]))
    assert ids == list(range(15))
    ref = s.points(0).cpu().numpy()
    _check(ref, c, 0.3, (-1.0, 30.0), None)
    has_intensity = [lay[4] >= 0 for lay in K.LAYOUTS.values() for _ in range(2)] + [f[1] for f in forms for _ in range(2)] + [True]
    for k, with_i in zip(ids, has_intensity):
        got = s.points(k).cpu().numpy()
        assert got[:, :3].tobytes() == ref[:, :3].tobytes(), k
        assert got[:, 3].tobytes() == ref[:, 3].tobytes() if with_i else not got[:, 3].any(), k


def test_batch_equals_single_calls():
    sizes = [5000, 20000, 0, 7777, 1, 1024]
    clouds = [_cloud(10 + k, n) if n else np.zeros((0, 4), F) for k, n in enumerate(sizes)]
    clouds[4] = np.array([[1.0, 2.0, 0.5, 9.0]], F)
    high = _cloud(17, 3000).copy()
    high[:, 2] += F(40.0)                                       # the z limits empty it completely
    clouds.append(high)
    poses = [_pose(k) for k in range(len(clouds))]
    s = KeyframeStore()
    s.ingest(_cloud(9, 2000), EYE)
    ids, counts = s.ingest_batch(clouds, poses, intensity=30.0)
    assert ids == list(range(1, 8)) and len(s) == 8
    assert counts[2] == 0 and counts[6] == 0 and counts[4] == 1 and np.all(counts[[0, 1, 3, 5]] > 0)
    assert _size(s) == (8, int(counts.sum()) + s.points(0).shape[0])
    again = KeyframeStore()
    ids2, counts2 = again.ingest_batch([torch.from_numpy(c.copy()).cuda() for c in clouds], poses, intensity=30.0)      # from the device
    assert ids2 == list(range(7)) and np.array_equal(counts, counts2)
    single = KeyframeStore()
    for k, (c, p) in enumerate(zip(clouds, poses)):
        assert single.ingest(c, p, intensity=30.0) == k
        a, b, d = s.points(ids[k]), again.points(k), single.points(k)
        assert a.shape[0] == counts[k] and torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(a.view(torch.int32), d.view(torch.int32))
        assert np.array_equal(s.pose(ids[k]), p)
        if k in (1, 3):
            _check(a.cpu().numpy(), c, 0.3, (-1.0, 30.0), 30.0)
    # one blob with offsets
    one = KeyframeStore()
    offs = np.concatenate([[0], np.cumsum([c.shape[0] for c in clouds])]).astype(np.int64)
    ids3, counts3 = one.ingest_batch(np.concatenate(clouds), poses, intensity=30.0, offsets=offs)
    assert np.array_equal(counts3, counts) and all(torch.equal(one.points(k), single.points(k)) for k in range(7))
    assert s.ingest_batch([], [])[0] == [] and len(s) == 8


def test_growth_and_hand_over():
    from mr_slam_amd.gicp import GicpBatch
    clouds = [_cloud(20 + k, 5000) for k in range(8)]
    poses = [_pose(k) for k in range(8)]
    s = KeyframeStore(capacity_hint=1000)
    early = []
    for k in range(8):
        assert s.ingest(clouds[k], poses[k], intensity=30.0) == k
        if k < 3:
            early.append(s.points(k).clone())
    assert all(torch.equal(s.points(k).view(torch.int32), early[k].view(torch.int32)) for k in range(3))
    _check(s.points(7).cpu().numpy(), clouds[7], 0.3, (-1.0, 30.0), 30.0)
    # the hand-over the store exists for: a store filled by append(points(id)) behaves the same
    t = KeyframeStore(capacity_hint=1000)
    for k in range(8):
        t.append(s.points(k), poses[k])
    assert s._counts == t._counts and _size(s) == _size(t)
    a, b = s.merge_nearest([3, 6], 1), t.merge_nearest([3, 6], 1)
    assert np.array_equal(a[1], b[1]) and a[1][-1] > 1000 and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
    tgt = s.merge_nearest([3, 6], 1, leaf=0.25)                  # the same places, voxelised differently
    res = []
    for src in (a, b):
        g = GicpBatch(2)
        g.set_sources(src)
        g.set_targets(tgt)
        res.append(g.align())
    assert all(np.array_equal(x, y) for x, y in zip(res[0], res[1]))


def test_errors_leave_the_store_usable():
    c = _cloud(1, 5000)
    s = KeyframeStore()
    s.ingest(c, EYE, intensity=30.0)
    good, size = s.points(0).clone(), _size(s)
    nan_pose = EYE.copy()
    nan_pose[1, 3] = np.nan
    bad = [dict(leaf=0.0), dict(leaf=-0.3), dict(leaf=float("nan")), dict(leaf=float("inf")), dict(z_limits=(float("nan"), 30.0)),
           dict(z_limits=(-1.0, float("nan"))), dict(z_limits=(2.0, 1.0)), dict(intensity=float("inf")), dict(intensity=float("nan")),
           dict(pose=nan_pose)]
    for kw in bad:
        kw = dict(kw)
        pose = kw.pop("pose", EYE)
        with pytest.raises(_lib.MrsError) as e:
            s.ingest(c, pose, **kw)
        assert e.value.status == 1, kw
    lib = _lib.load()
    offs, ids, counts = np.array([0, c.shape[0]], np.int64), np.zeros(1, np.int32), np.zeros(1, np.int64)
    pose, stream = EYE.reshape(16).copy(), _lib.current_stream(0)
    args = lambda **kw: [kw.get(k, v) for k, v in dict(kf=s._h, n=1, data=c, dev=0, offs=offs, step=16, x=0, y=4, z=8, i=12, leaf=0.3, lo=-1.0,  # noqa: E731
                                                       hi=30.0, set=1, val=30.0, pose=pose, ids=ids, counts=counts, stream=stream).items()]
    raw_bad = [dict(zip(("step", "x", "y", "z", "i"), lay)) for lay in (
        (8, 0, 4, 8, -1), (18, 0, 4, 8, -1), (16, -4, 4, 8, 12), (16, 0, 6, 8, 12), (16, 0, 4, 16, 12), (16, 0, 4, 8, 16), (16, 0, 4, 8, -2),
        (16, 0, 4, 8, 10), (16, 4, 0, 8, 12), (16, 0, 8, 4, 12), (16, 0, 4, 4, 12))]
    raw_bad += [dict(data=None), dict(offs=None), dict(pose=None), dict(ids=None), dict(counts=None), dict(n=-1), dict(set=2),
               dict(offs=np.array([1, c.shape[0]], np.int64)), dict(offs=np.array([0, -1], np.int64)),
               dict(offs=np.array([0, 2 ** 31], np.int64)),                                            # more than 2^31 - 1 points: refused unread
               dict(n=2, offs=np.array([0, 10, 5], np.int64), pose=np.tile(pose, 2), ids=np.zeros(2, np.int32), counts=np.zeros(2, np.int64))]
    for kw in raw_bad:
        with pytest.raises(_lib.MrsError) as e:
            lib.mrs_keyframes_ingest(*args(**kw))
        assert e.value.status == 1, kw
    # after the first launches: a grid whose keys need more than 63 bits
    wide = np.array([[-3e30, 0, 0, 1], [3e30, 1e25, -1e28, 1], [0, 0, 0, 1]], F)
    with pytest.raises(_lib.MrsError) as e:
        s.ingest(wide, EYE, leaf=0.001, z_limits=(-np.inf, np.inf))
    assert e.value.status == 1 and "63 bits" in str(e.value)
    with pytest.raises(_lib.MrsError) as e:
        s.ingest_batch([c, wide], [EYE, EYE], leaf=0.001, z_limits=(-np.inf, np.inf))
    assert e.value.status == 1
    # reading back: id out of range, a capacity one point short (nothing written)
    out, n = torch.full((good.shape[0], 4), -7.0, device="cuda:0"), np.zeros(1, np.int64)
    for kid, cap in ((1, good.shape[0]), (-1, good.shape[0]), (0, good.shape[0] - 1)):
        with pytest.raises(_lib.MrsError) as e:
            lib.mrs_keyframes_get_points(s._h, kid, out, 1, cap, n, stream)
        assert e.value.status == 1
    with pytest.raises(IndexError):
        s.points(1)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    # the store is as it was, and goes on working
    assert len(s) == 1 and _size(s) == size and torch.equal(s.points(0).view(torch.int32), good.view(torch.int32))
    assert s.ingest(c, EYE, intensity=30.0) == 1 and torch.equal(s.points(1).view(torch.int32), good.view(torch.int32))
    assert _size(s) == (2, 2 * size[1])


INTAKE_OUT = os.path.join(ROOT, "tests", "cpp", "build", "intake_test")


def test_intake_main_cpp():
    """the INTEGRATION.md section 2a snippet as a program: a 32-byte PointXYZI-shaped struct through mrs_keyframes_ingest / _get_points"""
    lib_dir = os.path.join(ROOT, "mr_slam_amd")
    os.makedirs(os.path.dirname(INTAKE_OUT), exist_ok=True)
    cmd = ["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "intake_main.cpp"),
           "-o", INTAKE_OUT, "-L" + lib_dir, "-lmrslam_hip", "-Wl,-rpath," + lib_dir]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([INTAKE_OUT], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("point ")]
    got = np.array([[float(v) for v in ln[2:6]] for ln in lines], F)
    want = K.ingest(HAND, 0.3, (-1.0, 30.0), 60.0).points
    assert got.shape == (4, 4) and got.tobytes() == want.tobytes(), r.stdout
    assert "keyframe 0: 4 points" in r.stdout and "store: 1 keyframes, 4 points" in r.stdout
