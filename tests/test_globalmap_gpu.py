"""GPU suite of the merged global map (row G8, csrc/mapcompose.hip) against the NumPy restatement tests/golden/globalmap_restate.py.

The comparison is test_submap_gpu.py's: the voxel count and the output order are exact, every mean lies within
(m + 1) * 2^-24 * max(max |v|, 1) of the restatement's float64 mean per voxel and channel, and the key of every returned mean that lies
clear of a cell boundary is recomputed on the restatement's grid.
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import globalmap_restate as G  # noqa: E402
import submap_restate as R  # noqa: E402

from mr_slam_amd import _lib, synth  # noqa: E402
from mr_slam_amd.globalmap import GlobalMap  # noqa: E402
from mr_slam_amd.submap import KeyframeStore  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
EYE = np.eye(4, dtype=F)


def _check(got, want, leaf, min_sure=0.5):
    """got: float32 [m, 4] from the device; want: the restatement's Result; min_sure: the least share of voxels whose mean must lie clear of
    every cell boundary (so that the key check is not vacuous)"""
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


def _stores(keyframes):
    """one KeyframeStore per list of clouds, every keyframe at the identity pose"""
    out = []
    for clouds in keyframes:
        s = KeyframeStore()
        for c in clouds:
            s.append(np.ascontiguousarray(c, F).reshape(-1, 4), EYE)
        out.append(s)
    return out


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------------
STORE0 = np.array([[0.1, 0.1, 0.1, 1], [0.3, 0.2, 0.4, 3], [np.nan, 0, 0, 1], [-0.05, -0.05, -0.05, 2], [100.25, -200.25, 3.0, 8]], F)
STORE1 = np.array([[0.2, 0.2, 0.2, 5], [1, 1, 1, 6]], F)
SHIFT = EYE.copy()
SHIFT[:3, 3] = [100, -200.5, 2.75]


def test_hand_case_two_stores():
    m = GlobalMap(_stores([[STORE0], [STORE1]]), leaf=0.5)
    pts = m.rebuild([(0, 0, EYE), (1, 0, SHIFT)])
    assert pts.dtype == torch.float32 and pts.is_cuda and tuple(pts.shape) == (5, 4) and pts is m.points
    got = pts.cpu().numpy()
    want = G.compose([(STORE0, EYE), (STORE1, SHIFT)], 0.5)
    assert want.keys.tolist() == [81600, 163813, 492249, 574257, 656675] and want.counts.tolist() == [1, 2, 1, 1, 1]
    _check(got, want, 0.5)
    assert got[0].tolist() == [F(-0.05), F(-0.05), F(-0.05), 2.0] and got[1, 3] == 2.0
    # the incremental branch on top of it: the old centroids count as one point each
    pts2 = m.add([(1, 0, SHIFT)])
    want2 = G.compose([(STORE1, SHIFT)], 0.5, prev=got)
    assert want2.keys.tolist() == want.keys.tolist() and want2.counts.tolist() == [1, 1, 2, 1, 2]
    _check(pts2.cpu().numpy(), want2, 0.5)
    assert pts2[0].tolist() == got[0].tolist()                  # an untouched voxel keeps its bits


# ---- 2, 3 ---------------------------------------------------------------------------------------------------------------------------------
def _pose(r, k):
    return R.pose(0.1 * k + 1.3 * r, (3.0 * k + 20.0 * r, 0.5 * k - 7.0 * r, 0.02 * k))


@functools.lru_cache(maxsize=None)
def _two_robots():
    clouds = [[R.with_intensity(synth.lidar_scan(10 * r + k, 20000, metric=True), 10 * r + k) for k in range(4)] for r in range(2)]
    stores = _stores(clouds)
    segs = [(r, k, _pose(r, k)) for k in range(4) for r in range(2)]       # r0k0, r1k0, r0k1, ...
    host = [(clouds[r][k], T) for r, k, T in segs]
    return stores, segs, host


@functools.lru_cache(maxsize=None)
def _two_robots_want(leaf):
    return G.compose(_two_robots()[2], leaf)


@pytest.mark.parametrize("leaf, voxels, largest, bits", [(0.5, 25845, 778, 20), (0.3, 44450, 582, 23), (0.2, 65097, 255, 24)])
def test_two_robots_interleaved(leaf, voxels, largest, bits):
    stores, segs, _ = _two_robots()
    want = _two_robots_want(leaf)
    assert (want.keys.size, int(want.counts.max()), G.key_bits(want, leaf)) == (voxels, largest, bits) and want.kept == 160000
    got = GlobalMap(stores, leaf=leaf).rebuild(segs)
    _check(got.cpu().numpy(), want, leaf)


def test_incremental():
    stores, segs, host = _two_robots()

    def run():
        m = GlobalMap(stores, leaf=0.3)
        first = m.rebuild(segs[:7]).clone()
        return first, m.add(segs[7:])

    first, second = run()
    _check(first.cpu().numpy(), G.compose(host[:7], 0.3), 0.3)
    want = G.compose(host[7:], 0.3, prev=first.cpu().numpy())
    assert want.kept == first.shape[0] + 20000
    _check(second.cpu().numpy(), want, 0.3)
    first2, second2 = run()
    assert _bits(first, first2) and _bits(second, second2)


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------------
def test_dropped_points_against_a_full_grid():
    rng = np.random.default_rng(7)
    rows = []
    for c in range(64):                                          # a 4 x 4 x 4 block of cells at leaf 0.5, 1 to 3 points near every centre
        centre = (np.array([c % 4, (c // 4) % 4, c // 16]) + 0.5) * 0.5
        for _ in range(1 + c % 3):
            rows.append(np.concatenate([centre + rng.uniform(-0.1, 0.1, 3), [rng.uniform(0, 255)]]))
    good = np.array(rows, F)[rng.permutation(len(rows))]
    bad = np.array([[np.nan, 1, 1, 1], [1, np.inf, 1, 2], [1, 1, -np.inf, 3], [np.inf, np.nan, 0, 4]], F)
    mixed = np.concatenate([np.concatenate([good[i:i + 3], bad[i // 3 % 4][None]]) for i in range(0, good.shape[0], 3)])
    half = mixed.shape[0] // 2
    blow = EYE.copy()
    blow[0, 0] = 3e38                                            # finite, and sends x = 10 beyond the largest float
    far = np.tile(np.array([[10.0, 0.5, 0.5, 9]], F), (50, 1))
    host = [(mixed[:half], EYE), (far, blow), (mixed[half:], EYE), (bad, EYE)]
    want = G.compose(host, 0.5)
    assert want.keys.tolist() == list(range(64)) and want.kept == good.shape[0] < mixed.shape[0]
    assert G.key_bits(want, 0.5) == 6                            # key 63 = 2^6 - 1 is occupied: a dropped key cut to 6 bits would land on it
    assert want.counts.tolist() == [1 + c % 3 for c in range(64)]
    m = GlobalMap(_stores([[mixed[:half], far], [mixed[half:], bad]]), leaf=0.5)
    got = m.rebuild([(0, 0, EYE), (0, 1, blow), (1, 0, EYE), (1, 1, EYE)])
    _check(got.cpu().numpy(), want, 0.5)
    # nothing but dropped points: an empty map
    assert m.rebuild([(1, 1, EYE), (0, 1, blow)]).shape[0] == 0


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------------
SIZES = [1024, 1, 0, 1023, 1025, 4097]


def test_tile_edges_one_large_voxel():
    n = 30000
    pts = np.tile(np.array([[1.23, -4.56, 0.78, 0]], F), (n, 1))
    pts[:, 3] = np.arange(n) % 251
    cuts = np.cumsum([0] + SIZES + [n - sum(SIZES)])
    clouds = [pts[a:b] for a, b in zip(cuts[:-1], cuts[1:])] + [np.array([[500, 500, 20, 7]], F)]
    host = [(c, EYE) for c in clouds]
    want = G.compose(host, 0.5)
    assert want.counts.tolist() == [30000, 1] and abs(want.means[0, 3] - 124.738) < 1e-9
    m = GlobalMap(_stores([clouds]), leaf=0.5)
    segs = [(0, k, EYE) for k in range(len(clouds))]
    got = m.rebuild(segs).clone()
    _check(got.cpu().numpy(), want, 0.5)
    assert got[0, :3].tolist() == [F(1.23), F(-4.56), F(0.78)]  # 30 000 equal float32 values sum exactly in float64
    assert _bits(got, m.rebuild(segs))


def test_tile_edges_of_the_sorted_runs():
    # voxels along x whose point counts put run ends on, just before and just after the 1024-position tiles of the reduction
    runs = [1024, 1, 1023, 1025, 2048, 3, 4097, 1, 1020, 4, 5000]
    rng = np.random.default_rng(12)
    rows = [np.concatenate([[(c + 0.5) * 0.5, 0.25, 0.25] + rng.uniform(-0.2, 0.2, 3), [rng.uniform(0, 255)]]) for c, m in enumerate(runs)
            for _ in range(m)]
    pts = np.array(rows, F)[rng.permutation(len(rows))]
    cuts = np.cumsum([0] + SIZES + [pts.shape[0] - sum(SIZES)])
    clouds = [pts[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    want = G.compose([(c, EYE) for c in clouds], 0.5)
    assert want.counts.tolist() == runs
    m = GlobalMap(_stores([clouds[:3], clouds[3:]]), leaf=0.5)
    segs = [(0, k, EYE) for k in range(3)] + [(1, k, EYE) for k in range(len(clouds) - 3)]
    got = m.rebuild(segs).clone()
    _check(got.cpu().numpy(), want, 0.5)
    assert _bits(got, m.rebuild(segs))


@pytest.mark.parametrize("n_seg", [1024, 1025])
def test_segment_lookup_in_lds_and_in_global_memory(n_seg):
    # up to 1024 segments the reduction keeps its segment lookup in LDS, above that in global memory; a keyframe may be listed many times
    rng = np.random.default_rng(5)
    clouds = [R.with_intensity(rng.uniform(-3, 3, (n, 3)), n) for n in (37, 1, 64)]
    stores = _stores([clouds[:2], clouds[2:]])
    segs = []
    for i in range(n_seg):
        T = R.pose(0.05 * (i % 7), (0.37 * (i % 40), 0.11 * (i // 40), 0.0))
        segs.append(((0, 0), (1, 0), (0, 1))[i % 3] + (T,))
    host = [(clouds[(0, 2, 1)[i % 3]], T) for i, (_, _, T) in enumerate(segs)]
    want = G.compose(host, 0.5)
    assert want.kept == sum(c.shape[0] for c, _ in host) > 30 * n_seg
    _check(GlobalMap(stores, leaf=0.5).rebuild(segs).cpu().numpy(), want, 0.5)


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------------
def test_wide_and_too_wide_grids():
    rng = np.random.default_rng(21)
    cluster = R.with_intensity(rng.uniform(-5, 5, (2000, 3)), 1)
    corners = np.array([[sx * 3e5, sy * 3e5, 0, 1] for sx in (-1, 1) for sy in (-1, 1)], F)
    clouds = [cluster[:900], corners[:2], cluster[900:], corners[2:]]
    want = G.compose([(c, EYE) for c in clouds], 0.05)
    assert G.key_bits(want, 0.05) > 32 and want.keys.max() > 2 ** 32
    print("key bits", G.key_bits(want, 0.05))
    stores = _stores([clouds[:2], clouds[2:]])
    m = GlobalMap(stores, leaf=0.05)
    segs = [(0, 0, EYE), (0, 1, EYE), (1, 0, EYE), (1, 1, EYE)]
    good = m.rebuild(segs).clone()
    _check(good.cpu().numpy(), want, 0.05)
    # too wide: 2e11 cells along every axis do not fit in 63 bits
    huge = np.array([[1e9, 1e9, 1e9, 1], [-1e9, -1e9, -1e9, 2]], F)
    stores[1].append(huge, EYE)
    with pytest.raises(_lib.MrsError) as e:
        GlobalMap(stores, leaf=0.01).rebuild(segs + [(1, 2, EYE)])
    assert e.value.status == 1 and "63 bits" in str(e.value)
    assert _bits(good, GlobalMap(stores, leaf=0.05).rebuild(segs))


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------------
def test_arguments():
    c = R.with_intensity(synth.lidar_scan(3, 3000, metric=True), 3)
    s0, s1, empty = KeyframeStore(), KeyframeStore(), KeyframeStore()
    s0.append(c[:2000], EYE)
    s1.append(c[2000:], EYE)
    lib, stream = _lib.load(), _lib.current_stream(0)
    handles = (C.c_void_p * 2)(s0._h.value, s1._h.value)
    out = torch.full((4000, 4), -7.0, dtype=torch.float32, device="cuda:0")
    prev = torch.zeros((10, 4), dtype=torch.float32, device="cuda:0")
    idx, kfs = np.array([0, 1], np.int32), np.array([0, 0], np.int32)
    Ts = np.ascontiguousarray(np.stack([EYE.reshape(16)] * 2))
    m = C.c_int64(-1)

    def call(idx=idx, kfs=kfs, Ts=Ts, prev=None, n_prev=0, leaf=0.5, out=out, capacity=3000, n_stores=2):
        lib.mrs_map_compose(n_stores, handles, 2, idx, kfs, Ts, prev, n_prev, leaf, out, capacity, C.byref(m), stream)

    nan_T = Ts.copy()
    nan_T[1, 3] = np.nan
    bad = [dict(idx=np.array([0, 2], np.int32)), dict(idx=np.array([-1, 0], np.int32)), dict(kfs=np.array([0, 1], np.int32)),
           dict(kfs=np.array([-1, 0], np.int32)), dict(leaf=0.0), dict(leaf=-0.5), dict(leaf=float("nan")), dict(leaf=float("inf")),
           dict(capacity=2999), dict(prev=prev, n_prev=10, capacity=3009), dict(Ts=nan_T), dict(n_stores=0), dict(n_stores=17),
           dict(prev=out[3000:3010], n_prev=10, capacity=3010), dict(prev=out[:10], n_prev=10, out=out[5:], capacity=3010)]
    for kw in bad:
        with pytest.raises(_lib.MrsError) as e:
            call(**kw)
        assert e.value.status == 1, kw
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and m.value == -1
    call()
    assert 0 < m.value <= 3000
    want = G.compose([(c[:2000], EYE), (c[2000:], EYE)], 0.5)
    _check(out[:m.value].cpu().numpy(), want, 0.5)
    call(prev=prev, n_prev=10, capacity=3010)                   # ten more points at the origin
    assert 0 < m.value <= 3010
    # nothing in, nothing out
    lib.mrs_map_compose(2, handles, 0, None, None, None, None, 0, 0.5, None, 0, C.byref(m), stream)
    assert m.value == 0
    assert GlobalMap([s0, s1]).rebuild([]).shape[0] == 0
    # three stores, one of them empty; the same store listed twice
    three = GlobalMap([s0, empty, s1], leaf=0.5).rebuild([(0, 0, EYE), (2, 0, EYE)])
    _check(three.cpu().numpy(), want, 0.5)
    twice = GlobalMap([s0, s1, s0], leaf=0.5).rebuild([(2, 0, EYE), (1, 0, EYE)])
    assert _bits(twice, three)
    with pytest.raises(_lib.MrsError):
        GlobalMap([s0, empty, s1]).rebuild([(1, 0, EYE)])


# ---- 8 ------------------------------------------------------------------------------------------------------------------------------------
def test_agrees_with_assemble_on_one_store():
    stores, segs, host = _two_robots()
    one = [(k, _pose(0, k)) for k in range(4)]
    new = GlobalMap(stores[:1], leaf=0.2).rebuild([(0, k, T) for k, T in one]).cpu().numpy()
    old, offs = stores[0].assemble([one], crop=3e38, leaf=0.2)
    old = old.cpu().numpy()
    assert offs.tolist() == [0, new.shape[0]] and new.shape[0] > 10000
    want = G.compose([(host[2 * k][0], T) for k, T in one], 0.2)
    bound = R.mean_bound(want.counts, want.vmax)
    assert np.all(np.abs(new.astype(np.float64) - old.astype(np.float64)) <= 2 * bound)
    _check(new, want, 0.2)
    _check(old, want, 0.2)
