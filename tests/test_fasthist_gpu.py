"""GPU suite for the Fast Histogram descriptor (fasthist.hip, the MRS_LOOPDB_FH loop database, mr_slam_amd.fasthist and the
pr_methods.FastHistogram drop-in) against tests/golden/ref_fasthist.npz, which the reference's own FastHistogram.py produced, and against the
NumPy restatement tests/golden/fasthist_restate.py, which tests/test_fasthist_cpu.py checks against that fixture.

Everything the kernels compute is an integer or a correctly rounded float64 operation, so every comparison here is exact: counts as
integers, the histogram, the largest range and the database distances bit for bit."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import fasthist_restate as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _F():
    from mr_slam_amd import fasthist
    return fasthist


def _pack(clouds, dtype=None, stride=3):
    dtype = dtype or clouds[0].dtype
    offs = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int64)
    pts = np.full((int(offs[-1]), stride), 7.5, dtype)         # columns past xyz hold something that must not matter
    if offs[-1]:
        pts[:, :3] = np.concatenate([np.asarray(c, dtype).reshape(-1, 3) for c in clouds if len(c)])
    return torch.from_numpy(pts).to(DEV), torch.from_numpy(offs)


def _run(clouds, bins=100, dtype=None, stride=3):
    """-> (hist [B, bins], counts [B, bins], M [B], unbound [B]) as numpy arrays"""
    pts, offs = _pack(clouds, dtype, stride)
    out = _F().range_histogram_batch(pts, offs, bins)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _check(got, k, cloud, bins, tag=None):
    """result row k of a batched call against the restatement of `cloud`"""
    hist, counts, M, unbound = got
    r = R.range_histogram(cloud, bins)
    assert counts.dtype == np.int32 and np.array_equal(counts[k], r.counts), tag
    assert _same_bits(hist[k], r.hist), tag
    assert _same_bits(M[k], r.M), tag
    assert unbound[k] == r.unbound, tag


@pytest.fixture(scope="module")
def g():
    return R.load()


@pytest.fixture(scope="module")
def f32_names(g):
    return [n for n, c in g.items() if c["cloud"].dtype == np.float32]


@pytest.fixture(scope="module")
def batched(g, f32_names):
    """every float32 fixture cloud, an empty cloud and a 1-point cloud in ONE ragged batch: computed once, read by several tests"""
    clouds = [g[n]["cloud"] for n in f32_names]
    clouds.insert(2, np.zeros((0, 3), np.float32))
    clouds.append(np.array([[3.0, 4.0, 12.0]], np.float32))
    names = list(f32_names)
    names.insert(2, "empty")
    names.append("one")
    return names, clouds, _run(clouds)


def test_fixture_parity(g, batched):
    names, clouds, (hist, counts, M, unbound) = batched
    for k, name in enumerate(names):
        if name in g:
            assert np.array_equal(counts[k], g[name]["counts"]), name
            assert _same_bits(hist[k], g[name]["hist"]), name
            assert _same_bits(M[k], R.range_histogram(clouds[k]).M), name
            assert unbound[k] == 0, name
    # the NCLT scan is stored in float64
    got = _run([g["nclt"]["cloud"]])
    assert np.array_equal(got[1][0], g["nclt"]["counts"]) and _same_bits(got[0][0], g["nclt"]["hist"])
    assert _same_bits(got[2][0], R.range_histogram(g["nclt"]["cloud"]).M) and got[3][0] == 0


def test_batch_equals_alone(batched):
    names, clouds, (hist, counts, M, unbound) = batched
    k = names.index("empty")
    assert not hist[k].any() and not counts[k].any() and M[k] == 0.0 and unbound[k] == 0
    k = names.index("one")
    assert M[k] == 13.0 and counts[k][99] == 1 and counts[k].sum() == 1 and hist[k][99] == 1.0
    for k, name in enumerate(names):
        alone = _run([clouds[k]])
        for a, b in zip(alone, (hist, counts, M, unbound)):
            assert _same_bits(a[0], b[k]), name


def test_input_forms(g, batched):
    names, clouds, ref = batched
    pick = [names.index(n) for n in ("gauss7", "gauss4097", "lidar", "edges")]
    sub = [clouds[k] for k in pick]
    for dtype, stride in ((np.float64, 3), (np.float32, 4), (np.float64, 7)):
        got = _run(sub, dtype=dtype, stride=stride)
        for a, b in zip(got, ref):
            assert _same_bits(a, b[pick]), (dtype, stride)


def test_tile_boundaries():
    T = _F().TILE_POINTS
    rng = np.random.default_rng(41)
    sizes = [T - 1, T, T + 1, 3 * T + 5]
    clouds = [(rng.normal(size=(n, 3)) * np.array([20.0, 9.0, 2.0])).astype(np.float32) for n in sizes]
    for c in clouds:
        c[-1] = (90.0, 40.0, 9.0)              # the farthest point is the last one of the last tile
    got = _run(clouds)
    for k, c in enumerate(clouds):
        _check(got, k, c, 100, sizes[k])


@pytest.mark.parametrize("bins", [1, 7, 100, 256])
def test_bin_counts(g, bins):
    clouds = [g[n]["cloud"] for n in ("gauss7", "gauss1000", "lidar", "edges", "grid", "zeros")]
    got = _run(clouds, bins)
    assert got[0].shape == (len(clouds), bins)
    for k, c in enumerate(clouds):
        _check(got, k, c, bins, (bins, k))
        assert got[1][k].sum() == len(c)


def test_bins_out_of_range():
    pts, offs = _pack([np.zeros((4, 3), np.float32)])
    for bins in (0, 257):
        with pytest.raises(ValueError):
            _F().range_histogram_batch(pts, offs, bins)
    from mr_slam_amd import _lib
    hist = torch.zeros(300, dtype=torch.float64, device=DEV)
    with pytest.raises(_lib.MrsError, match="bins in 1..256"):
        _lib.load().mrs_fh_batch(_lib.ctx(0), pts, 0, 3, offs.to(DEV), offs, 1, 257, hist, None, None, None, None)


def test_contention_one_bin():
    """50 000 points on a sphere of radius ~5 and one point at range 1000 (w = 10): every point but one lands in bucket 0"""
    rng = np.random.default_rng(43)
    v = rng.normal(size=(50000, 3))
    v = (5.0 * v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    cloud = np.concatenate([v, np.array([[1000.0, 0.0, 0.0]], np.float32)])
    got = _run([cloud])
    _check(got, 0, cloud, 100)
    assert got[1][0][0] == 50000 and got[1][0][99] == 1


def test_non_finite_points():
    """deviation 3: a point with a non-finite coordinate goes to the last bucket and does not take part in M"""
    rng = np.random.default_rng(47)
    cloud = (rng.normal(size=(3000, 3)) * 5.0).astype(np.float32)
    cloud[5, 0] = np.nan
    cloud[70, 1] = np.inf
    cloud[71, 2] = -np.inf
    cloud[2999] = (np.nan, np.inf, 0.0)
    big = np.array([[1e30, 1e30, 0.0]], np.float32)           # finite in float32 and in the float64 the kernel computes in
    got = _run([cloud, np.concatenate([cloud, big])], 7)
    _check(got, 0, cloud, 7)
    _check(got, 1, np.concatenate([cloud, big]), 7)
    assert np.isfinite(got[2]).all() and got[1][0].sum() == 3000
    finite = np.isfinite(cloud).all(axis=1)
    assert got[1][0][6] >= 4 and _same_bits(got[2][0], R.ranges(cloud[finite]).max())
    # a range that overflows float64 (finite coordinates) is treated like a non-finite point
    huge = np.array([[1e200, 1e200, 0.0], [3.0, 4.0, 0.0], [1.0, 0.0, 0.0]], np.float64)
    got = _run([huge], 5)
    _check(got, 0, huge, 5)
    assert got[2][0] == 5.0 and got[1][0].tolist() == [0, 1, 0, 0, 2]


def test_scalar_forms_agree(g, batched):
    """mrs_fh_host and the drop-in's statisticsOnRange against the batched call"""
    from mr_slam_amd import _lib
    from mr_slam_amd.compat import FastHistogram as D
    names, clouds, (hist, counts, M, unbound) = batched
    for name in ("gauss2", "gauss1000", "lidar", "grid", "zeros", "empty", "one"):
        k = names.index(name)
        c = np.ascontiguousarray(clouds[k])
        h, cn, rg, ub = np.full(100, -1.0), np.full(100, -1, np.int32), np.full(1, -1.0), np.full(1, -1, np.int32)
        _lib.load().mrs_fh_host(_lib.ctx(0), c, 0, 3, c.shape[0], 100, h, cn, rg, ub)
        assert _same_bits(h, hist[k]) and np.array_equal(cn, counts[k]) and _same_bits(rg[0], M[k]) and ub[0] == unbound[k], name
        v = D.statisticsOnRange(c)
        assert isinstance(v, np.ndarray) and v.dtype == np.float64 and v.shape == (100,) and _same_bits(v, hist[k]), name
        assert D.calculateRange(c) == (0.0, float(M[k])), name
    v = D.statisticsOnRange(g["lidar"]["cloud"].tolist(), b=7)       # a list of lists, as the reference accepts
    assert _same_bits(v, R.range_histogram(g["lidar"]["cloud"].astype(np.float64), 7).hist)
    one = _F().range_histogram(g["grid"]["cloud"])
    k = names.index("grid")
    assert _same_bits(one[0].cpu().numpy(), hist[k]) and float(one[2]) == M[k] and int(one[3]) == 0


# ---- database ------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def entries():
    """1 000 histograms of 100 buckets (counts of 500 draws / 500), rows 10, 400 and 999 equal to row 3"""
    rng = np.random.default_rng(53)
    e = np.stack([np.bincount(rng.integers(0, 100, 500), minlength=100) for _ in range(1000)]).astype(np.float64) / 500.0
    e[10] = e[400] = e[999] = e[3]
    return e


@pytest.fixture(scope="module")
def db(entries):
    """grown far past its capacity hint; the first half appended from host arrays, the second from device tensors"""
    d = _F().FastHistogramDatabase(0, capacity=8, bins=100)
    assert len(d) == 0
    dev = torch.from_numpy(entries).to(DEV)
    for i in range(500):
        d.append(entries[i])
    for i in range(500, 1000):
        d.append(dev[i])
    assert len(d) == 1000
    return d


def test_db_distances_bits(db, entries):
    rng = np.random.default_rng(59)
    for q in (entries[3], np.bincount(rng.integers(0, 100, 777), minlength=100) / 777.0):
        want = R.emd_all(q, entries)
        got = db.distances(q)
        assert got.is_cuda and got.dtype == torch.float64 and _same_bits(got.cpu().numpy(), want)
        got_dev = db.distances(torch.from_numpy(q).to(DEV))
        assert _same_bits(got_dev.cpu().numpy(), want)
    assert want.min() > 0.0 and R.emd_all(entries[3], entries)[[3, 10, 400, 999]].tolist() == [0.0] * 4


@pytest.mark.parametrize("k", [1, 10, 32])
def test_db_query_sorted_ties_low(db, entries, k):
    for q in (entries[3], entries[77] * 0.5 + entries[78] * 0.5):
        want = R.emd_all(q, entries)
        order = np.lexsort((np.arange(1000), want))[:k]
        idx, dist = db.query(q, k)
        assert idx.dtype == np.int32 and dist.dtype == np.float64 and len(idx) == k
        assert np.array_equal(idx, order) and _same_bits(dist, want[order])
        idx_d, dist_d = db.query(torch.from_numpy(q).to(DEV), k)
        assert np.array_equal(idx_d, idx) and _same_bits(dist_d, dist)
    if k >= 10:
        idx, dist = db.query(entries[3], k)
        assert idx[:4].tolist() == [3, 10, 400, 999] and not dist[:4].any() and dist[4] > 0


def test_db_empty_small_and_other_bins():
    F = _F()
    d = F.FastHistogramDatabase(0, capacity=4, bins=7)
    q = np.arange(7) / 21.0
    idx, dist = d.query(q, 5)
    assert len(d) == 0 and len(idx) == 0 and len(dist) == 0 and d.distances(q).shape == (0,)
    rows = np.stack([np.roll(q, s) for s in range(3)])
    for r in rows:
        d.append(r)
    idx, dist = d.query(q, 5)                                    # fewer entries than k
    want = R.emd_all(q, rows)
    assert idx.tolist() == [0, 1, 2][:3] and np.array_equal(idx, np.lexsort((np.arange(3), want))) and _same_bits(dist, want[idx])
    with pytest.raises(ValueError):
        d.query(q, 33)
    big = F.FastHistogramDatabase(0, capacity=2, bins=256)       # more buckets than one LDS block of the sweep, more entries than one workgroup
    rng = np.random.default_rng(61)
    rows = rng.random((130, 256))
    for r in rows:
        big.append(r)
    assert _same_bits(big.distances(rows[129]).cpu().numpy(), R.emd_all(rows[129], rows))


def test_db_wrong_kind_refused(db):
    from mr_slam_amd import _lib, m2dp
    api = _lib.load()
    other = m2dp.M2DPDatabase(0, 4)
    q = np.zeros(192, np.float64)
    idx, dist, cnt = np.zeros(1, np.int32), np.zeros(1, np.float64), C.c_int32(0)
    with pytest.raises(_lib.MrsError, match="not a Fast Histogram database") as e:
        api.mrs_loopdb_append_fh(other._h, q, 0, None)
    assert e.value.status == 1
    with pytest.raises(_lib.MrsError, match="not a Fast Histogram database"):
        api.mrs_loopdb_query_fh(other._h, q, 0, 1, idx, dist, C.byref(cnt), None)
    with pytest.raises(_lib.MrsError, match="not a Fast Histogram database"):
        api.mrs_loopdb_distances_fh(other._h, q, 0, None, None)
    with pytest.raises(_lib.MrsError, match="not an M2DP database.*mrs_loopdb_append_fh"):
        api.mrs_loopdb_append_m2dp(db._h, q, 0, None)
    with pytest.raises(_lib.MrsError, match="not a RING / RING\\+\\+ database.*mrs_loopdb_append_fh"):
        api.mrs_loopdb_append(db._h, q, 0, 1, None)
    with pytest.raises(_lib.MrsError, match="bins in 1..256"):
        api.mrs_loopdb_create(_lib.ctx(0), 5, 0, 4, C.byref(C.c_void_p()))
    assert len(db) == 1000 and len(other) == 0
