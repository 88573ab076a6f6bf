"""GPU suite for M2DP (m2dp.hip, the MRS_LOOPDB_M2DP loop database, mr_slam_amd.m2dp and the pr_methods.M2DP drop-in) against
tests/golden/ref_m2dp.npz, which the reference's own M2DP.py produced, and against the NumPy restatement tests/golden/m2dp_restate.py,
which tests/test_m2dp_cpu.py checks against that fixture.

Counts are integers and are compared exactly.  D is the number of (point, plane) pairs two count matrices bin differently, U the number
of pairs the restatement finds within 1e-9 maxRho of a bin edge (either side is then a correct answer): D <= U is demanded plane by plane,
and U itself is bounded, so the demand is effectively exact counts.  One case is structural: a 3-point cloud is coplanar with its centroid
and lies exactly edge-on to the four planes of elevation 0 (m2dp_restate.EDGE_ON_ROWS), where its 12 pairs sit ON a theta edge in exact
arithmetic and every implementation, the reference included, returns the sign of rounding noise; those 12 are left out of U's bound and
nothing else is."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import m2dp_restate as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = np.finfo(np.float64).eps


def _M():
    from mr_slam_amd import m2dp
    return m2dp


def _pack(clouds, dtype=None, stride=3):
    dtype = dtype or clouds[0].dtype
    offs = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int64)
    pts = np.full((int(offs[-1]), stride), 7.5, dtype)         # columns past xyz hold something that must not matter
    if offs[-1]:
        pts[:, :3] = np.concatenate([np.asarray(c, dtype).reshape(-1, 3) for c in clouds])
    return torch.from_numpy(pts).to(DEV), torch.from_numpy(offs)


def _run(clouds, dtype=None, stride=3):
    p, o = _pack(clouds, dtype, stride)
    desc, A = _M().m2dp_batch(p, o)
    torch.cuda.synchronize()
    return desc.cpu().numpy(), A.cpu().numpy()


def _cloud(seed, n):
    """anisotropic Gaussian (axis scales 25 : 10 : 1.75 up to +-15 %, so at least 1.5 apart), randomly turned, offset mean"""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    scale = np.array([25.0, 10.0, 1.75]) * rng.uniform(0.87, 1.15, 3)
    return (rng.normal(size=(n, 3)) * scale) @ q.T + rng.uniform(-15, 15, size=3)


def _counts(A, n):
    c = np.rint(A * n)
    assert np.abs(A * n - c).max() < 1e-6
    return c.astype(np.int64)


# --------------------------------------------------------------------------------------------------------------------- fixture parity
@pytest.fixture(scope="module")
def g():
    return R.load()


@pytest.fixture(scope="module")
def fixture_run(g):
    """every fixture cloud alone, as float64 (the contract: M2DP(cloud.astype(np.float64)))"""
    return {name: _run([c["cloud"].astype(np.float64)]) for name, c in g.items()}


@pytest.mark.parametrize("name", ["gauss3", "gauss64", "gauss1000", "gauss4097", "lidar", "nclt"])
def test_fixture_parity(g, fixture_run, name):
    c, (desc, A) = g[name], fixture_run[name]
    n = c["cloud"].shape[0]
    counts = _counts(A[0], n)
    assert (counts.sum(axis=1) == n).all() and np.abs(A[0].sum(axis=1) - 1.0).max() < 1e-12
    diff = R.differing_pairs(counts, c["counts"])
    noisy = list(R.EDGE_ON_ROWS) if n == 3 else []
    print(name, "differing pairs", int(diff.sum()))
    assert not np.delete(diff, noisy).any(), (name, int(diff.sum()))
    assert (diff[noisy] <= 3).all()
    bound = R.svd_bound(c["sigma1"], c["sigma2"])
    if diff.any():        # the edge-on rows of the 3-point cloud fell on the other side of the noise: LAPACK's vectors of the GPU's own A
        u, s, vh = np.linalg.svd(A[0])
        want, bound = R.canonical(np.concatenate([u[:, 0], vh[0]])), R.svd_bound(s[0], s[1])
    else:
        want = R.canonical(c["desc"])
    err = np.abs(desc[0] - want).max()
    print(name, "descriptor error", err, "bound", bound)
    assert desc[0][:64].sum() >= 0 and (desc[0] >= 0).all()
    assert err <= bound, (name, err, bound)


# ------------------------------------------------------------------------------------------- random clouds against the live restatement
def _sizes():
    t = _M().TILE_POINTS
    return [3, 63, 64, 65, t - 1, t + 1, 120000]


@pytest.fixture(scope="module")
def random_run():
    """the seven sizes in ONE batched call, the PCA stage of the same batch, and the restatement of each cloud"""
    clouds = [_cloud(100 + i, n) for i, n in enumerate(_sizes())]
    p, o = _pack(clouds)
    M = _M()
    desc, A = M.m2dp_batch(p, o)
    pca = M.pca_batch(p, o)
    torch.cuda.synchronize()
    return clouds, desc.cpu().numpy(), A.cpu().numpy(), pca.cpu().numpy(), [R.m2dp(c) for c in clouds]


@pytest.mark.parametrize("i", range(7))
def test_random_cloud_against_restatement(random_run, i):
    clouds, desc, A, pca, want = random_run
    n, r = len(clouds[i]), want[i]
    assert n == _sizes()[i]
    counts = _counts(A[i], n)
    assert (counts.sum(axis=1) == n).all()
    diff = R.differing_pairs(counts, r.counts)
    D, U = int(diff.sum()), r.uncertain
    structural = 4 * n if n == 3 else 0        # the 3-point cloud's pairs that lie ON a theta edge in exact arithmetic (module docstring)
    print("n", n, "D", D, "U", U, "structural", structural)
    assert U - structural <= 1e-6 * 64 * n + 1
    if structural:
        assert r.uncertain_rows[list(R.EDGE_ON_ROWS)].sum() >= structural
    assert D <= U and (diff <= r.uncertain_rows).all()
    mean, comps, max_rho = pca[i, 0:3], pca[i, 3:12].reshape(3, 3), pca[i, 12]
    print("maxRho", max_rho, r.max_rho)
    assert abs(max_rho - r.max_rho) <= 1e-12 * r.max_rho
    assert np.abs(comps @ comps.T - np.eye(3)).max() < 1e-14
    if D == 0:
        err = np.abs(desc[i] - r.desc).max()
        print("descriptor error", err)
        assert err <= R.svd_bound(r.sigma1, r.sigma2)


# ------------------------------------------------------------------------------------------------------------------------ ragged batch
def test_ragged_batch_is_bit_identical_to_single_runs():
    sizes = [5000, 0, 2, 4097, 1]
    clouds = [_cloud(200 + i, n) for i, n in enumerate(sizes)]
    desc, A = _run(clouds)
    desc2, A2 = _run(clouds)
    assert np.array_equal(desc, desc2) and np.array_equal(A, A2)
    for i, n in enumerate(sizes):
        if n < 3:
            assert not desc[i].any() and not A[i].any()
        else:
            d1, a1 = _run([clouds[i]])
            assert np.array_equal(d1[0], desc[i]) and np.array_equal(a1[0], A[i]), n
            assert np.abs(A[i].sum(axis=1) - 1.0).max() < 1e-12 and abs(np.linalg.norm(desc[i][:64]) - 1.0) < 1e-14


# ------------------------------------------------------------------------------------------------------------------------- input types
def test_float32_input_equals_its_widening_and_stride_does_not_matter():
    c32 = _cloud(300, 3000).astype(np.float32)
    d32, a32 = _run([c32], np.float32)
    d64, a64 = _run([c32.astype(np.float64)], np.float64)
    assert np.array_equal(d32, d64) and np.array_equal(a32, a64)
    for dt in (np.float32, np.float64):
        d4, a4 = _run([c32], dt, stride=4)
        assert np.array_equal(d4, d64) and np.array_equal(a4, a64)
    M = _M()
    d1, a1 = M.m2dp(c32)
    assert np.array_equal(d1.cpu().numpy(), d64[0]) and np.array_equal(a1.cpu().numpy(), a64[0])


# -------------------------------------------------------------------------------------------------------------------- degenerate clouds
def test_degenerate_clouds_are_finite():
    same = np.tile(np.array([[1.5, -2.0, 0.25]]), (500, 1))
    t = np.random.default_rng(400).normal(size=(700, 1))
    line = np.array([[3.0, 1.0, -2.0]]) + t * np.array([[0.6, -0.3, 0.74]])
    nonfinite = _cloud(401, 300)
    nonfinite[17, 1] = np.nan
    nonfinite[40, 0] = np.inf
    desc, A = _run([same, line, nonfinite])
    for i in (0, 1):
        assert np.isfinite(desc[i]).all() and np.isfinite(A[i]).all()
        assert np.abs(A[i].sum(axis=1) - 1.0).max() < 1e-12
    assert np.abs(A[2].sum(axis=1) - 1.0).max() < 1e-12          # non-finite input: every pair still lands in a bin of its own plane


# --------------------------------------------------------------------------------------------------------------------------- database
@pytest.fixture(scope="module")
def db_descs():
    """1000 descriptors from the builder itself: 1000 clouds of 200 points in one call"""
    rng = np.random.default_rng(500)
    clouds = [_cloud(int(s), 200) for s in rng.integers(1000, 1 << 30, 1000)]
    return _run(clouds)[0]


def _check_knn(idx, d2, entries, q, k):
    E = entries.astype(np.float32).astype(np.float64)
    want = ((E - q.astype(np.float32).astype(np.float64)) ** 2).sum(axis=1)
    slack = 2 * 192 * 2.0 ** -24 * want.max()
    order = np.argsort(want, kind="stable")
    cnt = min(k, len(E))
    assert len(idx) == len(d2) == cnt and len(set(idx.tolist())) == cnt
    assert np.abs(d2 - want[idx]).max() <= slack
    assert (np.diff(want[idx]) >= -slack).all()                                   # a valid ascending order
    assert (want[idx] <= want[order[cnt - 1]] + slack).all()                      # and a valid top k
    ws = want[order]
    for i in range(cnt):                                                          # the brute force's index wherever it is a clear winner
        lo = i == 0 or ws[i] - ws[i - 1] > slack
        hi = i + 1 >= len(ws) or ws[i + 1] - ws[i] > slack
        if lo and hi:
            assert idx[i] == order[i], i


def test_database_knn(db_descs):
    M = _M()
    db = M.M2DPDatabase(capacity=16)                              # grows while it is filled
    dev = torch.from_numpy(db_descs).to(DEV)
    for i in range(len(db_descs)):
        db.append(dev[i] if i % 2 else db_descs[i])               # device and host arguments alternate
    assert len(db) == 1000
    rng = np.random.default_rng(501)
    for qi in (3, 512):
        q = db_descs[qi] + rng.normal(0, 1e-3, 192)
        idx, d2 = db.query(q, 10)
        _check_knn(idx, d2, db_descs, q, 10)
        assert idx[0] == qi
        idx_d, d2_d = db.query(torch.from_numpy(q).to(DEV), 10)   # host and device arguments: the same result
        assert np.array_equal(idx, idx_d) and np.array_equal(d2, d2_d)
    idx, d2 = db.query(db_descs[7], 32)
    _check_knn(idx, d2, db_descs, db_descs[7], 32)
    assert idx[0] == 7 and d2[0] == 0.0


def test_database_small_empty_and_wrong_kind(db_descs):
    from mr_slam_amd import _lib, scancontext
    M = _M()
    db = M.M2DPDatabase()
    idx, d2 = db.query(db_descs[0], 5)                            # empty: count 0
    assert len(idx) == 0 and len(d2) == 0
    raw_i, raw_d, cnt = np.zeros(5, np.int32), np.zeros(5, np.float32), C.c_int32(7)
    _lib.load().mrs_loopdb_query_m2dp(db._h, db_descs[0].copy(), 0, 5, raw_i, raw_d, C.byref(cnt), None)
    assert cnt.value == 0 and (raw_i == -1).all() and np.isinf(raw_d).all()
    for i in range(3):
        db.append(db_descs[i])
    idx, d2 = db.query(db_descs[1], 10)                           # k > n
    _check_knn(idx, d2, db_descs[:3], db_descs[1], 10)
    assert len(idx) == 3 and idx[0] == 1
    with pytest.raises(ValueError):
        db.query(db_descs[0], 33)
    lib = _lib.load()
    sc = scancontext.ScanContextDatabase()
    buf, i32, f32 = np.zeros(120 * 120, np.float32), np.zeros(4, np.int32), np.zeros(4, np.float32)
    cnt = C.c_int32(0)
    for call in (lambda: lib.mrs_loopdb_append_m2dp(sc._h, db_descs[0].copy(), 0, None),
                 lambda: lib.mrs_loopdb_query_m2dp(sc._h, db_descs[0].copy(), 0, 1, i32, f32, C.byref(cnt), None),
                 lambda: lib.mrs_loopdb_append_sc(db._h, buf, 0, None),
                 lambda: lib.mrs_loopdb_query_sc(db._h, buf, 0, 1, 0.1, i32, f32, f32.copy(), i32.copy(), C.byref(cnt), None),
                 lambda: lib.mrs_loopdb_append(db._h, buf, 0, 1, None),
                 lambda: lib.mrs_loopdb_query_m2dp(db._h, db_descs[0].copy(), 0, 0, i32, f32, C.byref(cnt), None)):
        with pytest.raises(_lib.MrsError) as e:
            call()
        assert e.value.status == 1
    assert len(db) == 3 and len(sc) == 0


# ----------------------------------------------------------------------------------------------------------------------------- drop-in
def test_dropin():
    from mr_slam_amd import compat
    saved = {k: sys.modules.pop(k) for k in list(sys.modules) if k.split(".")[0] == "pr_methods"}
    try:
        compat.install(m2dp=True)
        from pr_methods.M2DP import M2DP
        cloud = _cloud(600, 2500)
        for c in (cloud, cloud.astype(np.float32)):
            desc, A = M2DP(c)
            assert isinstance(desc, np.ndarray) and isinstance(A, np.ndarray)
            assert desc.shape == (192,) and A.shape == (64, 128) and desc.dtype == A.dtype == np.float64
            d, a = _M().m2dp(c)
            assert np.array_equal(desc, d.cpu().numpy()) and np.array_equal(A, a.cpu().numpy())
        desc, A = M2DP(np.zeros((0, 3)))
        assert desc.shape == (192,) and A.shape == (64, 128) and not desc.any() and not A.any()
        desc, A = M2DP(cloud[:2])
        assert not desc.any() and not A.any()
    finally:
        for k in [k for k in sys.modules if k.split(".")[0] == "pr_methods"]:
            sys.modules.pop(k)
        sys.modules.update(saved)
