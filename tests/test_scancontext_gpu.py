"""GPU suite for Scan Context (scancontext.hip, the MRS_LOOPDB_SC loop database, mr_slam_amd.scancontext and the pr_methods.ScanContext
drop-in) against tests/golden/ref_scancontext.npz, which the reference's own ScanContext.py produced, and the NumPy restatement in
tests/golden/sc_restate.py, which tests/test_scancontext_cpu.py checks against that fixture."""
import ctypes as C
import os
import sys
import threading

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import sc_restate as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def g():
    return R.load()


def _cloud_inputs():
    import make_golden_scancontext as M
    return M.clouds()


def _check_align(gpu_dist, gpu_shift, sc1, sc2, ratio, ref_dist, ref_shift, sector_norms, ref_window):
    """dist within 1e-5; the shift exact where both stages have a clear winner (or an exact tie resolved to the first); elsewhere the
    dist must be the reference's window dist at the GPU's shift"""
    assert abs(gpu_dist - ref_dist) < 1e-5, (gpu_dist, ref_dist)
    s_ref = int(np.argmin(sector_norms))
    if R.clear_winner(sector_norms, s_ref, rel=1e-6) and R.clear_winner(ref_window, int(np.argmin(ref_window)), abs_=1e-5):
        assert gpu_shift == ref_shift, (gpu_shift, ref_shift)
    else:
        assert abs(gpu_dist - R.window_dists(sc1, sc2, [gpu_shift])[0]) < 1e-5


# ------------------------------------------------------------------------------------------------------------- descriptors and keys
def test_descriptors_bit_identical_and_keys(g):
    from mr_slam_amd import bev, scancontext as SC
    cl = _cloud_inputs()
    names = list(g["names"])[: int(g["n_cloud_descriptors"][0])]
    for name in names:
        got = SC.generate_scan_context(cl[name]).cpu().numpy()
        assert np.array_equal(got, g["sc"][names.index(name)]), name
    xyz, offs = bev.pack_scans([cl[n] for n in names], DEV)
    batch = SC.sc_descriptors(xyz, offs).cpu().numpy()
    assert np.array_equal(batch, g["sc"][: len(names), 0])
    ring, sector = SC.keys(torch.from_numpy(g["sc"]).to(DEV))
    assert np.abs(ring.cpu().numpy() - g["ringkey"]).max() < 1e-6
    assert np.abs(sector.cpu().numpy() - g["sectorkey"]).max() < 1e-6
    assert np.abs(SC.make_ringkey(torch.from_numpy(g["sc"][0]).to(DEV)).cpu().numpy() - g["ringkey"][0]).max() < 1e-6


# ------------------------------------------------------------------------------------------------------------- pairwise alignment
def test_pairwise_dist_align_and_distance(g):
    from mr_slam_amd import scancontext as SC
    D = torch.from_numpy(g["sc"]).to(DEV)
    P = g["pairs"]
    a, b = D[P[:, 0]], D[P[:, 1]]
    for q, ratio in enumerate(g["ratios"]):
        dist, shift = SC.dist_align_sc(a, b, float(ratio))
        dist, shift = dist.cpu().numpy(), shift.cpu().numpy()
        for p, (i, j) in enumerate(P):
            wd = g["window_dists"][q, p]
            _check_align(float(dist[p]), int(shift[p]), g["sc"][i], g["sc"][j], ratio, g["dist_align"][q, p, 0], int(g["dist_align"][q, p, 1]),
                         g["sector_norms"][p], wd[~np.isnan(wd)])
    d, yaw = SC.distance_sc(a, b)
    d, yaw = d.cpu().numpy(), yaw.cpu().numpy()
    for p, (i, j) in enumerate(P):
        assert abs(d[p] - g["distance_sc"][p, 0]) < 1e-5
        assert 1 <= int(yaw[p]) <= 120
    direct = SC.dist_direct_sc(a, b).cpu().numpy()
    assert np.abs(direct - g["dist_direct"]).max() < 1e-5


def test_pairwise_quirks(g):
    from mr_slam_amd import scancontext as SC
    names = list(g["names"])
    A = torch.from_numpy(g["sc"][names.index("A")]).to(DEV)
    Z = torch.zeros_like(A)
    for ratio, first in ((0.1, -6), (0.2, -12), (1.0, -60)):
        d, s = SC.dist_align_sc(A, Z, ratio)                 # exact sector-key tie -> s* = 0; all dists 1.0 -> start of the window
        assert float(d) == 1.0 and int(s) == first
        d, s = SC.dist_align_sc(Z, Z, ratio)
        assert float(d) == 1.0 and int(s) == first
        d, s = SC.dist_align_sc(Z, A, ratio)
        assert float(d) == 1.0
    d, yaw = SC.distance_sc(Z, A)
    assert float(d) == 1.0 and int(yaw) == 1
    d, s = SC.dist_align_sc(A, A, 0.1)
    assert abs(float(d)) < 1e-6 and int(s) == 0


def test_polar_geometry_and_limits():
    from mr_slam_amd import _lib, scancontext as SC
    rng = np.random.default_rng(7)
    a = (rng.random((3, 20, 60)) * (rng.random((3, 20, 60)) > 0.5)).astype(np.float32)
    b = np.roll(a, 13, axis=-1)
    d, s = SC.dist_align_sc(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV), 0.5)
    for i in range(3):
        wd, ws = R.dist_align(a[i], b[i], 0.5)[:2]
        assert abs(float(d[i]) - wd) < 1e-5 and int(s[i]) == ws and ws % 60 == 47     # roll(b, 47) == a
    big = torch.zeros((1, 129, 129), device=DEV)
    with pytest.raises(_lib.MrsError, match="UNSUPPORTED|unsupported|exceeds"):
        SC.dist_align_sc(big, big)


# ------------------------------------------------------------------------------------------------------------- database
def _distinct(g, count=64):
    """`count` distinct descriptors derived from the fixture's non-zero ones (rolled, re-weighted)"""
    base = [d[0] for d, n in zip(g["sc"], g["names"]) if d.any()]
    out = []
    for i in range(count):
        d = np.roll(base[i % len(base)], (7 * i) % 120, axis=-1)
        out.append((d * (1.0 + 0.05 * (i // len(base)))).astype(np.float32))
    return np.stack(out)


def _db_entries(g, n=10000):
    dist = _distinct(g)
    scale = (1.0 + np.arange(n) // 64 * 1e-4).astype(np.float32)
    return dist, scale


def _entry(dist, scale, e):
    return (dist[e % 64] * scale[e]).astype(np.float32)


@pytest.fixture(scope="module")
def big_db(g):
    from mr_slam_amd.scancontext import ScanContextDatabase
    dist, scale = _db_entries(g)
    db = ScanContextDatabase(0, capacity=1)
    for e in range(len(scale)):
        db.append(_entry(dist, scale, e) if e % 2 else torch.from_numpy(_entry(dist, scale, e)).to(DEV))
    torch.cuda.synchronize()
    ring = np.stack([R.keys(_entry(dist, scale, e))[0] for e in range(len(scale))]).astype(np.float32).astype(np.float64)
    return db, dist, scale, ring


def _queries(g):
    names = list(g["names"])
    return [g["sc"][names.index(n)][0] for n in ("A", "B_roll60", "C_empty", "S12")]


def test_database_query_top_k(g, big_db):
    db, dist, scale, ring = big_db
    assert len(db) == len(scale)
    for q in _queries(g):
        rq = R.keys(q)[0].astype(np.float32).astype(np.float64)      # the float32 keys, distances in fp64 (sklearn's metric)
        d2 = ((ring - rq[None, :]) ** 2).sum(1)
        order = np.lexsort((np.arange(len(d2)), d2))
        for k in (1, 10):
            idx, kd, dd, sh = db.query(q, num_candidates=k, search_ratio=0.1)
            assert list(idx) == list(order[:k])
            assert np.allclose(kd, np.sqrt(d2[order[:k]]), rtol=1e-5)
            for i, e in enumerate(idx):
                sc1 = _entry(dist, scale, e)
                wd, ws, _, win, nrm = R.dist_align(sc1, q, 0.1)
                _check_align(float(dd[i]), int(sh[i]), sc1, q, 0.1, wd, ws, nrm, win)


def test_database_query_all_and_host_device_bits(g, big_db):
    db, dist, scale, ring = big_db
    q = _queries(g)[0]
    d_all, s_all, best = db.query_all(q, 0.1)
    assert len(d_all) == len(scale)
    # the 64 distinct descriptors repeat under a scale factor that leaves every cosine as it is: check the distinct ones + a sample
    rng = np.random.default_rng(3)
    sample = sorted(set(rng.choice(len(scale), 256, replace=False)) | set(range(64)))
    for e in sample:
        sc1 = _entry(dist, scale, e)
        wd, ws, _, win, nrm = R.dist_align(sc1, q, 0.1)
        _check_align(float(d_all[e]), int(s_all[e]), sc1, q, 0.1, wd, ws, nrm, win)
    assert best == int(np.argmin(d_all))
    exp = np.array([R.dist_align(dist[i], q, 0.1)[0] for i in range(64)])
    assert abs(d_all[best] - exp.min()) < 1e-5
    d2, s2, b2 = db.query_all(torch.from_numpy(q).to(DEV), 0.1)
    assert np.array_equal(d_all.view(np.uint32), d2.view(np.uint32)) and np.array_equal(s_all, s2) and best == b2
    r1 = db.query(q, 10)
    r2 = db.query(torch.from_numpy(q).to(DEV), 10)
    for x, y in zip(r1, r2):
        assert np.array_equal(np.asarray(x).view(np.uint32), np.asarray(y).view(np.uint32))
    # the same query twice: same bits
    d3, s3, _ = db.query_all(q, 0.1)
    assert np.array_equal(d_all.view(np.uint32), d3.view(np.uint32)) and np.array_equal(s_all, s3)


def test_empty_database_and_wrong_kind_calls_raise(g):
    from mr_slam_amd import _lib
    from mr_slam_amd.node import LoopDatabase, DiscoDatabase
    from mr_slam_amd.scancontext import ScanContextDatabase
    lib = _lib.load()
    db = ScanContextDatabase(0, capacity=4)
    q = g["sc"][0][0]
    idx, kd, dd, sh = db.query(q, 10)
    assert len(idx) == 0
    assert db.query_all(q) [2] == -1 and len(db.query_all(q)[0]) == 0
    h = db._h
    buf = np.zeros(2 * 120 * 120, np.float32)
    i32 = np.zeros(64, np.int32)
    f32 = np.zeros(64, np.float32)
    cnt = C.c_int32(0)

    def rejected(fn, *args):
        with pytest.raises(_lib.MrsError) as e:
            fn(*args)
        assert e.value.status == 1

    # RING / RING++ / DiSCO entry points on an SC handle
    rejected(lib.mrs_loopdb_append, h, buf, 0, 1, None)
    rejected(lib.mrs_loopdb_query, h, buf, 0, 1.0, 4, i32, f32, i32, C.byref(cnt), 0, None, None, None, None)
    rejected(lib.mrs_loopdb_query_multi, h, buf, 0, 1, 4, f32, i32, C.byref(cnt), None)
    rejected(lib.mrs_loopdb_append_disco, h, buf, buf, 0, None)
    rejected(lib.mrs_loopdb_query_disco, h, buf, buf, 0, i32, f32, i32, None)
    assert len(db) == 0
    # SC entry points on RING and DiSCO handles
    for other in (LoopDatabase("ring", None, 0, 4), DiscoDatabase(0, 4)):
        rejected(lib.mrs_loopdb_append_sc, other._h, buf, 0, None)
        rejected(lib.mrs_loopdb_query_sc, other._h, buf, 0, 1, 0.1, i32, f32, f32, i32, C.byref(cnt), None)
        rejected(lib.mrs_loopdb_query_sc_all, other._h, buf, 0, 0.1, 4, f32, i32, C.byref(cnt), C.byref(cnt), None)
        assert len(other) == 0
    rejected(lib.mrs_loopdb_query_sc, h, buf, 0, 65, 0.1, i32, f32, f32, i32, C.byref(cnt), None)


def test_database_threads(g):
    """three callback threads, each appending to its own database and querying the other two (main_SC.py's rospy shape)"""
    from mr_slam_amd.scancontext import ScanContextDatabase
    dist = _distinct(g, 48)
    seq = [(r, dist[r * 16 + i]) for i in range(16) for r in range(3)]

    def run(parallel):
        dbs = [ScanContextDatabase(0, 1) for _ in range(3)]
        out = {r: [] for r in range(3)}
        steps = {r: [d for rr, d in seq if rr == r] for r in range(3)}
        barrier = threading.Barrier(3) if parallel else None

        def worker(r):
            for i, d in enumerate(steps[r]):
                if barrier:
                    barrier.wait()
                dbs[r].append(d)
                if barrier:
                    barrier.wait()
                for o in range(3):
                    if o != r:
                        res = dbs[o].query(d, 3, 0.1)
                        out[r].append((o, i, [np.asarray(x).tobytes() for x in res]))
        if parallel:
            th = [threading.Thread(target=worker, args=(r,)) for r in range(3)]
            [t.start() for t in th]
            [t.join() for t in th]
        else:
            for i in range(16):
                for r in range(3):
                    dbs[r].append(steps[r][i])
                for r in range(3):
                    for o in range(3):
                        if o != r:
                            res = dbs[o].query(steps[r][i], 3, 0.1)
                            out[r].append((o, i, [np.asarray(x).tobytes() for x in res]))
        return out
    assert run(True) == run(False)


# ------------------------------------------------------------------------------------------------------------- node replay, drop-in
def test_node_replay(g):
    from mr_slam_amd.scancontext import ScanContextDatabase
    dbs = {r: ScanContextDatabase(0, 1) for r in (1, 2, 3)}
    rows = []
    for step, (robot, di) in enumerate(g["sequence"]):
        cur = g["sc"][di]
        dbs[robot].append(cur)
        for cand in (1, 2, 3):
            if cand == robot or len(dbs[cand]) < 1:
                continue
            idx, kd, dist, shift = dbs[cand].query(torch.from_numpy(cur).to(DEV), num_candidates=1, search_ratio=0.1)
            rows.append((step, robot, cand, int(idx[0]), float(kd[0]), float(dist[0]), int(shift[0])))
    ref = g["replay"]
    assert len(rows) == len(ref)
    for got, want in zip(rows, ref):
        assert got[:4] == tuple(int(x) for x in want[:4])
        assert abs(got[4] - want[4]) < 1e-5 and abs(got[5] - want[5]) < 1e-5
        if want[5] < 1.0:
            assert got[6] == int(want[6]), (got, want)


def test_dropin_module(g):
    from mr_slam_amd import compat
    saved = {k: sys.modules.pop(k) for k in list(sys.modules) if k.split(".")[0] == "pr_methods"}
    try:
        compat.install(names=(), scancontext=True)
        import pr_methods.ScanContext as SC
        pub = sorted(n for n in dir(SC) if not n.startswith("_") and callable(getattr(SC, n)) and getattr(getattr(SC, n), "__module__", "")
                     == SC.__name__)
        assert pub == sorted(g["public_names"])
        D = g["sc"]
        for i in range(len(D)):
            rk, sk = SC.make_ringkey(D[i]), SC.make_sectorkey(D[i])
            assert rk.dtype == np.float64 and np.abs(rk - g["ringkey"][i]).max() < 1e-6 and np.abs(sk - g["sectorkey"][i]).max() < 1e-6
        for p, (i, j) in enumerate(g["pairs"]):
            d, s = SC.dist_align_sc(D[i], D[j], search_ratio=0.1)
            assert type(d) is float and type(s) is int
            wd = g["window_dists"][0, p]
            _check_align(d, s, D[i], D[j], 0.1, g["dist_align"][0, p, 0], int(g["dist_align"][0, p, 1]), g["sector_norms"][p], wd[~np.isnan(wd)])
            d, yaw = SC.distance_sc(D[i], D[j])
            assert type(d) is float and type(yaw) is int and abs(d - g["distance_sc"][p, 0]) < 1e-5
            assert abs(SC.dist_direct_sc(D[i], D[j]) - g["dist_direct"][p]) < 1e-5
            n, s = SC.fast_align_with_sectorkey(g["sectorkey"][i], g["sectorkey"][j])
            assert abs(n - g["sector_norms"][p].min()) < 1e-9 + 1e-6 * n
            if R.clear_winner(g["sector_norms"][p], int(g["sector_shift"][p]), rel=1e-6):
                assert s == g["sector_shift"][p]
        names = list(g["names"])
        A, A17 = D[names.index("A")], D[names.index("A_roll17")]
        n, s = SC.fast_align(A17, A)
        assert s == 17 and abs(n - np.linalg.norm(A17 - np.roll(A, 17, axis=-1))) < 1e-3
        d, s = SC.dist_align_cc(A, A)
        assert d < 1e-6 and s == 0
    finally:
        for k in [k for k in sys.modules if k.split(".")[0] == "pr_methods"]:
            sys.modules.pop(k)
        sys.modules.update(saved)
