"""GPU suite for the geometry-dependent paths of csrc/scancontext.hip and the nearest-ring-key search behind the Scan Context database, on
the cases of tests/sc_cases.py: odd and uneven row halves, the R = 120 template with S != 120, S on either side of a wave, windows of 1,
17, 33 and 2 S shifts, 128 x 128, more pairs than workgroups with a query per pair, and a database queried at the edges of its 256-entry
chunks.  Expected values are the fp64 restatement's (tests/golden/sc_restate.py, pinned to the reference by tests/test_sc_cases_cpu.py);
the comparison rule and its tolerances are the existing Scan Context tests' (sc_cases.check_align)."""
import ctypes as C

import numpy as np
import pytest
import torch

import sc_cases as sc
from sc_cases import R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_ids = lambda g: "%dx%d" % g      # noqa: E731


def _dev(x):
    return torch.from_numpy(np.array(x)).to(DEV)          # a writable copy of a shared read-only input


def _bits(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


# ------------------------------------------------------------------------------------------------------------------------------- keys
@pytest.mark.parametrize("geom", sc.GEOMETRIES, ids=_ids)
def test_keys(geom):
    from mr_slam_amd import scancontext as SC
    P = sc.pairs(geom)
    pool = [P["tiny"][1], P["AA"][0], P["other0"][0], P["noisy1"][0], P["ZZ"][0]]
    for n in (1, 2, 5):
        d = np.stack(pool[:n])
        ring, sector = SC.keys(_dev(d))
        assert ring.shape == (n, geom[0]) and sector.shape == (n, geom[1])
        ring, sector = ring.cpu().numpy(), sector.cpu().numpy()
        for i in range(n):
            rk, sk = R.keys(d[i])
            assert np.abs(ring[i] - rk).max() < sc.TOL_KEY and np.abs(sector[i] - sk).max() < sc.TOL_KEY, (n, i)
    one = _dev(pool[1])                                    # [R, S]: one descriptor -> [R] and [S], the batch's bits
    ring, sector = SC.keys(_dev(np.stack(pool[:2])))
    assert np.array_equal(_bits(SC.make_ringkey(one)), _bits(ring[1])) and np.array_equal(_bits(SC.make_sectorkey(one)), _bits(sector[1]))


@pytest.mark.parametrize("length", sc.KEY_LENGTHS)
def test_fast_align_with_sectorkey(length):
    from mr_slam_amd import scancontext as SC
    names, k1, k2 = sc.key_pairs(length)
    norm, shift = SC.fast_align_with_sectorkey(_dev(k1), _dev(k2))
    assert norm.dtype == torch.float64 and norm.shape == (len(names),)
    norm, shift = norm.cpu().numpy(), shift.cpu().numpy()
    for p, name in enumerate(names):
        nrm = R.sector_norms(k1[p], k2[p])
        s = int(np.argmin(nrm))
        assert np.isclose(norm[p], nrm[s], rtol=sc.REL_NORM, atol=sc.ABS_NORM), (name, norm[p], nrm[s])
        clear = R.clear_winner(nrm, s, rel=1e-6)
        if name in ("constant", "period"):                 # planted exact ties at 0: shift 0, not len / 2
            assert clear and s == 0 and nrm[0] == 0.0 and norm[p] == 0.0
        if clear:
            assert int(shift[p]) == s, (name, int(shift[p]), s)
        else:
            assert 0 <= int(shift[p]) < length and np.isclose(norm[p], nrm[int(shift[p])], rtol=sc.REL_NORM, atol=sc.ABS_NORM)
        n1, s1 = SC.fast_align_with_sectorkey(_dev(k1[p]), _dev(k2[p]))        # [len]: one pair
        assert n1.dim() == 0 and float(n1) == norm[p] and int(s1) == int(shift[p])


# ----------------------------------------------------------------------------------------------------------------- pairwise functions
@pytest.mark.parametrize("geom", sc.GEOMETRIES, ids=_ids)
def test_pairwise_functions(geom):
    """dist_direct_sc, dist_align_sc at every ratio and distance_sc, all of a geometry's pairs in one batch; then each pair as a batch
    of one, which must give the batch's bits"""
    from mr_slam_amd import scancontext as SC
    S = geom[1]
    names, a, b = sc.batch(geom)
    A, B = _dev(a), _dev(b)
    E = sc.expected(geom)
    got = {"direct": (SC.dist_direct_sc(A, B),), "distance": SC.distance_sc(A, B)}
    for lab, ratio in sc.ratios(S):
        got[lab] = SC.dist_align_sc(A, B, ratio)
    got = {k: tuple(x.cpu().numpy() for x in v) for k, v in got.items()}
    exact = total = 0
    for p, name in enumerate(names):
        assert abs(float(got["direct"][0][p]) - E[name]["direct"]) < sc.TOL_DIST, (name, got["direct"][0][p], E[name]["direct"])
        # distance_sc(sc1, sc2) rolls sc1: 1 - sim(t) = dist_direct_sc(sc2, roll(sc1, t)), t = 1 .. S, first maximum of sim
        d, yaw = float(got["distance"][0][p]), int(got["distance"][1][p])
        assert abs(d - E[name]["distance"][0]) < sc.TOL_DIST and 1 <= yaw <= S, (name, d, yaw, E[name]["distance"])
        dists = R.window_dists(b[p], a[p], range(1, S + 1))
        if not sc.never_exact(geom, name) and R.clear_winner(dists, int(np.argmin(dists)), abs_=sc.TOL_DIST):
            assert yaw == E[name]["distance"][1], (name, yaw, E[name]["distance"])
        else:
            assert abs(d - dists[yaw - 1]) < sc.TOL_DIST
        for lab, ratio in sc.ratios(S):
            dist, shift = got[lab]
            total += 1
            exact += sc.check_align(float(dist[p]), int(shift[p]), a[p], b[p], E[name]["align"][lab], not sc.never_exact(geom, name))
            if name == "ZA":                               # no s* is determined, but whichever it is, its window's first shift comes back
                assert float(dist[p]) == 1.0 and int(shift[p]) in {sc.window(s, ratio, S)[0] for s in range(S)}, (lab, int(shift[p]))
    print("%s: %d of %d shifts compared exactly" % (_ids(geom), exact, total))
    # a batch of one
    one = {k: [] for k in got}
    for p in range(len(names)):
        one["direct"].append((SC.dist_direct_sc(A[p], B[p]),))
        one["distance"].append(SC.distance_sc(A[p], B[p]))
        for lab, ratio in sc.ratios(S):
            one[lab].append(SC.dist_align_sc(A[p], B[p], ratio))
    for k, rows in one.items():
        for x, col in enumerate(got[k]):
            single = torch.stack([r[x] for r in rows])
            assert single.shape == (len(names),)
            assert np.array_equal(_bits(single), _bits(col)), (k, x)


@pytest.mark.parametrize("ratio,S,want", [(r, s, w) for r, s, w, _ in sc.RADIUS_TABLE])
def test_window_starts_at_the_reference_radius(ratio, S, want):
    """zero against zero: every window dist is 1.0, so the first shift of the window comes back, and the sector keys tie exactly, so
    s* = 0: the shift is -round(0.5 * ratio * S) with Python's round on the double product (ScanContext.py:132)"""
    from mr_slam_amd import scancontext as SC
    assert want == round(0.5 * ratio * S)
    Z = torch.zeros((4, S), device=DEV)
    d, s = SC.dist_align_sc(Z, Z, ratio)
    assert float(d) == 1.0 and int(s) == max(-S, -round(0.5 * ratio * S)), (int(s), -want)


def test_more_pairs_than_workgroups():
    """8 x CU + 5 pairs, each with its own query: the persistent loop reloads Q for every pair it takes"""
    from mr_slam_amd import scancontext as SC
    S = sc.MANY_GEOM[1]
    n = 8 * torch.cuda.get_device_properties(0).multi_processor_count + 5
    pairs = [sc.many_pair(i) for i in range(n)]
    dist, shift = SC.dist_align_sc(_dev(np.stack([p[0] for p in pairs])), _dev(np.stack([p[1] for p in pairs])), sc.MANY_RATIO)
    dist, shift = dist.cpu().numpy(), shift.cpu().numpy()
    assert dist.shape == (n,)
    exact = 0
    for i, (a, b) in enumerate(pairs):
        exact += sc.check_align(float(dist[i]), int(shift[i]), a, b, sc.many_expected(i % 6, (i // 6) % S))
    assert exact >= (1 - sc.MAX_WEAK) * n, (exact, n)


def test_refused_geometries_write_nothing():
    from mr_slam_amd import _lib, scancontext as SC
    lib, ctx, stream = _lib.load(), _lib.ctx(0), _lib.current_stream(0)
    n = 2
    for R_, S, status, msg in ((129, 1, 3, "exceeds 128 x 128"), (1, 129, 3, "exceeds 128 x 128"), (0, 5, 1, "must be >= 1")):
        src = torch.ones(n * 129 * 129, device=DEV)
        dist, keyf = torch.full((n,), -7.0, device=DEV), torch.full((n * 129,), -7.0, device=DEV)
        shift = torch.full((n,), -7, dtype=torch.int32, device=DEV)
        norm = torch.full((n,), -7.0, dtype=torch.float64, device=DEV)
        calls = [lambda: lib.mrs_sc_dist_align_pairs(ctx, src, src, n, R_, S, 0.1, dist, shift, stream),
                 lambda: lib.mrs_sc_dist_direct_pairs(ctx, src, src, n, R_, S, dist, stream),
                 lambda: lib.mrs_sc_distance_pairs(ctx, src, src, n, R_, S, dist, shift, stream),
                 lambda: lib.mrs_sc_keys(ctx, src, n, R_, S, keyf, keyf, stream),
                 lambda: lib.mrs_sc_key_align_pairs(ctx, src, src, n, S if S > 128 else R_, norm, shift, stream)]
        for call in calls:
            with pytest.raises(_lib.MrsError, match=msg) as e:
                call()
            assert e.value.status == status
        torch.cuda.synchronize()
        assert bool((dist == -7.0).all()) and bool((shift == -7).all()) and bool((keyf == -7.0).all()) and bool((norm == -7.0).all())
    for shape in ((1, 129, 1), (1, 1, 129)):
        big = torch.zeros(shape, device=DEV)
        with pytest.raises(_lib.MrsError, match="UNSUPPORTED|unsupported|exceeds"):
            SC.dist_align_sc(big, big)
        with pytest.raises(_lib.MrsError, match="UNSUPPORTED|unsupported|exceeds"):
            SC.keys(big)


# ------------------------------------------------------------------------------------------------------------- the 120 x 120 database
def _device_floats(ptr, count):
    """`count` floats at a device address of the library's, copied by the HIP runtime the process already has"""
    paths = sorted({line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line})
    assert len(paths) == 1, paths
    hip = C.CDLL(paths[0])
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    out = np.empty(count, np.float32)
    assert hip.hipMemcpy(out.ctypes.data, ptr, out.nbytes, 2) == 0          # hipMemcpyDeviceToHost
    return out


@pytest.fixture(scope="module")
def staged():
    """one database grown through sc_cases.DB_STAGES; at each stage its ring keys and the answers to every (query, k)"""
    from mr_slam_amd import scancontext as SC
    db = SC.ScanContextDatabase(0, capacity=1)
    Q = sc.db_queries()
    qkeys = {name: SC.keys(_dev(q))[0][0].cpu().numpy() for name, q in Q.items()}
    out, n = {}, 0
    for stage in sc.DB_STAGES:
        while n < stage:
            db.append(sc.db_entry(n) if n % 2 else torch.from_numpy(sc.db_entry(n)).to(DEV))
            n += 1
        assert len(db) == stage
        _, keys_ptr, cnt, _ = db.device_entries()
        assert cnt == stage
        ring = _device_floats(keys_ptr, stage * 120).reshape(stage, 120)
        out[stage] = (ring, {(name, k): db.query(q if k != 10 else _dev(q), k, sc.DB_RATIO) for name, q in Q.items() for k in sc.DB_KS})
    return db, qkeys, out


@pytest.mark.parametrize("stage", sc.DB_STAGES)
def test_database_ring_keys(staged, stage):
    ring = staged[2][stage][0]
    for e in sorted({0, 1, stage // 2, stage - 2, stage - 1} & set(range(stage))) + [e for e in sc.DB_DUPLICATE if e < stage]:
        assert np.abs(ring[e] - R.keys(sc.db_entry(e))[0]).max() < sc.TOL_KEY, e
    if stage > sc.DB_DUPLICATE[1]:
        assert np.array_equal(ring[sc.DB_DUPLICATE[0]].view(np.uint32), ring[sc.DB_DUPLICATE[1]].view(np.uint32))


@pytest.mark.parametrize("stage", sc.DB_STAGES)
def test_database_top_k_at_chunk_edges(staged, stage):
    _, qkeys, out = staged
    ring, answers = out[stage]
    ring = ring.astype(np.float64)
    Q = sc.db_queries()
    for name, q in Q.items():
        d2 = ((ring - qkeys[name].astype(np.float64)[None, :]) ** 2).sum(1)      # the float32 keys, distances in fp64 (sklearn's metric)
        order = np.lexsort((np.arange(stage), d2))                                 # ties: the lower index first
        for k in sc.DB_KS:
            idx, kd, dd, sh = answers[(name, k)]
            c = min(k, stage)
            assert len(idx) == len(kd) == len(dd) == len(sh) == c
            assert list(idx) == list(order[:c]), (name, k)
            assert np.allclose(kd, np.sqrt(d2[order[:c]]), rtol=1e-5)
            for i, e in enumerate(idx):
                sc.check_align(float(dd[i]), int(sh[i]), sc.db_entry(int(e)), q, sc.db_expected(int(e), name))
    idx, kd = answers[("stored", 1)][:2]
    assert idx[0] == 0 and kd[0] == 0.0                                            # the query is entry 0
    if stage > sc.DB_DUPLICATE[1]:
        idx, kd = answers[("duplicate", 10)][:2]
        assert list(idx[:2]) == list(sc.DB_DUPLICATE) and kd[0] == kd[1] == 0.0     # an exact tie of key distances


def test_database_uses_the_reference_radius(staged):
    """ratio 0.075 at 120 sectors: 0.5 * 0.075 * 120 = 4.5 in double, radius 4"""
    db = staged[0]
    n = sc.DB_STAGES[-1]
    assert len(db) == n and round(0.5 * 0.075 * 120) == 4
    zero = np.zeros((120, 120), np.float32)
    for q in (zero, _dev(zero)):
        idx, kd, dd, sh = db.query(q, 64, 0.075)
        assert len(idx) == 64 and np.all(dd == 1.0) and np.all(sh == -4), sorted(set(sh.tolist()))
        d_all, s_all, best = db.query_all(q, 0.075)
        assert len(d_all) == n and np.all(d_all == 1.0) and np.all(s_all == -4) and best == 0, sorted(set(s_all.tolist()))
