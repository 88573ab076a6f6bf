"""CPU suite for the global elevation map: the two NumPy restatements (tests/golden/gem_restate.py: a literal one over Python dicts and
the vectorised sort / join the kernels use) agree bit for bit on every case of tests/gem_cases.py, a snapped position re-keys to its own
key up to the key bound, the cases keep the margin the GPU suite relies on, the C ABI of the feature is declared and bound, and the
shared arithmetic header (gem_cell.hpp), compiled by g++ into a stand-alone program under the address and undefined-behaviour sanitizers,
returns the restatement's bits."""
import os
import subprocess

import numpy as np
import pytest

import gem_cases as GC
from mr_slam_amd import _lib, gem            # at import: without the feature no test of this module runs

R = GC.R
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same_store(a, b):
    assert len(a.subs) == len(b.subs)
    for k, (x, y) in enumerate(zip(a.subs, b.subs)):
        assert R.same(x, y), k
        assert np.array_equal(a.poses[k], b.poses[k]) and np.array_equal(a.centres[k], b.centres[k])


@pytest.mark.parametrize("name", sorted(GC.open_scripts()))
def test_open_submap_literal_equals_vectorised(name):
    a, b = GC.run(R.Literal(), GC.open_scripts()[name]), GC.run(R.Vectorised(), GC.open_scripts()[name])
    _same_store(a, b)


def test_open_submap_facts():
    """what the cases are there to show, on the literal restatement"""
    S = GC.open_scripts()
    sub = lambda name, k=0: GC.run(R.Literal(), S[name]).subs[k]
    assert [sub("n%d" % n).size for n in (0, 1, 65, 1025)] == [0, 1, 65, 1025]
    a = S["dup_in_call"][0][1]
    d = sub("dup_in_call")
    assert d.size == 81 and R.same(d[:5], a[:5])                    # the late copies of a[:5] won, in a's places
    assert np.array_equal(d["z"][6::3], a["z"][6:81:3] + F(1))       # every third record was replaced by b
    assert sub("dup_across_calls").size == 81
    z = sub("signed_zero")
    assert z.size == 4 and z["z"].tolist() == [1, 5, 3, 4]           # (0, 1), (-0, 1), (0, -0), (-0, 0) are four keys; (-0, 1) was replaced
    nd = sub("no_data")
    assert nd.size == 72 - 18 - 2 + 1 and not (nd["z"] == F(-10)).any()  # 18 cells without data; of the first 6, two emptied and one revived
    got = [sub("leaving%d" % k).size for k in range(9)]
    assert got[8] == 0 and all(0 < g < 35 for g in got[:8])        # a zero shift lets nothing in; no shift lets all 35 cells with data in
    st = GC.run(R.Literal(), S["two_submaps"])
    assert [s.size for s in st.subs][:2] == [81, 0] and st.subs[2].size > 27


def test_every_window_clause_is_hit_and_missed():
    w = GC.window_cells()
    half = F(10) * F(0.2) / F(2)
    cx, cy = F(0.25), F(-0.5)
    xl, xh, yl, yh = w["x"] < cx - half, w["x"] > cx + half, w["y"] < cy - half, w["y"] > cy + half
    for geo in (xl | yl, xh | yh, xl | yh, xh | yl, xl, xh, yl, yh):
        assert geo.any() and not geo.all()
    for v, lim in ((w["x"], cx - half), (w["x"], cx + half), (w["y"], cy - half), (w["y"], cy + half)):
        assert np.abs(v - lim).min() > GC.MARGIN


def _play(name, make):
    st, calls = GC.build(name, make)
    stats = []
    for opt in calls:
        st.update_global(opt)
        stats.append((st.dropped, st.matched))
    return st, stats


@pytest.mark.parametrize("name", sorted(GC.scenes()))
def test_update_global_literal_equals_vectorised(name):
    a, sa = _play(name, R.Literal)
    b, sb = _play(name, R.Vectorised)
    _same_store(a, b)
    assert sa == sb
    assert R.same(a.compose(), b.compose())


def test_update_global_facts():
    raw = {n: GC.build(n, R.Literal)[0] for n in GC.scenes()}
    done = {n: _play(n, R.Literal) for n in GC.scenes()}
    st, stats = done["k1"]
    assert stats == [(0, 0)] and R.same(st.subs[0], raw["k1"].subs[0])                  # K = 1: nothing moves, nothing fuses
    st, stats = done["k2_quirk"]
    assert stats == [(0, 0)] and R.same(st.subs[0], raw["k2_quirk"].subs[0])            # two in range: the quirk
    assert st.subs[1].size == raw["k2_quirk"].subs[1].size and not R.same(st.subs[1], raw["k2_quirk"].subs[1])     # moved, not snapped
    assert done["k2_min2"][1][0][1] > 0                                                 # the same two fuse with min_neighbours = 2
    st, stats = done["k3_weighted"]
    assert stats[0][0] == 8 and stats[0][1] > 100                                       # 4 unkeyed records in each of two submaps
    for s in st.subs:
        ok, kx, ky = R._keys_vec(s, GC.RES)
        p = R._pack(kx, ky)
        assert ok.all() and (np.diff(p) > 0).all()                                      # canonical: keyed, one record per key, key order
    # a cell in all three submaps ends with the same record in all three, and its value depends on the order of the pairs
    keys = [set(R._pack(*R._keys_vec(s, GC.RES)[1:]).tolist()) for s in st.subs]
    assert len(keys[0] & keys[1] & keys[2]) > 20
    assert not R.same(st.subs[0], done["k3_as_written"][0].subs[0])                     # the rule matters
    assert done["k3_twice"][1][1][1] > 0                                                # the second call fuses the snapped cells again
    assert done["k3_more_poses"][1][0][1] > 0
    st, stats = done["k3_fewer_poses"]
    assert stats == [(0, 0)] and R.same(st.subs[2], raw["k3_fewer_poses"].subs[2])      # K = 2: submap 2 untouched, the quirk for 0 and 1
    assert R.same(st.subs[0], raw["k3_fewer_poses"].subs[0])                            # submap 0 is never moved
    assert R.same(done["k3_no_poses"][0].compose(), raw["k3_no_poses"].compose())
    st, stats = done["k5"]
    assert st.subs[4].size == raw["k5"].subs[4].size and stats[0][0] == 0               # isolated: raw, duplicates and unkeyed records stay
    assert np.isnan(st.subs[4]["x"]).sum() == 1
    st9 = done["k5_radius9"][0]
    assert st9.subs[3].size == raw["k5_radius9"].subs[3].size and not R.same(st9.subs[3], raw["k5_radius9"].subs[3])
    assert raw["sizes"].subs[0].size == 4097 and raw["sizes"].subs[1].size == 1 and raw["sizes"].subs[2].size == 0


def test_var_gate_and_frontier_are_exercised():
    """one pair, new = submap 1, old = submap 0: a matched cell whose old variance is 0, 1, negative or NaN is left alone in both; an
    open gate gives both the same record with new's colours and the AND of the frontiers"""
    st = GC.build("k3_weighted", R.Literal)[0]
    v = R.Vectorised()
    old, ko = v._canonical(st.subs[0])
    new, kn = v._canonical(st.subs[1])
    st._fuse_pair(1, 0)
    assert st.subs[0].size == old.size and st.subs[1].size == new.size
    _, io, jn = np.intersect1d(ko, kn, return_indices=True)
    with np.errstate(invalid="ignore"):
        gate = (old["var"][io] > 0) & (old["var"][io] < 1)
    shut = old["var"][io][~gate]
    assert (shut == 0).any() and (shut == 1).any() and (shut < 0).any() and np.isnan(shut).any()
    assert R.same(st.subs[0][io[~gate]], old[io[~gate]]) and R.same(st.subs[1][jn[~gate]], new[jn[~gate]])
    a, b = st.subs[0][io[gate]], st.subs[1][jn[gate]]
    assert gate.sum() > 50 and R.same(a, b) and st.matched == gate.sum()
    for f in ("r", "g", "b", "intensity", "travers"):
        assert np.array_equal(a[f], new[f][jn[gate]])
    want = (old["frontier"][io[gate]] != 0) & (new["frontier"][jn[gate]] != 0)
    assert np.array_equal(a["frontier"], want.astype(np.int32)) and want.any() and not want.all()
    assert (old["frontier"] == 2).any()


def test_cases_keep_their_margin():
    m = GC.MARGIN
    for name, sc in GC.scenes().items():
        st, calls = GC.build(name, R.Vectorised)
        r2 = float(st.radius) ** 2
        C = np.array(st.centres, np.float64)
        d2 = ((C[:, None] - C[None]) ** 2).sum(-1)
        assert (np.abs(d2 - r2) > m * r2).all(), name
        for opt in calls:
            st.update_global(opt)
            for s in st.subs:
                v = s["var"][np.isfinite(s["var"])].astype(np.float64)
                v = v[(v != 0) & (v != 1)]
                assert (np.abs(v - 1) > m).all(), name                                  # gate inputs of a later pair or call (0: see gem_cases)
                assert (np.abs(s["z"][np.isfinite(s["z"])] + 10) > m * 10).all(), name
    for name, (cloud, origin, size, res, kw) in GC.costmap_cases().items():
        t = kw.get("travers_thresh", kw.get("z_thresh"))
        v = cloud["travers" if "travers_thresh" in kw else "z"].astype(np.float64)
        assert (np.abs(v - t) > m * max(abs(t), 1)).all(), name


@pytest.mark.parametrize("res", [0.05, 0.1, 0.2, 0.3])
def test_snapped_positions_rekey_to_themselves(res):
    """every key |k| < 2^23: ceil((double)(float)(k res - res / 2) / res) == k"""
    for lo in range(-R.KEY_BOUND + 1, R.KEY_BOUND, 1 << 22):
        k = np.arange(lo, min(lo + (1 << 22), R.KEY_BOUND), dtype=np.int64)
        snapped = (k.astype(np.float64) * res - res / 2.0).astype(F)
        assert np.array_equal(np.ceil(snapped.astype(np.float64) / res).astype(np.int64), k)
    assert R.key_of(R.centre_of(R.KEY_BOUND - 1, res), res) == R.KEY_BOUND - 1
    assert R.key_of(F(R.KEY_BOUND * res * 1.01), res) is None and R.key_of(F(np.nan), res) is None and R.key_of(F(-np.inf), res) is None


def _robot_stores(make):
    scripts, poses, local_maps, refs = GC.robots()
    stores = [GC.run(make(), s) for s in scripts]
    for st, p in zip(stores, poses):
        st.update_global(p)
    return stores, poses, local_maps, refs


@pytest.mark.parametrize("merge, rule", [(False, R.WEIGHTED), (True, R.WEIGHTED), (True, R.AS_WRITTEN)])
def test_compose_robots_literal_equals_vectorised(merge, rule):
    sa, poses, local_maps, refs = _robot_stores(R.Literal)
    sb = _robot_stores(R.Vectorised)[0]
    a, da = R.compose_robots_literal(sa, poses, local_maps, refs, merge, rule, GC.RES)
    b, db = R.compose_robots_vec(sb, poses, local_maps, refs, merge, rule, GC.RES)
    assert R.same(a, b) and da == db
    total = sum(s.compose().size for s in sa) + sum(m.size for m in local_maps)
    if not merge:
        assert a.size == total and da == 0
        assert R.same(a[-local_maps[1].size:], R._move_vec(local_maps[1], refs[1]))     # the local maps come last, in robot order
    else:
        p = R._pack(*R._keys_vec(a, GC.RES)[1:])
        assert da == 4 and a.size < total / 2 and (np.diff(p) > 0).all()                # one record per key, in key order


@pytest.mark.parametrize("name", sorted(GC.costmap_cases()))
def test_costmap_literal_equals_vectorised(name):
    cloud, origin, size, res, kw = GC.costmap_cases()[name]
    a, b = R.costmap_literal(cloud, origin, size, res, **kw), R.costmap_vec(cloud, origin, size, res, **kw)
    assert a.dtype == np.uint8 and a.shape == (size[1], size[0]) and np.array_equal(a, b)
    if name != "empty":
        assert a[0, 0] in (0, 254) and a[-1, -1] in (0, 254)                            # the points on the lower borders and just inside the upper
    if size == (130, 3):
        assert {0, 254, 255} <= set(a.reshape(-1).tolist())


def test_costmap_last_point_wins():
    cloud, origin, size, res, kw = GC.costmap_cases()["travers_130x3"]
    g = R.costmap_literal(cloud, origin, size, res, **kw)
    mx, my = int((float(cloud["x"][20]) - origin[0]) / res), int((float(cloud["y"][20]) - origin[1]) / res)
    in_cell = [n for n in range(cloud.size) if R.costmap_literal(cloud[n:n + 1], origin, size, res, **kw)[my, mx] != 255]
    assert len(in_cell) >= 70 and g[my, mx] == R.cell_cost(cloud["z"][in_cell[-1]], cloud["travers"][in_cell[-1]], 0.5, None)
    costs = {R.cell_cost(cloud["z"][n], cloud["travers"][n], 0.5, None) for n in in_cell}
    assert costs == {0, 254}


def test_abi_declares_and_binds_the_gem_family():
    protos = _lib.parse_header(_lib.HEADER)
    want = {"mrs_gem_" + n for n in ("create", "destroy", "append_cells", "append_leaving", "close_submap", "count", "get_submap", "update_global",
                                     "stats", "compose", "compose_robots", "costmap")}
    assert want <= set(protos)
    assert gem.CELL == R.CELL and gem.CELL.itemsize == 40
    assert (gem.WEIGHTED, gem.AS_WRITTEN) == (R.WEIGHTED, R.AS_WRITTEN)
    src = open(_lib.HEADER).read()
    assert "#define MRS_GEM_WEIGHTED 0" in src and "#define MRS_GEM_AS_WRITTEN 1" in src
    with pytest.raises(ValueError):
        gem.costmap(np.zeros(0, gem.CELL), (0, 0), (1, 1), 1.0)
    with pytest.raises(ValueError):
        gem._cells(np.zeros((3, 9), np.float32))


def test_cell_arithmetic_header_under_sanitizers(tmp_path):
    """gem_cell.hpp compiled for the host with -fsanitize=address,undefined, run stand-alone, against the restatement"""
    exe = os.path.join(ROOT, "tests", "cpp", "build", "gem_cell_test")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-static-libasan", "-static-libubsan",
                        os.path.join(ROOT, "tests", "cpp", "gem_cell_main.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    rng = np.random.default_rng(7)
    quad = rng.uniform(-2, 2, (300, 4)).astype(F)
    quad[:6, 1] = [0, 1, -0.5, np.nan, 1e-30, 1e30]
    quad[6:9, 3] = [0, np.nan, np.inf]
    coord = np.concatenate([rng.uniform(-50, 50, 500), [0.0, -0.0, 0.2, -0.2, 0.4, 1.0, np.nan, np.inf, -np.inf, 3e6, -3e6, 1677721.5, -1677721.75,
                                                             1677721.25, -1677721.5]]).astype(F)
    opt, pose = GC.pose(0.31, 4.0, -2.5, 0.2), GC.pose(0.3, 4.1, -2.4, 0.1)
    w = GC.window_cells()
    win = np.concatenate([np.stack([w["x"], w["y"], w["z"], np.full(36, 0.25, F), np.full(36, -0.5, F), np.full(36, s[0], F), np.full(36, s[1], F)], 1)
                          for s in GC.SHIFTS]).astype(F)
    half = F(10) * F(0.2) / F(2)
    # costmap points: random ones around a 13 x 7 grid, each border and the value next to it on either side, NaN, +-inf and huge coordinates
    origin, csize, cres, tt, zt = (-1.5, 2.0), (13, 7), 0.25, 0.5, 0.75
    edge = lambda v: [np.nextafter(F(v), F(-np.inf)), F(v), np.nextafter(F(v), F(np.inf))]
    special = [*edge(-1.5), *edge(1.75), *edge(2.0), *edge(3.75), np.nan, np.inf, -np.inf, 3e38, -3e38, 1e30, -1e30, 2.2e9, 4.4e9, 0.0, -0.0]
    pts = R.cells(400 + len(special) ** 2)
    pts["x"][:400], pts["y"][:400] = rng.uniform(-2.5, 2.75, 400), rng.uniform(1.0, 4.75, 400)
    pts["x"][400:], pts["y"][400:] = np.repeat(np.array(special, F), len(special)), np.tile(np.array(special, F), len(special))
    pts["z"] = rng.choice(np.array([-10, 10, 0.75, 0.5, 1.0, np.nan, np.inf], F), pts.size)
    pts["travers"] = rng.choice(np.array([-10, 0.5, 0.25, 0.75, np.nan, -np.inf], F), pts.size)
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(fin, "wb") as f:
        np.array([quad.shape[0], coord.size, win.shape[0], pts.size], np.int32).tofile(f)
        quad.tofile(f); coord.tofile(f); np.array([GC.RES]).tofile(f); opt.tofile(f); pose.tofile(f); win.tofile(f); np.array([half], F).tofile(f)
        np.stack([pts["x"], pts["y"], pts["z"], pts["travers"]], 1).astype(F).tofile(f)
        np.array([*origin, cres, tt, zt], np.float64).tofile(f); np.array(csize, np.int32).tofile(f)
    r = subprocess.run([exe, str(fin), str(fout)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stdout + r.stderr
    with open(fout, "rb") as f:
        fused = np.fromfile(f, np.uint32, quad.shape[0] * 4).reshape(-1, 4)
        key = np.fromfile(f, np.int32, coord.size * 2).reshape(-1, 2)
        centre = np.fromfile(f, np.uint32, coord.size)
        T = np.fromfile(f, np.uint32, 16)
        verdict = np.fromfile(f, np.int32, win.shape[0])
        cost = np.fromfile(f, np.int32, pts.size * 5).reshape(-1, 5)
        moved = np.fromfile(f, np.uint32, pts.size * 3).reshape(-1, 3)
        packed = np.fromfile(f, np.uint64, coord.size)
        assert f.read() == b""
    want = np.array([[*R.fuse_zvar(R.WEIGHTED, *q), *R.fuse_zvar(R.AS_WRITTEN, *q)] for q in quad], F)
    assert np.array_equal(fused, want.view(np.uint32))
    vz, vv = R._fuse_vec(R.WEIGHTED, *quad.T)
    assert np.array_equal(fused[:, 0], vz.view(np.uint32)) and np.array_equal(fused[:, 1], vv.view(np.uint32))
    ks = [R.key_of(v, GC.RES) for v in coord]
    assert key[:, 0].tolist() == [int(k is not None) for k in ks]
    assert [int(k) for k, ok in zip(key[:, 1], key[:, 0]) if ok] == [k for k in ks if k is not None]
    assert key[:, 0].sum() == coord.size - 7                                            # NaN, +-inf, +-3e6 and k = +-2^23; k = +-(2^23 - 1) are keyed
    assert min(k for k in ks if k is not None) == 1 - R.KEY_BOUND and max(k for k in ks if k is not None) == R.KEY_BOUND - 1
    want_c = np.array([R.centre_of(k, GC.RES) if k is not None else F(0) for k in ks], F)
    assert np.array_equal(centre, want_c.view(np.uint32))
    assert np.array_equal(T, R._correction_literal(opt, pose).view(np.uint32).reshape(-1))
    assert np.array_equal(T, R._correction_vec(opt, pose).view(np.uint32).reshape(-1))
    want_v = [int(R.leaves_window(*row, 10, 0.2)) for row in win]
    assert verdict.tolist() == want_v and 0 < sum(want_v) < len(want_v)
    # world_to_map and cell_cost against costmap_literal, one point at a time; the cost functions on every point, placed or not
    n_in = 0
    for n in range(pts.size):
        gt, gz = (R.costmap_literal(pts[n:n + 1], origin, csize, cres, **kw) for kw in (dict(travers_thresh=tt), dict(z_thresh=zt)))
        hit = np.argwhere(gt != 255)
        assert np.array_equal(hit, np.argwhere(gz != 255)) and len(hit) == cost[n, 0], n
        if len(hit):
            (my, mx), n_in = hit[0], n_in + 1
            assert (cost[n, 1], cost[n, 2]) == (mx, my) and (cost[n, 3], cost[n, 4]) == (gt[my, mx], gz[my, mx]), n
        assert (cost[n, 3], cost[n, 4]) == (R.cell_cost(pts["z"][n], pts["travers"][n], tt, None), R.cell_cost(pts["z"][n], pts["travers"][n], None, zt)), n
    assert 100 < n_in < pts.size - 100 and {0, 254} == set(cost[:, 3].tolist()) == set(cost[:, 4].tolist())
    assert set(cost[cost[:, 0] == 1, 1].tolist()) == set(range(13)) and set(cost[cost[:, 0] == 1, 2].tolist()) == set(range(7))
    mv = R._move_literal(pts, R._correction_literal(opt, pose))
    assert np.array_equal(moved, np.stack([mv["x"], mv["y"], mv["z"]], 1).view(np.uint32))
    nxt = ks[1:] + ks[:1]
    assert packed.tolist() == [int(R._pack(a, b)) if a is not None and b is not None else 0 for a, b in zip(ks, nxt)]
