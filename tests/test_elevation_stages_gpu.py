"""GPU: every stage of the elevation map (row N3) on its own.  Each test brings a map on the GPU to a state, reads that state back
(mrs_elev_get_layer / mrs_elev_get_frame), loads it into a fresh sequential restatement (oracle/elev_oracle.cpp,
orc_elev_set / orc_elev_set_frame), runs ONE stage on both and compares: both sides start from identical inputs, so whatever is
made of + - * / sqrt only is compared bit for bit.  Scenarios: tests/elev_cases.py; tests/test_oracle_elev.py pins the restatement
to the reference source on the same scenarios."""
import numpy as np
import pytest

import elev_cases as EC

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def elevation():
    import torch
    assert torch.cuda.is_available()
    from mr_slam_amd import _lib, elevation
    _lib.load()
    return elevation


def mirror(oracle, g, res, sensor_z, colours=None):
    """a fresh restatement holding the state of the GPU map g (colours from a map_feature() result of g, if given)"""
    r = oracle.ElevMap(g.L, res)
    for w in range(5):
        r.set(w, g.layer(w))
    for w, k in enumerate(("colorR", "colorG", "colorB")):
        if colours is not None:
            r.set(5 + w, colours[k])
    r.set_frame(*g.frame(), sensor_z)
    return r


def same_layers(g, r, what=""):
    for name, a, b in zip(EC.LAYERS, EC.layers(g), EC.layers(r)):
        np.testing.assert_array_equal(a, b, err_msg="%s %s" % (what, name))


def same_move(got, want, what=""):
    for name, a, b in zip(("central", "start", "aligned_shift"), got, want):
        np.testing.assert_array_equal(a, b, err_msg="%s %s" % (what, name))


# ------------------------------------------------------------------------------------------------ Move
@pytest.mark.parametrize("L", [8, 9])
def test_move_single_axis_shifts(elevation, oracle, L):
    """+-1, +-(L-1) keep what stays in the window; +-L, +-(L+1), +-(2L+3) and -50 L clear everything (traver too), whatever the
    sign: the reference is undefined for the negative ones"""
    heights = EC.planted(L)[5]
    for axis in (0, 1):
        for cells in EC.move_shifts(L):
            what = "L=%d axis=%d shift=%d" % (L, axis, cells)
            g = elevation.ElevationMap(L, EC.MOVE_RES)
            g.move([0, 0, 1.0])
            EC.fill_all(g, L)
            r = mirror(oracle, g, EC.MOVE_RES, 1.0, g.map_feature())       # after map_feature: traver is set in every cell
            np.testing.assert_array_equal(g.layer(1), heights)
            assert (g.layer(4) != -10).all()
            pos = [0.0, 0.0, 1.25]
            pos[axis] = EC.MOVE_RES * cells
            got = g.move(pos)
            same_move(got, r.move(pos), what)
            same_layers(g, r, what)
            d = [0, 0]
            d[axis] = cells
            np.testing.assert_array_equal(got[1], (-np.array(d)) % L, err_msg=what)
            if abs(cells) < L:
                np.testing.assert_array_equal(g.layer(1), EC.survivors(L, heights, (0, 0), d, got[1]), err_msg=what)
                assert (g.layer(4) != -10).all()
            else:
                assert (g.layer(1) == -10).all() and (g.layer(2) == -10).all() and (g.layer(4) == -10).all() and (g.layer(3) == 0).all()
            fg, fr = g.map_feature(), r.map_feature()
            for k in ("colorR", "colorG", "colorB", "elevation", "var", "intensity"):
                np.testing.assert_array_equal(fg[k], fr[k], err_msg=what + " " + k)


@pytest.mark.parametrize("L", [8, 9])
def test_move_random_walk_wraps_start(elevation, oracle, L):
    g = elevation.ElevationMap(L, EC.MOVE_RES)
    c, start = g.frame()
    model = np.full(L * L, -10, F)                  # the heights planted so far, carried along by the survivors rule alone
    for step, d in enumerate(EC.walk_shifts(L, 11)):
        p, sel = EC.refill_empty(g, L, g.layer(1), step)
        np.testing.assert_array_equal(sel, model == -10)
        model[sel] = p[5][sel]
        np.testing.assert_array_equal(g.layer(1), model)
        r = mirror(oracle, g, EC.MOVE_RES, 1.0 + 0.01 * (step - 1), g.map_feature())
        c = np.asarray(c, np.float64) + d * EC.MOVE_RES
        pos = [c[0], c[1], 1.0 + 0.01 * step]
        got = g.move(pos)
        same_move(got, r.move(pos), "step %d" % step)
        same_layers(g, r, "step %d" % step)
        np.testing.assert_array_equal(got[2], (d * EC.MOVE_RES).astype(F))
        model = EC.survivors(L, model, start, d, got[1])
        np.testing.assert_array_equal(g.layer(1), model, err_msg="step %d" % step)
        c, start = got[0], got[1]


def test_move_rejects_positions_it_cannot_turn_into_a_shift(elevation, oracle):
    from mr_slam_amd import _lib
    L = 9
    g = elevation.ElevationMap(L, EC.MOVE_RES)
    g.move([1.0, -0.5, 1.0])
    EC.fill_all(g, L)
    frame, elev = g.frame(), g.layer(1)
    edge = float(2 ** 30) * EC.MOVE_RES              # 2^30 cells from the centre (1, -0.5), to float precision
    bad = [(np.nan, 0, 1), (0, np.nan, 1), (np.inf, 0, 1), (0, -np.inf, 1), (1e12, 0, 1), (0, -1e12, 1), (edge, 0, 1)]
    calls = [(g.move, p) for p in bad + [(0, 0, np.nan), (0, 0, np.inf)]]
    calls += [(lambda p: g.map_optmove(p, 0.5), p[:2]) for p in bad] + [(lambda p: g.map_closeloop(p, 0.5), p[:2]) for p in bad]
    for fn, p in calls:
        with pytest.raises(_lib.MrsError) as e:
            fn(p)
        assert e.value.status == 1                  # MRS_ERR_ARG
        for a, b in zip(g.frame(), frame):
            np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(g.layer(1), elev)
    r = mirror(oracle, g, EC.MOVE_RES, 1.0)
    near = [1.0 - (2 ** 30 - 128) * EC.MOVE_RES, -0.5, 2.0]      # just inside the limit: accepted, clears the map
    same_move(g.move(near), r.move(near))
    same_layers(g, r)
    assert (g.layer(1) == -10).all()
    g.raytracing(); r.raytracing()                   # sensor_z was not touched by the rejected calls (nothing to see on an empty map,
    same_layers(g, r)                                # but the launch must be sound)


# ------------------------------------------------------------------------------------------------ Process_points
_points = {}


def points_calls(oracle, L, far):
    if (L, far) not in _points:
        _points[L, far] = EC.points_calls(oracle, L, far)
    return _points[L, far]


@pytest.mark.parametrize("far", [False, True])
@pytest.mark.parametrize("L", [60, 61])
def test_points_calls(elevation, oracle, L, far):
    """n = 1, 255, 256, 257, 6000, then 7 (stale sort keys), all points rejected, points on the edge cells and beyond, points one
    float either side of every cell border; map at the origin and near (-1234.6, 987.4) with a wrapped start"""
    g = elevation.ElevationMap(L, EC.POINTS_RES)
    EC.points_setup(g, far)
    worst = 0.0
    for name, xs, ys, zs, T in points_calls(oracle, L, far):
        r = mirror(oracle, g, EC.POINTS_RES, 0.9)
        got, want = EC.process(g, xs, ys, zs, T), EC.process(r, xs, ys, zs, T)
        for k in ("map_index", "x", "y", "z", "x_ts", "y_ts", "z_ts"):
            np.testing.assert_array_equal(got[k], want[k], err_msg=name + " " + k)
        worst = max(worst, float(np.abs(got["var"] - want["var"]).max()))
        print("L=%d far=%d %s: %d of %d points on the map, max |var - restatement| = %.3g" % (
            L, far, name, (got["map_index"] >= 0).sum(), xs.size, np.abs(got["var"] - want["var"]).max()))
        np.testing.assert_array_equal(got["var"], want["var"], err_msg=name + " var")
        np.testing.assert_array_equal(g.layer(0), r.layer(0), err_msg=name + " lowest")
    assert (g.layer(0) != 100).sum() > 1000


# ------------------------------------------------------------------------------------------------ Fuse
@pytest.mark.parametrize("name", list(EC.fuse_call_sets()))
def test_fuse_cases(elevation, oracle, name):
    """hand-made branch walk, 3000 points in one cell, the same permuted, n = 1, a second call on a fused map: against the
    restatement (state copied from the GPU before every call) and against the sequential float32 numpy reading, bit for bit"""
    L = 8
    g = elevation.ElevationMap(L, 0.5)
    for k, call in enumerate(EC.fuse_call_sets()[name]):
        state = EC.fused_state(g)
        r = mirror(oracle, g, 0.5, 0.0, dict(zip(("colorR", "colorG", "colorB"), state[3:])))
        g.fuse(*call); r.fuse(*call)
        hi, lo = EC.fuse_numpy(L, state, call)
        for what, a, b, c in zip(("elevation", "variance", "intensity", "R", "G", "B"), EC.fused_state(g), EC.fused_state(r), state):
            np.testing.assert_array_equal(a, b, err_msg="%s call %d %s (restatement)" % (name, k, what))
            np.testing.assert_array_equal(a, c, err_msg="%s call %d %s (numpy reading)" % (name, k, what))
        if name == "crowded":
            assert hi >= 20 and lo >= 20, (hi, lo)
        seen = state[0] != -10
        g.mapvar_update(2e-4); r.mapvar_update(2e-4)
        np.testing.assert_array_equal(g.layer(2), r.layer(2))
        np.testing.assert_array_equal(g.layer(2), state[1] + F(2e-4))         # every cell: the floor has lifted the never-seen ones to 1e-4
        if k == 0:
            assert (g.layer(2)[~seen] == F(0.0001) + F(2e-4)).all() and (~seen).any()


def test_fuse_keeps_the_order_of_a_cells_points(elevation):
    """permuting the 3000 points of the crowded cell changes the result (the numpy reading says so), on the GPU too"""
    L, sets = 8, EC.fuse_call_sets()
    a, b = EC.empty_state(L), EC.empty_state(L)
    EC.fuse_numpy(L, a, sets["crowded"][0]); EC.fuse_numpy(L, b, sets["permuted"][0])
    assert a[0][27] != b[0][27]
    ga, gb = elevation.ElevationMap(L, 0.5), elevation.ElevationMap(L, 0.5)
    ga.fuse(*sets["crowded"][0]); gb.fuse(*sets["permuted"][0])
    assert ga.layer(1)[27] == a[0][27] and gb.layer(1)[27] == b[0][27]


# ------------------------------------------------------------------------------------------------ Map_feature
@pytest.mark.parametrize("wrapped", [False, True])
@pytest.mark.parametrize("L", [20, 21])
def test_feature_scene(elevation, oracle, L, wrapped):
    """terrain cut by three map edges, isolated patches of exactly 7 and exactly 8 cells, start zero and wrapped; the restatement
    holds the GPU's fused state.  Copies and rough bit-exact; slope / traver under the rule of tests/test_elevation_gpu.py
    (|slope difference| < 2e-3 for more than 99.5 % of the cells, traver within 5e-3 there): the Jacobi sweep goes through
    sinf / cosf / atan2f / acosf, which device and host libm round differently."""
    g, r0 = elevation.ElevationMap(L, EC.FEATURE_RES), oracle.ElevMap(L, EC.FEATURE_RES)
    pos = [3 * EC.FEATURE_RES, -6 * EC.FEATURE_RES, 1.0] if wrapped else [0.0, 0.0, 1.0]
    mv = g.move(pos)
    same_move(mv, r0.move(pos))
    assert wrapped == bool(mv[1].any())
    call, pn = EC.feature_scene(L, mv[1])
    g.fuse(*call); r0.fuse(*call)                    # the restatement fuses too: its colours are its own ...
    g.mapvar_update(1e-4)
    for w in range(5):                               # ... and its float layers are the GPU's
        r0.set(w, g.layer(w))
    fg, fr = g.map_feature(), r0.map_feature()
    for k in ("elevation", "var", "intensity", "colorR", "colorG", "colorB", "rough"):
        np.testing.assert_array_equal(fg[k], fr[k], err_msg=k)
    assert ((fg["traver"] == -10) == (pn <= 7)).all() and (pn == 7).sum() >= 14 and (pn == 8).sum() >= 8
    assert (fg["slope"][pn <= 7] == 0).all() and (fg["rough"][pn <= 7] == 0).all()
    ok = np.abs(fg["slope"] - fr["slope"]) < 2e-3
    print("L=%d wrapped=%d: max slope difference %.3g, max traver difference %.3g" % (
        L, wrapped, np.abs(fg["slope"] - fr["slope"]).max(), np.abs(fg["traver"] - fr["traver"]).max()))
    assert ok.mean() > 0.995
    np.testing.assert_allclose(fg["traver"][ok], fr["traver"][ok], rtol=0, atol=5e-3)
    filled = fg["elevation"] != -10
    np.testing.assert_array_equal(g.layer(4)[filled], fg["traver"][filled])          # the traver layer is what was returned
    assert (g.layer(4)[~filled] == -10).all()


def test_plane_slopes_against_float64(elevation):
    """Interior cells of four tilted planes (0, 0.15, 0.3, 0.5 rad), L = 21: slope against the float64 eigen-decomposition of the
    same 5 x 5 patches (= atan(hypot(a, b)) to 1e-5).  The float Jacobi sweep stops at an off-diagonal of 0.01, so this is no ulp
    matter: the reference host build deviates by up to 3.731e-3 rad on these planes (tests/test_oracle_elev.py measures and
    asserts it); the GPU gets twice that, 7.48e-3 rad."""
    L = 21
    for tilt, direction in EC.PLANE_TILTS:
        f = EC.run_plane(elevation.ElevationMap(L, EC.FEATURE_RES), L, tilt, direction)
        want = EC.plane_slopes_f64(L, f["elevation"])
        assert np.abs(want - tilt).max() < 1e-5
        err = np.abs(EC.interior(L, f["slope"]) - want).max()
        print("tilt %.2f: worst |slope - float64| = %.3e" % (tilt, err))
        assert err <= 2 * EC.PLANE_SLOPE_REF_DEVIATION


# ------------------------------------------------------------------------------------------------ Raytracing
@pytest.mark.parametrize("start", list(EC.RAY_STARTS))
@pytest.mark.parametrize("L", [20, 21])
def test_ray_scene(elevation, oracle, L, start):
    """flat ground, a wall, hanging cells in the four quadrants, on the diagonals and on the robot's row / column; the
    restatement holds the GPU's state, so both take every decision on identical numbers.  A cell whose decision margin in the
    restatement is below 1e-5 m may differ (at most 1 % of the obstacle cells); on these scenes the restatement has none
    (tests/test_oracle_elev.py asserts that)."""
    g = elevation.ElevationMap(L, EC.RAY_RES)
    sensor_z, cells, frame = EC.ray_prepare(g, L, start)
    assert (start == "zero") == (not frame[1].any())
    r = mirror(oracle, g, EC.RAY_RES, sensor_z)
    before = EC.layers(g)
    g.raytracing(); r.raytracing()
    after, want = EC.layers(g), EC.layers(r)
    obstacle, cleared = EC.ray_outcome(before, after)
    _, want_cleared = EC.ray_outcome(before, want)
    tie = r.raytracing_margin() < 1e-5
    assert tie.sum() <= 0.01 * obstacle.sum()
    print("L=%d %s: %d obstacle cells, %d cleared (restatement %d), %d near ties" % (L, start, obstacle.sum(), cleared.sum(), want_cleared.sum(), tie.sum()))
    np.testing.assert_array_equal(cleared[~tie], want_cleared[~tie])
    assert cleared.sum() >= 10 and (obstacle & ~cleared).sum() >= 10
    assert (after[0] == 10).all()
    for w in (2, 3, 4):
        np.testing.assert_array_equal(after[w], before[w])
    np.testing.assert_array_equal(after[1][~tie], want[1][~tie])
    idx = lambda cs: EC.storage_index(L, frame[1], *np.array(cs).T)
    assert cleared[idx(cells["diagonal"])].all() and not cleared[idx(cells["axis"])].any() and not cleared[idx(cells["wall"])].any()


# ------------------------------------------------------------------------------------------------ two maps at once
def test_two_maps_do_not_share_state(elevation):
    """L = 20 and L = 61 alive together, their calls interleaved frame by frame: every output equals that of the same map run
    alone (the reference kept its one map in globals; here it lives in the handle)"""
    res = {20: 0.5, 61: 0.2}

    def alone(L):
        m, rng, pose = elevation.ElevationMap(L, res[L]), np.random.default_rng(L), np.array([0, 0, 0.9], F)
        return [EC.small_frame(m, rng, k, pose) for k in range(3)]
    want = {20: alone(20), 61: alone(61)}
    maps = {L: (elevation.ElevationMap(L, res[L]), np.random.default_rng(L), np.array([0, 0, 0.9], F)) for L in (20, 61)}
    got = {20: [], 61: []}
    for k in range(3):
        for L in (20, 61):
            got[L].append(EC.small_frame(*maps[L][:2], k, maps[L][2]))
    for L in (20, 61):
        a, b = EC.flatten(got[L]), EC.flatten(want[L])
        assert len(a) == len(b) and len(a) > 50
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)
        assert (got[L][-1][3][1] != -10).sum() > (100 if L == 20 else 300)


# ------------------------------------------------------------------------------------------------ create / destroy
def test_create_refuses_bad_lengths_and_leaves_no_handle(elevation):
    import ctypes as C
    from mr_slam_amd import _lib
    for length in (0, 8193):
        h = C.c_void_p()
        with pytest.raises(_lib.MrsError) as e:
            _lib.load().mrs_elev_create(_lib.ctx(0), length, 0.5, 2.0, 0.6, C.byref(h))
        assert e.value.status == 1 and not h.value          # MRS_ERR_ARG, no handle


def _small_session(elevation):
    """an 8 x 8 map through move, process_points and fuse with 16 points behind the robot, all of them on the map"""
    L, rng = 8, np.random.default_rng(88)
    m = elevation.ElevationMap(L, 0.5)
    out = [m.move([0.5, -0.5, 0.9])]
    xs, ys, zs = rng.uniform(-1.9, 1.9, 16).astype(F), rng.uniform(-1.95, -1.55, 16).astype(F), rng.uniform(-0.7, -0.5, 16).astype(F)
    assert EC.passes_filter(xs, ys).all()
    res = EC.process(m, xs, ys, zs, EC.transform(0, 0.9, (0.5, -0.5)))
    assert (res["map_index"] >= 0).all()
    m.fuse(res["map_index"], *EC.colours_for(rng, 16), res["z_ts"], res["var"])
    out += [res, EC.layers(m), m.map_feature()]
    assert (out[2][1] != -10).sum() >= 4
    return out


def test_destroy_then_a_fresh_map_reproduces(elevation):
    """the five layers and map_feature of a small session, on a map created after the first one was destroyed: the same bits"""
    first = EC.flatten(_small_session(elevation))           # its map is destroyed when the session returns
    again = EC.flatten(_small_session(elevation))
    assert len(first) == len(again) >= 25
    for a, b in zip(first, again):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
