"""CPU suite: the elevation-mapping restatement (oracle/elev_oracle.cpp, the checker of row N3) pinned to the reference's
own source: Mapping/src/elevation_mapping_periodical/elevation_mapping/cuda/gpu_process.cu compiled for the host by
oracle/Makefile (threads in gid order, stand-ins for the CUDA runtime and the few Eigen operations it uses)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from elev_session import session  # noqa: E402


@pytest.mark.parametrize("L", [60, 61])
def test_restatement_equals_the_reference_source_run_on_the_host(oracle, L):
    if oracle.ref_lib("elev") is None:
        pytest.skip("oracle/_ref/libref_elev.so not built (no reference tree at build time)")
    want = session(oracle.RefElevMap(L, 0.2), np.random.default_rng(3), 5, L)
    got = session(oracle.ElevMap(L, 0.2), np.random.default_rng(3), 5, L)
    assert len(got) == len(want)
    worst = {}
    for (kg, g), (kw, w) in zip(got, want):
        assert kg == kw
        if kg in ("move", "frame"):
            for a, b in zip(g, w):
                np.testing.assert_array_equal(a, b)
        elif kg == "optmove":
            np.testing.assert_array_equal(g, w)
        elif kg == "points":
            for k in ("map_index", "x", "y", "z", "x_ts", "y_ts", "z_ts"):
                np.testing.assert_array_equal(g[k], w[k])
            assert (g["map_index"] >= 0).sum() > 500
            np.testing.assert_allclose(g["var"], w["var"], rtol=1e-6, atol=1e-12)
            worst["var"] = max(worst.get("var", 0), float(np.abs(g["var"] - w["var"]).max()))
        elif kg == "feature":
            for k in ("colorR", "colorG", "colorB"):
                np.testing.assert_array_equal(g[k], w[k])
            for k in ("elevation", "var", "intensity"):
                np.testing.assert_allclose(g[k], w[k], rtol=2e-6, atol=2e-6, err_msg=k)
                worst[k] = max(worst.get(k, 0), float(np.abs(g[k] - w[k]).max()))
            seen = w["elevation"] != -10      # empty cells: the reference returns before writing rough / slope / traver, its
            assert seen.sum() > 300           # output there is whatever cudaMalloc handed out (gpu_process.cu:577-578,1267-1269)
            for k in ("rough", "slope", "traver"):
                np.testing.assert_allclose(g[k][seen], w[k][seen], rtol=2e-6, atol=2e-6, err_msg=k)
                worst[k] = max(worst.get(k, 0), float(np.abs(g[k][seen] - w[k][seen]).max()))
        else:
            for i, (a, b) in enumerate(zip(g, w)):
                np.testing.assert_allclose(a, b, rtol=2e-6, atol=2e-6, err_msg=f"layer {i}")
    print("largest differences:", worst)


# ---- the stage scenarios of tests/elev_cases.py: the restatement against the reference source on the regimes the GPU stage tests
# ---- (tests/test_elevation_stages_gpu.py) rely on it for.  The reference keeps one map per process: one scenario after another.
import elev_cases as EC  # noqa: E402


def _ref(oracle, L, res):
    if oracle.ref_lib("elev") is None:
        pytest.skip("oracle/_ref/libref_elev.so not built (no reference tree at build time)")
    return oracle.RefElevMap(L, res)


def _same(got, want, worst, seen=None):
    """outputs of one run on the restatement and on the reference: integers, frames and fuse-only layers bit-exact, everything
    that went through libm (var: powf; slope / traver: the Jacobi sweep) at the 2e-6 this file uses; records the differences"""
    for (kg, g), (kw, w) in zip(got, want):
        assert kg == kw
        if kg == "move":
            for a, b in zip(g, w):
                np.testing.assert_array_equal(a, b, err_msg=kg)
        elif kg == "layers" or kg.endswith(".lowest"):
            for name, a, b in zip(EC.LAYERS, g, w) if kg == "layers" else [("lowest", g, w)]:
                if name == "traver":
                    np.testing.assert_allclose(a, b, rtol=2e-6, atol=2e-6, err_msg=name)
                else:
                    np.testing.assert_array_equal(a, b, err_msg=kg + " " + name)
                worst[name] = max(worst.get(name, 0), float(np.abs(a - b).max()))
        elif kg == "feature":
            filled = w["elevation"] != -10     # elsewhere the reference's rough / slope / traver are uninitialised
            for k in ("elevation", "var", "intensity", "colorR", "colorG", "colorB"):
                np.testing.assert_array_equal(g[k], w[k], err_msg=k)
            for k in ("rough", "slope", "traver"):
                np.testing.assert_allclose(g[k][filled], w[k][filled], rtol=2e-6, atol=2e-6, err_msg=k)
                worst[k] = max(worst.get(k, 0), float(np.abs(g[k][filled] - w[k][filled]).max(initial=0)))
        else:                                   # a Process_points call
            for k in ("map_index", "x", "y", "z", "x_ts", "y_ts", "z_ts"):
                np.testing.assert_array_equal(g[k], w[k], err_msg=kg + " " + k)
            np.testing.assert_allclose(g["var"], w["var"], rtol=1e-6, atol=1e-12)
            worst["var"] = max(worst.get("var", 0), float(np.abs(g["var"] - w["var"]).max()))


@pytest.mark.parametrize("L", [8, 9])
def test_move_cases_equal_the_reference_where_it_is_defined(oracle, L):
    """every single-axis shift the reference can run (|shift| < L of either sign, and shift >= L: its clear-all), plus the
    survivors rule, which needs no Move code at all; the shifts <= -L (undefined in the reference) must empty the map"""
    worst = {}
    for axis in (0, 1):
        for cells in EC.move_shifts(L):
            got = EC.run_move_single(oracle.ElevMap(L, EC.MOVE_RES), L, axis, cells)
            (c, s, a), lay = got[0][1], got[1][1]
            d = [0, 0]
            d[axis] = cells
            np.testing.assert_array_equal(a, np.array(d, np.float32) * EC.MOVE_RES)
            np.testing.assert_array_equal(s, (-np.array(d)) % L)
            if abs(cells) < L:
                np.testing.assert_array_equal(lay[1], EC.survivors(L, EC.planted(L)[5], (0, 0), d, s))
                assert ((lay[4] != -10) == (EC.planted(L)[5] != -10)).all()      # traver only falls to a clear-all
            else:
                for w in (1, 2, 4):
                    assert (lay[w] == -10).all()
                assert (lay[3] == 0).all() and (lay[0] == 100).all()
            if cells > -L:
                _same(got, EC.run_move_single(_ref(oracle, L, EC.MOVE_RES), L, axis, cells), worst)
    print("L=%d move cases, largest differences restatement - reference:" % L, worst)


@pytest.mark.parametrize("L", [8, 9])
def test_move_walk_equals_the_reference(oracle, L):
    worst = {}
    _same(EC.run_move_walk(oracle.ElevMap(L, EC.MOVE_RES), L, 11), EC.run_move_walk(_ref(oracle, L, EC.MOVE_RES), L, 11), worst)
    print("L=%d move walk, largest differences restatement - reference:" % L, worst)


@pytest.mark.parametrize("far", [False, True])
@pytest.mark.parametrize("L", [60, 61])
def test_points_cases_equal_the_reference(oracle, L, far):
    calls = EC.points_calls(oracle, L, far)
    got = EC.run_points(oracle.ElevMap(L, EC.POINTS_RES), far, calls)
    worst = {}
    _same(got, EC.run_points(_ref(oracle, L, EC.POINTS_RES), far, calls), worst)
    out = dict(got)
    assert (out["rejected"]["map_index"] == -1).all() and (out["n1"]["map_index"] >= 0).all()
    assert (out["n6000"]["map_index"] >= 0).sum() > (2000 if far else 500) and (out["n7"]["map_index"] >= 0).any()
    for side in "xy":                                      # the planted borders: inside | outside at both map edges, and every
        mi = out["border_" + side]["map_index"].reshape(-1, 4)     # interior border separates two different cells
        assert mi.shape[0] == L + 1
        assert (mi[:, 0] == mi[:, 1]).all() and (mi[:, 2] == mi[:, 3]).all() and (mi[:, 1] != mi[:, 2]).all()
        assert (mi[0, :2] == -1).all() and (mi[0, 2:] >= 0).all() and (mi[-1, :2] >= 0).all() and (mi[-1, 2:] == -1).all()
        assert (mi[1:-1] >= 0).all()
    for name in ("edge_x0", "edge_x1", "edge_y0", "edge_y1"):
        mi = out[name]["map_index"].reshape(3, L)          # on the edge cells, one cell beyond, two cells beyond
        assert (mi[0] >= 0).all() and len(set(mi[0])) == L and (mi[2] == -1).all()
        if L % 2 == 0 and name.endswith("0"):              # even L truncates towards zero: grid cell 0 is two cells wide
            np.testing.assert_array_equal(mi[1], mi[0])
        else:
            assert (mi[1] == -1).all()
    print("L=%d far=%d points, largest differences restatement - reference:" % (L, far), worst)


def test_fuse_cases_equal_the_reference_and_the_numpy_reading(oracle):
    L = 8
    results = {}
    for name, calls in EC.fuse_call_sets().items():
        want_np = EC.empty_state(L)
        r, m = _ref(oracle, L, 0.5), oracle.ElevMap(L, 0.5)
        counts = []
        for k, call in enumerate(calls):
            r.fuse(*call); m.fuse(*call)
            counts.append(EC.fuse_numpy(L, want_np, call))
            if k == 0 and len(calls) > 1:
                r.mapvar_update(2e-4); m.mapvar_update(2e-4)
                want_np[1][want_np[1] != -10] += np.float32(2e-4)
        got, ref = EC.fused_state(m), EC.fused_state(r)
        for a, b, c in zip(got, ref, want_np):
            np.testing.assert_array_equal(a, b, err_msg=name)
            np.testing.assert_array_equal(a, c, err_msg=name)
        results[name] = (got, counts)
    hi, lo = results["crowded"][1][0]
    assert hi >= 20 and lo >= 20, (hi, lo)                 # both outlier branches, as the issue asks
    assert not np.array_equal(results["crowded"][0][0], results["permuted"][0][0])      # the order of a cell's points matters
    e, v, it, cr, cg, cb = results["hand"][0]
    assert e[63] == -10 and v[63] == np.float32(0.0001) and v[0] == np.float32(0.0001) and cr[0] == 0      # floor reaches empty cells
    assert (cr[19], cg[19], cb[19]) == (12, 22, 32) and it[19] == np.float32(0.7)


@pytest.mark.parametrize("wrapped", [False, True])
@pytest.mark.parametrize("L", [20, 21])
def test_feature_scene_equals_the_reference(oracle, L, wrapped):
    worst = {}
    got = EC.run_features(oracle.ElevMap(L, EC.FEATURE_RES), L, wrapped)
    _same(got, EC.run_features(_ref(oracle, L, EC.FEATURE_RES), L, wrapped), worst)
    f, (_, pn) = got[1][1], EC.feature_scene(L, got[0][1][1])
    assert ((f["traver"] == -10) == (pn <= 7)).all() and (f["traver"][pn == 8] != -10).all() and (pn == 7).any() and (pn == 8).any()
    print("L=%d wrapped=%d feature scene, largest differences restatement - reference:" % (L, wrapped), worst)


def test_plane_slopes_of_the_reference_against_float64(oracle):
    """What the float Jacobi sweep (it stops at an off-diagonal of 0.01) costs on tilted planes: the reference host build's
    worst deviation from the float64 eigen-decomposition of the same 5 x 5 patches, and from atan(hypot(a, b)).  The GPU test
    allows twice the former."""
    L, worst, worst_exact = 21, 0.0, 0.0
    for tilt, direction in EC.PLANE_TILTS:
        f = EC.run_plane(_ref(oracle, L, EC.FEATURE_RES), L, tilt, direction)
        g = EC.run_plane(oracle.ElevMap(L, EC.FEATURE_RES), L, tilt, direction)
        want = EC.plane_slopes_f64(L, f["elevation"])
        assert np.abs(want - tilt).max() < 1e-5          # the float64 answer is the plane's tilt
        worst = max(worst, float(np.abs(EC.interior(L, f["slope"]) - want).max()))
        worst_exact = max(worst_exact, float(np.abs(EC.interior(L, f["slope"]) - tilt).max()))
        np.testing.assert_allclose(g["slope"], f["slope"], rtol=2e-6, atol=2e-6)
    print("plane slopes, reference host build: worst |slope - float64 eigen| = %.3e, worst |slope - tilt| = %.3e" % (worst, worst_exact))
    assert worst <= EC.PLANE_SLOPE_REF_DEVIATION


@pytest.mark.parametrize("start", list(EC.RAY_STARTS))
@pytest.mark.parametrize("L", [20, 21])
def test_ray_scene_equals_the_reference_and_is_not_vacuous(oracle, L, start):
    m = oracle.ElevMap(L, EC.RAY_RES)
    before, after, cells, frame = EC.run_ray(m, L, start)
    rb, ra, _, rframe = EC.run_ray(_ref(oracle, L, EC.RAY_RES), L, start)
    for a, b in zip(frame, rframe):
        np.testing.assert_array_equal(a, b)
    for name, a, b, c, d in zip(EC.LAYERS, before, rb, after, ra):
        if name == "traver":
            np.testing.assert_allclose(a, b, rtol=2e-6, atol=2e-6)
        else:
            np.testing.assert_array_equal(a, b, err_msg=name)
            np.testing.assert_array_equal(c, d, err_msg=name + " after")
    obstacle, cleared = EC.ray_outcome(before, after)
    assert (after[0] == 10).all()
    assert cleared.sum() >= 10 and (obstacle & ~cleared).sum() >= 10, (cleared.sum(), obstacle.sum())
    margin = m.raytracing_margin()
    assert margin[np.isfinite(margin)].min() >= 1e-5       # no decision of the scene is a near tie: nothing to exclude
    idx = lambda cs: EC.storage_index(L, frame[1], *np.array(cs).T)
    assert cleared[idx(cells["diagonal"])].all() and cleared[idx(cells["quadrant"])].sum() >= 8
    assert obstacle[idx(cells["axis"])].all() and not cleared[idx(cells["axis"])].any()      # the early return on the robot's row / column
    assert obstacle[idx(cells["wall"])].all() and not cleared[idx(cells["wall"])].any()
    print("L=%d %s: %d obstacle cells, %d cleared, smallest margin %.3g" % (L, start, obstacle.sum(), cleared.sum(), margin[np.isfinite(margin)].min()))


def test_move_jumps_past_the_map_are_clean_under_the_sanitizers(tmp_path):
    """tests/cpp/elev_move_main.cpp (stand-alone, its own main) drives the restatement's Move through +-L, +-(L+1), +-(2L+3) and
    -50 L under AddressSanitizer + UBSan.  With the reference's one-sided `shift >= L` test the negative jumps overflow the heap
    (clear_region writes L * |shift| cells); with |shift| >= L they clear the map."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "elev_move")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fno-fast-math", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", os.path.join(root, "tests", "cpp", "elev_move_main.cpp"),
           os.path.join(root, "oracle", "elev_oracle.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "all jumps clear the map" in r.stdout and "Sanitizer" not in r.stderr, r.stdout[-800:] + r.stderr[-2000:]
