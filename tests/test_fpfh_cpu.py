"""CPU suite for FPFH: the NumPy restatement (tests/golden/fpfh_restate.py) reproduces what the reference's own get_spfh / describe computed
for the fixture scenes (tests/golden/ref_fpfh.npz), the fixture keeps the margins that make exact comparisons fair, the new C-ABI symbols
are declared, exported and bound, and the drop-in modules are only registered when asked for."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import fpfh_restate as R  # noqa: E402

NAMES = ("mrs_radius_count", "mrs_radius_fill", "mrs_fpfh_spfh", "mrs_fpfh_spfh_from_neighbors", "mrs_fpfh_describe", "mrs_iss_saliency",
         "mrs_iss_nonmax")


@pytest.fixture(scope="module")
def fx():
    return R.load()


def test_fixture_cases(fx):
    scenes, runs = fx
    assert [(r["scene"], r["bins"]) for r in runs] == list(R.RUNS)
    assert sorted(scenes) == ["analytic", "edge", "perturbed", "scaled"]
    for name, s in scenes.items():
        n = len(s["points"])
        assert s["points"].dtype == np.float32 and s["normals"].dtype == np.float32 and s["normals"].shape == (n, 3)
        assert n == (8 if name == "edge" else 600) and len(s["lists"]) == n
        assert all(i in s["lists"][i] for i in range(n))                      # sklearn's lists hold the point itself
    assert os.path.getsize(R.FIXTURE) < 512 * 1024
    # even bin counts only with perturbed normals
    assert all(r["scene"] == "perturbed" for r in runs if r["bins"] % 2 == 0)
    # the scaled scene drops some alpha: the three sums of a point differ somewhere
    c = [r for r in runs if r["scene"] == "scaled"][0]["counts"]
    assert (c[:, :5].sum(1) != c[:, 5:10].sum(1)).any()


def test_fixture_margins(fx):
    """the conditions under which tools/make_fpfh_golden.py accepts a fixture"""
    scenes, runs = fx
    for name, s in scenes.items():
        assert R.radius_margin(s["points"], s["radius"]) > 1e-5, name
        rows = R.radius_rows(s["points"], s["radius"])
        for i, lst in enumerate(s["lists"]):                                  # the lists are the brute-force rows plus the point
            assert sorted(set(lst.tolist()) - {i}) == rows[i].tolist(), (name, i)
    for r in runs:
        s = scenes[r["scene"]]
        _, _, alpha, phi, theta = R.pair_features(s["points"], s["normals"], s["lists"])
        for v, lo, hi in ((alpha, -1.0, 1.0), (phi, -1.0, 1.0), (theta, -np.pi, np.pi)):
            assert R.edge_margin(v, lo, hi, r["bins"]) >= 1e-9, (r["scene"], r["bins"])
    p = scenes["perturbed"]["points"]
    for radius in (R.ISS_SALIENT, R.ISS_NONMAX):
        assert R.radius_margin(p, radius) > 1e-5
    kp, sal, margin = R.iss(p, R.ISS_SALIENT, R.ISS_NONMAX)
    assert margin >= 1e-6 and 0 < len(kp) < len(p) and (sal[kp] > 0).all()


def test_edge_scene_sits_on_the_closed_edges(fx):
    """points 0 and 1 see each other at phi == 1.0 and theta == +-pi exactly"""
    scenes, _ = fx
    s = scenes["edge"]
    I, J, alpha, phi, theta = R.pair_features(s["points"], s["normals"], [np.array([1]), np.array([0])] + [np.zeros(0, np.int64)] * 6)
    assert phi.tolist() == [1.0, 1.0] and np.abs(theta).tolist() == [np.pi, np.pi] and alpha.tolist() == [0.0, 0.0]
    assert R.bin_of(phi, -1.0, 1.0, 5).tolist() == [4, 4]
    assert set(R.bin_of(theta, -np.pi, np.pi, 5).tolist()) <= {0, 4}


def test_restatement_reproduces_reference(fx):
    """SPFH counts exactly and all three thirds of the values bit for bit (alpha and phi carry the reference's bits by construction, theta
    passes through the same libm here); FPFH within the forward-error bound of the unknown summation order of np.dot"""
    scenes, runs = fx
    for r in runs:
        s, B = scenes[r["scene"]], r["bins"]
        tag = (r["scene"], B)
        counts, values = R.spfh(s["points"], s["normals"], s["lists"], B)
        has = r["has"]
        assert has.all() or r["scene"] == "edge", tag
        assert np.array_equal(counts[has], r["counts"][has]), tag
        assert values[has].tobytes() == r["spfh"][has].tobytes(), tag
        rows = [np.unique(l) for l in s["lists"]]                              # ascending, as the contract sums
        got = R.fpfh(s["points"], rows, values, s["keypoints"])
        m = np.array([len(rows[i]) - 1 for i in s["keypoints"]])
        tol = R.fpfh_tolerance(m, B)[:, None]
        assert np.array_equal(got == 0, r["fpfh"] == 0), tag
        assert (np.abs(got - r["fpfh"]) <= tol * np.abs(r["fpfh"])).all(), (tag, np.max(np.abs(got - r["fpfh"]) / np.maximum(np.abs(r["fpfh"]), 1e-300)))


def test_restatement_deviations():
    """a neighbour at distance 0 is skipped and not counted, an empty histogram gives zeros, a keypoint without neighbours gives zeros"""
    pts = np.array([[0, 0, 0], [0, 0, 0], [1, 0, 0], [9, 9, 9]], np.float32)
    nrm = np.array([[0, 0, 1], [0, 0, 1], [0, 1, 0], [1, 0, 0]], np.float32)
    rows = R.radius_rows(pts, 2.0)
    assert [r.tolist() for r in rows] == [[1, 2], [0, 2], [0, 1], []]
    counts, s = R.spfh(pts, nrm, rows, 5)
    assert counts[0].reshape(3, 5).sum(1).tolist() == [1, 1, 1] and not counts[3].any() and not s[3].any() and np.isfinite(s).all()
    f = R.fpfh(pts, rows, s)
    assert not f[3].any() and np.isfinite(f).all() and abs(np.linalg.norm(f[0]) - 1) < 1e-12
    # the two coincident points have the same neighbours at the same distances and the same normals: the same descriptor
    assert f[0].tobytes() == f[1].tobytes()


def test_restatement_bins():
    e = R.bin_edges(-1.0, 1.0, 4)
    assert e.tolist() == [-1.0, -0.5, 0.0, 0.5, 1.0]
    v = np.array([-1.0, -0.5, np.nextafter(-0.5, -1), 0.0, 1.0, np.nextafter(1.0, 2), np.nextafter(-1.0, -2), np.nan, 0.75])
    assert R.bin_of(v, -1.0, 1.0, 4).tolist() == [0, 1, 0, 2, 3, -1, -1, -1, 3]
    for B in (1, 4, 5, 11, 32):
        for lo, hi in ((-1.0, 1.0), (-np.pi, np.pi)):
            assert np.array_equal(R.bin_edges(lo, hi, B), np.linspace(lo, hi, B + 1))
            x = np.random.default_rng(B).uniform(lo - 0.1, hi + 0.1, 2000)
            b = R.bin_of(x, lo, hi, B)
            assert np.array_equal(np.bincount(b[b >= 0], minlength=B), np.histogram(x, bins=B, range=(lo, hi))[0])


def test_fpfh_symbols_declared_exported_and_bound():
    from mr_slam_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    protos = _lib.parse_header(_lib.HEADER)
    lib = C.CDLL(_lib.LIB_PATH)
    api = _lib.load()
    for n in NAMES:
        assert n in protos and hasattr(lib, n) and callable(getattr(api, n)), n
    assert lib.mrs_abi_version() == 1
    assert "#define MRS_FPFH_MAX_BINS 32" in open(_lib.HEADER).read()
    from mr_slam_amd import fpfh
    assert fpfh.MAX_BINS == 32 and fpfh.DEFAULT_BINS == 5
    h_off = np.array([0, 4], np.int64)
    for call in (lambda: api.mrs_radius_count(None, None, 3, None, h_off, 1, 0.5, None, None, None),
                 lambda: api.mrs_radius_fill(None, None, 3, None, h_off, 1, 0.5, None, 0, None, None),
                 lambda: api.mrs_fpfh_spfh(None, None, 3, None, None, 1, 4, None, None, 0, 5, None, None, None),
                 lambda: api.mrs_fpfh_spfh_from_neighbors(None, None, 3, None, None, 1, 4, None, None, 0, 5, None, None, None),
                 lambda: api.mrs_fpfh_describe(None, None, 3, None, 1, 4, None, None, 0, 5, None, None, 0, None, None),
                 lambda: api.mrs_iss_saliency(None, None, 3, None, 1, 4, None, None, 0, 5, 0.975, 0.975, None, None),
                 lambda: api.mrs_iss_nonmax(None, None, 1, 4, None, None, 0, None, None, None)):
        with pytest.raises(_lib.MrsError) as e:                   # the C side's null check, no GPU involved
            call()
        assert e.value.status == 1 and "null pointer" in str(e.value)
    with pytest.raises(_lib.MrsError, match="d_points.*no CPU fallback"):
        api.mrs_radius_count(None, np.zeros((4, 3), np.float32), 3, None, h_off, 1, 0.5, None, None, None)
    with pytest.raises(ValueError):
        fpfh._check_bins(33)


def test_install_registers_fpfh_only_when_asked():
    from mr_slam_amd import compat
    mine = ("FPFH", "ISS", "pr_methods", "util") + compat._NAMES
    saved = {k: sys.modules.pop(k) for k in list(sys.modules) if k.split(".")[0] in mine}
    try:
        compat.install()
        assert "FPFH" not in sys.modules and "ISS" not in sys.modules
        compat.install(scancontext=True, m2dp=True, fasthistogram=True)
        assert "FPFH" not in sys.modules and "ISS" not in sys.modules
        compat.install(fpfh=True)
        import FPFH
        import ISS
        from mr_slam_amd.compat import FPFH as mod, ISS as iss_mod
        assert FPFH is mod and ISS is iss_mod
        assert callable(FPFH.get_spfh) and callable(FPFH.describe) and callable(ISS.iss) and FPFH.point_cloud_normals is None
        import inspect
        for f in (FPFH.get_spfh, FPFH.describe):
            assert list(inspect.signature(f).parameters) == ["point_cloud", "nearest_idx", "keypoint_id", "radius", "B"]
        with pytest.raises(NameError):                            # the reference's failure without its __main__ global
            FPFH.get_spfh(np.zeros((2, 3)), [np.array([0, 1]), np.array([0, 1])], 0, 1.0, 5)
        with pytest.raises(ValueError):                           # no universal radii
            ISS.iss(np.zeros((2, 3)))
    finally:
        for k in [k for k in sys.modules if k.split(".")[0] in mine]:
            sys.modules.pop(k)
        sys.modules.update(saved)
