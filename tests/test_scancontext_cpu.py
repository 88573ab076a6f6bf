"""CPU suite for Scan Context: the reference fixture is self-consistent, the new C-ABI symbols are exported, and the drop-in is only
registered when asked for."""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import sc_restate as R  # noqa: E402


def test_fixture_restatement_reproduces_reference():
    g = R.load()
    D = g["sc"]
    assert D.shape[1:] == (1, 120, 120) and D.dtype == np.float32
    assert not D[list(g["names"]).index("zero")].any()
    for i, d in enumerate(D):
        rk, sk = R.keys(d)
        assert np.abs(rk - g["ringkey"][i]).max() < 1e-6 and np.abs(sk - g["sectorkey"][i]).max() < 1e-6
    for p, (i, j) in enumerate(g["pairs"]):
        nrm = R.sector_norms(g["sectorkey"][i], g["sectorkey"][j])
        assert np.allclose(nrm, g["sector_norms"][p], rtol=1e-9, atol=1e-12)
        if R.clear_winner(g["sector_norms"][p], int(np.argmin(nrm)), rel=1e-6):
            assert int(np.argmin(nrm)) == g["sector_shift"][p]
        assert abs(R.window_dists(D[i], D[j], [0])[0] - g["dist_direct"][p]) < 1e-5
        for q, ratio in enumerate(g["ratios"]):
            wd_ref = g["window_dists"][q, p]
            wd_ref = wd_ref[~np.isnan(wd_ref)]
            win = list(range(g["window_start"][q, p], g["window_start"][q, p] + len(wd_ref)))
            assert np.abs(R.window_dists(D[i], D[j], win) - wd_ref).max() < 1e-5
            dist, shift = g["dist_align"][q, p]
            assert abs(wd_ref.min() - dist) < 1e-7 and win[int(np.argmin(wd_ref))] == shift
        d, yaw = R.distance_sc(D[i], D[j])
        assert abs(d - g["distance_sc"][p, 0]) < 1e-5
    # the quirks the GPU tests rely on: the all-zero pair gives 1.0 at the start of the window; identical columns give 0 at shift 0
    names = list(g["names"])
    z, a = names.index("zero"), names.index("A")
    pz = [p for p, (i, j) in enumerate(g["pairs"]) if (i, j) == (a, z)][0]
    assert np.all(g["dist_align"][:, pz, 0] == 1.0) and list(g["dist_align"][:, pz, 1]) == [-6, -12, -60]


def test_fixture_replay_is_complete():
    g = R.load()
    rep = g["replay"]
    assert rep.shape[1] == 7 and len(rep) >= 10
    assert set(g["public_names"]) == {"make_ringkey", "make_sectorkey", "distance_sc", "fast_align", "fast_align_with_sectorkey",
                                      "dist_direct_sc", "dist_align_sc", "dist_align_cc"}
    assert os.path.getsize(os.path.join(HERE, "golden", "ref_scancontext.npz")) < 1 << 20


def test_scancontext_symbols_exported():
    from mr_slam_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = C.CDLL(_lib.LIB_PATH)
    for n in ("mrs_loopdb_append_sc", "mrs_loopdb_query_sc", "mrs_loopdb_query_sc_all", "mrs_sc_keys", "mrs_sc_key_align_pairs",
              "mrs_sc_dist_direct_pairs", "mrs_sc_dist_align_pairs", "mrs_sc_distance_pairs"):
        assert hasattr(lib, n), n
    assert lib.mrs_abi_version() == 1
    src = open(os.path.join(os.path.dirname(HERE), "include", "mrslam_hip.h")).read()
    assert "MRS_LOOPDB_SC = 3" in src


def test_install_registers_pr_methods_only_when_asked():
    from mr_slam_amd import compat
    saved = {k: sys.modules.pop(k) for k in list(sys.modules) if k.split(".")[0] in ("pr_methods",) + compat._NAMES + ("util",)}
    try:
        compat.install()
        assert "pr_methods" not in sys.modules and "pr_methods.ScanContext" not in sys.modules
        compat.install(node=True)
        assert "pr_methods" not in sys.modules and "pr_methods.ScanContext" not in sys.modules
        compat.install(scancontext=True)
        import pr_methods.ScanContext as SC
        from mr_slam_amd.compat import ScanContext
        assert SC is ScanContext
        assert set(R.load()["public_names"]) <= {n for n in dir(SC) if not n.startswith("_") and callable(getattr(SC, n))}
    finally:
        for k in [k for k in sys.modules if k.split(".")[0] in ("pr_methods",) + compat._NAMES + ("util",)]:
            sys.modules.pop(k)
        sys.modules.update(saved)
