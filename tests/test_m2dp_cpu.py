"""CPU suite for M2DP: the NumPy restatement (tests/golden/m2dp_restate.py) reproduces what the reference's own M2DP.py computed for the
fixture clouds (tests/golden/ref_m2dp.npz), the eigen-solver behind the PCA stage holds its accuracy, the new C-ABI symbols are exported
and bound, and the drop-in is only registered when asked for."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import m2dp_restate as R  # noqa: E402


@pytest.fixture(scope="module")
def g():
    return R.load()


def test_fixture_cases(g):
    assert list(g) == ["gauss3", "gauss64", "gauss1000", "gauss4097", "lidar", "nclt"]
    assert [c["cloud"].shape[0] for c in g.values()][:4] == [3, 64, 1000, 4097] and 4097 < g["lidar"]["cloud"].shape[0] <= 20000
    assert all(c["cloud"].dtype == np.float32 for n, c in g.items() if n != "nclt")
    assert os.path.getsize(R.FIXTURE) < 512 * 1024


def test_restatement_reproduces_reference(g):
    """Integer counts exactly, the descriptor (after the sign rule) within the SVD bound.  The 3-point cloud lies exactly edge-on to the four
    planes of elevation 0 (m2dp_restate.EDGE_ON_ROWS): there the reference's own counts are the sign of rounding noise, and only the number
    of differing pairs is bounded, by the number of uncertain ones."""
    for name, c in g.items():
        r = R.m2dp(c["cloud"])
        n = c["cloud"].shape[0]
        assert c["counts"].sum() == 64 * n and (c["counts"].sum(axis=1) == n).all()
        diff = R.differing_pairs(r.counts, c["counts"])
        noisy = list(R.EDGE_ON_ROWS) if n == 3 else []
        assert not np.delete(r.uncertain_rows, noisy).any(), name            # exact-match cases by construction
        assert not np.delete(diff, noisy).any(), (name, diff.sum())
        assert (diff <= r.uncertain_rows).all(), name
        if not diff.any():
            assert abs(r.sigma1 - c["sigma1"]) < 1e-13 and abs(r.sigma2 - c["sigma2"]) < 1e-13
            err = np.abs(r.desc - R.canonical(c["desc"])).max()
            assert err <= R.svd_bound(c["sigma1"], c["sigma2"]), (name, err)
        d = R.canonical(c["desc"])
        assert (d >= -1e-15).all(), name                                      # the sign rule makes both vectors non-negative


def test_restatement_small_clouds():
    for n in (0, 1, 2):
        r = R.m2dp(np.ones((n, 3)))
        assert not r.A.any() and not r.desc.any() and r.A.shape == (64, 128) and r.desc.shape == (192,)


def test_eigvecs_match_lapack(tmp_path):
    """sym3_eigvecs_desc (eig3.hpp, the PCA stage's solver) compiled for the host: eigenvectors of random anisotropic covariances against
    LAPACK.  The bound is the perturbation bound of a backward-stable solver, 64 eps ||A|| / gap per component."""
    src = tmp_path / "eig.cpp"
    src.write_text('#include "eig3.hpp"\nextern "C" void eigvecs(const double* c, double* w, double* v) { mrs::sym3_eigvecs_desc(c, w, v); }\n')
    so = tmp_path / "libeig.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "mr_slam_amd", "csrc"), str(src), "-o", str(so)],
                   check=True)
    lib = C.CDLL(str(so))
    rng = np.random.default_rng(5)
    eps = np.finfo(np.float64).eps
    for trial in range(200):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        lam = np.sort(rng.uniform(0.1, 1.0, 3) * np.array([100.0, 10.0, 1.0 if trial % 4 else 0.0]))[::-1]
        if lam[0] < 1.5 * lam[1] or lam[1] < 1.5 * lam[2]:
            continue
        cov = (q * lam) @ q.T
        cov = 0.5 * (cov + cov.T)
        w, v = np.zeros(3), np.zeros(9)
        lib.eigvecs(cov.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p))
        v = v.reshape(3, 3)
        wl, vl = np.linalg.eigh(cov)
        assert np.abs(w - wl[::-1]).max() <= 64 * eps * lam[0]
        gap = min(lam[0] - lam[1], lam[1] - lam[2])
        for k in range(3):
            ref = vl[:, 2 - k]
            err = min(np.abs(v[k] - ref).max(), np.abs(v[k] + ref).max())
            assert err <= 64 * eps * lam[0] / gap, (trial, k, err)
        assert np.abs(v @ v.T - np.eye(3)).max() <= 16 * eps
    w, v = np.zeros(3), np.zeros(9)
    zero = np.zeros(9)
    lib.eigvecs(zero.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p))
    assert np.isfinite(v).all() and np.abs(v.reshape(3, 3) @ v.reshape(3, 3).T - np.eye(3)).max() <= 16 * eps     # all points equal


def test_m2dp_symbols_exported_and_bound():
    from mr_slam_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = C.CDLL(_lib.LIB_PATH)
    names = ("mrs_m2dp_batch", "mrs_m2dp_pca_batch", "mrs_m2dp_host", "mrs_loopdb_append_m2dp", "mrs_loopdb_query_m2dp")
    for n in names:
        assert hasattr(lib, n), n
    assert lib.mrs_abi_version() == 1
    api = _lib.load()
    for n in names:
        assert callable(getattr(api, n)), n
    src = open(_lib.HEADER).read()
    assert "MRS_LOOPDB_M2DP = 4" in src
    from mr_slam_amd import m2dp
    assert m2dp.TILE_POINTS >= 64 and m2dp.KIND_M2DP == 4
    with pytest.raises(_lib.MrsError) as e:                       # the C side's null check, no GPU involved
        api.mrs_m2dp_batch(None, None, 0, 3, None, None, 1, None, None, None)
    assert e.value.status == 1
    with pytest.raises(_lib.MrsError, match="d_points.*no CPU fallback"):
        api.mrs_m2dp_batch(None, np.zeros((4, 3), np.float32), 0, 3, None, None, 1, None, None, None)


def test_install_registers_m2dp_only_when_asked():
    from mr_slam_amd import compat
    saved = {k: sys.modules.pop(k) for k in list(sys.modules) if k.split(".")[0] in ("pr_methods",) + compat._NAMES + ("util",)}
    try:
        compat.install()
        assert "pr_methods" not in sys.modules
        compat.install(scancontext=True)
        assert "pr_methods.M2DP" not in sys.modules
        compat.install(m2dp=True)
        from pr_methods.M2DP import M2DP
        from mr_slam_amd.compat import M2DP as mod
        assert M2DP is mod.M2DP and sys.modules["pr_methods"].ScanContext is sys.modules["pr_methods.ScanContext"]
        desc, A = M2DP(np.zeros((0, 3)))                          # fewer than 3 points: zeros without device work
        assert desc.shape == (192,) and A.shape == (64, 128) and desc.dtype == A.dtype == np.float64 and not desc.any() and not A.any()
    finally:
        for k in [k for k in sys.modules if k.split(".")[0] in ("pr_methods",) + compat._NAMES + ("util",)]:
            sys.modules.pop(k)
        sys.modules.update(saved)
