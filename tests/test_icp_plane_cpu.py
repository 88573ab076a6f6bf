"""CPU suite for the point-to-plane ICP (row G12): the public surface, the NumPy restatement
(tests/golden/icp_plane_restate.py) on known motions and planes, the conditions on the fixtures of tests/test_icp_plane_gpu.py, and
mr_slam_amd/csrc/icp_plane_update.hpp -- the least-squares fit the device kernel compiles -- built for the HOST with g++ from that very
header, against LAPACK and under the address / undefined-behaviour sanitizers (a stand-alone program).  No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
from scipy.spatial.transform import Rotation as Rot

import icp_plane_cases as PK

R, PR = PK.R, PK.PR
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "cpp", "build")
SRC = os.path.join(ROOT, "tests", "cpp", "icp_plane_update_host.cpp")
HDRS = [os.path.join(ROOT, "mr_slam_amd", "csrc", f) for f in ("icp_plane_update.hpp", "icp_update.hpp", "eig3.hpp")]


def test_public_surface():
    """the C ABI declares the struct and the entry points (ABI version unchanged), and GicpBatch carries the methods"""
    hdr = open(os.path.join(ROOT, "include", "mrslam_hip.h")).read()
    m = re.search(r"typedef struct mrs_icp_plane_params \{(.*?)\} mrs_icp_plane_params;", hdr, flags=re.S)
    assert m
    fields = re.findall(r"\b(int32_t|double)\s+(\w+)(\[3\])?;", re.sub(r"/\*.*?\*/", "", m[1], flags=re.S))
    assert [f[:2] for f in fields] == [("int32_t", "max_iterations"), ("int32_t", "force_iterations"), ("double", "max_correspondence_distance"),
                                       ("double", "transformation_epsilon"), ("double", "rotation_epsilon"), ("double", "euclidean_fitness_epsilon"),
                                       ("int32_t", "normal_k"), ("double", "viewpoint")]
    assert fields[-1][2] == "[3]"
    from mr_slam_amd import _lib, gicp
    protos = _lib.parse_header(_lib.HEADER)
    want = {"mrs_icp_plane_default_params": 1, "mrs_gicp_batch_compute_normals": 5, "mrs_gicp_batch_get_normals": 3,
            "mrs_gicp_batch_set_normals": 5, "mrs_gicp_batch_set_normals_host": 4, "mrs_gicp_batch_align_icp_plane": 8,
            "mrs_gicp_batch_icp_plane_step": 8, "mrs_gicp_batch_icp_plane_profile": 7}
    assert {n: len(protos[n][1]) for n in want} == want
    assert "#define MRS_ABI_VERSION 1\n" in hdr
    for name in ("compute_normals", "normals", "set_normals", "align_icp_plane", "icp_plane_step", "icp_plane_profile"):
        assert callable(getattr(gicp.GicpBatch, name))
    assert [f[0] for f in gicp.IcpPlaneParams._fields_] == [f[1] for f in fields]
    assert gicp.IcpPlaneParams._fields_[:6] == gicp.IcpParams._fields_
    assert C.sizeof(gicp.IcpPlaneParams) == 72 and gicp.IcpPlaneParams.viewpoint.offset == 48
    assert gicp.ICP_PLANE_STATES[PR.DEGENERATE] == "DEGENERATE" and gicp.ICP_PLANE_STATES[:6] == gicp.ICP_STATES


# ---- the restatement itself --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [6, 103])
def test_restatement_recovers_the_known_motion(seed):
    """Ten forced iterations from the identity.  The bound is the estimator's own: with independent noise of sigma = 0.01 m on both clouds
    the residual n . (d - s) has variance 2 sigma^2, so the six unknowns have covariance 2 sigma^2 M^-1 (M = sum a a^T of the last
    iteration); every unknown within five of its standard deviations."""
    src, tgt, Ttrue = PK.pair(seed)
    N = PK.target_normals(seed)["normals"]
    r = PR.icp(src, tgt, N, force_iterations=10, max_correspondence_distance=2.0)
    corr, _ = R.correspondences(src, R.Target(tgt), r["X"], 2.0)
    M, _ = PR.unpack(PR.sums29(src, tgt, N, r["X"], corr))
    sd = np.sqrt(2 * 0.01 ** 2 * np.diag(np.linalg.inv(M)))
    E = r["X"] @ np.linalg.inv(Ttrue)
    err = np.concatenate([Rot.from_matrix(E[:3, :3]).as_rotvec(), E[:3, 3]])
    print(seed, err / sd, PK.pose_err(r["X"], Ttrue))
    assert (np.abs(err) <= 5 * sd).all(), err / sd
    assert PK.pose_err(r["X"], Ttrue)[0] < 0.01 * PK.pose_err(np.eye(4), Ttrue)[0]


def test_restated_normals_on_a_noisy_plane():
    """Against numpy.linalg.eigh on neighbours found by brute force in float64 (the same vectors up to rounding), turned towards the
    viewpoint, and within the noise of the plane's own normal: k points of in-plane spread lambda1 and noise sigma tilt the fitted normal by
    about sigma / sqrt(k lambda1) per axis; five times that."""
    rng = np.random.default_rng(5)
    n, k, sigma = 600, 15, 0.005
    nt = np.array([0.3, -0.2, 1.0]); nt /= np.linalg.norm(nt)
    u = np.cross(nt, [1.0, 0, 0]); u /= np.linalg.norm(u)
    P = (rng.uniform(-3, 3, (n, 1)) * u + rng.uniform(-3, 3, (n, 1)) * np.cross(nt, u) + rng.normal(0, sigma, (n, 1)) * nt + [0, 0, -4]).astype(np.float32)
    for vp in ((0.0, 0.0, 0.0), (0.0, 0.0, -20.0)):
        w = PR.normals(P, k, vp)
        Pd = P.astype(np.float64)
        idx = np.argsort(((Pd[:, None] - Pd[None]) ** 2).sum(2), axis=1, kind="stable")[:, :k]
        assert w["contains_self"].all() and (idx[:, 0] == np.arange(n)).all()
        for i in range(n):
            q = Pd[idx[i]]
            lam, v = np.linalg.eigh(np.cov(q.T, bias=True))
            got = w["normals"][i, :3].astype(np.float64)
            assert min(np.abs(got - v[:, 0]).max(), np.abs(got + v[:, 0]).max()) < 2e-7 + 1e-12 * lam[2] / (lam[1] - lam[0])
            assert got @ (np.asarray(vp) - Pd[i]) > 0
            assert abs(w["normals"][i, 3] - lam[0] / lam.sum()) <= 1e-7
            assert np.arccos(min(1.0, abs(got @ nt))) < 5 * np.sqrt(2) * sigma / np.sqrt(k * w["lam"][i, 1])
    assert (np.sign(PR.normals(P, k, (0, 0, 0))["normals"][:, :3] @ nt) == 1).all()
    assert (np.sign(PR.normals(P, k, (0, 0, -20))["normals"][:, :3] @ nt) == -1).all()


def test_restated_normals_of_small_clouds():
    c = PK.normal_clouds()
    assert np.isnan(PR.normals(c["two"], 15)["normals"]).all() and PR.normals(c["two"][:0], 15)["normals"].shape == (0, 4)
    w = PR.normals(c["ten"], 15)                         # fewer points than k: every point sees the whole cloud
    assert np.isfinite(w["normals"]).all() and np.abs(np.abs(w["normals"][:, :3] @ w["normals"][0, :3]) - 1).max() < 1e-6
    w = PR.normals(c["plane"], 15)                       # an exact plane: curvature 0 to rounding, the plane's normal
    nt = np.array([0.5, -0.25, -1.0]) / np.linalg.norm([0.5, -0.25, -1.0])
    assert np.abs(w["normals"][:, 3]).max() < 1e-12 and np.abs(np.abs(w["normals"][:, :3] @ nt) - 1).max() < 1e-6


def test_restated_loop_ends():
    """too few correspondences (5), a target whose normals are all parallel (6: the pose stays), the iteration limit, a forced count"""
    rng = np.random.default_rng(1)
    B = rng.normal(size=(300, 3)).astype(np.float32)
    N = PR.normals(B, 15)["normals"]
    g = np.eye(4); g[:3, 3] = [0.1, 0.2, 0.3]
    r = PR.icp(B[:2], B, N, g)
    assert (r["state"], r["converged"], r["iterations"]) == (R.NO_CORRESPONDENCES, False, 0)
    assert np.array_equal(r["T"], g.astype(np.float32).astype(np.float64))
    r = PR.icp(B, B, np.full((300, 4), np.nan, np.float32))           # no finite normal: nothing is kept
    assert r["state"] == R.NO_CORRESPONDENCES
    flat = np.c_[rng.uniform(-5, 5, (500, 2)), np.zeros(500)].astype(np.float32)
    r = PR.icp(flat + np.float32(0.01), flat, np.tile(np.float32([0, 0, 1, 0]), (500, 1)), g)
    assert (r["state"], r["converged"], r["iterations"]) == (PR.DEGENERATE, False, 0)
    assert np.array_equal(r["T"], g.astype(np.float32).astype(np.float64))
    r = PR.icp(B + np.float32(0.01), B, N, max_iterations=1)
    assert (r["state"], r["converged"], r["iterations"]) == (R.ITERATIONS, True, 1)
    r = PR.icp(B + np.float32(0.01), B, N, force_iterations=4, transformation_epsilon=1.0)
    assert (r["state"], r["converged"], r["iterations"], len(r["trace"])) == (R.NOT_CONVERGED, False, 4, 4)


# ---- conditions on the fixtures of the GPU suite ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,seed", PK.NATURAL)
def test_margin_condition_of_the_natural_stopping_fixtures(name, seed):
    """A condition on the INPUTS of tests/test_icp_plane_gpu.py, not a measurement: no criterion value of the restatement's trace lies within
    a factor 1.25 of its threshold.  A fixture that fails this gets another seed (tests/icp_plane_cases.py), never another factor."""
    r = PK.natural(name, seed)
    m = np.array(R.margins(r["trace"], **PK.SETTINGS[name]))
    assert r["converged"] and m.shape == (r["iterations"], 4)
    assert m.min() >= PK.MARGIN, (m.min(0), r["trace"])
    Ttrue = PK.pair(seed)[2]
    assert PK.pose_err(r["X"], Ttrue)[0] < 0.05 * PK.pose_err(np.eye(4), Ttrue)[0]


def test_natural_fixtures_cover_both_rules():
    states = {(n, s): PK.natural(n, s)["state"] for n, s in PK.NATURAL}
    assert all(states[("MAPPING_890", s)] == R.TRANSFORM for s in (5, 6, 43, 103))
    assert states[("REL_MSE", 3)] == R.REL_MSE and R.TRANSFORM in (states[("REL_MSE", 4)], states[("REL_MSE", 6)])
    its = [PK.natural(n, s)["iterations"] for n, s in PK.NATURAL]
    assert len(set(its)) >= 3 and max(PK.natural("MAPPING_890", s)["iterations"] for s in (5, 6, 43, 103)) <= 4


def _normal_fixtures():
    for name in ("scan", "ten", "plane"):
        for k in PK.NORMAL_K:
            for vp in PK.VIEWPOINTS:
                yield name, k, vp


@pytest.mark.parametrize("name,k,vp", list(_normal_fixtures()))
def test_normals_fixtures_are_well_conditioned(name, k, vp):
    """at most 1 % of a cloud's points have an eigen-gap below 1e-6 or the viewpoint within 1e-6 of their tangent plane (those points are
    compared up to sign, or not at all, on the GPU), and every neighbour list holds its own point"""
    w = PK.cloud_normals(name, k, vp)
    bad = PK.unreliable(w)
    print(name, k, vp, "unreliable", bad.mean(), "ties at the k-th place", w["tie"].mean())
    assert bad.mean() <= 0.01
    assert w["contains_self"].all()
    if name == "scan":
        assert w["tie"].mean() <= 0.01
        lam = w["lam"]
        assert ((lam[:, 1] - lam[:, 0]) / lam[:, 2]).min() > 1e-6


# ---- the host build of csrc/icp_plane_update.hpp and of eig3.hpp's eigenvalues ------------------------------------------------------------
def _stale(out):
    return not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(p) for p in [SRC] + HDRS)


def _host_lib():
    so = os.path.join(BUILD, "libicp_plane_update_host.so")
    os.makedirs(BUILD, exist_ok=True)
    if _stale(so):
        r = subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-shared", "-fPIC", SRC, "-o", so], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    return C.CDLL(so)


def _host_fit(S):
    S = np.ascontiguousarray(S, np.float64).reshape(-1, 29)
    n = S.shape[0]
    ok = np.empty(n, np.int32); x = np.empty((n, 6)); D = np.empty((n, 16)); mse = np.empty(n)
    _host_lib().icp_plane_host_fit(S.ctypes.data_as(C.c_void_p), n, ok.ctypes.data_as(C.c_void_p), x.ctypes.data_as(C.c_void_p),
                                   D.ctypes.data_as(C.c_void_p), mse.ctypes.data_as(C.c_void_p))
    return ok.astype(bool), x, D.reshape(n, 4, 4), mse


def _pack(M, g, n=100.0, e=1.0):
    iu = np.triu_indices(6)
    return np.concatenate([np.full((M.shape[0], 1), n), M[:, iu[0], iu[1]], g, np.full((M.shape[0], 1), e)], 1)


def _systems(rng):
    """10 000 SPD systems M x = g: a unit-diagonal-like core Q diag(lambda) Q^T with lambda over eight decades, scaled on both sides by
    diag(10^u), u in [-3, 3] (the rotational and translational unknowns of a real system differ by the clouds' extent), and 40 rank-deficient
    ones (rank 5, rank 3, a zero diagonal entry)"""
    n = 10000
    Q, _ = np.linalg.qr(rng.normal(size=(n, 6, 6)))
    lam = 10.0 ** rng.uniform(-8, 0, (n, 6))
    lam[:, 0] = 1.0
    core = np.einsum("nij,nj,nkj->nik", Q, lam, Q)
    d = 10.0 ** rng.uniform(-3, 3, (n, 6))
    M = core * d[:, :, None] * d[:, None, :]
    M = 0.5 * (M + M.transpose(0, 2, 1))
    g = rng.normal(size=(n, 6)) * d
    bad = []
    for rank in (5, 3):
        B = rng.normal(size=(15, 6, rank))
        bad.append(np.einsum("nir,njr->nij", B, B) * rng.uniform(0.1, 1e4, (15, 1, 1)))
    Z = M[:10].copy()
    for i in range(10):
        Z[i, i % 6, :] = 0; Z[i, :, i % 6] = 0
    bad.append(Z)
    return M, g, np.concatenate(bad)


def test_host_solve_equals_lapack_on_10000_systems():
    M, g, bad = _systems(np.random.default_rng(4))
    ok, x, D, mse = _host_fit(_pack(M, g, 100.0, 7.0))
    assert ok.all() and np.array_equal(mse, np.full(M.shape[0], 0.07))
    want = np.linalg.solve(M, g[:, :, None])[:, :, 0]
    cond = np.linalg.cond(M)
    rel = np.linalg.norm(x - want, axis=1) / np.linalg.norm(want, axis=1)
    print("conditioning", cond.min(), cond.max(), "largest error / (1e-10 cond)", (rel / (1e-10 * cond)).max())
    assert np.log10(cond.max() / cond.min()) >= 8 and (rel <= 1e-10 * cond).all()
    # the increment: pcl's Rz Ry Rx of the solution, a proper rotation whatever the angles
    for i in range(0, M.shape[0], 97):
        assert np.abs(D[i] - PR.delta(x[i])).max() < 1e-12 * max(1.0, np.abs(x[i, 3:]).max())
    Rm = D[:, :3, :3]
    assert np.abs(np.einsum("nij,nkj->nik", Rm, Rm) - np.eye(3)).max() < 1e-12 and np.abs(np.linalg.det(Rm) - 1).max() < 1e-12
    assert np.array_equal(D[:, 3], np.broadcast_to([0.0, 0, 0, 1], (M.shape[0], 4)))
    # the restatement takes the same decisions and gives the same solutions
    for i in range(0, M.shape[0], 97):
        xr = PR.solve(_pack(M[i:i + 1], g[i:i + 1])[0])
        assert xr is not None and np.linalg.norm(xr - x[i]) <= 1e-10 * cond[i] * np.linalg.norm(x[i])
    okb, xb, Db, _ = _host_fit(_pack(bad, np.ones((bad.shape[0], 6))))
    assert not okb.any() and np.array_equal(Db, np.broadcast_to(np.eye(4), Db.shape)) and not xb.any()
    assert all(PR.solve(s) is None for s in _pack(bad, np.ones((bad.shape[0], 6))))
    nan = _pack(M[:2].copy(), g[:2]); nan[0, 1] = np.nan; nan[1, 8] = np.inf
    assert not _host_fit(nan)[0].any()


def test_host_fit_equals_the_restatement_on_a_fixture():
    """the sums of a real iteration (seed 6 at the identity, and 500 m from the origin): the same increment to 1e-9"""
    src, tgt, _ = PK.pair(6)
    N = PK.target_normals(6)["normals"]
    for shift in (0.0, 500.0):
        A = (src.astype(np.float64) + shift).astype(np.float32)
        B = (tgt.astype(np.float64) + shift).astype(np.float32)
        _, _, s, D, state = PR.step(A, B, N, np.eye(4), 2.0)
        ok, x, Dh, mse = _host_fit(s)
        assert ok[0] and state == R.NOT_CONVERGED and np.abs(Dh[0] - D).max() <= 1e-9 and abs(mse[0] - s[28] / s[0]) < 1e-15


def _curvature_deviation(w):
    """largest |curvature from the host build of eig3.hpp - curvature from eigvalsh| over a cloud's covariances"""
    Cm = np.ascontiguousarray(w["cov"][np.isfinite(w["cov"]).all((1, 2))])
    got = np.empty((Cm.shape[0], 3))
    _host_lib().eig3_host_eigvals(Cm.ctypes.data_as(C.c_void_p), Cm.shape[0], got.ctypes.data_as(C.c_void_p))
    lam = np.linalg.eigvalsh(Cm)
    with np.errstate(invalid="ignore", divide="ignore"):
        a = np.where(got.sum(1) > 0, got[:, 2] / got.sum(1), 0.0)
        b = np.where(lam.sum(1) > 0, lam[:, 0] / lam.sum(1), 0.0)
    return np.abs(a - b).max()


def test_curvature_of_the_host_eig3_on_the_fixture_covariances():
    """The measurement behind the GPU suite's curvature tolerance (4 x this + half a float32 ulp): PK.EIG3_CURVATURE_DEV bounds what the
    closed-form eigenvalues of eig3.hpp deviate from LAPACK's on the covariances of every normals fixture."""
    dev = max(_curvature_deviation(PK.cloud_normals(name, k, vp)) for name, k, vp in _normal_fixtures())
    print("largest curvature deviation of eig3.hpp from eigvalsh", dev)
    assert dev <= PK.EIG3_CURVATURE_DEV


def test_host_program_is_clean_under_asan_and_ubsan(tmp_path):
    """The same source as a stand-alone program, compiled with -fsanitize=address,undefined (runtimes linked statically: the program runs in
    the environment it inherits), over the 10 040 systems: no report, and the results of the plain build."""
    exe = os.path.join(BUILD, "icp_plane_update_host_san")
    os.makedirs(BUILD, exist_ok=True)
    if _stale(exe):
        r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-static-libasan", "-static-libubsan", SRC, "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    M, g, bad = _systems(np.random.default_rng(4))
    S = np.concatenate([_pack(M, g), _pack(bad, np.ones((bad.shape[0], 6)))])
    fin, fout = tmp_path / "s.bin", tmp_path / "r.bin"
    S.tofile(fin)
    r = subprocess.run([exe, str(fin), str(fout)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "10040 systems" in r.stdout, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr
    got = np.fromfile(fout).reshape(-1, 23)
    ok, x, D, _ = _host_fit(S)
    assert np.array_equal(got[:, 0], ok.astype(np.float64))
    scale = np.maximum(1.0, np.abs(x).max(1, keepdims=True))
    assert (np.abs(got[:, 1:7] - x) <= 1e-13 * scale).all() and (np.abs(got[:, 7:] - D.reshape(-1, 16)) <= 1e-13 * scale).all()
