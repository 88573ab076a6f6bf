"""CPU suite for the point-to-point ICP (row G9): the public surface, the NumPy restatement (tests/golden/icp_restate.py) against SciPy and
hand-made traces, the margin condition on the fixtures of tests/test_icp_gpu.py, and mr_slam_amd/csrc/icp_update.hpp -- the rigid fit and
the stopping rules the device kernel compiles -- built for the HOST with g++ from that very header, against LAPACK's SVD and under the
address / undefined-behaviour sanitizers (a stand-alone program).  No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
from scipy.spatial.transform import Rotation as Rot

import icp_cases as K

R = K.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "cpp", "build")
SRC = os.path.join(ROOT, "tests", "cpp", "icp_update_host.cpp")
HDRS = [os.path.join(ROOT, "mr_slam_amd", "csrc", f) for f in ("icp_update.hpp", "eig3.hpp")]
DBL_MAX = R.DBL_MAX


def test_public_surface():
    """the C ABI declares the struct and the three functions (ABI version unchanged), and GicpBatch carries the two methods"""
    hdr = open(os.path.join(ROOT, "include", "mrslam_hip.h")).read()
    m = re.search(r"typedef struct mrs_icp_params \{(.*?)\} mrs_icp_params;", hdr, flags=re.S)
    assert m
    fields = re.findall(r"\b(int32_t|double)\s+(\w+);", re.sub(r"/\*.*?\*/", "", m[1], flags=re.S))
    assert fields == [("int32_t", "max_iterations"), ("int32_t", "force_iterations"), ("double", "max_correspondence_distance"),
                      ("double", "transformation_epsilon"), ("double", "rotation_epsilon"), ("double", "euclidean_fitness_epsilon")]
    from mr_slam_amd import _lib, gicp
    protos = _lib.parse_header(_lib.HEADER)
    assert [len(protos[n][1]) for n in ("mrs_icp_default_params", "mrs_gicp_batch_align_icp", "mrs_gicp_batch_icp_step")] == [1, 8, 7]
    assert "#define MRS_ABI_VERSION 1\n" in hdr
    assert callable(gicp.GicpBatch.align_icp) and callable(gicp.GicpBatch.icp_step)
    assert [f[0] for f in gicp.IcpParams._fields_] == [f[1] for f in fields]
    assert C.sizeof(gicp.IcpParams) == 40


def test_restated_rigid_fit_equals_scipy_align_vectors():
    rng = np.random.default_rng(0)
    for n in (3, 4, 10, 500):
        for _ in range(20):
            a = rng.normal(size=(n, 3)) * rng.uniform(0.1, 30, 3) + rng.normal(size=3) * 20
            Rt = Rot.from_rotvec(rng.normal(size=3) * rng.uniform(0, 1.5)).as_matrix()
            b = a @ Rt.T + rng.normal(size=3) * 5 + rng.normal(size=(n, 3)) * 0.05
            D = R.rigid_fit(a, b)
            want, _ = Rot.align_vectors(b - b.mean(0), a - a.mean(0))       # b - bbar ~ R (a - abar)
            assert np.abs(D[:3, :3] - want.as_matrix()).max() < 1e-9
            assert np.abs(D[:3, 3] - (b.mean(0) - D[:3, :3] @ a.mean(0))).max() < 1e-12
            assert abs(np.linalg.det(D[:3, :3]) - 1) < 1e-12


def _increment(angle, t):
    D = np.eye(4)
    D[:3, :3] = Rot.from_rotvec([0, 0, angle]).as_matrix()
    D[:3, 3] = t
    return D


# (name, settings, iteration, increment, mse, previous mse) -> state: one hand-made iteration per state
SET = dict(max_iterations=50, transformation_epsilon=1e-3, rotation_epsilon=0.0, euclidean_fitness_epsilon=1e-3)
HAND = [
    ("goes on", SET, 3, _increment(0.1, [0.2, 0, 0]), 0.5, 0.9, R.NOT_CONVERGED),
    ("iteration limit, whatever else holds", SET, 50, _increment(0.0, [0, 0, 0]), 0.5, 0.5, R.ITERATIONS),
    ("small increment", SET, 3, _increment(1e-3, [0.02, 0.01, 0]), 0.5, 0.9, R.TRANSFORM),
    ("the epsilon bounds the SQUARED translation: |t| = 0.04 > 1e-3 still counts as small", SET, 3, _increment(0.0, [0.03, 0, 0]), 0.5, 0.9, R.TRANSFORM),
    ("|t|^2 = 1.6e-3 > 1e-3", SET, 3, _increment(0.0, [0.04, 0, 0]), 0.5, 0.9, R.NOT_CONVERGED),
    ("rotation beyond 1 - cos = 1e-3 (0.0447 rad)", SET, 3, _increment(0.05, [0, 0, 0]), 0.5, 0.9, R.NOT_CONVERGED),
    ("explicit rotation epsilon replaces 1 - transformation_epsilon", dict(SET, rotation_epsilon=1 - 1e-8), 3, _increment(1e-3, [0, 0, 0]), 0.5, 0.9,
     R.NOT_CONVERGED),
    ("same error twice", dict(SET, transformation_epsilon=0.0), 3, _increment(0.1, [0.2, 0, 0]), 0.5, 0.5 + 1e-13, R.ABS_MSE),
    ("relative change 5e-4 < 1e-3", SET, 3, _increment(0.1, [0.2, 0, 0]), 0.5, 0.50025, R.REL_MSE),
    ("TRANSFORM and REL_MSE both hold: TRANSFORM wins", SET, 3, _increment(1e-3, [0.01, 0, 0]), 0.5, 0.50025, R.TRANSFORM),
    ("first iteration: the previous error is DBL_MAX, relative change 1", SET, 1, _increment(0.1, [0.2, 0, 0]), 0.5, DBL_MAX, R.NOT_CONVERGED),
    ("PCL's defaults go on after any increment that moves at all", dict(R.DEFAULTS), 9, _increment(0.0, [1e-9, 0, 0]), 0.5, 0.5 + 1e-9, R.NOT_CONVERGED),
    ("PCL's defaults: an increment that is exactly the identity", dict(R.DEFAULTS), 9, _increment(0.0, [0, 0, 0]), 0.5, 0.5 + 1e-9, R.TRANSFORM),
]


def _restated_state(settings, it, D, mse, prev):
    cos, t2, d_abs, rel = R.criteria(D, mse, prev)
    return R.converged(it, cos, t2, d_abs, rel, settings["max_iterations"], settings["transformation_epsilon"],
                       settings["rotation_epsilon"], settings["euclidean_fitness_epsilon"])


@pytest.mark.parametrize("case", HAND, ids=[h[0] for h in HAND])
def test_restated_state_machine_on_hand_made_iterations(case):
    _, settings, it, D, mse, prev, want = case
    assert _restated_state(settings, it, D, mse, prev) == want


def test_restated_loop_ends():
    """whole runs: too few correspondences (state 5, not converged, pose = guess narrowed to float32), the iteration limit, a forced count"""
    rng = np.random.default_rng(1)
    B = rng.normal(size=(300, 3)).astype(np.float32)
    g = np.eye(4); g[:3, 3] = [0.1, 0.2, 0.3]
    r = R.icp(B[:2], B, g)
    assert (r["state"], r["converged"], r["iterations"]) == (R.NO_CORRESPONDENCES, False, 0)
    assert np.array_equal(r["T"], g.astype(np.float32).astype(np.float64))
    r = R.icp(B + np.float32(500), B, max_correspondence_distance=2.0)
    assert (r["state"], r["converged"], r["iterations"]) == (R.NO_CORRESPONDENCES, False, 0)
    r = R.icp(B + np.float32(0.01), B, max_iterations=1)
    assert (r["state"], r["converged"], r["iterations"]) == (R.ITERATIONS, True, 1)
    r = R.icp(B + np.float32(0.01), B, force_iterations=4, transformation_epsilon=1.0)
    assert (r["state"], r["converged"], r["iterations"], len(r["trace"])) == (R.NOT_CONVERGED, False, 4, 4)


@pytest.mark.parametrize("name,seed", K.NATURAL)
def test_margin_condition_of_the_natural_stopping_fixtures(name, seed):
    """A condition on the INPUTS of tests/test_icp_gpu.py, not a measurement: no criterion value of the restatement's trace lies within a
    factor 1.25 of its threshold, so rounding differences between the kernel and the restatement cannot change where a pair stops.
    A fixture that fails this gets another seed (tests/icp_cases.py), never another factor."""
    r = K.natural(name, seed)
    m = np.array(R.margins(r["trace"], **K.SETTINGS[name]))
    assert r["converged"] and m.shape == (r["iterations"], 4)
    assert m.min() >= K.MARGIN, (m.min(0), r["trace"])
    Ttrue = K.pair(seed)[2]
    assert K.pose_err(r["X"], Ttrue)[0] < 0.5 * K.pose_err(np.eye(4), Ttrue)[0]       # and the run moved towards the true transform


def test_natural_fixtures_cover_both_rules():
    states = {(n, s): K.natural(n, s)["state"] for n, s in K.NATURAL}
    assert all(states[("MAPPING_890", s)] == R.TRANSFORM for s in (23, 4, 5, 6))
    assert states[("REL_MSE", 3)] == states[("REL_MSE", 43)] == R.REL_MSE
    # seed 4 under the REL_MSE settings ends in an iteration where TRANSFORM and REL_MSE both hold
    r = K.natural("REL_MSE", 4)
    cos, t2, _, rel, _ = r["trace"][-1]
    assert r["state"] == R.TRANSFORM and rel < 1e-3 and t2 <= 1e-10 and cos >= 1 - 1e-12
    assert len({K.natural(n, s)["iterations"] for n, s in K.NATURAL}) >= 4


# ---- the host build of csrc/icp_update.hpp -----------------------------------------------------------------------------------------------
def _stale(out):
    return not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(p) for p in [SRC] + HDRS)


def _host_lib():
    so = os.path.join(BUILD, "libicp_update_host.so")
    os.makedirs(BUILD, exist_ok=True)
    if _stale(so):
        r = subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-shared", "-fPIC", SRC, "-o", so], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    lib = C.CDLL(so)
    lib.icp_host_converged.restype = C.c_int
    lib.icp_host_converged.argtypes = [C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_double, C.c_void_p]
    return lib


def _host_rotation(H):
    H = np.ascontiguousarray(H, np.float64).reshape(-1, 9)
    out = np.empty_like(H)
    _host_lib().icp_host_rotation(H.ctypes.data_as(C.c_void_p), H.shape[0], out.ctypes.data_as(C.c_void_p))
    return out.reshape(-1, 3, 3)


def _random_H(rng):
    """10 000 matrices: full rank of any conditioning and scale, planar (rank 2), collinear (rank 1), reflections, and a few special ones"""
    def ortho(n):
        Q, _ = np.linalg.qr(rng.normal(size=(n, 3, 3)))
        return Q
    def compose(U, s, V):
        return np.einsum("nij,nj,nkj->nik", U, s, V)
    n = 2400
    full = compose(ortho(n), np.sort(10.0 ** rng.uniform(-8, 0, (n, 3)), axis=1)[:, ::-1], ortho(n))
    s2 = np.sort(10.0 ** rng.uniform(-6, 0, (n, 3)), axis=1)[:, ::-1]; s2[:, 2] = 0
    planar = compose(ortho(n), s2, ortho(n))
    s1 = np.zeros((n, 3)); s1[:, 0] = 10.0 ** rng.uniform(-3, 3, n)
    line = compose(ortho(n), s1, ortho(n))
    U, V = ortho(n), ortho(n)
    flip = np.sign(np.linalg.det(U) * np.linalg.det(V))
    U[:, :, 2] *= -flip[:, None]                                    # det(V U^T) < 0 for every one of them
    refl = compose(U, np.sort(rng.uniform(0.05, 1, (n, 3)), axis=1)[:, ::-1], V)
    a = rng.normal(size=(380, 40, 3)); b = rng.normal(size=(380, 40, 3))
    clouds = np.einsum("nki,nkj->nij", a - a.mean(1, keepdims=True), b - b.mean(1, keepdims=True))   # generic, about half of them reflections
    special = np.stack([np.zeros((3, 3)), np.eye(3), -np.eye(3), np.diag([1.0, 1.0, 0.0]), np.diag([0.0, 0.0, 2.0]), np.full((3, 3), 1e-300),
                        np.full((3, 3), 1e300), np.diag([1.0, 1e-200, 0.0]), np.ones((3, 3)), np.diag([2.0, 2.0, 2.0])] * 2)
    H = np.concatenate([full, planar, line, refl, clouds, special])
    scale = 10.0 ** rng.uniform(-6, 9, H.shape[0])
    scale[-special.shape[0]:] = 1.0
    assert H.shape[0] == 10000 and (np.linalg.det(refl) < 0).all()
    return H * scale[:, None, None]


def test_host_rotation_attains_the_svd_optimum_on_10000_matrices():
    H = _random_H(np.random.default_rng(2))
    Rm = _host_rotation(H)
    assert np.isfinite(Rm).all()
    assert np.abs(np.einsum("nij,nkj->nik", Rm, Rm) - np.eye(3)).max() < 1e-12          # orthogonal
    assert np.abs(np.linalg.det(Rm) - 1).max() < 1e-12                                  # proper
    U, s, Vt = np.linalg.svd(H)
    d = np.sign(np.linalg.det(np.einsum("nji,nkj->nik", Vt, U)))                        # det(V U^T)
    d[s[:, 2] <= 1e-13 * s[:, 0]] = 0                                                   # rank-deficient: sigma_3 does not count
    best = s[:, 0] + s[:, 1] + d * s[:, 2]
    got = np.einsum("nij,nji->n", Rm, H)                                                # tr(R H)
    ok = best > 0
    assert ok.sum() >= 9990 and (np.abs(got - best)[ok] <= 1e-12 * best[ok]).all(), np.abs(got / best - 1)[ok].max()
    assert np.array_equal(Rm[~ok], np.broadcast_to(np.eye(3), Rm[~ok].shape))           # the zero matrix: identity


def test_host_rigid_fit_equals_the_restatement_from_the_sums():
    """icp_rigid_fit forms H from the 17 sums (sum a b^T - n abar bbar^T); the restatement centres the points.  Also far from the origin."""
    rng = np.random.default_rng(3)
    lib = _host_lib()
    for shift in (np.zeros(3), np.array([55.0, -48.0, 3.0])):
        for n in (3, 50, 5000):
            a = rng.normal(size=(n, 3)) * [20, 15, 2] + shift
            b = a @ Rot.from_rotvec([0.01, -0.02, 0.05]).as_matrix().T + [0.3, -0.2, 0.05] + rng.normal(size=(n, 3)) * 0.02
            s = np.concatenate([[n], a.sum(0), b.sum(0), (a.T @ b).reshape(-1), [((b - a) ** 2).sum()]])
            D = np.empty(16); mse = np.empty(1)
            lib.icp_host_rigid_fit(s.ctypes.data_as(C.c_void_p), 1, D.ctypes.data_as(C.c_void_p), mse.ctypes.data_as(C.c_void_p))
            assert np.abs(D.reshape(4, 4) - R.rigid_fit(a, b)).max() < 1e-9
            assert abs(mse[0] - ((b - a) ** 2).sum() / n) < 1e-12


@pytest.mark.parametrize("case", HAND, ids=[h[0] for h in HAND])
def test_host_state_machine_equals_the_restatement(case):
    _, st, it, D, mse, prev, want = case
    p = C.c_double(prev)
    Dc = np.ascontiguousarray(D, np.float64)
    got = _host_lib().icp_host_converged(st["max_iterations"], 0, st["transformation_epsilon"], st["rotation_epsilon"], st["euclidean_fitness_epsilon"],
                                         it, Dc.ctypes.data_as(C.c_void_p), mse, C.byref(p))
    assert got == want
    assert p.value == (mse if want == R.NOT_CONVERGED else prev)        # the previous error moves on only when the pair does
    forced = _host_lib().icp_host_converged(st["max_iterations"], 7, st["transformation_epsilon"], st["rotation_epsilon"],
                                            st["euclidean_fitness_epsilon"], it, Dc.ctypes.data_as(C.c_void_p), mse, C.byref(p))
    assert forced == R.NOT_CONVERGED                                    # force_iterations disables every rule


def test_host_program_is_clean_under_asan_and_ubsan(tmp_path):
    """The same source as a stand-alone program, compiled with -fsanitize=address,undefined (runtimes linked statically: the program runs in
    the environment it inherits), over the 10 000 matrices: no report, and the rotations of the plain build."""
    exe = os.path.join(BUILD, "icp_update_host_san")
    os.makedirs(BUILD, exist_ok=True)
    if _stale(exe):
        r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", SRC,
                            "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    H = _random_H(np.random.default_rng(2))
    fin, fout = tmp_path / "h.bin", tmp_path / "r.bin"
    H.tofile(fin)
    r = subprocess.run([exe, str(fin), str(fout)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "10000 matrices" in r.stdout, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr
    got = np.fromfile(fout).reshape(-1, 3, 3)
    assert np.abs(got - _host_rotation(H)).max() < 1e-13
