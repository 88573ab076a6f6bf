"""CPU suite for the pose-graph optimiser: the NumPy / scipy restatement (tests/golden/posegraph_restate.py) has Jacobians that are the
derivatives of its error under the contract's retraction, composes a pure chain exactly and does not depend on the order of its solves; the
test scenes keep the conditions the GPU suite relies on; the kernels' per-factor and per-pose arithmetic (posegraph_factor.hpp, compiled by
g++ into a stand-alone program, and once more under the address and undefined-behaviour sanitizers) agrees with the restatement; the C-ABI
symbols are exported and bound; the host helpers of the Python layer do what they say."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import posegraph_cases as PC

R = PC.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _args(s):
    return s.chain_lengths, s.odom, s.li, s.lj, s.lZ


def _factor_inputs(seed=5, n=64, extent=200.0, reach=30.0):
    """poses and measurements as the optimiser meets them: far from consistent (the stage-1 values have zero translations)"""
    rng = np.random.default_rng(seed)
    Ti = np.array([PC.pose(rng.normal(0, 1.0, 3), rng.uniform(-extent, extent, 3)) for _ in range(n)])
    Tj = np.array([PC.pose(rng.normal(0, 1.0, 3), rng.uniform(-extent, extent, 3)) for _ in range(n)])
    Z = np.array([PC.pose(rng.normal(0, 1.5, 3), rng.uniform(-reach, reach, 3)) for _ in range(n)])
    Z[0, :3, :3] = PC.rot([0, 0, np.pi])                         # a half turn
    Z[1] = np.eye(4)
    return Ti, Tj, Z


def test_jacobians_are_the_derivatives_of_the_error():
    Ti, Tj, Z = _factor_inputs(n=12)
    h = 1e-5
    worst = 0.0
    for k in range(Ti.shape[0]):
        Hi, Hj = R.factor_jacobians(Ti[k], Tj[k], Z[k])
        for side, H in ((0, Hi), (1, Hj)):
            for c in range(6):
                d = np.zeros((1, 6))
                d[0, c] = h
                plus, minus = R.retract((Ti[k], Tj[k])[side][None], d)[0], R.retract((Ti[k], Tj[k])[side][None], -d)[0]
                ep = R.factor_error(plus, Tj[k], Z[k]) if side == 0 else R.factor_error(Ti[k], plus, Z[k])
                em = R.factor_error(minus, Tj[k], Z[k]) if side == 0 else R.factor_error(Ti[k], minus, Z[k])
                worst = max(worst, np.abs((ep - em) / (2 * h) - H[:, c]).max())
    assert worst < 1e-6, worst


def test_vectorised_linearisation_is_the_per_factor_one():
    Ti, Tj, Z = _factor_inputs()
    n = Ti.shape[0]
    e, Hi, Hj = R._linearize(np.concatenate([Ti, Tj]), np.arange(n), n + np.arange(n), Z)
    for k in range(n):
        a, b = R.factor_jacobians(Ti[k], Tj[k], Z[k])
        assert np.array_equal(Hi[k], a) and np.array_equal(Hj[k], b)
        assert np.abs(e[k] - R.factor_error(Ti[k], Tj[k], Z[k])).max() < 1e-12


@pytest.mark.parametrize("name", ["chain_1", "chain_2", "chain_3", "chain_65"])
def test_pure_chain_is_the_composed_odometry(name):
    s = PC.scene(name)
    r = PC.expected(name)
    X = np.tile(np.eye(4), (s.chain_lengths[0], 1, 1))
    for k in range(1, X.shape[0]):
        X[k] = X[k - 1] @ s.odom[k - 1]
    assert np.abs(r.T - X).max() < 1e-12
    assert r.error_final <= 1e-20 and r.converged and r.iterations < 20


@pytest.mark.parametrize("name", PC.NAMES + ("quirks_prior",))
def test_scene_conditions_and_solve_order(name):
    """on the restatement alone: every stage-1 matrix is far from singular, the iteration count is determined (no max|delta| within a factor
    4 of eps), and a dense Cholesky of a permuted system ends where the sparse solve ends after the same number of iterations"""
    _, X = PC.expected_initial(name)
    assert np.linalg.svd(X, compute_uv=False).min() >= 0.5
    r = PC.expected(name)
    d = np.array(r.deltas)
    assert r.converged and r.iterations < 40, (r.iterations, r.deltas)
    assert not ((d > PC.EPS / 4) & (d < PC.EPS * 4)).any(), r.deltas
    s = PC.with_prior() if name == "quirks_prior" else PC.scene(name)
    other = R.optimize(*_args(s), prior=s.prior, order=7, iterations=r.iterations)
    assert np.abs(other.T - r.T).max() < 1e-11
    assert np.abs(r.T[:, :3, 3]).max() < 300.0
    if len(s.li):
        assert r.error_final < r.error_initial


def test_scenes_cover_what_they_claim():
    nb = PC.header_int("MRS_PGO_PANEL_WIDTH")
    e2 = PC.panel_separator_counts()
    for w in (1, 2):
        assert {w * nb - 6, w * nb, w * nb + 6} <= {6 * e for e in e2}
        assert {w * nb - 3, w * nb, w * nb + 3} <= {3 * (e + 2) for e in e2}
    for e in e2:
        s = PC.scene("panel_E%d" % e)
        assert np.unique(np.concatenate([s.li, s.lj])).size == e and 0 not in s.li and 0 not in s.lj
    s = PC.scene("runs")
    touched = sorted(int(p) for p in set(s.li) | set(s.lj) if p < 260)
    assert touched == [10, 11, 13, 77, 142, 208] and [b - a - 1 for a, b in zip(touched, touched[1:])] == [0, 1, 63, 64, 65]
    q = PC.scene("quirks")
    pairs = list(zip(q.li.tolist(), q.lj.tolist()))
    assert len(pairs) != len(set(pairs)) and any(j == i + 1 for i, j in pairs) and any(j < i for i, j in pairs)
    assert any(i == 0 for i, _ in pairs) and any(j == 0 for _, j in pairs) and (39, 69) in pairs
    half = q.lZ[pairs.index((0, 70))]
    assert abs(np.trace(half[:3, :3]) + 1.0) < 1e-12
    assert not R.connected((3, 3), [0], [2]) and R.connected((3, 3), [4], [2]) and R.connected((5,), [], [])


def test_restatement_stop_rule():
    r = PC.expected("r3x2")
    one = PC.expected("r3x2", PC.EPS, 1)
    assert one.iterations == 1 and not one.converged and np.abs(one.T - r.T).max() > 1e-6
    fixed = PC.expected("r3x2", 0.0, 200)
    assert fixed.iterations == 200 and not fixed.converged and np.abs(fixed.T - r.T).max() < 1e-11


@pytest.fixture(scope="module")
def factor_programs(tmp_path_factory):
    """the stand-alone program twice: as the kernels are compiled (no contraction), and under the address and undefined-behaviour sanitizers"""
    d = tmp_path_factory.mktemp("pgo")
    base = ["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-I" + os.path.join(ROOT, "mr_slam_amd", "csrc"),
            os.path.join(ROOT, "tests", "cpp", "posegraph_factor_host.cpp")]
    subprocess.run(base + ["-O2", "-o", str(d / "plain")], check=True)
    subprocess.run(base + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(d / "sanitized")], check=True)
    return d


def _run(d, exe, mode, parts, shape):
    with open(d / "in.bin", "wb") as f:
        for p in parts:
            np.ascontiguousarray(p).tofile(f)
    r = subprocess.run([str(d / exe), mode, str(d / "in.bin"), str(d / "out.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return np.fromfile(d / "out.bin", np.float64).reshape(shape)


@pytest.mark.parametrize("extent, reach", [(5.0, 3.0), (200.0, 30.0)])
@pytest.mark.parametrize("exe", ["plain", "sanitized"])
def test_factor_header_matches_restatement(factor_programs, exe, extent, reach):
    """1e-13 where the quantities are of order one to a hundred (a site of +-5 m, loops of 3 m); at the extent of the scenes (+-200 m, 30 m)
    the same bound relative to the size of each quantity, which is what fp64 can hold"""
    Ti, Tj, Z = _factor_inputs(extent=extent, reach=reach)
    n = Ti.shape[0]
    got = _run(factor_programs, exe, "factor", [np.array([n], np.int32), Ti, Tj, Z], (n, 103))
    e, Hi, Hj = R._linearize(np.concatenate([Ti, Tj]), np.arange(n), n + np.arange(n), Z)
    big = extent > 5.0
    se, sh = (np.abs(e).max(), np.abs(Hi).max() ** 2) if big else (1.0, 1.0)
    assert np.abs(got[:, :12] - e).max() < 1e-13 * se
    assert np.abs(got[:, 12:48] - np.einsum("fka,fkb->fab", Hi, Hi).reshape(n, 36)).max() < 1e-13 * sh
    assert np.abs(got[:, 48:84] - np.einsum("fka,fkb->fab", Hi, Hj).reshape(n, 36)).max() < 1e-13 * sh
    sg = np.abs(Hi).max() * se if big else 1.0
    assert np.abs(got[:, 84:90] + np.einsum("fka,fk->fa", Hi, e)).max() < 1e-13 * sg
    assert np.abs(got[:, 90:96] + np.einsum("fka,fk->fa", Hj, e)).max() < 1e-13 * sg
    assert np.abs(got[:, 96] - 0.5 * (e * e).sum(axis=1)).max() < 1e-13 * (se * se if big else 1e3)
    HjHj = np.einsum("fka,fkb->fab", Hj, Hj)
    assert np.abs(HjHj - np.diag([2.0, 2, 2, 1, 1, 1])).max() < 1e-13 and np.array_equal(got[:, 97:], np.tile([2.0, 2, 2, 1, 1, 1], (n, 1)))


@pytest.mark.parametrize("exe", ["plain", "sanitized"])
def test_pose_header_matches_restatement(factor_programs, exe):
    rng = np.random.default_rng(6)
    n = 64
    T = np.array([PC.pose(rng.normal(0, 1.0, 3), rng.uniform(-200, 200, 3)) for _ in range(n)])
    D = rng.normal(0, 1.0, (n, 6)) * 10.0 ** rng.uniform(-12, 0.5, (n, 1))
    D[0] = 0.0
    D[1, :3] = [0.99e-4 / np.sqrt(3)] * 3                        # either side of the series threshold
    D[2, :3] = [1.01e-4 / np.sqrt(3)] * 3
    D[3, :3] = [np.pi, 0, 0]
    # what stage 1 solves for: rotations shrunk and perturbed, some of them mirrored
    X = np.array([PC.rot(rng.normal(0, 1.5, 3)) * rng.uniform(0.6, 1.0) + rng.normal(0, 0.05, (3, 3)) for _ in range(n)])
    X[:8] = X[:8] @ np.diag([1.0, 1.0, -1.0])
    X[8] = PC.rot([0.3, 0.2, 0.1])                               # a rotation already: three equal singular values
    X[9] = np.eye(3)
    got = _run(factor_programs, exe, "pose", [np.array([n], np.int32), T, D, X.reshape(n, 9)], (n, 21))
    want_T = R.retract(T, D)[:, :3, :].reshape(n, 12)
    assert np.abs(got[:, :12].reshape(n, 3, 4)[:, :, :3] - want_T.reshape(n, 3, 4)[:, :, :3]).max() < 1e-13
    assert np.abs(got[:, :12] - want_T).max() < 1e-13 * 200
    want_R = np.array([R.closest_rotation(x) for x in X])
    assert np.abs(got[:, 12:].reshape(n, 3, 3) - want_R).max() < 1e-13
    assert np.abs(np.linalg.det(got[:, 12:].reshape(n, 3, 3)) - 1.0).max() < 1e-13


def test_pgo_symbols_exported_and_bound():
    from mr_slam_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = C.CDLL(_lib.LIB_PATH)
    names = ("mrs_pgo_create", "mrs_pgo_destroy", "mrs_pgo_set_odometry", "mrs_pgo_add_loops", "mrs_pgo_clear_loops", "mrs_pgo_count",
             "mrs_pgo_set_prior", "mrs_pgo_set_segment_length", "mrs_pgo_initialize", "mrs_pgo_optimize", "mrs_pgo_last_stage_ms")
    for n in names:
        assert hasattr(lib, n), n
    assert lib.mrs_abi_version() == 1
    api = _lib.load()
    h = C.c_void_p()
    one = np.ones(1, np.int32)
    for call in (lambda: api.mrs_pgo_create(None, 1, one, C.byref(h)), lambda: api.mrs_pgo_set_odometry(None, None, 0),
                 lambda: api.mrs_pgo_add_loops(None, None, None, None, 1), lambda: api.mrs_pgo_clear_loops(None),
                 lambda: api.mrs_pgo_count(None, None), lambda: api.mrs_pgo_set_prior(None, None),
                 lambda: api.mrs_pgo_set_segment_length(None, 0), lambda: api.mrs_pgo_initialize(None, None),
                 lambda: api.mrs_pgo_optimize(None, 1e-9, 200, None, None), lambda: api.mrs_pgo_last_stage_ms(None, None)):
        with pytest.raises(_lib.MrsError) as e:                  # the C side's null checks, no GPU involved
            call()
        assert e.value.status == 1 and "null pointer" in str(e.value)
    assert api.mrs_pgo_destroy(None) == 0
    with pytest.raises(TypeError, match="h_Z.*float32"):
        api.mrs_pgo_add_loops(None, None, None, np.zeros((1, 4, 4), np.float32), 1)
    from mr_slam_amd import posegraph
    assert (posegraph.MAX_CHAINS, posegraph.MAX_POSES, posegraph.MAX_LOOPS, posegraph.MAX_SEPARATORS) == (16, 65536, 8192, 1024)


def test_host_helpers():
    from mr_slam_amd import globalmap, pcm, posegraph
    rng = np.random.default_rng(8)
    X = PC.trajectory(rng, 12)
    odom = posegraph.odometry_from_trajectory(X)
    assert odom.shape == (11, 4, 4)
    back = pcm.chain_odometry(odom)                              # starts at the identity: X up to its first pose
    assert np.abs(X[0] @ back - X).max() < 1e-12
    assert posegraph.odometry_from_trajectory(X[:1]).shape == (0, 4, 4)
    assert np.abs(posegraph.between(X[2], X[5]) - PC.inv(X[2]) @ X[5]).max() < 1e-13
    assert np.abs(posegraph.between(X[:3], X[3:6])[1] - PC.inv(X[1]) @ X[4]).max() < 1e-13
    A, B = X[:4], X[4:8]
    got = posegraph.correction(A, B)
    assert got.dtype == np.float32 and got.shape == (4, 4, 4)
    for k in range(4):
        assert np.array_equal(got[k], globalmap.pose_product(A[k].astype(np.float32), B[k].astype(np.float32)))
    with pytest.raises(ValueError):
        posegraph.correction(A, X[:3])


def test_the_handle_is_created_and_destroyed_once(monkeypatch):
    """without the library: PoseGraph owns its C handle through a plain _lib.Handle, so the package's set of Handle subclasses stays as it is"""
    import gc
    from mr_slam_amd import _lib, posegraph
    calls = []

    class Fake:
        def __getattr__(self, name):
            def call(*args):
                calls.append((name, args))
                if name.endswith("_create"):
                    args[-1]._obj.value = 0x2000
                return 0
            return call

    monkeypatch.setattr(_lib, "load", lambda: Fake())
    monkeypatch.setattr(_lib, "ctx", lambda device=0: "ctx%d" % device)
    g = posegraph.PoseGraph([3, 2])
    assert calls[0][0] == "mrs_pgo_create" and calls[0][1][:2] == ("ctx0", 2) and calls[0][1][2].tolist() == [3, 2]
    assert g.n_poses == 5 and g._h.value == 0x2000 and not isinstance(g, _lib.Handle)
    assert not [c for c in _lib.Handle.__subclasses__() if c.__module__ == "mr_slam_amd.posegraph"]
    g.set_segment_length(7)
    assert calls[-1] == ("mrs_pgo_set_segment_length", (g._h, 7))
    h = g._h
    del g
    gc.collect()
    assert [n for n, _ in calls].count("mrs_pgo_destroy") == 1 and calls[-1] == ("mrs_pgo_destroy", (h,))
