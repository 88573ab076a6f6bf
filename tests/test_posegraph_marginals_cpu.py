"""CPU suite for the pose-graph optimiser's marginal covariances: the restatement
(tests/golden/posegraph_marginals_restate.py) against itself (two exact routes to the inverse, H Sigma = I, the Pose3 frame and the
covariance of a relative pose against numerical Jacobians); the backward segment walk of mr_slam_amd/csrc/posegraph_marginal.hpp, compiled
by g++ into a stand-alone program and once more under the address and undefined-behaviour sanitizers, against the restatement's blocks on
every case and segment length; the host function between_covariance; the new C-ABI symbols exported and bound."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import posegraph_cases as PC
import posegraph_marginals_cases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MR, R = MC.MR, MC.R
EPS = np.finfo(np.float64).eps
SYMBOLS = ("mrs_pgo_mark_poses", "mrs_pgo_compute_marginals", "mrs_pgo_get_marginals", "mrs_pgo_get_joint_marginals", "mrs_pgo_last_marginal_ms")


@pytest.mark.parametrize("name", MC.NAMES)
def test_two_routes_agree_and_invert(name):
    """the spread is what the bound of the GPU comparison is made of, so it has to be small itself: on the unit-model scenes at most the
    5e-11 the bounds were planned with (a bound of 5e-9 at most).  H Sigma = I in the same measure, max |H Sigma - I| / max |I|, for both
    routes: the residual of a backward-stable inverse is bounded by a modest multiple of eps cond(H); cond_1 = |H|_1 |Sigma|_1 is taken as
    that bound with the multiple at 1 (observed: a factor 100 and more below it)."""
    H, a, b = MC.routes(name)
    s = MC.two_route_spread(name)
    k1 = np.linalg.norm(H, 1) * np.linalg.norm(a, 1)
    ra, rb = MR.spread(H @ a, np.eye(H.shape[0])), MR.spread(H @ b, np.eye(H.shape[0]))
    print("%s: order %d two-route spread %.3g bound %.3g  |H S - I| %.3g %.3g  eps cond_1 %.3g" % (name, H.shape[0], s, MC.bound(name), ra, rb, EPS * k1))
    assert np.isfinite(s) and MC.bound(name) == MC.FACTOR * max(s, MC.SPREAD_FLOOR)
    if name in MC.PLAIN_NAMES:
        assert s <= 5e-11
    assert ra <= EPS * k1 and rb <= EPS * k1
    assert np.linalg.eigvalsh(0.5 * (a + a.T)).min() > 0


def _log_so3(Rm):
    c = np.clip(0.5 * (np.trace(Rm) - 1.0), -1.0, 1.0)
    t = np.arccos(c)
    v = 0.5 * np.array([Rm[2, 1] - Rm[1, 2], Rm[0, 2] - Rm[2, 0], Rm[1, 0] - Rm[0, 1]])
    return v if t < 1e-7 else v * t / np.sin(t)


def _local_pose3(T, Tn):
    """Pose3 local coordinates of Tn at T to first order: (Log(R^T Rn), R^T (tn - t))"""
    return np.concatenate([_log_so3(T[:3, :3].T @ Tn[:3, :3]), T[:3, :3].T @ (Tn[:3, 3] - T[:3, 3])])


def _retract_pose3(T, xi):
    """the first-order Pose3 retraction: R Exp(xi[:3]), t + R xi[3:]"""
    out = T.copy()
    out[:3, :3] = T[:3, :3] @ R.exp_so3(xi[:3])
    out[:3, 3] = T[:3, 3] + T[:3, :3] @ xi[3:]
    return out


def _central(f, n, h=1e-5):
    cols = []
    for k in range(n):
        d = np.zeros(n)
        d[k] = h
        cols.append((f(d) - f(-d)) / (2 * h))
    return np.array(cols).T


def test_pose3_frame_is_the_jacobian_of_the_local_coordinates():
    """M = blockdiag(I, R^T) per pose against central differences of the Pose3 local coordinates of the optimiser's retraction
    (R Exp(d[:3]), t + d[3:]); the truncation of a step of 1e-5 is 1e-10"""
    s = PC.scene("r3x2")
    T = s.truth
    M = MR.frame_matrix(T)
    for p in range(T.shape[0]):
        J = _central(lambda d: _local_pose3(T[p], R.retract(T[p:p + 1], d[None])[0]), 6)
        assert np.abs(J - M[6 * p:6 * p + 6, 6 * p:6 * p + 6]).max() < 1e-8
    S = np.cov(np.random.default_rng(5).normal(size=(6 * T.shape[0], 200)))
    assert np.array_equal(MR.in_frame(S, T, MR.CHORDAL), S)
    assert np.allclose(MR.in_frame(S, T, MR.POSE3), M @ S @ M.T, rtol=0, atol=1e-15)
    assert np.array_equal(MR.marginals(S)[3], S[18:24, 18:24]) and np.array_equal(MR.joint(S, 4, 1)[:6, 6:], S[24:30, 6:12])


def test_between_covariance_against_central_differences():
    """J = [-Ad(Z^-1), I] against central differences of the local coordinates of Z = Ti^-1 Tj under Pose3 perturbations of both poses,
    for the restatement and for the package's host function"""
    from mr_slam_amd import posegraph
    rng = np.random.default_rng(11)
    for _ in range(4):
        Ti, Tj = PC.pose(rng.normal(0, 1, 3), rng.normal(0, 5, 3)), PC.pose(rng.normal(0, 1, 3), rng.normal(0, 5, 3))
        Z = PC.inv(Ti) @ Tj
        J = _central(lambda d: _local_pose3(Z, PC.inv(_retract_pose3(Ti, d[:6])) @ _retract_pose3(Tj, d[6:])), 12)
        A = rng.normal(size=(12, 12))
        S = A @ A.T
        want = J @ S @ J.T
        for got in (MR.between_covariance(S, Ti, Tj), posegraph.between_covariance(S, Ti, Tj)):
            assert got.shape == (6, 6) and MR.spread(got, want) < 1e-8
            assert np.abs(got - got.T).max() <= 1e-12 * np.abs(got).max()
    with pytest.raises(ValueError):
        posegraph.between_covariance(np.eye(6), Ti, Tj)


@pytest.fixture(scope="module")
def walk_programs(tmp_path_factory):
    """the stand-alone program twice: plain, and under the address and undefined-behaviour sanitizers"""
    d = tmp_path_factory.mktemp("pgo_marginal")
    base = ["g++", "-std=c++17", "-Wall", "-ffp-contract=off", "-I" + os.path.join(ROOT, "mr_slam_amd", "csrc"),
            os.path.join(ROOT, "tests", "cpp", "posegraph_marginal_host.cpp")]
    subprocess.run(base + ["-O2", "-o", str(d / "plain")], check=True)
    subprocess.run(base + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(d / "sanitized")], check=True)
    return d


def _block(S, p, q):
    return S[6 * p:6 * p + 6, 6 * q:6 * q + 6]


@pytest.mark.parametrize("exe", ["plain", "sanitized"])
@pytest.mark.parametrize("name", MC.NAMES)
def test_header_walk_equals_restatement(walk_programs, name, exe):
    """every segment of the case at every segment length (and once with three marked poses), walked by the header from the restatement's
    blocks at the bounding separators: the diagonal and the successor blocks of every pose a segment holds, within the case's bound"""
    c = MC.case(name)
    s = c.scene
    H, Sig, _ = MC.routes(name)
    H, Sig = MR.with_held_pose(H), MR.with_held_pose(Sig)
    N = H.shape[0] // 6
    ends = np.cumsum(s.chain_lengths) - 1
    Hpp = np.array([_block(H, p, p) for p in range(N)])
    Hpn = np.array([_block(H, p, p + 1) if p not in ends else np.zeros((6, 6)) for p in range(N)])
    zero = np.zeros((6, 6))
    marked = [p for p in (N // 3, N // 2, N - 2) if 0 < p < N]
    problems = [(L, ()) for L in MC.SEGMENT_LENGTHS] + [(0, marked)]
    fin, fout = walk_programs / ("in_%s_%s.bin" % (name, exe)), walk_programs / ("out_%s_%s.bin" % (name, exe))
    segs = []
    with open(fin, "wb") as f:
        for L, marks in problems:
            is_sep = MR.separators(s.chain_lengths, s.li, s.lj, L, marks)
            sg = MR.segments(s.chain_lengths, is_sep)
            segs.append((is_sep, sg))
            np.array([N, len(sg)], np.int32).tofile(f)
            Hpp.tofile(f)
            Hpn.tofile(f)
            for first, m, left, right in sg:
                np.array([first, m, left >= 0, right >= 0], np.int32).tofile(f)
                for a, b in ((left, left), (right, left), (right, right)):
                    np.ascontiguousarray(zero if a < 0 or b < 0 else _block(Sig, a, b)).tofile(f)
    r = subprocess.run([str(walk_programs / exe), str(fin), str(fout)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "FAILED" not in r.stdout, r.stdout + r.stderr
    got = np.fromfile(fout, np.float64).reshape(len(problems), 2, N, 6, 6)
    os.remove(fin)
    os.remove(fout)
    scale, worst = np.abs(Sig).max(), 0.0
    for (L, marks), (is_sep, sg), g in zip(problems, segs, got):
        held = np.zeros(N, bool)
        for first, m, left, right in sg:
            held[first:first + m] = True
            for p in range(first - (left >= 0), first + m):
                if p not in ends and (p + 1 < first + m or right >= 0):
                    worst = max(worst, np.abs(g[1, p] - _block(Sig, p, p + 1)).max() / scale)
        assert np.array_equal(held, ~is_sep)
        for p in np.flatnonzero(held):
            worst = max(worst, np.abs(g[0, p] - _block(Sig, p, p)).max() / scale)
            assert np.array_equal(g[0, p], g[0, p].T)
        assert not g[0][~held].any()
    print("%s (%s): header walk against the restatement %.3g, bound %.3g" % (name, exe, worst, MC.bound(name)))
    assert worst <= MC.bound(name)


def test_tile_scenes_straddle_the_tile():
    tile = PC.header_int("MRS_PGO_MARGINAL_TILE")
    counts = MC.tile_separator_counts()
    assert tile == 32 and counts == [5, 6, 10, 11]
    for w in (1, 2):
        assert any(6 * e < w * tile for e in counts) and any(w * tile < 6 * e <= w * tile + 6 for e in counts)
    for e in counts:
        c = MC.case("panel_E%d" % e)
        assert int(MR.separators(c.scene.chain_lengths, c.scene.li, c.scene.lj, 0).sum()) - 1 == e


def test_marginal_prototypes_parse_and_symbols_exported():
    from mr_slam_amd import _lib
    protos = _lib.parse_header(_lib.HEADER)
    assert protos["mrs_pgo_mark_poses"] == ("int", [("mrs_pgo", 1, "pgo"), ("int32_t", 1, "h_poses"), ("int32_t", 0, "n")])
    assert protos["mrs_pgo_compute_marginals"] == ("int", [("mrs_pgo", 1, "pgo"), ("int64_t", 1, "h_info")])
    assert protos["mrs_pgo_get_marginals"][1][1:] == [("int32_t", 1, "h_poses"), ("int32_t", 0, "n"), ("int32_t", 0, "frame"), ("double", 1, "h_cov")]
    assert [p[2] for p in protos["mrs_pgo_get_joint_marginals"][1]] == ["pgo", "h_i", "h_j", "n", "frame", "h_cov"]
    assert (_lib.header_int("MRS_PGO_FRAME_CHORDAL"), _lib.header_int("MRS_PGO_FRAME_POSE3"), _lib.header_int("MRS_PGO_MARGINAL_INFO")) == (0, 1, 4)
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = C.CDLL(_lib.LIB_PATH)
    for n in SYMBOLS:
        assert hasattr(lib, n), n
    assert lib.mrs_abi_version() == 1
    api = _lib.load()
    cov = np.zeros((1, 6, 6))
    for call in (lambda: api.mrs_pgo_mark_poses(None, None, 0), lambda: api.mrs_pgo_compute_marginals(None, None),
                 lambda: api.mrs_pgo_get_marginals(None, None, 1, 0, cov), lambda: api.mrs_pgo_last_marginal_ms(None, None),
                 lambda: api.mrs_pgo_get_joint_marginals(None, np.zeros(1, np.int32), np.ones(1, np.int32), 1, 0, np.zeros((1, 12, 12)))):
        with pytest.raises(_lib.MrsError) as e:                  # the C side's null checks, no GPU involved
            call()
        assert e.value.status == 1 and "null pointer" in str(e.value)
    with pytest.raises(TypeError, match="h_info.*int32"):
        api.mrs_pgo_compute_marginals(None, np.zeros(4, np.int32))
    from mr_slam_amd import posegraph
    assert posegraph.FRAMES == {"chordal": 0, "pose3": 1} and posegraph.MarginalInfo._fields == ("separators", "order", "bytes")


def test_python_layer_passes_its_arguments(monkeypatch):
    """without the library: what the Python layer hands to the C ABI"""
    from mr_slam_amd import _lib, posegraph
    calls = []

    class Fake:
        def __getattr__(self, name):
            def call(*args):
                calls.append((name, args))
                if name.endswith("_create"):
                    args[-1]._obj.value = 0x2000
                if name == "mrs_pgo_compute_marginals":
                    args[1][:] = [7, 42, 1234, 0]
                return 0
            return call

    monkeypatch.setattr(_lib, "load", lambda: Fake())
    monkeypatch.setattr(_lib, "ctx", lambda device=0: "ctx%d" % device)
    g = posegraph.PoseGraph([3, 2])
    g.mark_poses([4, 1])
    assert calls[-1][0] == "mrs_pgo_mark_poses" and calls[-1][1][1].tolist() == [4, 1] and calls[-1][1][2] == 2
    g.mark_poses(None)
    assert calls[-1] == ("mrs_pgo_mark_poses", (g._h, None, 0))
    assert g.marginal_info() == posegraph.MarginalInfo(7, 42, 1234)
    m = g.marginals(frame="pose3")
    assert [c[0] for c in calls[-2:]] == ["mrs_pgo_compute_marginals", "mrs_pgo_get_marginals"]
    assert calls[-1][1][1:4] == (None, 5, 1) and m.shape == (5, 6, 6)
    m = g.marginals([2, 3, 3])
    assert calls[-1][1][1].tolist() == [2, 3, 3] and calls[-1][1][2:4] == (3, 0) and m.shape == (3, 6, 6)
    j = g.joint_marginals([0, 1], [4, 2], frame="pose3")
    assert calls[-1][0] == "mrs_pgo_get_joint_marginals" and calls[-1][1][3:5] == (2, 1) and j.shape == (2, 12, 12)
    with pytest.raises(ValueError):
        g.marginals(frame="world")
    with pytest.raises(ValueError):
        g.joint_marginals([0, 1], [2])
