"""CPU suite for pairwise consistency with covariances: the NumPy restatement (tests/golden/pcm_cov_restate.py) has gtsam's
Jacobians, an additive and invertible SPAN chain and the reference's marginals; the arithmetic of the kernels (pcm_cov.hpp, compiled by g++
into a stand-alone program, and once more under the address and undefined-behaviour sanitizers) agrees with it within the measured
tolerance; the scenes keep the conditions the GPU suite relies on; the C-ABI symbols are exported and bound; the host helpers do what they
say."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pcm_cov_cases as CC

PC, R, RC = CC.PC, CC.R, CC.RC
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _exp(xi):
    """Pose3::Expmap: rotation by omega, translation V u (V = I without a rotation)"""
    w, u = xi[:3], xi[3:]
    th = np.linalg.norm(w)
    if th == 0.0:
        return PC.pose(w, u)
    W = RC.skew(w)
    V = np.eye(3) + (1 - np.cos(th)) / th ** 2 * W + (th - np.sin(th)) / th ** 3 * (W @ W)
    T = np.eye(4)
    T[:3, :3] = PC.rotation(w)
    T[:3, 3] = V @ u
    return T


def _numeric(f, a, b, which, h=1e-6):
    """central differences of Logmap(f(a, b)^-1 f(a', b')) with a' = a Exp(h e) (which = 0) or b' = b Exp(h e)"""
    base = f(a, b)
    J = np.empty((6, 6))
    for e in range(6):
        d = np.zeros(6)
        d[e] = h
        hi = f(a @ _exp(d), b) if which == 0 else f(a, b @ _exp(d))
        lo = f(a @ _exp(-d), b) if which == 0 else f(a, b @ _exp(-d))
        J[:, e] = (R.logmap(R.inverse(base) @ hi) - R.logmap(R.inverse(base) @ lo)) / (2 * h)
    return J


def test_jacobians_against_central_differences():
    rng = np.random.default_rng(11)
    for _ in range(5):
        a, b = PC.random_pose(rng, 5.0, 1.0), PC.random_pose(rng, 5.0, 1.0)
        Ha, Hb = RC.compose_jacobians(a, b)
        assert np.abs(Ha - _numeric(lambda x, y: x @ y, a, b, 0)).max() < 1e-7
        assert np.abs(Hb - _numeric(lambda x, y: x @ y, a, b, 1)).max() < 1e-7
        Ha, Hb = RC.between_jacobians(a, b)
        assert np.abs(Ha - _numeric(lambda x, y: R.inverse(x) @ y, a, b, 0)).max() < 1e-7
        assert np.abs(Hb - _numeric(lambda x, y: R.inverse(x) @ y, a, b, 1)).max() < 1e-7
        assert np.abs(RC.inverse_jacobian(a) - _numeric(lambda x, y: R.inverse(x), a, b, 0)).max() < 1e-7
    A = RC.adjoint(a)
    assert np.array_equal(A[:3, 3:], np.zeros((3, 3))) and np.array_equal(A[3:, :3], RC.skew(a[:3, 3]) @ a[:3, :3])
    assert np.abs(RC.adjoint(a @ b) - A @ RC.adjoint(b)).max() < 1e-12


def test_span_chain_is_additive_and_symmetric_under_inversion():
    XA, _, QA, _, _, _, _, _, _ = CC.scene(65)
    T = RC.Trajectory(RC.SPAN, XA, QA)
    for i, j, m in ((0, 7, 39), (3, 3, 20), (12, 30, 31)):
        rjm = R.inverse(XA[j]) @ XA[m]
        want = T.between(i, m)[1]
        got = RC.pose_compose(R.inverse(XA[i]) @ XA[j], T.between(i, j)[1], rjm, T.between(j, m)[1])[1]
        assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max(), (i, j, m)
    assert not T.between(5, 5)[1].any()
    for i, j in ((2, 9), (0, 39), (17, 18)):
        r, S = T.between(i, j)
        rb, Sb = T.between(j, i)
        assert np.array_equal(rb, R.inverse(XA[j]) @ XA[i])
        assert np.abs(Sb - RC.pose_inverse(r, S)[1]).max() <= 1e-14 * np.abs(S).max()
        back = RC.pose_inverse(rb, Sb)[1]                            # inverting twice returns the forward covariance
        assert np.abs(back - S).max() <= 1e-12 * np.abs(S).max()
        assert np.linalg.eigvalsh(Sb).min() > 0
    assert len(T.sweeps) <= 8                                       # one sweep per distinct start pose


def test_reference_mode_reproduces_the_chain_marginals():
    from mr_slam_amd import pcm
    rng = np.random.default_rng(4)
    odom = np.stack([PC.random_pose(rng, 1.0, 0.2) for _ in range(12)])
    X = pcm.chain_odometry(odom)
    fixed = RC.FIXED_COVARIANCE
    want = RC.chain_odometry_covariance(odom, None)
    T = RC.Trajectory(RC.REFERENCE, X, None, None)
    assert np.abs(T.M - want).max() <= 1e-12 * np.abs(want).max() and np.array_equal(T.M[0], fixed)
    got = pcm.chain_odometry_covariance(odom, None)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    Q = np.stack([CC.random_covariance(rng, 0.5, 2.0) for _ in range(12)])
    first = CC.random_covariance(rng, 0.5, 2.0)
    assert np.abs(pcm.chain_odometry_covariance(odom, Q, first) - RC.chain_odometry_covariance(odom, Q, first)).max() < 1e-15
    assert np.array_equal(pcm.FIXED_COVARIANCE, fixed) and pcm.chain_odometry_covariance(np.zeros((0, 4, 4)), None).shape == (1, 6, 6)
    # composeOnTrajectory -> poseBetween of two marginals
    r, S = T.between(2, 9)
    A = RC.adjoint(R.inverse(r))
    assert np.abs(S - (A @ T.M[2] @ A.T + T.M[9])).max() <= 1e-15
    with pytest.raises(ValueError):
        pcm.chain_odometry_covariance(odom, Q[:3])


def _build(tmp, flags, name):
    exe = tmp / name
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", *flags, "-I" + os.path.join(ROOT, "mr_slam_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "pcm_cov_host.cpp"), "-o", str(exe)], check=True)
    return exe


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("pcm_cov")
    return _build(d, [], "pcm_cov_host"), _build(d, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "pcm_cov_host_san"), d


def _run(exe, d, mode, parts, tag="x"):
    with open(d / ("in_%s.bin" % tag), "wb") as f:
        for p in parts:
            np.ascontiguousarray(p).tofile(f)
    subprocess.run([str(exe), mode, str(d / ("in_%s.bin" % tag)), str(d / ("out_%s.bin" % tag))], check=True, timeout=300)
    return np.fromfile(d / ("out_%s.bin" % tag), np.float64)


def _pairs(exe, d, sc, mode, first=None):
    """(XI [P, 6], SE [P, 6, 6], d2 [P]) of the host build for every pair u < v in row-major order"""
    XA, XB, QA, QB, ia, kb, Z, Cv, _ = sc
    head = np.array([RC.MODES[mode], XA.shape[0], XB.shape[0], len(ia)], np.int32)
    first = RC.FIXED_COVARIANCE if first is None else first
    out = _run(exe, d, "pairs", [head, XA, XB, QA, QB, first, ia, kb, Z, Cv]).reshape(-1, 43)
    return out[:, :6], out[:, 6:42].reshape(-1, 6, 6), out[:, 42]


def _deviation(got, want, L):
    """(largest |xi| difference, largest relative deviation of Sigma_E, of d2) of a host run from the restatement"""
    XI, SE, d2 = got
    D, WXI, WSE = want
    u, v = np.triu_indices(L, 1)
    return np.abs(XI - WXI[u, v]).max(), CC.rel_sigma(SE, WSE[u, v]).max(), CC.rel_d(d2, D[u, v]).max()


@pytest.fixture(scope="module")
def host_results(programs):
    """the host build's pairs of every scene and mode, computed once"""
    exe, _, d = programs
    return {(L, mode): _pairs(exe, d, CC.scene(L), mode) for L in CC.SIZES if L > 1 for mode in CC.MODES}


def test_header_matches_restatement_within_the_measured_tolerance(host_results, capsys):
    """MEASURED_REL is what this test measures; TOL_REL = 4 x that is what the GPU suite allows"""
    worst_xi = worst_s = worst_d = 0.0
    for (L, mode), got in host_results.items():
        dxi, ds, dd = _deviation(got, CC.expected(L, mode), L)
        worst_xi, worst_s, worst_d = max(worst_xi, dxi), max(worst_s, ds), max(worst_d, dd)
        assert np.array_equal(got[1], np.swapaxes(got[1], -1, -2)), (L, mode)             # symmetric by construction
    with capsys.disabled():
        print("\npcm_cov host build vs direct chain: xi %.3g, Sigma_E %.3g, d2 %.3g (relative)" % (worst_xi, worst_s, worst_d))
    assert worst_xi < CC.XI_TOL
    assert max(worst_s, worst_d) <= CC.MEASURED_REL
    assert CC.TOL_REL == 4 * CC.MEASURED_REL and CC.MARGIN_REL == 10 * CC.TOL_REL


def test_header_under_sanitizers(programs, host_results):
    """the same program built with -fsanitize=address,undefined returns the same bytes and reports nothing"""
    _, san, d = programs
    for L, mode in ((65, "span"), (65, "reference")):
        got = _pairs(san, d, CC.scene(L), mode)
        for a, b in zip(got, host_results[(L, mode)]):
            assert np.array_equal(a, b)                              # no contraction in either build: the same arithmetic


def test_long_scene_cancellation_tolerance_and_skip_cap(programs, capsys):
    exe, _, d = programs
    sc = CC.long_scene()
    D, XI, SE = CC.expected_long()
    L = 33
    got = _pairs(exe, d, sc, "span")
    dxi, ds, dd = _deviation(got, (D, XI, SE), L)
    with capsys.disabled():
        print("\npcm_cov long scene: xi %.3g, Sigma_E %.3g, d2 %.3g (relative)" % (dxi, ds, dd))
    assert max(ds, dd) <= CC.LONG_MEASURED_REL and CC.LONG_TOL_REL == 4 * CC.LONG_MEASURED_REL
    skipped = CC.in_margin(D, CC.THRESHOLDS, CC.LONG_MARGIN_REL).sum() / (L * (L - 1))
    assert skipped <= CC.LONG_SKIP_CAP
    assert np.isfinite(D).all() and np.linalg.norm(XI[..., :3], axis=-1).max() < 3.0


@pytest.mark.parametrize("mode", CC.MODES)
def test_scene_conditions(mode):
    """what the GPU suite relies on: finite distances, cycle rotations below 3 rad, both kinds of pairs from 63 loops on, and no d2 within
    MARGIN_REL x threshold of a threshold"""
    for L in CC.SIZES:
        D, XI, SE = CC.expected(L, mode)
        assert np.isfinite(D).all() and np.array_equal(D, D.T) and not D.diagonal().any()
        assert np.linalg.norm(XI[..., :3], axis=-1).max() < 3.0
        assert not CC.in_margin(D, CC.THRESHOLDS, CC.MARGIN_REL).any(), L
        if L >= 63:
            off = ~np.eye(L, dtype=bool)
            for t in CC.THRESHOLDS:
                A = RC.consistency_matrix(D, t)
                assert 10 < A.sum() < off.sum() - 10, (L, t)
    D, _, _ = CC.expected_special(mode)
    assert np.isfinite(D).all() and not CC.in_margin(D, CC.THRESHOLDS, CC.MARGIN_REL).any()


def test_special_scene_takes_the_edges():
    XA, XB, QA, QB, ia, kb, Z, Cv, _ = CC.special_scene()
    n = XA.shape[0]
    assert ia[1] == ia[2] and kb[1] == kb[2] and ia[4] > ia[5] and kb[4] < kb[5]
    assert (ia[0], kb[0], ia[3], kb[3]) == (0, 0, n - 1, n - 1)
    D, XI, SE = CC.expected_special("span")
    # zero spans: Sigma_E is the two loop covariances alone, C_v + Ad(E^-1) C_u Ad(E^-1)^T
    E = R.inverse(Z[1]) @ Z[2]
    A = RC.adjoint(R.inverse(E))
    assert np.abs(SE[1, 2] - (Cv[2] + A @ Cv[1] @ A.T)).max() <= 1e-15


def test_span_clique_has_no_outlier_and_differs_from_the_plain_test():
    """the end-to-end scene of the GPU suite: under SPAN with chi2_upper(0.99) the heuristic's clique holds inliers only; the reference's
    plain test with its 0.872 on the same scene returns another clique"""
    XA, XB, QA, QB, ia, kb, Z, Cv, inlier = CC.scene(129)
    D, _, _ = CC.expected(129, "span")
    size, members = R.max_clique_heu(RC.consistency_matrix(D, 16.812))
    assert size >= 10 and inlier[members].all()
    plain = R.consistency_distances(XA, XB, ia, kb, Z)
    psize, pmembers = R.max_clique_heu(R.consistency_matrix(plain, 0.872))
    assert sorted(pmembers) != sorted(members)


def test_restatement_nan_and_non_pd():
    XA, XB, QA, QB, ia, kb, Z, Cv, _ = CC.scene(2)
    Zb = Z.copy()
    Zb[1, 0, 3] = np.nan
    D, _, _ = RC.evaluate("span", XA, XB, ia, kb, Zb, Cv, QA, QB)
    assert np.isnan(D[0, 1]) and not RC.consistency_matrix(D, 16.812).any()
    assert np.isnan(RC.mahalanobis2(np.ones(6), -np.eye(6))) and np.isnan(RC.mahalanobis2(np.ones(6), np.zeros((6, 6))))
    assert RC.mahalanobis2(np.full(6, 2.0), 4 * np.eye(6)) == 6.0


def test_header_positive_definite_check(programs):
    exe, _, d = programs
    rng = np.random.default_rng(3)
    good = CC.random_covariance(rng, 1, 1)
    upper_junk = good.copy()
    upper_junk[0, 5] = np.nan                                      # only the lower triangle is read
    cases = [good, upper_junk, np.zeros((6, 6)), -good, np.diag([1, 1, 1, 1, 1, 0.0]), np.diag([1, 1, -1e-300, 1, 1, 1.0])]
    bad = good.copy()
    bad[4, 2] = np.nan
    cases.append(bad)
    bad = good.copy()
    bad[5, 5] = np.inf
    cases.append(bad)
    indef = np.eye(6)
    indef[1, 0] = 2.0
    cases.append(indef)
    got = _run(exe, d, "pd", [np.array([len(cases)], np.int32), np.stack(cases)], "pd")
    assert got.tolist() == [1, 1, 0, 0, 0, 0, 0, 0, 0]


def test_pcm_cov_symbols_exported_and_bound():
    from mr_slam_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = C.CDLL(_lib.LIB_PATH)
    names = ("mrs_pcm_set_covariances", "mrs_pcm_add_loops_cov", "mrs_pcm_get_pair")
    api = _lib.load()
    for n in names:
        assert hasattr(lib, n) and callable(getattr(api, n)), n
    text = open(_lib.HEADER).read()
    for k, v in (("NONE", 0), ("SPAN", 1), ("REFERENCE", 2)):
        assert "#define MRS_PCM_COV_%s %d" % (k, v) in text
    from mr_slam_amd import pcm
    assert pcm.COV_MODES == {"none": 0, "span": 1, "reference": 2}
    for call in (lambda: api.mrs_pcm_set_covariances(None, 1, None, None, None), lambda: api.mrs_pcm_add_loops_cov(None, None, None, None, None, 1),
                 lambda: api.mrs_pcm_get_pair(None, 0, 1, None, None, None)):
        with pytest.raises(_lib.MrsError) as e:                  # the C side's null checks, no GPU involved
            call()
        assert e.value.status == 1 and "null pointer" in str(e.value)
    with pytest.raises(TypeError, match="h_C.*float32"):
        api.mrs_pcm_add_loops_cov(None, None, None, None, np.zeros((1, 6, 6), np.float32), 1)


def test_chi2_upper():
    from mr_slam_amd import pcm
    qs = (0.90, 0.95, 0.99, 0.999)
    assert [pcm.chi2_upper(q) for q in qs] == [10.645, 12.592, 16.812, 22.458]
    assert {q: pcm.chi2_upper(q) for q in RC.CHI2_UPPER} == RC.CHI2_UPPER
    for q in (0.0, 0.5, 0.991, 1.0, 0.01):
        with pytest.raises(ValueError):
            pcm.chi2_upper(q)
    try:
        from scipy.stats import chi2
    except ImportError:
        return
    for q in qs:
        assert abs(chi2.ppf(q, 6) - pcm.chi2_upper(q)) < 5e-4
