"""CPU suite for per-factor noise, Levenberg-Marquardt step control and robust loop kernels of the pose-graph optimiser: the weighted and
robust arithmetic of posegraph_factor.hpp (compiled by g++ into a stand-alone program, plain and under the address and undefined-behaviour
sanitizers) agrees with the restatement (tests/golden/posegraph_robust_restate.py); the kernels' weights are the derivatives of their costs;
the reference's noise constants convert to what the reference's conversion gives; the new C-ABI symbols are exported and bound; and the
scenes of posegraph_robust_cases.py keep, on the restatement alone, the conditions the GPU suite relies on.

Scene conditions observed (restatement, sparse solve against two permuted dense solves): T agrees within 1.4e-12 on every case that runs
to convergence and within 1.5e-10 on the 20 bounded Huber solves, lambda bit for bit (5.4e-13 relative on the Huber case); `inconsistent`
takes 167 solves (166 accepted) where 200 full Gauss-Newton steps end at max|delta| = 3.3e-7."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import posegraph_cases as PC
import posegraph_robust_cases as RC
import test_posegraph_cpu as TC

R, RR = PC.R, RC.RR
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = (RR.HUBER, RR.CAUCHY, RR.GEMAN_MCCLURE)


@pytest.fixture(scope="module")
def robust_programs(tmp_path_factory):
    """the stand-alone program twice: as the kernels are compiled (no contraction), and under the address and undefined-behaviour sanitizers"""
    d = tmp_path_factory.mktemp("pgo_robust")
    base = ["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-I" + os.path.join(ROOT, "mr_slam_amd", "csrc"),
            os.path.join(ROOT, "tests", "cpp", "posegraph_robust_host.cpp")]
    subprocess.run(base + ["-O2", "-o", str(d / "plain")], check=True)
    subprocess.run(base + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(d / "sanitized")], check=True)
    return d


def _order_one_covariances(seed, n):
    """full covariances whose converted weights stay within 0.3 .. 3.3, so that the bounds of the unweighted header test carry over"""
    rng = np.random.default_rng(seed)
    out = np.empty((n, 6, 6))
    for k in range(n):
        Qr, _ = np.linalg.qr(rng.normal(0, 1, (3, 3)))
        Qt, _ = np.linalg.qr(rng.normal(0, 1, (3, 3)))
        Cc = np.zeros((6, 6))
        Cc[:3, :3] = Qr @ np.diag(rng.uniform(0.5, 2.0, 3)) @ Qr.T
        Cc[3:, 3:] = Qt @ np.diag(rng.uniform(0.3, 3.0, 3)) @ Qt.T
        Cc[:3, 3:] = rng.normal(0, 0.1, (3, 3))                  # ignored by the conversion
        Cc[3:, :3] = Cc[:3, 3:].T
        out[k] = 0.5 * (Cc + Cc.T)
    return out


@pytest.mark.parametrize("extent, reach", [(5.0, 3.0), (200.0, 30.0)])
@pytest.mark.parametrize("exe", ["plain", "sanitized"])
def test_weighted_header_matches_restatement(robust_programs, exe, extent, reach):
    """the bounds of test_factor_header_matches_restatement: 1e-13 where the quantities are of order one to a hundred, and the same bound
    relative to the size of each quantity at the extent of the scenes; the weights here are of order one (0.3 .. 3.3)"""
    Ti, Tj, Z = TC._factor_inputs(extent=extent, reach=reach)
    n = Ti.shape[0]
    Cv = _order_one_covariances(15, n)
    Tk = np.array([PC.pose(v, [0, 0, 0]) for v in np.random.default_rng(16).normal(0, 1.5, (n, 3))])      # rotations far from the identity
    got = TC._run(robust_programs, exe, "weighted", [np.array([n], np.int32), Ti, Tj, Z, Cv, Tk], (n, 107))
    Lam = np.array([RR.chordal_information(Cv[k], Tk[k, :3, :3]) for k in range(n)])
    idx = np.arange(n)
    T = np.concatenate([Ti, Tj])
    e, Hii, Hij, Hjj, gi, gj = RR.blocks(T, idx, n + idx, Z, Lam)
    _, Hi, _ = R._linearize(T, idx, n + idx, Z)
    big = extent > 5.0
    se, sh = (np.abs(e).max(), np.abs(Hi).max() ** 2) if big else (1.0, 1.0)
    lmax = np.abs(Lam).max()
    assert lmax < 3.4
    assert np.abs(got[:, 0] - Lam[:, 0, 0]).max() < 1e-13 and np.abs(got[:, 1:10].reshape(n, 3, 3) - Lam[:, 9:, 9:]).max() < 1e-13
    assert np.array_equal(got[:, 1:10].reshape(n, 3, 3), got[:, 1:10].reshape(n, 3, 3).transpose(0, 2, 1))
    assert np.abs(got[:, 11:23] - e).max() < 1e-13 * se
    assert np.abs(got[:, 10] - RR.squared_residuals(T, idx, n + idx, Z, Lam)).max() < 1e-13 * lmax * (se * se if big else 1e3)
    assert np.abs(got[:, 23:59] - Hii.reshape(n, 36)).max() < 1e-13 * lmax * sh
    assert np.abs(got[:, 59:95] - Hij.reshape(n, 36)).max() < 1e-13 * lmax * sh
    sg = np.abs(Hi).max() * se if big else 1.0
    assert np.abs(got[:, 95:101] - gi).max() < 1e-13 * lmax * sg
    assert np.abs(got[:, 101:107] - gj).max() < 1e-13 * lmax * sg
    # Hj^T L Hj is what the gather assumes: wr diag(2, 2, 2) and Lt
    want = np.zeros((n, 6, 6))
    want[:, :3, :3] = 2.0 * Lam[:, 0, 0, None, None] * np.eye(3)
    want[:, 3:, 3:] = Lam[:, 9:, 9:]
    assert np.abs(Hjj - want).max() < 1e-13 * lmax


@pytest.mark.parametrize("exe", ["plain", "sanitized"])
def test_unit_covariance_gives_the_unweighted_blocks(robust_programs, factor_programs, exe):
    """C = diag(1, 1, 1, 0.99, 0.99, 0.99): wr is exactly 1, P exactly I, and the weighted blocks are the unweighted header's within rounding"""
    Ti, Tj, Z = TC._factor_inputs(extent=5.0, reach=3.0)
    n = Ti.shape[0]
    Tk = np.array([PC.pose(v, [0, 0, 0]) for v in np.random.default_rng(17).normal(0, 1.5, (n, 3))])
    got = TC._run(robust_programs, exe, "weighted", [np.array([n], np.int32), Ti, Tj, Z, np.tile(RC.UNIT_COVARIANCE, (n, 1, 1)), Tk], (n, 107))
    plain = TC._run(factor_programs, exe, "factor", [np.array([n], np.int32), Ti, Tj, Z], (n, 103))
    assert np.array_equal(got[:, 0], np.ones(n)) and np.abs(got[:, 1:10] - np.eye(3).reshape(9)).max() < 1e-15
    assert np.array_equal(got[:, 11:23], plain[:, :12])
    assert np.abs(got[:, 23:95] - plain[:, 12:84]).max() < 1e-12 and np.abs(got[:, 95:107] - plain[:, 84:96]).max() < 1e-12
    assert np.abs(0.5 * got[:, 10] - plain[:, 96]).max() < 1e-12


factor_programs = TC.factor_programs


@pytest.mark.parametrize("kind", KINDS)
def test_kernel_weight_is_the_derivative_of_the_cost(robust_programs, kind):
    """w(r) r = d rho / d r by central differences, on the restatement and on the header (both executables)"""
    k = 1.345 if kind == RR.HUBER else 0.7
    r = np.concatenate([np.linspace(0.01, 0.95 * k, 12), np.linspace(1.05 * k, 40.0, 30)])      # Huber's kink at r = k is left out
    h = 1e-6
    slope = (RR.kernel_cost(kind, k, r + h) - RR.kernel_cost(kind, k, r - h)) / (2 * h)
    assert np.abs(RR.kernel_weight(kind, k, r) * r - slope).max() < 1e-8
    assert np.all(RR.kernel_weight(kind, k, r) <= 1.0) and abs(float(RR.kernel_weight(kind, k, 0.0)) - 1.0) < 1e-15
    assert abs(float(RR.kernel_cost(kind, k, 1e-4)) - 0.5e-8) < 1e-15          # rho ~ r^2 / 2 at small residuals
    n = r.size
    for exe in ("plain", "sanitized"):
        got = TC._run(robust_programs, exe, "kernel", [np.array([n], np.int32), np.full(n, float(kind)), np.full(n, k), r * r], (n, 2))
        assert np.abs(got[:, 0] - RR.kernel_weight(kind, k, r)).max() < 1e-14
        assert np.abs(got[:, 1] - RR.kernel_cost(kind, k, r)).max() < 1e-13 * max(1.0, float(RR.kernel_cost(kind, k, r).max()))
        lo = TC._run(robust_programs, exe, "kernel", [np.array([n], np.int32), np.full(n, float(kind)), np.full(n, k), (r - h) ** 2], (n, 2))
        hi = TC._run(robust_programs, exe, "kernel", [np.array([n], np.int32), np.full(n, float(kind)), np.full(n, k), (r + h) ** 2], (n, 2))
        assert np.abs(got[:, 0] * r - (hi[:, 1] - lo[:, 1]) / (2 * h)).max() < 1e-8
    none = TC._run(robust_programs, "plain", "kernel", [np.array([n], np.int32), np.zeros(n), np.full(n, k), r * r], (n, 2))
    assert np.array_equal(none[:, 0], np.ones(n)) and np.array_equal(none[:, 1], 0.5 * (r * r))


def test_reference_constants_convert_as_the_reference_converts_them(robust_programs):
    """loopNoise gives rotation weight 10 and translation information 50 Rhat Rhat^T, odometryNoise 1 and 1 / 1.01"""
    from mr_slam_amd import posegraph
    assert np.array_equal(posegraph.REFERENCE_LOOP_COVARIANCE, RC.REFERENCE_LOOP_COVARIANCE)
    assert np.array_equal(posegraph.REFERENCE_ODOMETRY_COVARIANCE, RC.REFERENCE_ODOMETRY_COVARIANCE)
    assert np.array_equal(RC.REFERENCE_LOOP_COVARIANCE, np.diag([0.1] * 3 + [0.01] * 3)) and np.array_equal(RC.REFERENCE_ODOMETRY_COVARIANCE, np.eye(6))
    Ti, Tj, Z = TC._factor_inputs(n=8, extent=5.0, reach=3.0)
    Tk = np.array([PC.pose(v, [0, 0, 0]) for v in np.random.default_rng(18).normal(0, 1.5, (8, 3))])
    for Cv, wr, wt in ((RC.REFERENCE_LOOP_COVARIANCE, 10.0, 50.0), (RC.REFERENCE_ODOMETRY_COVARIANCE, 1.0, 1.0 / 1.01)):
        for k in range(8):
            L = RR.chordal_information(Cv, Tk[k, :3, :3])
            assert np.abs(L[:9, :9] - wr * np.eye(9)).max() < 1e-14 * wr
            assert np.abs(L[9:, 9:] - wt * Tk[k, :3, :3] @ Tk[k, :3, :3].T).max() < 1e-13 * wt and not L[:9, 9:].any()
        got = TC._run(robust_programs, "plain", "weighted", [np.array([8], np.int32), Ti, Tj, Z, np.tile(Cv, (8, 1, 1)), Tk], (8, 107))
        assert np.abs(got[:, 0] - wr).max() < 1e-14 * wr
        assert np.abs(got[:, 1:10].reshape(8, 3, 3) - wt * Tk[:, :3, :3] @ Tk[:, :3, :3].transpose(0, 2, 1)).max() < 1e-13 * wt


def test_robust_symbols_exported_and_bound():
    from mr_slam_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = C.CDLL(_lib.LIB_PATH)
    for n in ("mrs_pgo_set_odometry_noise", "mrs_pgo_add_loops_noise", "mrs_pgo_set_loop_kernel", "mrs_pgo_optimize_lm", "mrs_pgo_get_loop_state"):
        assert hasattr(lib, n), n
    assert lib.mrs_abi_version() == 1
    api = _lib.load()
    for call in (lambda: api.mrs_pgo_set_odometry_noise(None, None, 0), lambda: api.mrs_pgo_add_loops_noise(None, None, None, None, None, 1),
                 lambda: api.mrs_pgo_set_loop_kernel(None, 1, 1.0), lambda: api.mrs_pgo_optimize_lm(None, 1e-9, 200, None, None),
                 lambda: api.mrs_pgo_get_loop_state(None, None, None, 0)):
        with pytest.raises(_lib.MrsError) as e:                  # the C side's null checks, no GPU involved
            call()
        assert e.value.status == 1 and "null pointer" in str(e.value)
    with pytest.raises(TypeError, match="h_C.*float32"):
        api.mrs_pgo_add_loops_noise(None, None, None, None, np.zeros((1, 6, 6), np.float32), 1)
    from mr_slam_amd import posegraph
    assert PC.header_int("MRS_PGO_LM_INFO_DOUBLES") == 8 and posegraph._INFO_LM == 8
    assert [posegraph.KERNELS[RC.KERNEL_NAMES[k]] for k in (RR.NONE,) + KINDS] == [RR.NONE, RR.HUBER, RR.CAUCHY, RR.GEMAN_MCCLURE]
    assert posegraph.ResultLM._fields == ("T", "solves", "accepted", "converged", "max_delta", "cost_initial", "cost_final", "separators", "lam")
    text = open(os.path.join(ROOT, "include", "mrslam_hip.h")).read()
    for name, value in (("LAMBDA_INITIAL", RR.LAMBDA_INITIAL), ("LAMBDA_MIN", RR.LAMBDA_MIN), ("LAMBDA_MAX", RR.LAMBDA_MAX), ("PRED_FLOOR", RR.PRED_FLOOR)):
        assert float(text.split("#define MRS_PGO_LM_%s " % name)[1].split()[0]) == value


@pytest.mark.parametrize("name", RC.LM_NAMES)
def test_lm_scene_conditions(name):
    """on the restatement alone.  Every accept / reject decision is a factor 10 away from flipping in pred / (1e-10 c) or is decided by a
    cost difference above 1e-12 c; no accepted step's max|delta| is within 2 % of eps; the restatement under two permuted dense solve
    orders agrees with the sparse one within 1e-10 on T and on lambda (relative), and in its solve and accept counts"""
    r = RC.expected_lm(name)
    if RC.case(name).max_solves is None:
        assert r.converged and r.solves < RR.MAX_SOLVES_DEFAULT, (r.solves, r.max_delta)
    else:                                                        # a fixed number of solves: see BOUNDED_SOLVES
        assert not r.converged and r.solves == RC.case(name).max_solves and r.accepted < r.solves
    for ratio, rel in RR.decision_margins(r.log):
        assert ratio < 0.1 or ratio > 10.0 or rel > 1e-12, (ratio, rel)
        assert ratio < 0.1 or rel > 1e-12, (ratio, rel)         # stricter: above the floor the cost difference itself must be resolved
    for s in r.log:
        assert not (s.accepted and RR.EPS_DEFAULT / 1.02 < s.max_delta < RR.EPS_DEFAULT * 1.02), s
    # an iterate that has not converged is known less well than a result: the bounded case agrees with itself within 1.5e-10 (1.3e-10 to
    # 3.1e-10 over k = 0.1 .. 10 and six seeds, whatever the kernel does), which is above the 1e-10 every other case keeps
    bound = 1e-10 if RC.case(name).max_solves is None else 2.5e-10
    for order in (7, 8):
        o = RC.expected_lm(name, order)
        assert (o.solves, o.accepted, o.converged) == (r.solves, r.accepted, r.converged)
        assert np.abs(o.T - r.T).max() < bound and abs(o.lam - r.lam) < 1e-10 * r.lam, (np.abs(o.T - r.T).max(), o.lam, r.lam)
        assert np.abs(o.weights - r.weights).max() < 1e-10
    assert np.abs(r.T[:, :3, 3]).max() < 300.0 and r.cost_final < r.cost_initial


@pytest.mark.parametrize("name", RC.GN_NAMES)
def test_gn_scene_conditions(name):
    """the conditions of test_scene_conditions_and_solve_order, for the weighted Gauss-Newton restatement"""
    r = RC.expected_gn(name)
    d = np.array(r.deltas)
    assert r.converged and r.iterations < 40, (r.iterations, r.deltas)
    assert not ((d > PC.EPS / 4) & (d < PC.EPS * 4)).any(), r.deltas
    o = RC.expected_gn(name, 7)
    assert o.iterations == r.iterations and np.abs(o.T - r.T).max() < 1e-11
    assert r.error_final < r.error_initial


def test_weighted_restatement_with_unit_information_is_the_plain_one():
    s = PC.scene("quirks")
    want = PC.expected("quirks")
    got = RR.gn_optimize(s.chain_lengths, s.odom, s.li, s.lj, s.lZ)
    assert got.iterations == want.iterations and np.abs(got.T - want.T).max() < 1e-11
    assert abs(got.error_final - want.error_final) < 1e-12 * want.error_final
    first = RC.expected_lm("quirks", None, 1)                    # solve 1 is the parent's Gauss-Newton step
    assert first.solves == 1 and first.accepted == 1 and np.abs(first.T - PC.expected("quirks", PC.EPS, 1).T).max() < 1e-11


def test_inconsistent_scene_needs_the_step_control():
    """full Gauss-Newton steps do not reach max|delta| < 1e-9 in 200 iterations; Levenberg-Marquardt does"""
    c = RC.case("inconsistent")
    plain = R.optimize(*RC._args(c), max_iterations=200)
    assert plain.iterations == 200 and not plain.converged and plain.max_delta > 1e-8
    lm = RC.expected_lm("inconsistent")
    assert lm.converged and lm.max_delta < 1e-9 and lm.solves < 200
    assert lm.cost_final < R.total_error(plain.T, *R.factors(*RC._args(c))) * (1 + 1e-9)


def test_outlier_scene_weights():
    """Geman-McClure (and Cauchy at k = 0.3, checked below) ends with every outlier below 0.1 and every inlier above 0.9, and within a metre of the truth where the same graph
    without a kernel is tens of metres off"""
    c = RC.case("outliers_geman_mcclure")
    r = RC.expected_lm("outliers_geman_mcclure")
    out = np.zeros(c.scene.li.size, bool)
    out[list(RC.OUTLIER_LOOPS)] = True
    assert (r.weights[out] < 0.1).all() and (r.weights[~out] > 0.9).all(), r.weights
    truth = np.array([PC.inv(c.scene.truth[0]) @ X for X in c.scene.truth])
    assert np.abs(r.T[:, :3, 3] - truth[:, :3, 3]).max() < 1.0
    r = RC.expected_lm("outliers_cauchy")
    assert (r.weights[out] < 0.1).all() and (r.weights[~out] > 0.9).all(), r.weights
