"""GPU suite for per-factor noise, Levenberg-Marquardt step control and robust loop kernels of the pose-graph optimiser
(mr_slam_amd/posegraph.py over mrs_pgo_*): both optimisers against the restatement (tests/golden/posegraph_robust_restate.py) on every case
of posegraph_robust_cases.py and every segment length; the same bits from call to call, from a fresh handle and from appended loops; the
weighted instantiation with unit weights against the plain one; clearing noise and kernel; the refusals.

Observed against the restatement on an MI355X: see DESIGN.md 4.23(i)."""
import numpy as np
import pytest

import posegraph_cases as PC
import posegraph_robust_cases as RC

pytestmark = pytest.mark.gpu
RR = RC.RR
TOL = 1e-9


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    assert torch.cuda.is_available()        # PyTorch's runtime has to see the device before the library's does


def _add_loops(g, c, sel):
    """the loops `sel` in order, in runs of loops that carry a covariance and runs that do not"""
    s = c.scene
    sel = list(sel)
    a = 0
    while a < len(sel):
        has = c.lC is not None and c.lC[sel[a]] is not None
        b = a
        while b < len(sel) and (c.lC is not None and c.lC[sel[b]] is not None) == has:
            b += 1
        u = sel[a:b]
        g.add_loops(s.li[u], s.lj[u], s.lZ[u], np.array([c.lC[v] for v in u]) if has else None)
        a = b


def _graph(c, segment_length=None, loops=None, kernel=True):
    from mr_slam_amd import posegraph
    s = c.scene
    g = posegraph.PoseGraph(s.chain_lengths)
    g.set_odometry(s.odom)
    if c.oC is not None:
        g.set_odometry_noise(c.oC)
    _add_loops(g, c, range(s.li.size) if loops is None else loops)
    if s.prior is not None:
        g.set_prior(s.prior)
    if kernel and c.kernel != RR.NONE:
        g.set_loop_kernel(RC.KERNEL_NAMES[c.kernel], c.k)
    if segment_length is not None:
        g.set_segment_length(segment_length)
    return g


def _lm(g, c):
    return g.optimize(method="lm", max_iterations=c.max_solves or RR.MAX_SOLVES_DEFAULT)


def _same(a, b):
    return np.array_equal(a.T, b.T) and a[1:] == b[1:]


def _rel(a, b):
    return abs(a - b) / abs(b) if b else abs(a)


@pytest.mark.parametrize("name", RC.LM_NAMES)
def test_lm_matches_restatement(name):
    c, want = RC.case(name), RC.expected_lm(name)
    for L in PC.SEGMENT_LENGTHS:
        g = _graph(c, segment_length=L)
        got = _lm(g, c)
        w, r2 = g.loop_state()
        dR, dt = np.abs(got.T[:, :3, :3] - want.T[:, :3, :3]).max(), np.abs(got.T[:, :3, 3] - want.T[:, :3, 3]).max()
        rel = (_rel(got.cost_initial, want.cost_initial), _rel(got.cost_final, want.cost_final), _rel(got.lam, want.lam))
        dw = np.abs(w - want.weights).max() if w.size else 0.0
        dr2 = max((_rel(a, b) for a, b in zip(r2, want.r2)), default=0.0)
        print("lm %s L=%d: dR %.3g dt %.3g solves %d/%d accepted %d/%d costs rel %.3g %.3g lambda %.6g rel %.3g weights %.3g r2 rel %.3g separators %d"
              % (name, L, dR, dt, got.solves, want.solves, got.accepted, want.accepted, rel[0], rel[1], got.lam, rel[2], dw, dr2, got.separators))
        assert dR < TOL and dt < TOL
        assert (got.solves, got.accepted, got.converged) == (want.solves, want.accepted, want.converged)
        assert rel[0] < TOL and rel[1] < TOL and rel[2] < TOL
        assert dw < TOL and dr2 < TOL
        assert np.array_equal(got.T[:, 3], np.tile([0.0, 0, 0, 1], (got.T.shape[0], 1)))


@pytest.mark.parametrize("name", RC.GN_NAMES)
def test_weighted_gauss_newton_matches_restatement(name):
    c, want = RC.case(name), RC.expected_gn(name)
    for L in PC.SEGMENT_LENGTHS:
        g = _graph(c, segment_length=L)
        got = g.optimize()
        w, r2 = g.loop_state()
        dR, dt = np.abs(got.T[:, :3, :3] - want.T[:, :3, :3]).max(), np.abs(got.T[:, :3, 3] - want.T[:, :3, 3]).max()
        rel = (_rel(got.error_initial, want.error_initial), _rel(got.error_final, want.error_final))
        print("weighted gn %s L=%d: dR %.3g dt %.3g its %d/%d errors rel %.3g %.3g" % (name, L, dR, dt, got.iterations, want.iterations, rel[0], rel[1]))
        assert dR < TOL and dt < TOL and got.iterations == want.iterations and got.converged == want.converged
        assert rel[0] < TOL and rel[1] < TOL
        assert np.array_equal(w, np.ones(c.scene.li.size)) and r2.shape == w.shape and (r2 >= 0).all()


@pytest.mark.parametrize("name", ["mixed", "outliers_geman_mcclure"])
def test_same_bits_from_call_to_call_and_from_appended_loops(name):
    from mr_slam_amd import posegraph
    c = RC.case(name)
    g = _graph(c)
    a, sa = _lm(g, c), g.loop_state()
    b, sb = _lm(g, c), g.loop_state()
    assert _same(a, b) and np.array_equal(sa[0], sb[0]) and np.array_equal(sa[1], sb[1])
    fresh = _graph(c)
    assert _same(a, _lm(fresh, c)) and np.array_equal(fresh.loop_state()[1], sa[1])
    n = c.scene.li.size
    h = _graph(c, loops=range(0, 2))                             # the first two loops connect the three chains
    for lo, hi in ((2, n // 2), (n // 2, n)):
        _lm(h, c)
        _add_loops(h, c, range(lo, hi))
    assert len(h) == n and _same(_lm(h, c), a) and np.array_equal(h.loop_state()[0], sa[0])
    if "gn" in c.methods:
        assert _same(g.optimize(), _graph(c).optimize())


def test_unit_covariances_tie_the_weighted_path_to_the_plain_one():
    """C = diag(1, 1, 1, 0.99, 0.99, 0.99) on every factor: every weight is exactly 1, and the weighted instantiation ends within 1e-12 of
    the plain one, under both optimisers"""
    for name in ("quirks", "runs"):
        s = PC.scene(name)
        unit = RC.Case(name, s, np.tile(RC.UNIT_COVARIANCE, (s.odom.shape[0], 1, 1)), [RC.UNIT_COVARIANCE] * s.li.size, RR.NONE, 1.0, ("gn", "lm"))
        plain = RC.Case(name, s, None, None, RR.NONE, 1.0, ("gn", "lm"))
        for L in (3, 64):
            a, b = _graph(unit, segment_length=L).optimize(), _graph(plain, segment_length=L).optimize()
            print("unit weights %s L=%d gn: max |dT| %.3g" % (name, L, np.abs(a.T - b.T).max()))
            assert np.abs(a.T - b.T).max() < 1e-12 and a.iterations == b.iterations
            assert _rel(a.error_final, b.error_final) < 1e-12 and _rel(a.error_initial, b.error_initial) < 1e-12
            a, b = _graph(unit, segment_length=L).optimize(method="lm"), _graph(plain, segment_length=L).optimize(method="lm")
            print("unit weights %s L=%d lm: max |dT| %.3g" % (name, L, np.abs(a.T - b.T).max()))
            assert np.abs(a.T - b.T).max() < 1e-12 and (a.solves, a.accepted, a.converged) == (b.solves, b.accepted, b.converged)


def test_clearing_noise_and_kernel_restores_the_plain_path():
    s = PC.scene("quirks")
    plain = RC.Case("quirks", s, None, None, RR.NONE, 1.0, ("gn", "lm"))
    want_gn, want_lm = _graph(plain).optimize(), _graph(plain).optimize(method="lm")
    c = RC.case("roles")._replace(oC=RC._covs(21, s.odom.shape[0]), kernel=RR.CAUCHY, k=2.0)
    g = _graph(c)
    changed = g.optimize(method="lm")
    assert np.abs(changed.T - want_lm.T).max() > 1e-6
    g.set_odometry_noise(None)
    g.set_loop_kernel(None)
    g.clear()
    g.add_loops(s.li, s.lj, s.lZ)
    got_gn = g.optimize()
    assert np.array_equal(got_gn.T, want_gn.T) and got_gn[1:] == want_gn[1:]
    assert _same(g.optimize(method="lm"), want_lm)
    w, r2 = g.loop_state()
    assert np.array_equal(w, np.ones(s.li.size)) and (r2 > 0).all()


def test_kernel_needs_the_step_control():
    from mr_slam_amd import _lib
    c = RC.case("outliers_geman_mcclure")
    g = _graph(c)
    with pytest.raises(_lib.MrsError) as e:
        g.optimize()
    assert e.value.status == 1 and "mrs_pgo_optimize_lm" in str(e.value)
    assert _same(_lm(g, c), _lm(_graph(c), c))
    g.set_loop_kernel(None)
    assert g.optimize(max_iterations=3).iterations == 3          # full steps on this graph need not converge: only that the call runs


def test_noise_refusals_leave_the_graph_as_it_was():
    from mr_slam_amd import _lib
    c = RC.case("roles")
    s = c.scene
    g = _graph(c)
    want = g.optimize(method="lm")
    Z, ok = s.lZ[:1], RC._covs(30, 2)
    api, n_odo = _lib.load(), s.odom.shape[0]

    def refused(call):
        with pytest.raises(_lib.MrsError) as e:
            call()
        assert e.value.status == 1, str(e.value)
        assert len(g) == s.li.size and _same(g.optimize(method="lm"), want)

    def bad(edit):
        Cb = ok.copy()
        edit(Cb[1])
        return Cb

    def neg_rotation(Cm):
        Cm[:3, :3] = -np.eye(3)

    def indefinite(Cm):
        Cm[3:, 3:] = np.diag([1.0, -0.02, 1.0])

    def at(r, c_, v):
        def edit(Cm):
            Cm[r, c_] = v
        return edit

    for edit in (at(0, 0, np.nan), at(4, 5, np.inf), at(2, 4, np.nan), neg_rotation, indefinite, at(3, 3, -0.011)):
        refused(lambda: g.add_loops([3, 4], [9, 10], np.concatenate([Z, Z]), bad(edit)))     # the good one before it is not added either
        odo = RC._covs(31, n_odo)
        edit(odo[n_odo // 2])
        refused(lambda: g.set_odometry_noise(odo))
    zero_rotation = ok.copy()
    zero_rotation[0, :3, :3] = 0.0                               # max(C00, C11, C22) = 0: the reference would divide by DBL_MIN
    refused(lambda: g.add_loops([3, 4], [9, 10], np.concatenate([Z, Z]), zero_rotation))
    refused(lambda: api.mrs_pgo_set_odometry_noise(g._h, np.ascontiguousarray(RC._covs(32, n_odo - 1)), n_odo - 1))      # a wrong count
    refused(lambda: api.mrs_pgo_set_odometry_noise(g._h, None, 3))
    refused(lambda: g.add_loops([3], [3], Z, ok[:1]))
    refused(lambda: g.add_loops([3], [g.n_poses], Z, ok[:1]))
    for k in (0.0, -1.0, np.inf, np.nan):
        refused(lambda: g.set_loop_kernel("huber", k))
    refused(lambda: api.mrs_pgo_set_loop_kernel(g._h, 4, 1.0))
    refused(lambda: api.mrs_pgo_set_loop_kernel(g._h, -1, 1.0))
    refused(lambda: g.optimize(method="lm", eps=-1.0))
    refused(lambda: g.optimize(method="lm", max_iterations=0))
    w = np.zeros(2)
    refused(lambda: api.mrs_pgo_get_loop_state(g._h, w, w.copy(), 2))                        # capacity below the number of loops
    # a C whose translation block alone is singular is fine: the 0.01 I makes it positive definite
    flat = ok[:1].copy()
    flat[0, 3:, 3:] = 0.0
    g.add_loops([3], [9], (PC.inv(s.truth[3]) @ s.truth[9])[None], flat)
    assert len(g) == s.li.size + 1
    with pytest.raises(_lib.MrsError):                           # the graph changed: the loop state is that of no result
        g.loop_state()
    assert g.optimize(method="lm").converged
    with pytest.raises(ValueError):
        g.optimize(method="newton")
    with pytest.raises(ValueError):
        g.set_loop_kernel("tukey")
