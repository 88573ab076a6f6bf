"""GPU suite for the sparse elimination tier of the pose-graph optimiser (PoseGraph.set_solver("sparse") over mrs_pgo_set_solver): both stages
against the NumPy / scipy restatement on every scene and segment length with everything, or all but four separators, eliminated by the
tier; a graph of 1149 separators, which the dense solver refuses; the same bits from call to call, from a fresh handle, from appended
loops, across solver changes, and the dense solver's own bits where nothing is eliminated; Levenberg-Marquardt with covariances and a
kernel through the tier; the refusals; a failed pivot of a sparse column as a status.

Observed against the restatement on an MI355X: see DESIGN.md 4.23(j)."""
import numpy as np
import pytest

import posegraph_cases as PC
import posegraph_robust_cases as RC
import posegraph_sparse_cases as SC
from test_posegraph_gpu import ALL, TOL, _graph, _same, _scene

pytestmark = pytest.mark.gpu
OR = SC.OR
LIMITS = (0, 4)


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    assert torch.cuda.is_available()        # PyTorch's runtime has to see the device before the library's does


def _sparse(s, dense_limit=None, segment_length=None, **kw):
    g = _graph(s, segment_length=segment_length, **kw)
    g.set_solver("sparse", dense_limit=dense_limit)
    return g


def _stats_of(name, L, stage, limit):
    return tuple(OR.stats(SC.order(name, L, stage, limit))) + ("sparse",)


@pytest.mark.parametrize("limit", LIMITS)
@pytest.mark.parametrize("name", ALL)
def test_stage1_rotations(name, limit):
    want, _ = PC.expected_initial(name)
    s = _scene(name)
    worst = 0.0
    for L in PC.SEGMENT_LENGTHS:
        g = _sparse(s, limit, L)
        T = g.initialize()
        worst = max(worst, np.abs(T - want).max())
        assert tuple(g.solver_stats(1)) == _stats_of(name, L, 1, limit)
        assert not T[:, :3, 3].any() and np.array_equal(T[:, 3], np.tile([0.0, 0, 0, 1], (T.shape[0], 1)))
    print("stage 1 %s dense_limit %d: max |R - restatement| = %.3g" % (name, limit, worst))
    assert worst < TOL


@pytest.mark.parametrize("limit", LIMITS)
@pytest.mark.parametrize("name", ALL)
def test_optimize_matches_restatement(name, limit):
    want = PC.expected(name)
    s = _scene(name)
    for L in PC.SEGMENT_LENGTHS:
        g = _sparse(s, limit, L)
        got = g.optimize()
        st = g.solver_stats()
        dR, dt = np.abs(got.T[:, :3, :3] - want.T[:, :3, :3]).max(), np.abs(got.T[:, :3, 3] - want.T[:, :3, 3]).max()
        rel = [abs(a - b) / max(abs(b), 1e-300) if b else abs(a) for a, b in ((got.error_initial, want.error_initial), (got.error_final, want.error_final))]
        print("optimize %s L=%d dense_limit %d: dR %.3g dt %.3g its %d/%d errors rel %.3g %.3g separators %d eliminated %d levels %d"
              % (name, L, limit, dR, dt, got.iterations, want.iterations, rel[0], rel[1], got.separators, st.eliminated, st.levels))
        assert tuple(st) == _stats_of(name, L, 2, limit) and st.separators == got.separators and st.core == min(limit, got.separators)
        assert dR < TOL and dt < TOL
        assert got.iterations == want.iterations and got.converged == want.converged
        if want.error_final > 1e-18:
            assert rel[0] < TOL and rel[1] < TOL
        else:                                                    # a pure chain: both ends are rounding
            assert got.error_final <= 1e-18
            assert rel[0] < TOL or want.error_initial == 0.0
        assert np.array_equal(got.T[:, 3], np.tile([0.0, 0, 0, 1], (got.T.shape[0], 1)))


def test_three460_optimises_past_the_dense_limit():
    """1149 separators of Gauss-Newton: refused by the dense solver, 125 of them eliminated by the tier at the default limit.  Two exact solve
    orders of the restatement differ by 1.4e-12 m on this scene (test_posegraph_sparse_cpu.py), 700 times below TOL."""
    from mr_slam_amd import _lib, posegraph
    s = SC.scene("three460")
    want = SC.expected("three460")
    assert want.iterations == 44 and want.converged
    g = posegraph.PoseGraph(s.chain_lengths)
    g.set_odometry(s.odom)
    with pytest.raises(_lib.MrsError) as e:
        g.add_loops(s.li, s.lj, s.lZ)
    assert e.value.status == 3 and len(g) == 0
    g.set_solver("sparse")
    g.add_loops(s.li, s.lj, s.lZ)
    got = g.optimize()
    dR, dt = np.abs(got.T[:, :3, :3] - want.T[:, :3, :3]).max(), np.abs(got.T[:, :3, 3] - want.T[:, :3, 3]).max()
    print("three460: dR %.3g dt %.3g its %d/%d separators %d stats %s" % (dR, dt, got.iterations, want.iterations, got.separators, g.solver_stats()))
    assert dR < TOL and dt < TOL
    assert got.iterations == 44 and got.converged and got.separators == 1149
    cap = posegraph.MAX_SEPARATORS
    assert tuple(g.solver_stats()) == _stats_of("three460", posegraph.DEFAULT_SEGMENT_LENGTH, 2, cap)
    assert tuple(g.solver_stats(1)) == _stats_of("three460", posegraph.DEFAULT_SEGMENT_LENGTH, 1, cap)
    assert np.abs(g.initialize() - R_initial("three460")).max() < TOL
    with pytest.raises(_lib.MrsError) as e:                      # back to the dense solver: refused, and the graph stays as it is
        g.set_solver("dense")
    assert e.value.status == 3 and len(g) == s.li.size and g.solver_stats().solver == "sparse"
    assert _same(g.optimize(), got)


def R_initial(name):
    s = SC.scene(name)
    return PC.R.initialize(s.chain_lengths, s.odom, s.li, s.lj, s.lZ, prior=s.prior)[0]


def test_repeated_calls_and_fresh_handles_give_the_same_bits():
    s = PC.scene("r3x100")
    g = _sparse(s, 4)
    a, b = g.optimize(), g.optimize()
    assert _same(a, b) and np.array_equal(g.initialize(), g.initialize())
    assert _same(a, _sparse(s, 4).optimize())


def test_appended_loops_end_as_a_fresh_handle():
    from mr_slam_amd import posegraph
    s = PC.scene("r3x100")
    n = s.li.size
    g = posegraph.PoseGraph(s.chain_lengths)
    g.set_odometry(s.odom)
    g.set_solver("sparse", dense_limit=4)
    cuts = [0, 2, n // 2, n]                                     # the first two loops connect the three chains
    for a, b in zip(cuts, cuts[1:]):
        g.add_loops(s.li[a:b], s.lj[a:b], s.lZ[a:b])
        last = g.optimize()
    assert len(g) == n and _same(last, _sparse(s, 4).optimize())


def test_solver_changes_return_the_first_bits():
    s = PC.scene("r3x130")
    g = _graph(s)
    dense = g.optimize()
    assert g.solver_stats() == (dense.separators, 0, dense.separators, 0, 0, 0, 0, "dense")
    g.set_solver("sparse", dense_limit=4)
    sparse = g.optimize()
    assert g.solver_stats().eliminated == dense.separators - 4
    assert np.abs(sparse.T - dense.T).max() < TOL
    g.set_solver("dense")
    assert _same(g.optimize(), dense)
    g.set_solver("sparse", dense_limit=4)
    assert _same(g.optimize(), sparse)
    # nothing to eliminate: the dense solver's own bits
    g.set_solver("sparse", dense_limit=1024)
    assert g.solver_stats() == (dense.separators, 0, dense.separators, 0, 0, 0, 0, "sparse")
    assert _same(g.optimize(), dense) and _same(_sparse(s, 1024).optimize(), dense)
    assert np.array_equal(_sparse(s, 1024).initialize(), _graph(s).initialize())


def test_lm_with_noise_and_a_kernel_goes_through_the_tier():
    from test_posegraph_robust_gpu import _graph as robust_graph, _lm, _rel
    name = "outliers_huber"
    c, want = RC.case(name), RC.expected_lm(name)
    g = robust_graph(c)
    g.set_solver("sparse", dense_limit=0)
    got = _lm(g, c)
    w, r2 = g.loop_state()
    assert g.solver_stats().core == 0 and g.solver_stats().eliminated == got.separators > 0
    dR, dt = np.abs(got.T[:, :3, :3] - want.T[:, :3, :3]).max(), np.abs(got.T[:, :3, 3] - want.T[:, :3, 3]).max()
    rel = (_rel(got.cost_initial, want.cost_initial), _rel(got.cost_final, want.cost_final), _rel(got.lam, want.lam))
    dw, dr2 = np.abs(w - want.weights).max(), max(_rel(a, b) for a, b in zip(r2, want.r2))
    print("lm %s dense_limit 0: dR %.3g dt %.3g solves %d/%d costs rel %.3g %.3g lambda rel %.3g weights %.3g r2 rel %.3g"
          % (name, dR, dt, got.solves, want.solves, rel[0], rel[1], rel[2], dw, dr2))
    assert dR < TOL and dt < TOL
    assert (got.solves, got.accepted, got.converged) == (want.solves, want.accepted, want.converged)
    assert rel[0] < TOL and rel[1] < TOL and rel[2] < TOL and dw < TOL and dr2 < TOL


def test_refusals_leave_the_graph_as_it_was():
    from mr_slam_amd import _lib
    s = PC.scene("r3x130")
    g = _sparse(s, 4)
    want, stats = g.optimize(), g.solver_stats()
    need = SC.order("r3x130", 64, 2, 0).blocks
    need1 = SC.order("r3x130", 64, 1, 0).blocks

    def refused(call, status):
        with pytest.raises(_lib.MrsError) as e:
            call()
        assert e.value.status == status, str(e.value)
        assert g.solver_stats() == stats and _same(g.optimize(), want)

    refused(lambda: g.set_solver("sparse", dense_limit=0, max_blocks=need - 1), 3)
    refused(lambda: g.set_solver("sparse", dense_limit=1025), 1)
    refused(lambda: g.set_solver("sparse", dense_limit=-2), 1)
    refused(lambda: g.set_solver("sparse", max_blocks=-1), 1)
    refused(lambda: _lib.load().mrs_pgo_set_solver(g._h, 2, -1, 0), 1)
    refused(lambda: _lib.load().mrs_pgo_get_solver_stats(g._h, 3, np.zeros(8, np.int64)), 1)
    with pytest.raises(ValueError):
        g.set_solver("banded")
    # a budget both stages fit in is taken, and then bounds what may be added: a segment length that needs more blocks is refused
    g.set_solver("sparse", dense_limit=0, max_blocks=max(need, need1))
    tight, stats = g.optimize(), g.solver_stats()
    assert stats.blocks == need and stats.core == 0 and np.abs(tight.T - want.T).max() < TOL
    assert SC.order("r3x130", 1, 2, 0).blocks > max(need, need1)
    with pytest.raises(_lib.MrsError) as e:
        g.set_segment_length(1)
    assert e.value.status == 3 and "blocks" in str(e.value)
    assert g.solver_stats() == stats and _same(g.optimize(), tight)


def test_failed_pivot_of_a_sparse_column_is_a_status():
    """as test_posegraph_gpu.py::test_singular_system_is_a_status, with the chain's last pose a cut, which the tier eliminates"""
    from mr_slam_amd import _lib, posegraph
    s = PC.scene("chain_3")
    g = posegraph.PoseGraph(s.chain_lengths)
    g.set_segment_length(1)
    g.set_solver("sparse", dense_limit=0)
    odom = s.odom.copy()
    odom[1, :3, :3] = 1e200                                      # Hi^T Hi overflows: the pivot block is not finite
    g.set_odometry(odom)
    with pytest.raises(_lib.MrsError) as e:
        g.optimize()
    assert e.value.status == 5 and "pose" in str(e.value)
    g.set_odometry(s.odom)
    got = g.optimize()
    assert g.solver_stats().eliminated == got.separators > 0 and g.solver_stats().core == 0
    assert np.abs(got.T - PC.expected("chain_3").T).max() < TOL
