"""GPU suite for the pose-graph optimiser's marginal covariances (PoseGraph.marginals / joint_marginals / mark_poses over mrs_pgo_*;
DESIGN.md 4.23(k)): all marginals and the answered joint marginals against the NumPy / scipy restatement
(tests/golden/posegraph_marginals_restate.py) on every case of posegraph_marginals_cases.py, at every segment length and in both frames;
symmetry to the bit, positive diagonal blocks, agreement across segment lengths; the same bits from call to call, from a fresh handle and
around the optimiser; marked poses; the refusals.

The reference of a comparison is the inverse of the information matrix the restatement forms from public results of the handle under
test (its poses, its stage-1 poses, its loop weights), so the comparison isolates the inversion.  The measure is
max |Sigma_gpu - Sigma_ref| / max |Sigma_ref| over all blocks returned for a case; its bound is posegraph_marginals_cases.bound.

Observed on an MI355X: see DESIGN.md 4.23(k)."""
import itertools

import numpy as np
import pytest

import posegraph_cases as PC
import posegraph_marginals_cases as MC
import posegraph_robust_cases as RC
from test_posegraph_robust_gpu import _add_loops

pytestmark = pytest.mark.gpu
MR, RR = MC.MR, MC.RR
FRAMES = (("chordal", MR.CHORDAL), ("pose3", MR.POSE3))


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    assert torch.cuda.is_available()        # PyTorch's runtime has to see the device before the library's does


def _graph(c, segment_length=None, marks=None):
    from mr_slam_amd import posegraph
    s = c.scene
    g = posegraph.PoseGraph(s.chain_lengths)
    g.set_odometry(s.odom)
    if c.oC is not None:
        g.set_odometry_noise(c.oC)
    _add_loops(g, c, range(s.li.size))
    if s.prior is not None:
        g.set_prior(s.prior)
    if c.kernel != RR.NONE:
        g.set_loop_kernel(RC.KERNEL_NAMES[c.kernel], c.k)
    if segment_length is not None:
        g.set_segment_length(segment_length)
    if marks is not None:
        g.mark_poses(marks)
    return g


def _optimize(g, c):
    if c.method == "lm":
        return g.optimize(method="lm", max_iterations=c.max_solves or RR.MAX_SOLVES_DEFAULT)
    return g.optimize()


def _reference(name, g, res):
    """Sigma [6 N]^2 of the optimiser's tangent from the handle's own poses, stage-1 poses and loop weights"""
    w, _ = g.loop_state()
    return MC.reference(name, res.T, g.initialize(), w)


def _pairs(c, is_sep):
    """the pairs every handle answers: the loops' (i, j), every consecutive pair of a chain, pose 0 with a separator, an interior pose's
    neighbour and the last pose"""
    s = c.scene
    N = int(sum(s.chain_lengths))
    ends = set((np.cumsum(s.chain_lengths) - 1).tolist())
    pairs = [(int(i), int(j)) for i, j in zip(s.li, s.lj)]
    pairs += [(p, p + 1) for p in range(N - 1) if p not in ends] + [(p + 1, p) for p in range(0, N - 1, 7) if p not in ends]
    pairs += [(0, int(p)) for p in np.flatnonzero(is_sep)[1:4]] + [(int(p), 0) for p in np.flatnonzero(is_sep)[1:2]]
    return pairs


def _check_blocks(got, want, scale):
    """-> max |got - want| / scale after the exact properties: symmetric to the bit, positive diagonal blocks"""
    assert got.shape == want.shape and np.isfinite(got).all()
    assert np.array_equal(got, got.transpose(0, 2, 1))
    return float(np.abs(got - want).max() / scale) if got.size else 0.0


@pytest.mark.parametrize("name", MC.NAMES)
def test_marginals_and_joints_match_restatement(name):
    c = MC.case(name)
    s = c.scene
    N, bound = int(sum(s.chain_lengths)), MC.bound(name)
    first = None
    for L in MC.SEGMENT_LENGTHS:
        g = _graph(c, segment_length=L)
        res = _optimize(g, c)
        info = g.marginal_info()
        Sref = _reference(name, g, res)
        is_sep = MR.separators(s.chain_lengths, s.li, s.lj, L)
        assert info.separators == res.separators == int(is_sep.sum()) - 1 and info.order == 6 * info.separators
        assert info.bytes >= 8 * (info.order ** 2 + 72 * N)
        pairs = _pairs(c, is_sep)
        pi, pj = [p[0] for p in pairs], [p[1] for p in pairs]
        worst, all_got = 0.0, []
        for frame, fid in FRAMES:
            S = MR.in_frame(Sref, res.T, fid)
            scale = np.abs(S).max()
            m, j = g.marginals(frame=frame), g.joint_marginals(pi, pj, frame=frame)
            em = _check_blocks(m, MR.marginals(S), scale)
            ej = _check_blocks(j, np.array([MR.joint(S, a, b) for a, b in pairs]).reshape(len(pairs), 12, 12), scale)
            assert not m[0].any() and np.linalg.eigvalsh(m[1:]).min() > 0
            for u, (a, b) in enumerate(pairs):
                if a == 0:
                    assert not j[u][:6].any() and not j[u][:, :6].any()
                if b == 0:
                    assert not j[u][6:].any() and not j[u][:, 6:].any()
            sub = [1, N - 1, N // 2]
            assert np.array_equal(g.marginals(sub, frame=frame), m[sub])
            worst = max(worst, em, ej)
            all_got.append((m, j, scale))
            print("marginals %s L=%d %s: marginals %.3g joints %.3g (%d pairs) bound %.3g separators %d bytes %d"
                  % (name, L, frame, em, ej, len(pairs), bound, info.separators, info.bytes))
        assert worst <= bound
        if first is None:
            first = all_got
        else:                                                    # the segment length changes the elimination order, not the result
            for (m0, _, scale), (m, _, _) in zip(first, all_got):
                d = float(np.abs(m - m0).max() / scale)
                print("marginals %s L=%d against L=%d: %.3g" % (name, L, MC.SEGMENT_LENGTHS[0], d))
                assert d <= bound


@pytest.mark.parametrize("name", ["r3x64", "runs", "chain_65", "outliers_cauchy"])
def test_marked_poses_answer_their_joints(name):
    c = MC.case(name)
    s = c.scene
    N, bound = int(sum(s.chain_lengths)), MC.bound(name)
    base_sep = MR.separators(s.chain_lengths, s.li, s.lj, 64)
    interior = np.flatnonzero(~base_sep)
    marks = [int(interior[k]) for k in (1, interior.size // 2, interior.size - 2)]
    g0 = _graph(c)
    r0, T0 = _optimize(g0, c), g0.initialize()
    from mr_slam_amd import _lib, posegraph
    with pytest.raises(_lib.MrsError) as e:                      # unmarked: refused, the pose to mark named
        g0.joint_marginals([marks[0]], [marks[1]])
    assert e.value.status == 1 and "pose %d is not a separator" % marks[0] in str(e.value) and "mrs_pgo_mark_poses" in str(e.value)
    g = _graph(c, marks=marks + [0])                             # marking pose 0 changes nothing
    res = _optimize(g, c)
    is_sep = MR.separators(s.chain_lengths, s.li, s.lj, 64, marks)
    assert res.separators == int(is_sep.sum()) - 1 and res.separators - r0.separators == int(is_sep.sum()) - int(base_sep.sum()) > 0
    assert np.array_equal(g.initialize(), T0)                    # stage 1 never sees the marks
    assert np.abs(res.T - r0.T).max() < 1e-9
    Sref = _reference(name, g, res)
    pairs = list(itertools.permutations(marks, 2)) + [(0, marks[2])]
    for frame, fid in FRAMES:
        S = MR.in_frame(Sref, res.T, fid)
        scale = np.abs(S).max()
        j = g.joint_marginals([p[0] for p in pairs], [p[1] for p in pairs], frame=frame)
        ej = _check_blocks(j, np.array([MR.joint(S, a, b) for a, b in pairs]), scale)
        em = _check_blocks(g.marginals(frame=frame), MR.marginals(S), scale)
        print("marked %s %s: joints %.3g marginals %.3g bound %.3g" % (name, frame, ej, em, bound))
        assert max(ej, em) <= bound
    Ti, Tj = res.T[marks[0]], res.T[marks[2]]                    # the covariance of the relative pose, as a PCM loop would take it
    jp = g.joint_marginals([marks[0]], [marks[2]], frame="pose3")[0]
    Cz = posegraph.between_covariance(jp, Ti, Tj)
    assert MR.spread(Cz, MR.between_covariance(jp, Ti, Tj)) < 1e-12 and np.linalg.eigvalsh(0.5 * (Cz + Cz.T)).min() > 0
    g.mark_poses(None)                                           # cleared: the bits of a handle that never had marks
    r1 = _optimize(g, c)
    assert np.array_equal(r1.T, r0.T) and r1.separators == r0.separators
    assert np.array_equal(g.marginals(), g0.marginals())


@pytest.mark.parametrize("name", ["r3x64", "outliers_geman_mcclure"])
def test_same_bits(name):
    c = MC.case(name)
    s = c.scene
    g = _graph(c)
    alone = _optimize(g, c)
    state = g.loop_state()
    pi, pj = s.li[:4], s.lj[:4]
    a, ja, ia = g.marginals(), g.joint_marginals(pi, pj, frame="pose3"), g.marginal_info()
    b, jb, ib = g.marginals(), g.joint_marginals(pi, pj, frame="pose3"), g.marginal_info()      # call to call; compute twice
    assert np.array_equal(a, b) and np.array_equal(ja, jb) and ia == ib
    st = g.loop_state()                                          # the computation reads the result and does not change it
    assert np.array_equal(st[0], state[0]) and np.array_equal(st[1], state[1])
    again = _optimize(g, c)                                      # optimize after marginals: the bits of optimize alone
    assert np.array_equal(again.T, alone.T) and again[1:] == alone[1:]
    assert np.array_equal(g.marginals(), a)                      # and the marginals of the new, equal result
    h = _graph(c)                                                # a fresh handle
    _optimize(h, c)
    assert np.array_equal(h.marginals(), a) and np.array_equal(h.joint_marginals(pi, pj, frame="pose3"), ja)
    h.mark_poses([])                                             # an empty set is the default: nothing changes, not even the result
    assert np.array_equal(h.marginals(), a)


def test_refusals_leave_the_handle_as_it_was():
    from mr_slam_amd import _lib, posegraph
    c = MC.case("r3x64")
    s = c.scene
    g = _graph(c)

    def refused(call, status, text):
        with pytest.raises(_lib.MrsError) as e:
            call()
        assert e.value.status == status and text in str(e.value), str(e.value)

    refused(g.marginals, 1, "no optimisation of the graph as it stands has finished")                # no result
    refused(lambda: g.joint_marginals([1], [2]), 1, "no optimisation")
    res = g.optimize()
    cov = np.zeros((1, 6, 6))
    refused(lambda: _lib.load().mrs_pgo_get_marginals(g._h, np.array([1], np.int32), 1, 0, cov), 1, "mrs_pgo_compute_marginals has not run")
    a = g.marginals()
    is_sep = MR.separators(s.chain_lengths, s.li, s.lj, 64)
    interior = np.flatnonzero(~is_sep)
    p, q = int(interior[0]), int(interior[-1])
    ok = g.joint_marginals([p], [p + 1])
    refused(lambda: g.joint_marginals([p, p], [p + 1, q]), 1, "is not a separator of stage 2")       # nothing is written either
    refused(lambda: g.joint_marginals([p], [p]), 1, "two different poses")
    refused(lambda: g.joint_marginals([p], [g.n_poses]), 1, "outside the graph")
    refused(lambda: g.marginals([-1]), 1, "outside the graph")
    refused(lambda: _lib.load().mrs_pgo_get_marginals(g._h, np.array([1], np.int32), 1, 2, cov), 1, "MRS_PGO_FRAME")
    refused(lambda: _lib.load().mrs_pgo_get_joint_marginals(g._h, np.array([p], np.int32), np.array([p + 1], np.int32), 1, -1, np.zeros((1, 12, 12))),
            1, "MRS_PGO_FRAME")
    with pytest.raises(ValueError):
        g.marginals(frame="world")
    refused(lambda: g.mark_poses([3, g.n_poses]), 1, "outside the graph")
    refused(lambda: g.mark_poses([3, -1]), 1, "outside the graph")
    refused(lambda: g.mark_poses([3, 5, 3]), 1, "marked twice")
    assert np.array_equal(g.marginals(), a) and np.array_equal(g.joint_marginals([p], [p + 1]), ok)   # every refusal left the handle alone
    assert not cov.any()
    g.add_loops([p], [q], PC.inv(res.T[p]) @ res.T[q])            # the graph changed since
    refused(g.marginals, 1, "no optimisation of the graph as it stands has finished")
    g.optimize()
    assert g.joint_marginals([p], [q]).shape == (1, 12, 12)       # the new loop's poses are separators now
    g.set_segment_length(3)
    refused(g.marginal_info, 1, "no optimisation")
    # marks past the separator limit: host work only
    big = posegraph.PoseGraph([posegraph.MAX_SEPARATORS + 40])
    big.mark_poses(np.arange(1, 1001))
    refused(lambda: big.mark_poses(np.arange(1, posegraph.MAX_SEPARATORS + 2)), 3, "separators")
    assert big.solver_stats().separators >= 1000                 # the refused set did not replace the earlier one


def test_sparse_tier_is_refused_and_an_idle_one_is_the_dense_path():
    from mr_slam_amd import _lib
    c = MC.case("r3x64")
    s = c.scene
    d = _graph(c)
    d.optimize()
    want, jw = d.marginals(frame="pose3"), d.joint_marginals(s.li, s.lj)
    g = _graph(c)
    g.set_solver("sparse", dense_limit=0)
    g.optimize()
    assert g.solver_stats().eliminated > 0
    for call in (g.marginals, g.marginal_info, lambda: g.joint_marginals(s.li, s.lj)):
        with pytest.raises(_lib.MrsError) as e:
            call()
        assert e.value.status == 3 and "sparse tier" in str(e.value)
    g.set_solver("sparse")                                       # the default limit: nothing is eliminated on this scene
    g.optimize()
    assert g.solver_stats().eliminated == 0
    assert np.array_equal(g.marginals(frame="pose3"), want) and np.array_equal(g.joint_marginals(s.li, s.lj), jw)
