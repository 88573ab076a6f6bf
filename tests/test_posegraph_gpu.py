"""GPU suite for the pose-graph optimiser (mr_slam_amd/posegraph.py over mrs_pgo_*): both stages against the NumPy / scipy restatement on
every scene of posegraph_cases.py and every segment length, the stop rule's two ends, bit-for-bit determinism over repeated calls, appended
loops and segment-length changes, the refusals, and the hand-over to GlobalMap.rebuild.

Observed against the restatement on an MI355X (all scenes, all segment lengths): see DESIGN.md 4.23."""
import numpy as np
import pytest

import posegraph_cases as PC

pytestmark = pytest.mark.gpu
R = PC.R
TOL = 1e-9
ALL = PC.NAMES + ("quirks_prior",)


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    assert torch.cuda.is_available()        # PyTorch's runtime has to see the device before the library's does


def _scene(name):
    return PC.with_prior() if name == "quirks_prior" else PC.scene(name)


def _graph(s, loops=slice(None), segment_length=None):
    from mr_slam_amd import posegraph
    g = posegraph.PoseGraph(s.chain_lengths)
    g.set_odometry(s.odom)
    g.add_loops(s.li[loops], s.lj[loops], s.lZ[loops])
    if s.prior is not None:
        g.set_prior(s.prior)
    if segment_length is not None:
        g.set_segment_length(segment_length)
    return g


def _same(a, b):
    return (np.array_equal(a.T, b.T) and a.iterations == b.iterations and a.converged == b.converged and a.max_delta == b.max_delta
            and a.error_initial == b.error_initial and a.error_final == b.error_final)


@pytest.mark.parametrize("name", ALL)
def test_stage1_rotations(name):
    want, _ = PC.expected_initial(name)
    s = _scene(name)
    worst = 0.0
    for L in PC.SEGMENT_LENGTHS:
        T = _graph(s, segment_length=L).initialize()
        worst = max(worst, np.abs(T - want).max())
        assert not T[:, :3, 3].any() and np.array_equal(T[:, 3], np.tile([0.0, 0, 0, 1], (T.shape[0], 1)))
    print("stage 1 %s: max |R - restatement| = %.3g" % (name, worst))
    assert worst < TOL


@pytest.mark.parametrize("name", ALL)
def test_optimize_matches_restatement(name):
    want = PC.expected(name)
    s = _scene(name)
    for L in PC.SEGMENT_LENGTHS:
        got = _graph(s, segment_length=L).optimize()
        dR, dt = np.abs(got.T[:, :3, :3] - want.T[:, :3, :3]).max(), np.abs(got.T[:, :3, 3] - want.T[:, :3, 3]).max()
        rel = [abs(a - b) / max(abs(b), 1e-300) if b else abs(a) for a, b in ((got.error_initial, want.error_initial), (got.error_final, want.error_final))]
        print("optimize %s L=%d: dR %.3g dt %.3g its %d/%d errors rel %.3g %.3g separators %d"
              % (name, L, dR, dt, got.iterations, want.iterations, rel[0], rel[1], got.separators))
        assert dR < TOL and dt < TOL
        assert got.iterations == want.iterations and got.converged == want.converged
        if want.error_final > 1e-18:
            assert rel[0] < TOL and rel[1] < TOL
        else:                                                    # a pure chain: both ends are rounding
            assert got.error_final <= 1e-18
            assert rel[0] < TOL or want.error_initial == 0.0
        assert np.array_equal(got.T[:, 3], np.tile([0.0, 0, 0, 1], (got.T.shape[0], 1)))


def test_eps_zero_runs_every_iteration():
    want = PC.expected("quirks", 0.0, 200)
    got = _graph(PC.scene("quirks")).optimize(eps=0.0, max_iterations=200)
    assert got.iterations == 200 and not got.converged and want.iterations == 200
    assert np.abs(got.T - want.T).max() < TOL
    assert np.abs(got.T - PC.expected("quirks").T).max() < TOL


@pytest.mark.parametrize("name", ["r3x2", "quirks", "runs"])
def test_one_iteration_is_centralized_estimation(name):
    want = PC.expected(name, PC.EPS, 1)
    got = _graph(PC.scene(name)).optimize(max_iterations=1)
    assert got.iterations == 1 and not got.converged
    assert np.abs(got.T - want.T).max() < TOL
    assert abs(got.max_delta - want.max_delta) < 1e-9 * want.max_delta


def test_repeated_calls_give_the_same_bits():
    s = PC.scene("r3x100")
    g = _graph(s)
    a, b = g.optimize(), g.optimize()
    assert _same(a, b) and np.array_equal(g.initialize(), g.initialize())
    assert _same(a, _graph(s).optimize())


def test_appended_loops_end_as_a_fresh_handle():
    """the node's shape: one optimisation after every closure"""
    from mr_slam_amd import posegraph
    s = PC.scene("r3x100")
    n = s.li.size
    g = posegraph.PoseGraph(s.chain_lengths)
    g.set_odometry(s.odom)
    cuts = [0, 2, n // 2, n]                                     # the first two loops connect the three chains
    for a, b in zip(cuts, cuts[1:]):
        g.add_loops(s.li[a:b], s.lj[a:b], s.lZ[a:b])
        last = g.optimize()
    assert len(g) == n and _same(last, _graph(s).optimize())
    g.clear()
    assert len(g) == 0
    g.add_loops(s.li, s.lj, s.lZ)
    assert _same(g.optimize(), last)


def test_segment_length_back_and_forth():
    s = PC.scene("runs")
    g = _graph(s)
    first = {}
    for L in (64, 3, 0, 1, 3, 64, 0, 1):
        g.set_segment_length(L)
        r = g.optimize()
        if L in first:
            assert _same(r, first[L]), L
        first[L] = r
    assert first[64].separators < first[3].separators < first[1].separators and first[0].separators <= first[64].separators
    assert _same(first[3], _graph(s, segment_length=3).optimize())


def test_refusals_leave_the_graph_as_it_was():
    from mr_slam_amd import _lib, posegraph
    s = PC.scene("quirks")
    g = _graph(s)
    want = g.optimize()
    N = g.n_poses
    Z = s.lZ[:1]

    def refused(call, status):
        with pytest.raises(_lib.MrsError) as e:
            call()
        assert e.value.status == status, str(e.value)
        assert len(g) == s.li.size and _same(g.optimize(), want)

    refused(lambda: g.add_loops([3], [3], Z), 1)                 # i == j
    refused(lambda: g.add_loops([3], [N], Z), 1)                 # an index past N
    refused(lambda: g.add_loops([-1], [4], Z), 1)
    bad = Z.copy()
    bad[0, 1, 3] = np.nan
    refused(lambda: g.add_loops([3, 4], [9, 10], np.concatenate([Z, bad])), 1)      # a non-finite Z: the finite one before it is not added either
    bad[0, 1, 3] = np.inf
    refused(lambda: g.add_loops([3], [9], bad), 1)
    refused(lambda: g.set_odometry(s.odom[:-1]), 1)              # a wrong odometry count
    refused(lambda: g.set_odometry(np.concatenate([s.odom, s.odom[:1]])), 1)
    refused(lambda: g.set_segment_length(-1), 1)
    refused(lambda: g.optimize(eps=-1.0), 1)
    refused(lambda: g.optimize(max_iterations=0), 1)
    # a disconnected chain: the call is refused until a loop reaches it, and the graph then optimises as if nothing had happened
    h = posegraph.PoseGraph(s.chain_lengths)
    h.set_odometry(s.odom)
    inter = [u for u in range(s.li.size) if min(s.li[u], s.lj[u]) < 40 <= max(s.li[u], s.lj[u]) < 70]
    h.add_loops(s.li[inter], s.lj[inter], s.lZ[inter])            # chains 0 and 1 only
    for call in (h.optimize, h.initialize):
        with pytest.raises(_lib.MrsError) as e:
            call()
        assert e.value.status == 1 and "not connected" in str(e.value)
    rest = [u for u in range(s.li.size) if u not in inter]
    h.add_loops(s.li[rest], s.lj[rest], s.lZ[rest])
    order = inter + rest
    f = posegraph.PoseGraph(s.chain_lengths)
    f.set_odometry(s.odom)
    f.add_loops(s.li[order], s.lj[order], s.lZ[order])
    assert _same(h.optimize(), f.optimize())
    # odometry not set
    e0 = posegraph.PoseGraph((3,))
    with pytest.raises(_lib.MrsError) as e:
        e0.optimize()
    assert e.value.status == 1


def test_too_many_separators_are_unsupported():
    from mr_slam_amd import _lib, posegraph
    from mr_slam_amd import pcm
    n = 2 * posegraph.MAX_SEPARATORS + 80
    odom = np.tile(PC.pose([0.0, 0.0, 0.05], [1.0, 0.0, 0.0]), (n - 1, 1, 1))      # laps of a circle of 20 m
    X = pcm.chain_odometry(odom)
    g = posegraph.PoseGraph((n,))
    g.set_odometry(odom)
    g.set_segment_length(64)
    want = g.optimize()
    assert want.separators == (n - 1) // 65 and want.converged
    with pytest.raises(_lib.MrsError) as e:                      # every other pose a cut
        g.set_segment_length(1)
    assert e.value.status == 3
    assert _same(g.optimize(), want)
    i = np.arange(1, 2 * posegraph.MAX_SEPARATORS + 40, 2, dtype=np.int32)          # more than MAX_SEPARATORS poses touched
    Z = posegraph.between(X[i], X[i + 1])
    with pytest.raises(_lib.MrsError) as e:
        g.add_loops(i, i + 1, Z)
    assert e.value.status == 3 and len(g) == 0
    assert _same(g.optimize(), want)
    with pytest.raises(_lib.MrsError) as e:
        posegraph.PoseGraph((posegraph.MAX_POSES, 1))
    assert e.value.status == 3
    with pytest.raises(_lib.MrsError) as e:
        posegraph.PoseGraph([1] * (posegraph.MAX_CHAINS + 1))
    assert e.value.status == 1


def test_singular_system_is_a_status():
    """an odometry pose that is not a rigid motion (a zero rotation block) leaves stage 1's system positive definite and Gauss-Newton's
    finite; a graph whose pivot fails is reported with its pose, never a hang"""
    from mr_slam_amd import _lib, posegraph
    s = PC.scene("chain_3")
    g = posegraph.PoseGraph(s.chain_lengths)
    odom = s.odom.copy()
    odom[1, :3, :3] = 1e200                                      # Hi^T Hi overflows: the pivot block is not finite
    g.set_odometry(odom)
    with pytest.raises(_lib.MrsError) as e:
        g.optimize()
    assert e.value.status == 5 and "pose" in str(e.value)
    g.set_odometry(s.odom)
    assert np.abs(g.optimize().T - PC.expected("chain_3").T).max() < TOL


def test_correction_feeds_the_global_map():
    """two stores of two keyframes each: the map rebuilt with the optimiser's poses is the map rebuilt with the restatement's"""
    from mr_slam_amd import globalmap, posegraph, submap
    s = PC.scene("r3x2")
    got, want = _graph(s).optimize(), PC.expected("r3x2")
    rng = np.random.default_rng(4)
    stores, segments_got, segments_want = [], [], []
    origin = np.tile(np.eye(4), (4, 1, 1))
    origin[:, :3, 3] = rng.uniform(-1, 1, (4, 3))
    Cg, Cw = posegraph.correction(got.T[:4], origin), posegraph.correction(want.T[:4], origin)
    assert np.abs(Cg - Cw).max() < 1e-5
    for r in range(2):
        st = submap.KeyframeStore()
        for k in range(2):
            pts = np.concatenate([rng.uniform(-4, 4, (300, 3)), rng.uniform(0, 255, (300, 1))], axis=1).astype(np.float32)
            st.append(pts, np.eye(4, dtype=np.float32))
            segments_got.append((r, k, Cg[2 * r + k]))
            segments_want.append((r, k, Cw[2 * r + k]))
        stores.append(st)
    gm = globalmap.GlobalMap(stores, leaf=0.5)
    a = gm.rebuild(segments_got).cpu().numpy()
    b = gm.rebuild(segments_want).cpu().numpy()
    assert a.shape == b.shape and a.shape[0] > 100
    assert np.abs(a - b).max() < 1e-4
