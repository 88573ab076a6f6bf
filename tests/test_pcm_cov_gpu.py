"""GPU suite for pairwise consistency with covariances: the squared Mahalanobis distances and the consistency matrix of the
kernels against the direct-chain restatement, single pairs, appending, defaults, the untouched plain test, the cancellation scene, the
clique end to end, and the refused inputs."""
import numpy as np
import pytest

import pcm_cov_cases as CC

PC, R, RC = CC.PC, CC.R, CC.RC
pytestmark = pytest.mark.gpu


def _graph(sc, mode, threshold, capacity=None, loops=True, first=None):
    from mr_slam_amd import pcm
    XA, XB, QA, QB, ia, kb, Z, Cv, _ = sc
    g = pcm.PcmGraph(capacity=capacity or len(ia), threshold=threshold)
    g.set_trajectories(XA, XB)
    g.set_covariances(mode, QA, QB, first)
    if loops:
        g.add_loops(ia, kb, Z, Cv)
    return g


def _check_distances(got, want, tol):
    assert np.array_equal(got, got.T) and not got.diagonal().any()
    worst = CC.rel_d(got, want).max() if got.size else 0.0
    print("largest relative deviation of d2: %.3g (allowed %.3g)" % (worst, tol))
    assert worst <= tol


@pytest.mark.parametrize("threshold", CC.THRESHOLDS)
@pytest.mark.parametrize("mode", CC.MODES)
@pytest.mark.parametrize("L", CC.SIZES)
def test_distances_and_matrix_match_the_restatement(L, mode, threshold):
    sc = CC.scene(L)
    D, _, _ = CC.expected(L, mode)
    g = _graph(sc, mode, threshold)
    assert len(g) == L
    _check_distances(g.distances(), D, CC.TOL_REL)
    A = g.matrix()
    assert np.array_equal(A, A.T) and not A.diagonal().any()
    assert np.array_equal(A, RC.consistency_matrix(D, threshold))
    g.clear()
    assert len(g) == 0
    g.add_loops(*sc[4:8])
    assert g.matrix().tobytes() == A.tobytes()


@pytest.mark.parametrize("mode", CC.MODES)
def test_single_pairs_match_the_restatement(mode):
    sc = CC.special_scene()
    D, XI, SE = CC.expected_special(mode)
    g = _graph(sc, mode, 16.812)
    Dg = g.distances()
    for u, v in CC.SPECIAL_PAIRS:
        xi, cov, d = g.pair(u, v)
        xi2, cov2, d2 = g.pair(v, u)
        assert xi.tobytes() == xi2.tobytes() and cov.tobytes() == cov2.tobytes() and d == d2
        print("pair", (u, v), "xi %.3g Sigma %.3g d2 %.3g" % (np.abs(xi - XI[u, v]).max(), CC.rel_sigma(cov, SE[u, v]), CC.rel_d(d, D[u, v])))
        assert np.abs(xi - XI[u, v]).max() < CC.XI_TOL
        assert np.array_equal(cov, cov.T) and CC.rel_sigma(cov, SE[u, v]) <= CC.TOL_REL
        assert CC.rel_d(d, D[u, v]) <= CC.TOL_REL
        assert CC.rel_d(Dg[u, v], D[u, v]) <= CC.TOL_REL and CC.rel_d(d, Dg[u, v]) <= CC.TOL_REL      # host and device evaluation


@pytest.mark.parametrize("capacity", [129, 4096])
def test_appending_gives_the_matrix_of_the_whole(capacity):
    sc = CC.scene(129)
    ia, kb, Z, Cv = sc[4:8]
    whole = _graph(sc, "span", 16.812, capacity)
    parts = _graph(sc, "span", 16.812, capacity, loops=False)
    at = 0
    for n in (1, 62, 1, 65):
        parts.add_loops(ia[at:at + n], kb[at:at + n], Z[at:at + n], Cv[at:at + n])
        at += n
    assert len(parts) == 129
    assert parts.matrix().tobytes() == whole.matrix().tobytes()
    assert parts.distances().tobytes() == whole.distances().tobytes()
    assert np.array_equal(whole.matrix(), RC.consistency_matrix(CC.expected(129, "span")[0], 16.812))
    (c1, r1), (c2, r2) = whole.solve(), parts.solve()
    assert c1.tolist() == c2.tolist() and r1 == r2


def test_defaults_are_the_fixed_covariance():
    from mr_slam_amd import pcm
    XA, XB, _, _, ia, kb, Z, _, _ = CC.scene(65)
    F = np.array(pcm.FIXED_COVARIANCE)
    n = XA.shape[0]
    for mode in CC.MODES:
        a = pcm.PcmGraph(capacity=65, threshold=16.812)
        a.set_trajectories(XA, XB)
        a.set_covariances(mode)
        a.add_loops(ia, kb, Z)                                     # plain add_loops on a covariance handle
        b = pcm.PcmGraph(capacity=65, threshold=16.812)
        b.set_trajectories(XA, XB)
        b.set_covariances(mode, np.stack([F] * (n - 1)), np.stack([F] * (n - 1)), F)
        b.add_loops(ia, kb, Z, np.stack([F] * 65))
        assert a.distances().tobytes() == b.distances().tobytes() and a.matrix().tobytes() == b.matrix().tobytes()
        a.clear()
        a.add_loops(ia, kb, Z, cov=None)
        assert a.distances().tobytes() == b.distances().tobytes()
        D, _, _ = RC.evaluate(mode, XA, XB, ia, kb, Z)
        _check_distances(a.distances(), D, CC.TOL_REL)


def test_plain_test_is_untouched():
    from mr_slam_amd import pcm
    XA, XB, ia, kb, Z = PC.scene(129)
    fresh = pcm.PcmGraph(capacity=129, p=0.01)
    fresh.set_trajectories(XA, XB)
    fresh.add_loops(ia, kb, Z)
    D, A = fresh.distances(), fresh.matrix()
    assert np.abs(D - PC.expected(129)).max() < 1e-9
    g = pcm.PcmGraph(capacity=129, p=0.01)
    g.set_trajectories(XA, XB)
    g.set_covariances("span")
    g.add_loops(ia, kb, Z)
    assert g.distances().tobytes() != D.tobytes()
    g.set_trajectories(XA, XB)                                     # resets the mode
    assert len(g) == 0
    g.add_loops(ia, kb, Z)
    assert g.distances().tobytes() == D.tobytes() and g.matrix().tobytes() == A.tobytes()
    g.set_covariances("reference")
    g.set_covariances(mode="none")
    assert len(g) == 0
    g.add_loops(ia, kb, Z)
    assert g.distances().tobytes() == D.tobytes() and g.matrix().tobytes() == A.tobytes()
    xi, cov, d = g.pair(3, 100)
    assert np.array_equal(cov, np.eye(6)) and abs(d - D[3, 100]) < 1e-12 and abs(np.linalg.norm(xi) - d) < 1e-12


def test_cancellation_on_a_long_trajectory():
    """400 poses: the prefix difference cancels; LONG_TOL_REL is 4 x the deviation of the g++ build on this scene"""
    sc = CC.long_scene()
    D, _, _ = CC.expected_long()
    for threshold in CC.THRESHOLDS:
        g = _graph(sc, "span", threshold)
        _check_distances(g.distances(), D, CC.LONG_TOL_REL)
        skip = CC.in_margin(D, (threshold,), CC.LONG_MARGIN_REL)
        assert skip.sum() <= CC.LONG_SKIP_CAP * D.size
        A, want = g.matrix(), RC.consistency_matrix(D, threshold)
        assert np.array_equal(A[~skip], want[~skip]) and np.array_equal(A, A.T)


def test_clique_end_to_end():
    import pcm_exact_restate as RX
    sc = CC.scene(129)
    inlier = sc[8]
    A = RC.consistency_matrix(CC.expected(129, "span")[0], 16.812)
    g = _graph(sc, "span", 16.812)
    clique, rejected = g.solve()
    size, members = R.max_clique_heu(A)
    assert clique.tolist() == list(members) and rejected == 129 - size and inlier[clique].all()
    exact, _ = g.solve_exact()
    want_size = RX.max_clique_exact(A)[0]
    assert g.proof == 2 and exact.size == want_size and A[np.ix_(exact, exact)].sum() == want_size * (want_size - 1)


def test_edges_and_refused_inputs():
    from mr_slam_amd import _lib, pcm
    XA, XB, QA, QB, ia, kb, Z, Cv, _ = CC.scene(65)
    # a one-pose trajectory: no odometry, Sigma_E from the other side and the loops
    one = pcm.PcmGraph(capacity=4, threshold=16.812)
    one.set_trajectories(XA[:1], XB)
    one.set_covariances("span", None, QB)
    k = np.array([2, 9, 30], np.int32)
    one.add_loops(np.zeros(3, np.int32), k, Z[:3], Cv[:3])
    D, _, _ = RC.evaluate("span", XA[:1], XB, np.zeros(3, np.int32), k, Z[:3], Cv[:3], None, QB)
    _check_distances(one.distances(), D, CC.TOL_REL)
    with pytest.raises(_lib.MrsError) as e:
        one.set_covariances("span", np.zeros((0, 6, 6)), QB)
    assert e.value.status == 1 and len(one) == 3

    g = _graph(CC.scene(65), "span", 16.812, capacity=70)          # room for two more: the refusals are not for want of capacity
    A = g.matrix()

    def refused(call):
        with pytest.raises(_lib.MrsError) as e:
            call()
        assert e.value.status == 1
        assert len(g) == 65 and g.matrix().tobytes() == A.tobytes()

    bad = Cv[:2].copy()
    bad[1, 4, 1] = np.nan
    refused(lambda: g.add_loops(ia[:2], kb[:2], Z[:2], bad))
    notpd = Cv[:2].copy()
    notpd[0] = -notpd[0]
    refused(lambda: g.add_loops(ia[:2], kb[:2], Z[:2], notpd))
    badq = QA.copy()
    badq[5] = np.diag([1, 1, 1, 1, 1, 0.0])
    refused(lambda: g.set_covariances("span", badq, QB))
    refused(lambda: _lib.load().mrs_pcm_set_covariances(g._h, 3, None, None, None))
    for u, v in ((4, 4), (-1, 2), (0, 65)):
        refused(lambda: g.pair(u, v))
    with pytest.raises(ValueError):
        g.set_covariances("mahalanobis")
    # a NaN in Z isolates its vertex
    g.clear()
    Zn = Z.copy()
    Zn[7, 2, 3] = np.nan
    g.add_loops(ia, kb, Zn, Cv)
    An, Dn = g.matrix(), g.distances()
    assert not An[7].any() and not An[:, 7].any() and np.isnan(np.delete(Dn[7], 7)).all()
    keep = np.delete(np.arange(65), 7)
    assert np.array_equal(An[np.ix_(keep, keep)], A[np.ix_(keep, keep)])
    # covariances on a handle without a covariance mode
    plain = pcm.PcmGraph(capacity=8, p=0.01)
    plain.set_trajectories(XA, XB)
    plain.add_loops(ia[:3], kb[:3], Z[:3])
    P = plain.matrix()
    with pytest.raises(_lib.MrsError) as e:
        plain.add_loops(ia[3:5], kb[3:5], Z[3:5], Cv[3:5])
    assert e.value.status == 1 and len(plain) == 3 and plain.matrix().tobytes() == P.tobytes()
