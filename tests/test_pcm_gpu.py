"""GPU suite for pairwise consistency (mr_slam_amd/pcm.py over mrs_pcm_*): the clique stage alone against what the reference's own clique
finder returned (tests/golden/ref_pcm_clique.npz), the consistency matrix and its distances against the NumPy restatement
(tests/golden/pcm_restate.py), appending, the whole path, and the edges.  Inputs and expected values come from tests/pcm_cases.py, computed
once; test_pcm_cpu.py checks the conditions they rely on."""
import numpy as np
import pytest

import pcm_cases as PC

R = PC.R
pytestmark = pytest.mark.gpu
TOL = 1e-9          # distances: six chained fp64 pose products at |t| <= 1e3 round to about 1e-11, Logmap below 3 rad carries that to 1e-10


@pytest.fixture(scope="module")
def pcm():
    from mr_slam_amd import pcm
    return pcm


@pytest.fixture(scope="module")
def graphs():
    return R.load()


def _loaded(pcm, L, p, capacity=None):
    g = pcm.PcmGraph(capacity=capacity or max(L, 1), p=p)
    XA, XB, ia, kb, Z = PC.scene(L)
    g.set_trajectories(XA, XB)
    g.add_loops(ia, kb, Z)
    return g


# ------------------------------------------------------------------ the clique stage alone
def test_clique_of_every_fixture_graph(pcm, graphs):
    """size and member list as recorded from the reference, within size + 1 rounds, and the same again on a second solve"""
    g = pcm.PcmGraph(capacity=256)
    for k, (n, edges, size, members) in enumerate(graphs):
        A = R.adjacency(n, edges)
        g.set_matrix(A)
        assert len(g) == n
        clique, rejected = g.solve()
        assert clique.dtype == np.int32 and clique.tolist() == members.tolist(), (k, n)
        assert rejected == n - size and 1 <= g.rounds <= size + 1, (k, g.rounds, size)
        again, _ = g.solve()
        assert again.tolist() == members.tolist(), k
        assert np.array_equal(g.matrix(), A), k


def test_clique_of_4096_vertices(pcm):
    """the last lane and the last word: a planted near-clique of 600 that includes vertex 4095, background density 0.02"""
    A, size, members = PC.big_graph()
    assert size > 100 and 4095 in members
    g = pcm.PcmGraph()
    assert g.capacity == 4096
    g.set_matrix(A)
    clique, rejected = g.solve()
    assert clique.tolist() == list(members) and rejected == 4096 - size and g.rounds <= size + 1
    assert A[np.ix_(clique, clique)].sum() == size * (size - 1)


# ------------------------------------------------------------------ the matrix
@pytest.mark.parametrize("p", [0.01, 0.75])
@pytest.mark.parametrize("L", PC.SIZES)
def test_matrix_and_distances(pcm, L, p):
    want_d = PC.expected(L)
    thr = R.THRESHOLDS[p]
    off = ~np.eye(L, dtype=bool)
    assert L == 1 or np.abs(want_d[off] - thr).min() > PC.MARGIN          # a condition on the inputs: no pair is excluded
    g = _loaded(pcm, L, p)
    assert len(g) == L and g.threshold == thr
    d = g.distances()
    print("L = %d p = %g: max |d - restatement| = %.3g" % (L, p, np.abs(d - want_d).max() if L > 1 else 0.0))
    assert np.abs(d - want_d).max() <= TOL
    assert np.array_equal(d, d.T) and not d.diagonal().any()
    A = g.matrix()
    assert A.dtype == bool and np.array_equal(A, R.consistency_matrix(want_d, thr))
    assert np.array_equal(A, A.T) and not A.diagonal().any()
    g.clear()
    XA, XB, ia, kb, Z = PC.scene(L)
    g.add_loops(ia, kb, Z)
    assert np.array_equal(g.matrix(), A) and g.distances().tobytes() == d.tobytes()      # the same bits on a second run


def test_every_logmap_branch(pcm):
    """two-loop scenes whose consistency pose is a given one: no rotation, the small-angle and series branches, half turns about each axis
    and a skew one.  At 7.840 the half turns (distance about 3.7) are consistent, at 0.872 they are not."""
    for p, want_bits in ((0.01, [False] * 7), (0.75, [True, False, True, True, True, True, True])):
        g = pcm.PcmGraph(capacity=2, p=p)
        bits = []
        for k, sc in enumerate(PC.branch_scenes()):
            want = R.consistency_distances(*sc)
            g.set_trajectories(sc[0], sc[1])
            g.add_loops(*sc[2:])
            d = g.distances()
            assert np.abs(d - want).max() <= TOL, (k, d[0, 1], want[0, 1])
            assert abs(want[0, 1] - g.threshold) > PC.MARGIN
            assert np.array_equal(g.matrix(), R.consistency_matrix(want, g.threshold)), k
            bits.append(bool(g.matrix()[0, 1]))
        assert bits == want_bits, (p, bits)


# ------------------------------------------------------------------ appending
def test_appending_gives_the_same_bits(pcm):
    L = 129
    XA, XB, ia, kb, Z = PC.scene(L)
    whole = _loaded(pcm, L, 0.75)
    A, clique = whole.matrix(), whole.solve()[0]
    g = pcm.PcmGraph(capacity=L, p=0.75)
    g.set_trajectories(XA, XB)
    lo = 0
    for n in (1, 62, 1, 65):
        g.add_loops(ia[lo:lo + n], kb[lo:lo + n], Z[lo:lo + n])
        lo += n
        assert len(g) == lo and np.array_equal(g.matrix(), A[:lo, :lo]), lo
    assert np.array_equal(g.solve()[0], clique)
    g.clear()
    assert len(g) == 0 and g.matrix().shape == (0, 0)
    g.add_loops(ia, kb, Z)
    assert np.array_equal(g.matrix(), A) and np.array_equal(g.solve()[0], clique)
    g.set_trajectories(XA, XB)                                   # clears the loops as well
    assert len(g) == 0


# ------------------------------------------------------------------ end to end
@pytest.mark.parametrize("p", [0.01, 0.75])
@pytest.mark.parametrize("L", PC.SIZES)
def test_solve_end_to_end(pcm, L, p):
    size, members = PC.expected_clique(L, p)
    g = _loaded(pcm, L, p, capacity=4096 if L == 129 else None)    # a capacity above the loops held: rows wider than they need
    clique, rejected = g.solve()
    assert clique.tolist() == list(members) and rejected == L - size and g.rounds <= size + 1
    A = g.matrix()
    assert len(set(clique.tolist())) == size and A[np.ix_(clique, clique)].sum() == size * (size - 1)


# ------------------------------------------------------------------ edges
def test_no_loops(pcm):
    g = pcm.PcmGraph(capacity=8)
    clique, rejected = g.solve()
    assert clique.size == 0 and clique.dtype == np.int32 and rejected == 0 and g.rounds == 0
    assert g.matrix().shape == (0, 0) and g.distances().shape == (0, 0)
    g.set_matrix(np.zeros((0, 0)))
    assert g.solve()[0].size == 0


def test_nan_loop_is_an_isolated_vertex(pcm):
    L = 65
    XA, XB, ia, kb, Z = PC.scene(L)
    Z = Z.copy()
    Z[7, 1, 3] = np.nan
    Z[64, 0, 0] = np.inf
    g = pcm.PcmGraph(capacity=L, p=0.75)
    g.set_trajectories(XA, XB)
    g.add_loops(ia, kb, Z)
    A = g.matrix()
    for u in (7, 64):
        assert not A[u].any() and not A[:, u].any()
    keep = np.ones(L, bool)
    keep[[7, 64]] = False
    want = R.consistency_matrix(PC.expected(L), g.threshold)
    assert np.array_equal(A[np.ix_(keep, keep)], want[np.ix_(keep, keep)])
    clique, _ = g.solve()
    assert clique.tolist() == R.max_clique_heu(A)[1] and 7 not in clique and 64 not in clique
    assert np.isnan(g.distances()[7, 8])


def test_refusals(pcm):
    from mr_slam_amd import _lib
    XA, XB, ia, kb, Z = PC.scene(63)
    g = pcm.PcmGraph(capacity=64)
    g.set_trajectories(XA, XB)
    g.add_loops(ia[:10], kb[:10], Z[:10])
    A = g.matrix()
    for bad_ia, bad_kb in (([0, PC.N_POSES], [0, 0]), ([0, 0], [0, PC.N_POSES]), ([-1, 0], [0, 0]), ([0, 0], [0, -1])):
        with pytest.raises(_lib.MrsError) as e:                   # an index outside its trajectory: nothing is added
            g.add_loops(bad_ia, bad_kb, Z[:2])
        assert e.value.status == 1 and len(g) == 10
    with pytest.raises(_lib.MrsError) as e:                       # one loop more than the capacity
        g.add_loops(ia[:55], kb[:55], Z[:55])
    assert e.value.status == 3 and len(g) == 10 and np.array_equal(g.matrix(), A)
    g.add_loops(ia[:54], kb[:54], Z[:54])
    assert len(g) == 64
    with pytest.raises(_lib.MrsError) as e:
        pcm.PcmGraph(capacity=4097)
    assert e.value.status == 3
    for bad in (dict(capacity=0), dict(threshold=0.0), dict(threshold=float("nan")), dict(threshold=float("inf"))):
        with pytest.raises(_lib.MrsError) as e:
            pcm.PcmGraph(**bad)
        assert e.value.status == 1
    with pytest.raises(ValueError):
        pcm.PcmGraph(p=0.3)
    # a given matrix must be symmetric with a zero diagonal; a refused one changes nothing
    S = np.zeros((5, 5), bool)
    S[1, 2] = S[2, 1] = True
    g.set_matrix(S)
    for r, c in ((0, 3), (4, 4)):
        B = S.copy()
        B[r, c] = True
        with pytest.raises(_lib.MrsError) as e:
            g.set_matrix(B)
        assert e.value.status == 1 and np.array_equal(g.matrix(), S)
    with pytest.raises(_lib.MrsError) as e:
        g.set_matrix(np.zeros((65, 65)))
    assert e.value.status == 3
    assert g.solve()[0].tolist() == [1, 2]
    for call in (g.distances, lambda: g.add_loops(ia[:1], kb[:1], Z[:1])):       # given vertices have no geometry
        with pytest.raises(_lib.MrsError) as e:
            call()
        assert e.value.status == 1
    g.clear()
    g.add_loops(ia[:1], kb[:1], Z[:1])
    assert len(g) == 1 and g.solve()[0].tolist() == [0]
