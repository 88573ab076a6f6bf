"""GPU suite for the exact maximum clique of pairwise consistency (PcmGraph.solve_exact over mrs_pcm_solve_exact): every
fixture graph against what the reference's own FMC::maxClique returned (tests/golden/ref_pcm_maxclique.npz), the whole path from geometry
against the restatement (tests/golden/pcm_exact_restate.py), the order of loading, the heuristic left alone, the node budget, and the
edges.  test_pcm_exact_cpu.py checks the conditions on the inputs."""
import numpy as np
import pytest

import pcm_cases as PC

import pcm_exact_restate as X  # noqa: E402  (pcm_cases puts tests/golden on the path)

R = PC.R
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pcm():
    from mr_slam_amd import pcm
    return pcm


@pytest.fixture(scope="module")
def graphs():
    return X.load()


def _loaded(pcm, L, seed, p, parts=(None,)):
    g = pcm.PcmGraph(capacity=L, p=p)
    XA, XB, ia, kb, Z = PC.scene(L, seed)
    g.set_trajectories(XA, XB)
    lo = 0
    for n in parts:
        hi = L if n is None else lo + n
        g.add_loops(ia[lo:hi], kb[lo:hi], Z[lo:hi])
        lo = hi
    assert len(g) == L
    return g


# ------------------------------------------------------------------ 1. the fixture graphs
def test_exact_clique_of_every_fixture_graph(pcm, graphs):
    """size and member list as recorded from the reference, proven within the default budget"""
    g = pcm.PcmGraph(capacity=320)
    assert {1, 2, 3, 63, 64, 65, 128, 129} <= {n for _, n, _, _, _ in graphs}
    for name, n, edges, size, members in graphs:
        g.set_matrix(X.adjacency(n, edges))
        clique, rejected = g.solve_exact()
        print("%-24s n = %3d  size = %3d  proof = %d  nodes = %d" % (name, n, clique.size, g.proof, g.nodes))
        assert g.proof == 2, name
        assert clique.dtype == np.int32 and clique.tolist() == members.tolist(), name
        assert rejected == n - size and 0 < g.nodes <= pcm.EXACT_DEFAULT_NODES + pcm.EXACT_OVERSHOOT, name


# ------------------------------------------------------------------ 2. geometry end to end
@pytest.mark.parametrize("p", [0.01, 0.25])
@pytest.mark.parametrize("L", [65, 129])
def test_solve_exact_end_to_end(pcm, L, p):
    for seed in (0, 3):
        A = R.consistency_matrix(R.consistency_distances(*PC.scene(L, seed)), R.THRESHOLDS[p])
        size, members, _ = X.max_clique_exact(A)
        g = _loaded(pcm, L, seed, p)
        assert np.array_equal(g.matrix(), A)
        clique, rejected = g.solve_exact()
        assert g.proof == 2 and clique.tolist() == members and rejected == L - size, (L, seed, p)
        if (L, seed, p) == (129, 3, 0.25):
            assert len(clique) > len(g.solve()[0])


# ------------------------------------------------------------------ 3. the order of loading
def test_order_of_loading(pcm):
    whole = _loaded(pcm, 129, 3, 0.25).solve_exact()[0]
    g = _loaded(pcm, 129, 3, 0.25, parts=(1, 63, None))
    clique, _ = g.solve_exact()
    assert g.proof == 2 and clique.tolist() == whole.tolist()


# ------------------------------------------------------------------ 4. the heuristic is left alone
def test_heuristic_untouched(pcm):
    g = _loaded(pcm, 129, 3, 0.25)
    before, rounds = g.solve()[0], g.rounds
    exact, _ = g.solve_exact()
    assert g.rounds == rounds                                    # solve_exact does not write it
    after = g.solve()[0]
    assert before.tolist() == after.tolist() and g.rounds == rounds
    assert before.tolist() == list(PC.expected_clique(129, 0.25, 3)[1]) and exact.size > before.size


# ------------------------------------------------------------------ 5. the budget
def test_budget(pcm):
    A, size, members = PC.big_graph()
    g = pcm.PcmGraph()
    g.set_matrix(A)
    clique, rejected = g.solve_exact(max_nodes=20000)
    print("big graph, budget 20000: size = %d (heuristic %d)  proof = %d  nodes = %d" % (clique.size, size, g.proof, g.nodes))
    assert 0 <= g.nodes <= 20000 + pcm.EXACT_OVERSHOOT and g.proof in (0, 1, 2)
    assert A[np.ix_(clique, clique)].sum() == clique.size * (clique.size - 1)            # every pair adjacent
    assert (np.diff(clique) > 0).all() and clique.size >= size and rejected == 4096 - clique.size
    clique, _ = g.solve_exact(max_nodes=0)
    assert clique.tolist() == sorted(members) and g.proof == 0 and g.nodes == 0


# ------------------------------------------------------------------ 6. repeatability and edges
def test_repeatable(pcm, graphs):
    _, n, edges, size, members = {g[0]: g for g in graphs}["random_5_200_0.5_20"]
    g = pcm.PcmGraph(capacity=n)
    g.set_matrix(X.adjacency(n, edges))
    first, _ = g.solve_exact()
    assert g.proof == 2
    second, _ = g.solve_exact()
    assert g.proof == 2 and first.tolist() == second.tolist() == members.tolist()


def test_no_loops_and_refusals(pcm):
    from mr_slam_amd import _lib
    g = pcm.PcmGraph(capacity=8)
    clique, rejected = g.solve_exact()
    assert clique.size == 0 and clique.dtype == np.int32 and rejected == 0 and g.proof == 2 and g.nodes == 0
    with pytest.raises(_lib.MrsError) as e:
        g.solve_exact(max_nodes=-1)
    assert e.value.status == 1
    g.set_matrix(np.zeros((5, 5)))                               # no edges: the last vertex
    assert g.solve_exact()[0].tolist() == [4] and g.proof == 2
