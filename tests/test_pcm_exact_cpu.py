"""CPU suite for the exact maximum clique of pairwise consistency: the fixture of what the reference's own FMC::maxClique
returned (tests/golden/ref_pcm_maxclique.npz) is present and complete, the plain-Python restatement (tests/golden/pcm_exact_restate.py)
returns its sizes and lists number for number, an independent enumeration of all maximum cliques confirms the rule behind the lists, the
fixture has graphs on which the heuristic falls short, and the C-ABI symbol is exported, bound and checks its arguments."""
import ctypes as C
import os

import numpy as np
import pytest

import pcm_cases as PC

import pcm_exact_restate as X  # noqa: E402  (pcm_cases puts tests/golden on the path)

R = PC.R


@pytest.fixture(scope="module")
def graphs():
    return X.load()


@pytest.fixture(scope="module")
def restated(graphs):
    return [X.max_clique_exact(X.adjacency(n, e)) for _, n, e, _, _ in graphs]


def test_fixture_present_and_complete(graphs):
    names = [g[0] for g in graphs]
    assert names[:26] == ["clique_fixture_%d" % k for k in range(26)]
    shared = R.load()
    for k in range(26):                                          # the graphs of ref_pcm_clique.npz, stored there only
        assert graphs[k][1] == shared[k][0] and np.array_equal(graphs[k][2], shared[k][1])
    want = ["random_5_300_0.3_30", "random_5_200_0.5_20", "pair_without_edge", "pair_with_edge"]
    want += ["scene_%d_%d_%g" % (L, s, p) for L in (65, 129) for s in range(4) for p in (0.01, 0.25)]
    assert sorted(names[26:]) == sorted(want)
    ns = {g[1] for g in graphs}
    for n in (1, 2, 3, 63, 64, 65, 128, 129):
        assert n in ns, n
    by_name = {g[0]: g for g in graphs}
    assert by_name["pair_without_edge"][3] == 1 and by_name["pair_without_edge"][4].tolist() == [1]      # no edges: [L - 1]
    assert by_name["pair_with_edge"][4].tolist() == [0, 1]
    assert (70, 0, 1, [69]) in [(g[1], len(g[2]), g[3], g[4].tolist()) for g in graphs]                        # an empty graph
    assert (65, 65 * 64 // 2, 65, list(range(65))) in [(g[1], len(g[2]), g[3], g[4].tolist()) for g in graphs]    # a complete one
    for name, n, edges, size, members in graphs:
        A = X.adjacency(n, edges)
        assert members.size == size and (np.diff(members) > 0).all(), name                   # ascending
        assert A[np.ix_(members, members)].sum() == size * (size - 1), name                  # a clique
    assert os.path.getsize(X.FIXTURE) < 512 * 1024


def test_scene_graphs_are_the_scenes_and_keep_the_margin(graphs):
    """the fixture's scene graphs are the restatement's matrices of pcm_cases.scene, and no distance lies within MARGIN of a threshold: the
    GPU suite loads the same scenes as geometry and expects the same matrices"""
    by_name = {g[0]: g for g in graphs}
    for L in (65, 129):
        for seed in range(4):
            D = R.consistency_distances(*PC.scene(L, seed))
            off = ~np.eye(L, dtype=bool)
            for p in (0.01, 0.25):
                assert np.abs(D[off] - R.THRESHOLDS[p]).min() > PC.MARGIN, (L, seed, p)
                _, n, edges, _, _ = by_name["scene_%d_%d_%g" % (L, seed, p)]
                assert np.array_equal(X.adjacency(n, edges), R.consistency_matrix(D, R.THRESHOLDS[p])), (L, seed, p)


def test_restatement_returns_the_reference_cliques(graphs, restated):
    """the recorded size AND member list of every graph"""
    for (name, n, _, size, members), (got_size, got, nodes) in zip(graphs, restated):
        assert got_size == size and got == members.tolist(), name
        assert nodes >= size
    assert X.max_clique_exact(np.zeros((0, 0), bool)) == (0, [], 0)
    assert X.max_clique_exact(np.zeros((5, 5), bool))[:2] == (1, [4])


def test_rule_agrees_with_the_restatement_on_small_graphs(graphs, restated):
    """all maximum cliques by Bron-Kerbosch, the lexicographically largest descending sequence of them: the restatement's list"""
    checked = tied = 0
    for (name, n, edges, _, _), (size, members, _) in zip(graphs, restated):
        if n > 70:
            continue
        A = X.adjacency(n, edges)
        assert X.canonical_maximum_clique(A) == (size, members), name
        tied += len(X.all_maximum_cliques(A)) > 1
        checked += 1
    assert checked >= 15 and tied >= 3                           # the rule is exercised: several graphs have more than one maximum clique
    T = np.zeros((4, 4), bool)                                   # two maximum cliques {0, 3} and {1, 2}: descending (3, 0) beats (2, 1)
    T[0, 3] = T[3, 0] = T[1, 2] = T[2, 1] = True
    assert X.canonical_maximum_clique(T) == (2, [0, 3]) and X.max_clique_exact(T)[:2] == (2, [0, 3])
    assert X.canonical_maximum_clique(np.zeros((0, 0), bool)) == (0, [])


def test_fixture_keeps_its_teeth(graphs):
    """on at least four graphs the exact size exceeds the heuristic's, among them the ones the GPU suite names"""
    larger = [name for name, n, edges, size, _ in graphs if size > R.max_clique_heu(X.adjacency(n, edges))[0]]
    assert len(larger) >= 4, larger
    for name in ("clique_fixture_15", "clique_fixture_19", "random_5_300_0.3_30", "random_5_200_0.5_20", "scene_129_0_0.25", "scene_129_3_0.25"):
        assert name in larger, name
    for name, n, edges, size, _ in graphs:
        assert size >= R.max_clique_heu(X.adjacency(n, edges))[0], name


def test_solve_exact_exported_bound_and_checked():
    from mr_slam_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = C.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "mrs_pcm_solve_exact") and lib.mrs_abi_version() == 1
    api = _lib.load()
    assert callable(api.mrs_pcm_solve_exact)
    from mr_slam_amd import pcm
    header = open(_lib.HEADER).read()
    assert "#define MRS_PCM_EXACT_DEFAULT_NODES %d" % pcm.EXACT_DEFAULT_NODES in header and pcm.EXACT_DEFAULT_NODES > 0
    assert "#define MRS_PCM_EXACT_OVERSHOOT %d" % pcm.EXACT_OVERSHOOT in header
    launch = int(header.split("#define MRS_PCM_EXACT_LAUNCH_NODES")[1].split()[0])
    waves = int(header.split("#define MRS_PCM_EXACT_MAX_WAVES")[1].split()[0])
    assert pcm.EXACT_OVERSHOOT == launch * waves                 # concurrent waves x the per-launch cap
    n, proof, nodes = C.c_int32(0), C.c_int32(0), C.c_int64(0)
    clique = np.zeros(4, np.int32)
    with pytest.raises(_lib.MrsError) as e:                      # the C side's checks, no GPU involved
        api.mrs_pcm_solve_exact(None, 10, clique, C.byref(n), C.byref(proof), C.byref(nodes))
    assert e.value.status == 1 and "null pointer" in str(e.value)
    with pytest.raises(_lib.MrsError) as e:
        api.mrs_pcm_solve_exact(None, -1, clique, C.byref(n), C.byref(proof), C.byref(nodes))
    assert e.value.status == 1 and "negative" in str(e.value)
    with pytest.raises(TypeError):                               # the binding takes the element type from the header
        api.mrs_pcm_solve_exact(None, 10, np.zeros(4, np.int64), C.byref(n), C.byref(proof), C.byref(nodes))
