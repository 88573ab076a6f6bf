"""Plain-Python restatement of the reference's exact clique finder FMC::maxClique(gio, 0, data)
(Mapping/src/global_manager/src/pairwise_consistency_maximization/third_parties/fast_max-clique_finder/src/findClique.cpp:29-154), the call
GlobalMap keeps as a comment beside its heuristic (global_map.cpp:52), and an independent rule for what it returns.  DESIGN.md 4.21 holds
the contract.

The reference takes its start vertices from n - 1 down, gives each the smaller neighbours it has not started from, and in its helper always
pops the LARGEST candidate and keeps the smaller common neighbours: it walks cliques, written as descending sequences, in descending
lexicographic order, and adopts strict improvements only.  So it returns the size of a maximum clique and, of all maximum cliques, the one
whose descending sequence is lexicographically largest; the members are pushed while the recursion unwinds, that is in ascending order.  Its
two prunes (size of clique + candidates left <= best; degree in the whole graph < best) never cut a strict improvement off.

Vertex sets are Python integers used as bit sets.  ref_pcm_maxclique.npz (written by tools/make_pcm_exact_golden.py) holds graphs and what
the reference's own maxClique returned for them."""
import os

import numpy as np

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref_pcm_maxclique.npz")


def bit_rows(A):
    """the rows of a boolean adjacency as integers: bit v of rows[u] is A[u, v]"""
    A = np.asarray(A, bool)
    return [int.from_bytes(np.packbits(A[u], bitorder="little").tobytes(), "little") for u in range(A.shape[0])]


def max_clique_exact(A):
    """FMC::maxClique(gio, 0, data) on a symmetric boolean adjacency with a zero diagonal -> (size, ascending member list, nodes).  A node is
    one vertex taken into the current clique, a start vertex included.  (0, [], 0) for no vertex."""
    N = bit_rows(A)
    n = len(N)
    deg = [bin(r).count("1") for r in N]
    state = {"best": 0, "members": [], "nodes": 0, "elig_for": None, "elig": 0}
    path = []

    def eligible():
        # the vertices whose degree is at least the best size so far (Pruning 3 / 5); the mask is rebuilt when the best size rises
        if state["elig_for"] != state["best"]:
            state["elig_for"] = state["best"]
            state["elig"] = sum(1 << v for v in range(n) if deg[v] >= state["best"])
        return state["elig"]

    def helper(U, size):
        if not U:
            if size > state["best"]:
                state["best"], state["members"] = size, sorted(path)
            return
        while U:
            if size + bin(U).count("1") <= state["best"]:
                return
            v = U.bit_length() - 1                               # the back of the reference's ascending list
            U ^= 1 << v
            state["nodes"] += 1
            path.append(v)
            helper(U & N[v] & eligible(), size + 1)
            path.pop()

    for i in range(n - 1, -1, -1):
        if deg[i] < state["best"]:                               # Pruning 1
            continue
        state["nodes"] += 1
        path.append(i)
        helper(N[i] & ((1 << i) - 1) & eligible(), 1)            # Pruning 2: only the vertices not started from yet, all of them smaller
        path.pop()
    return state["best"], state["members"], state["nodes"]


def all_maximum_cliques(A):
    """every maximum clique as an ascending tuple: Bron-Kerbosch with a pivot over all maximal cliques, the largest kept"""
    N = bit_rows(A)
    n = len(N)
    out = {"size": 0, "cliques": []}

    def bits(x):
        while x:
            low = x & -x
            yield low.bit_length() - 1
            x ^= low

    def expand(R, P, X):
        if not P and not X:
            if len(R) > out["size"]:
                out["size"], out["cliques"] = len(R), []
            if len(R) == out["size"]:
                out["cliques"].append(tuple(sorted(R)))
            return
        if len(R) + bin(P).count("1") < out["size"]:
            return
        pivot = max(bits(P | X), key=lambda u: bin(P & N[u]).count("1"))
        for v in bits(P & ~N[pivot]):
            expand(R + [v], P & N[v], X & N[v])
            P &= ~(1 << v)
            X |= 1 << v

    if n:
        expand([], (1 << n) - 1, 0)
    return out["cliques"]


def canonical_maximum_clique(A):
    """the rule: of all maximum cliques the one whose members, sorted descending, are lexicographically largest -> (size, ascending list)"""
    cliques = all_maximum_cliques(A)
    if not cliques:
        return 0, []
    best = max(cliques, key=lambda c: c[::-1])
    return len(best), list(best)


def load():
    """[(name, n, edges int32 [m, 2] with u < v in row-major order, size, ascending members)] of the fixture.  The graphs it shares with
    ref_pcm_clique.npz are stored there only: `source` names their index, -1 marks a graph of this file's own."""
    import pcm_restate
    z = np.load(FIXTURE)
    shared = pcm_restate.load()
    out = []
    for g in range(z["n"].size):
        src = int(z["source"][g])
        edges = shared[src][1] if src >= 0 else z["edges_%d" % g]
        out.append((str(z["names"][g]), int(z["n"][g]), edges, int(z["size"][g]), z["members_%d" % g]))
    return out


def adjacency(n, edges):
    A = np.zeros((n, n), bool)
    if len(edges):
        A[edges[:, 0], edges[:, 1]] = True
        A[edges[:, 1], edges[:, 0]] = True
    return A
