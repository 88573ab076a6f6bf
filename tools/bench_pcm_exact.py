"""The exact maximum clique on the GPU (PcmGraph.solve_exact): wall time, launches, nodes, nodes per second, proof, and the
size beside the heuristic's, on
  - the scene of tools/bench_pcm.py (two 2 000-pose trajectories, 70 % inliers) at L = 256 / 1024 / 4096 and p = 0.01, and
  - scenes in the style of tests/pcm_cases.py (40 random poses per trajectory, 60 % inliers) at L = 256 / 1024 and p = 0.25.
Prints ONE JSON line and, with --out, writes it to a file.  Run on its own; neither the tests nor bench.py call it.

Both baselines are measured in the same run, never taken from the new code:
  (a) the reference's own FMC::maxClique on the same graph, through the Matrix-Market file the reference writes, under a time limit, when
      `tools/make_pcm_exact_golden.py --keep-binary` has built it on this machine; "did not finish in T s" or "not available" otherwise;
  (b) the plain-Python restatement (tests/golden/pcm_exact_restate.py), in a child process under the same limit.
Where a baseline finishes, its size and list are compared with the GPU's."""
import argparse
import json
import multiprocessing
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

CASES = (("bench_pcm", 256, 0.01), ("bench_pcm", 1024, 0.01), ("bench_pcm", 4096, 0.01), ("pcm_cases", 256, 0.25), ("pcm_cases", 1024, 0.25))
FMC_BINARY = os.path.join(ROOT, "build", "pcm_fmc_exact_ref")


def _restate(A, q):
    import pcm_exact_restate as X
    t0 = time.perf_counter()
    size, members, nodes = X.max_clique_exact(A)
    q.put((size, members, nodes, (time.perf_counter() - t0) * 1e3))


def restatement(A, limit):
    """(size, members, nodes, ms) of the Python restatement in a child process, or None after `limit` seconds"""
    ctx = multiprocessing.get_context("spawn")                   # a fresh process: the parent holds the GPU
    q = ctx.Queue()
    child = ctx.Process(target=_restate, args=(A, q))
    child.start()
    try:
        return q.get(timeout=limit)
    except Exception:
        return None
    finally:
        if child.is_alive():
            child.terminate()
        child.join()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--limit", type=float, default=20.0, help="seconds each baseline may take per graph")
    ap.add_argument("--max-nodes", type=int, default=None)
    a = ap.parse_args()
    import torch
    import bench_pcm
    import make_pcm_exact_golden as M
    import pcm_cases as PC
    from mr_slam_amd import pcm
    assert torch.cuda.is_available(), "needs a GPU (there is no CPU fallback)"
    have_fmc = os.path.exists(FMC_BINARY)
    out = {"metric": "pcm_exact", "runs": "one run; wall time is the median of %d calls (one call where it took more than 5 s)" % a.reps, "baseline_limit_s": a.limit,
           "default_nodes": pcm.EXACT_DEFAULT_NODES, "max_nodes": pcm.EXACT_DEFAULT_NODES if a.max_nodes is None else a.max_nodes, "cases": {}}
    for style, L, p in CASES:
        scene = bench_pcm.make_scene(L)[:5] if style == "bench_pcm" else PC.scene(L, 0)
        g = pcm.PcmGraph(capacity=L, p=p)
        g.set_trajectories(scene[0], scene[1])
        g.add_loops(*scene[2:])
        A = g.matrix()
        heuristic, _ = g.solve()
        wall = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            clique, _ = g.solve_exact(a.max_nodes)
            wall.append((time.perf_counter() - t0) * 1e3)
            if wall[-1] > 5e3:                                   # a call of seconds is not repeated
                break
        ms = float(np.median(wall))
        assert A[np.ix_(clique, clique)].sum() == clique.size * (clique.size - 1), "not a clique"
        r = {"loops": L, "p": p, "edges": int(A.sum() // 2), "solve_exact_wall_ms": ms, "launches": g.launches, "nodes": g.nodes,
             "nodes_per_s": g.nodes / (ms * 1e-3), "proof": g.proof, "size": int(clique.size), "heuristic_size": int(heuristic.size)}
        t0 = time.perf_counter()
        g.solve()
        r["solve_heuristic_wall_ms"] = (time.perf_counter() - t0) * 1e3
        if have_fmc:
            with tempfile.TemporaryDirectory() as d:
                got = M.run_fmc(FMC_BINARY, L, M.G.edges_of(A), d, limit=a.limit)
            if got is None:
                r["baseline_reference_maxclique_ms"] = "did not finish in %g s" % a.limit
            else:
                r["baseline_reference_maxclique_ms"] = got[2]
                if g.proof == 2:
                    assert got[0] == clique.size and got[1].tolist() == clique.tolist(), "the reference's maxClique disagrees"
        else:
            r["baseline_reference_maxclique_ms"] = "not available"
        got = restatement(A, a.limit)
        if got is None:
            r["baseline_python_restatement_ms"] = "did not finish in %g s" % a.limit
        else:
            r["baseline_python_restatement_ms"], r["baseline_python_restatement_nodes"] = got[3], got[2]
            if g.proof == 2:
                assert got[0] == clique.size and got[1] == clique.tolist(), "the restatement disagrees"
        out["cases"]["%s_L%d_p%g" % (style, L, p)] = r
        print("%s L = %d p = %g done" % (style, L, p), file=sys.stderr, flush=True)
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
