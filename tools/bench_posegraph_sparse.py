"""The sparse elimination tier of the pose-graph optimiser (PoseGraph.set_solver("sparse")) on the scenes of
tools/bench_posegraph.py: three robots of 2 000 poses each with 256 random loops under both solvers, and with 1024, 2048 and 4096 loops,
which the dense solver refuses, under the sparse one.  Per leg: whole blocking `optimize` calls (wall clock; stage 1 is computed again in
every call), the stages and the tier's own time between HIP events (the library's development timing switch), and the symbolic phase's
numbers.  Prints ONE JSON line and, with --out, writes it to a file.  Run on its own.

Both baselines are measured in the same run, never taken from the new code: the dense solver at 256 loops (the path every graph took before
the tier existed) and the NumPy / scipy restatement (tests/golden/posegraph_restate.py, sparse LU per iteration) with the same stop rule,
against which every leg's result is also compared.

--stats-only needs no GPU: levels, blocks and block products per scene for MRS_PGO_SPARSE_DEGREE_SLACK = 0 and 1 from the ordering
restatement (tests/golden/posegraph_order_restate.py), the trade the constant decides (the library itself is built with one value)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_posegraph import POSES, ROBOTS, STAGES, make_scene  # noqa: E402

BOTH, SPARSE_ONLY = (256,), (1024, 2048, 4096)
STATS = ("separators", "eliminated", "core", "levels", "blocks", "updates", "max_degree")


def slack_trade(scene, segment_length, dense_limit):
    """{slack: the symbolic phase's numbers of stage 2} by the ordering restatement"""
    import posegraph_order_restate as OR
    chain_lengths, _, li, lj, _ = scene
    sep, edges = OR.block_graph(chain_lengths, li.tolist(), lj.tolist(), segment_length, 2)
    out = {}
    for slack in (0, 1):
        t0 = time.perf_counter()
        o = OR.order(len(sep), edges, dense_limit, slack)
        out[str(slack)] = dict(zip(STATS, OR.stats(o)), restatement_seconds=time.perf_counter() - t0)
    return out


def leg(g, solver, dense_limit, reps, want):
    g.set_solver(solver, dense_limit=dense_limit)
    t0 = time.perf_counter()
    got = g.optimize()                                            # warm: the symbolic phase and the allocations
    first = (time.perf_counter() - t0) * 1e3
    wall, stages, tier = [], [], []
    for _ in range(reps):
        g.set_prior(np.eye(4))                                    # marks the graph changed: stage 1 runs again, as after a new closure
        t0 = time.perf_counter()
        got = g.optimize()
        wall.append((time.perf_counter() - t0) * 1e3)
        stages.append(g.stage_ms())
        tier.append(g.tier_ms())
    med, tmed = np.median(np.array(stages), axis=0), np.median(np.array(tier), axis=0)
    e = {"solver": solver, "dense_limit": dense_limit, "first_call_wall_ms": first, "optimize_wall_ms": float(np.median(wall)), "optimize_wall_ms_min_max": [min(wall), max(wall)],
         "iterations": got.iterations, "converged": got.converged, "separators": got.separators,
         "stages_ms": {k: float(v) for k, v in zip(STAGES, med)},
         "tier_ms": {"columns_and_core_update": float(tmed[0]), "way_back": float(tmed[1]), "per_iteration": float(tmed.sum()) / got.iterations},
         "stats_stage1": g.solver_stats(1)._asdict(), "stats_stage2": g.solver_stats(2)._asdict()}
    if want is not None:
        e["max_abs_vs_restatement_R"] = float(np.abs(got.T[:, :3, :3] - want.T[:, :3, :3]).max())
        e["max_abs_vs_restatement_t"] = float(np.abs(got.T[:, :3, 3] - want.T[:, :3, 3]).max())
        e["restatement_iterations"] = want.iterations
    return e, got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--loops", type=int, nargs="*", default=list(BOTH + SPARSE_ONLY))
    ap.add_argument("--dense-limit", type=int, default=None, help="the sparse legs' dense_limit (default: the library's)")
    ap.add_argument("--no-restatement", dest="restatement", action="store_false", help="skip the scipy restatement (baseline and check)")
    ap.add_argument("--stats-only", action="store_true", help="no GPU: the symbolic phase for both values of the degree slack")
    a = ap.parse_args()
    out = {"metric": "posegraph_sparse", "robots": ROBOTS, "poses_per_robot": POSES, "scenes": {}}
    if a.stats_only:
        import re
        header = open(os.path.join(ROOT, "include", "mrslam_hip.h")).read()
        cap, seglen = (int(re.search(r"#define\s+%s\s+(\d+)" % n, header)[1]) for n in ("MRS_PGO_MAX_SEPARATORS", "MRS_PGO_DEFAULT_SEGMENT_LENGTH"))
        limit = cap if a.dense_limit is None else a.dense_limit
        out.update(segment_length=seglen, dense_limit=limit)
        for L in a.loops:
            out["scenes"][str(L)] = {"loops": L, "slack": slack_trade(make_scene(L), seglen, limit)}
            print("loops %d: %s" % (L, out["scenes"][str(L)]["slack"]), file=sys.stderr, flush=True)
    else:
        os.environ["MRS_DEV"] = "1"
        os.environ["MRS_PGO_TIMING"] = "1"
        import torch
        import posegraph_restate as R
        assert torch.cuda.is_available(), "needs a GPU (there is no CPU fallback)"
        from mr_slam_amd import posegraph
        out.update(eps=posegraph.DEFAULT_EPS, segment_length=posegraph.DEFAULT_SEGMENT_LENGTH, degree_slack=posegraph.SPARSE_DEGREE_SLACK,
                   dense_limit=posegraph.MAX_SEPARATORS if a.dense_limit is None else a.dense_limit,
                   runs="one run; medians of %d repetitions after a warm call" % a.reps)
        for L in a.loops:
            scene = make_scene(L)
            chain_lengths, odom, li, lj, lZ = scene
            r = {"loops": L, "legs": []}
            want = None
            if a.restatement:
                t0 = time.perf_counter()
                want = R.optimize(*scene)
                r["baseline_restatement_ms"] = (time.perf_counter() - t0) * 1e3
                r["baseline_restatement_iterations"] = want.iterations
            g = posegraph.PoseGraph(chain_lengths)
            g.set_odometry(odom)
            g.set_solver("sparse", dense_limit=a.dense_limit)
            t0 = time.perf_counter()
            g.add_loops(li, lj, lZ)
            r["add_loops_with_budget_check_ms"] = (time.perf_counter() - t0) * 1e3
            # where both solvers take the graph: a third leg with every separator through the tier, the same system as the dense leg's
            for solver, limit in ((("dense", None), ("sparse", a.dense_limit), ("sparse", 0)) if L in BOTH else (("sparse", a.dense_limit),)):
                e, got = leg(g, solver, limit, a.reps, want)
                if want is not None and got.iterations == want.iterations:
                    assert max(e["max_abs_vs_restatement_R"], e["max_abs_vs_restatement_t"]) < 1e-8, e
                r["legs"].append(e)
                print("loops %d %s: %.1f ms, %d iterations, tier %.2f ms per iteration, %s" % (L, solver, e["optimize_wall_ms"], got.iterations,
                                                                                            e["tier_ms"]["per_iteration"], e["stats_stage2"]),
                      file=sys.stderr, flush=True)
                if a.out:                                         # what is measured so far survives a leg that runs out of time
                    out["scenes"][str(L)] = r
                    _write(a.out, out)
            out["scenes"][str(L)] = r
    print(json.dumps(out))
    if a.out:
        _write(a.out, out)


def _write(path, out):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
