"""Pose-graph optimisation on the GPU (mr_slam_amd/posegraph.py): three robots of 2 000 poses each (1 m steps, 2 cm / 3 mrad odometry noise)
with 64 and with 256 loop factors (2 cm / 5 mrad), the time of whole blocking `optimize` calls (wall clock; stage 1 is computed again in
every call) and of the stages between HIP events (the library's development timing switch), for a sweep of segment lengths.  Prints ONE JSON
line and, with --out, writes it to a file.  Run on its own.

Both baselines are measured in the same run, never taken from the new code:
  (a) the NumPy / scipy restatement (tests/golden/posegraph_restate.py, sparse LU per iteration) with the same stop rule;
  (b) the restatement with 200 unconditional iterations, which is what the reference's loop does (evaluation_utils.cpp:321).
gtsam itself is not in the reference tree and cannot be timed here.  Every scene also checks the result against (a)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

ROBOTS, POSES = 3, 2000
LOOPS = (64, 256)
SEGMENT_LENGTHS = (16, 32, 64, 128, 256, 0)
STAGES = ("stage1", "linearize", "segment_walks", "assemble", "dense_solve", "retract")


def make_scene(n_loops, seed=0):
    """(chain_lengths, odom, li, lj, lZ): the trajectories of tests/posegraph_cases.py at the workload's size; the first loops join the robots,
    the others join random poses of any two (or one) of them"""
    import posegraph_restate as R
    rng = np.random.default_rng(seed)

    def pose(rv, t):
        T = np.eye(4)
        T[:3, :3] = R.exp_so3(np.asarray(rv, np.float64))
        T[:3, 3] = t
        return T

    def inv(T):
        Ti = np.eye(4)
        Ti[:3, :3] = T[:3, :3].T
        Ti[:3, 3] = -T[:3, :3].T @ T[:3, 3]
        return Ti

    chains = []
    for _ in range(ROBOTS):
        X = np.empty((POSES, 4, 4))
        X[0] = pose([0, 0, rng.uniform(-np.pi, np.pi)], np.append(rng.uniform(-20, 20, 2), rng.uniform(-1, 1)))
        for k in range(1, POSES):
            X[k] = X[k - 1] @ pose([rng.normal(0, 0.01), rng.normal(0, 0.01), rng.normal(0.05, 0.1)], [1.0 + rng.uniform(-0.05, 0.05), 0.0, 0.0])
        chains.append(X)
    truth = np.concatenate(chains)
    odom = np.array([inv(X[k]) @ X[k + 1] @ pose(rng.normal(0, 0.003, 3), rng.normal(0, 0.02, 3)) for X in chains for k in range(POSES - 1)])
    li = rng.integers(0, ROBOTS * POSES, n_loops)
    lj = rng.integers(0, ROBOTS * POSES, n_loops)
    li[:ROBOTS - 1] = rng.integers(0, POSES, ROBOTS - 1)
    lj[:ROBOTS - 1] = POSES * np.arange(1, ROBOTS) + rng.integers(0, POSES, ROBOTS - 1)
    lj = np.where(li == lj, (lj + 1) % (ROBOTS * POSES), lj)
    lZ = np.array([inv(truth[i]) @ truth[j] @ pose(rng.normal(0, 0.005, 3), rng.normal(0, 0.02, 3)) for i, j in zip(li, lj)])
    return (POSES,) * ROBOTS, odom, li.astype(np.int32), lj.astype(np.int32), lZ


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loops", type=int, nargs="*", default=list(LOOPS))
    ap.add_argument("--segment-lengths", type=int, nargs="*", default=list(SEGMENT_LENGTHS))
    ap.add_argument("--reference-iterations", type=int, default=200, help="iterations of baseline (b); 0 skips it")
    a = ap.parse_args()
    os.environ["MRS_DEV"] = "1"
    os.environ["MRS_PGO_TIMING"] = "1"
    import torch
    import posegraph_restate as R
    assert torch.cuda.is_available(), "needs a GPU (there is no CPU fallback)"
    from mr_slam_amd import posegraph
    out = {"metric": "posegraph", "robots": ROBOTS, "poses_per_robot": POSES, "eps": posegraph.DEFAULT_EPS,
           "default_segment_length": posegraph.DEFAULT_SEGMENT_LENGTH, "runs": "one run; medians of %d repetitions" % a.reps,
           "gtsam": "not in the reference tree: not timed", "scenes": {}}
    for L in a.loops:
        scene = make_scene(L)
        chain_lengths, odom, li, lj, lZ = scene
        r = {"loops": L, "segment_lengths": {}}
        t0 = time.perf_counter()
        want = R.optimize(*scene)
        r["baseline_restatement_same_stop_rule_ms"] = (time.perf_counter() - t0) * 1e3
        r["baseline_restatement_iterations"] = want.iterations
        r["restatement_last_deltas"] = want.deltas[-3:]
        if a.reference_iterations:
            t0 = time.perf_counter()
            ref = R.optimize(*scene, eps=0.0, max_iterations=a.reference_iterations)
            r["baseline_restatement_%d_iterations_ms" % a.reference_iterations] = (time.perf_counter() - t0) * 1e3
            r["restatement_%d_vs_stop_rule_max_abs" % a.reference_iterations] = float(np.abs(ref.T - want.T).max())
        g = posegraph.PoseGraph(chain_lengths)
        g.set_odometry(odom)
        g.add_loops(li, lj, lZ)
        for sl in a.segment_lengths:
            g.set_segment_length(sl)
            got = g.optimize()                                    # warm: allocations
            wall, stages = [], []
            for _ in range(a.reps):
                g.set_prior(np.eye(4))                            # marks the graph changed: stage 1 runs again, as after a new closure
                t0 = time.perf_counter()
                got = g.optimize()
                wall.append((time.perf_counter() - t0) * 1e3)
                stages.append(g.stage_ms())
            med = np.median(np.array(stages), axis=0)
            e = {"optimize_wall_ms": float(np.median(wall)), "iterations": got.iterations, "converged": got.converged,
                 "separators": got.separators, "stages_ms": {k: float(v) for k, v in zip(STAGES, med)},
                 "max_abs_vs_restatement_R": float(np.abs(got.T[:, :3, :3] - want.T[:, :3, :3]).max()),
                 "max_abs_vs_restatement_t": float(np.abs(got.T[:, :3, 3] - want.T[:, :3, 3]).max())}
            if got.iterations == want.iterations:
                assert max(e["max_abs_vs_restatement_R"], e["max_abs_vs_restatement_t"]) < 1e-8, e
            r["segment_lengths"][str(sl)] = e
            print("loops %d segment length %d: %.1f ms, %d separators" % (L, sl, e["optimize_wall_ms"], got.separators), file=sys.stderr, flush=True)
        # exactly 200 iterations at the default segment length, the reference's count
        g.set_segment_length(posegraph.DEFAULT_SEGMENT_LENGTH)
        g.set_prior(np.eye(4))
        t0 = time.perf_counter()
        fixed = g.optimize(eps=0.0, max_iterations=200)
        r["optimize_200_iterations_wall_ms"] = (time.perf_counter() - t0) * 1e3
        r["optimize_200_vs_stop_rule_max_abs"] = float(np.abs(fixed.T - want.T).max())
        r["error_initial"], r["error_final"] = got.error_initial, got.error_final
        out["scenes"][str(L)] = r
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
