"""Pose-graph optimisation on the GPU (mr_slam_amd/posegraph.py): three robots of 2 000 poses each (1 m steps, 2 cm / 3 mrad odometry noise)
with 64 and with 256 loop factors (2 cm / 5 mrad), the time of whole blocking `optimize` calls (wall clock; stage 1 is computed again in
every call) and of the stages between HIP events (the library's development timing switch), for a sweep of segment lengths.  Prints ONE JSON
line and, with --out, writes it to a file.  Run on its own.

Both baselines are measured in the same run, never taken from the new code:
  (a) the NumPy / scipy restatement (tests/golden/posegraph_restate.py, sparse LU per iteration) with the same stop rule;
  (b) the restatement with 200 unconditional iterations, which is what the reference's loop does (evaluation_utils.cpp:321).
gtsam itself is not in the reference tree and cannot be timed here.  Every scene also checks the result against (a).

The `robust` legs (--method, --noise, --kernel) run the same scenes with and without 10 % gross outliers among the loops
(5 m / 0.5 rad) through the chosen optimiser, noise and loop kernel, at the default segment length.  Their baselines, again of the same run:
the plain `optimize()` on the same graph (time per Gauss-Newton iteration, and whether it converged) and the restatement
tests/golden/posegraph_robust_restate.py on one thread."""
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


def with_outliers(scene, fraction, seed=1):
    """the scene with `fraction` of its loops (never the ones that join the robots) right-multiplied by a pose of N(0, 0.5) rad, N(0, 5) m"""
    import posegraph_restate as R
    chain_lengths, odom, li, lj, lZ = scene
    rng = np.random.default_rng(seed)
    n = int(round(fraction * li.size))
    lZ = lZ.copy()
    for u in (rng.choice(np.arange(ROBOTS - 1, li.size), n, replace=False) if n else ()):
        P = np.eye(4)
        P[:3, :3] = R.exp_so3(rng.normal(0, 0.5, 3))
        P[:3, 3] = rng.normal(0, 5.0, 3)
        lZ[u] = lZ[u] @ P
    return chain_lengths, odom, li, lj, lZ


def robust_legs(a, scene, reps):
    """{outlier fraction: figures} for one scene"""
    import posegraph_robust_restate as RR
    from mr_slam_amd import posegraph
    kinds = {"none": RR.NONE, "huber": RR.HUBER, "cauchy": RR.CAUCHY, "geman_mcclure": RR.GEMAN_MCCLURE}
    out = {}
    for fraction in a.outliers:
        chain_lengths, odom, li, lj, lZ = s = with_outliers(scene, fraction)
        oC = np.tile(posegraph.REFERENCE_ODOMETRY_COVARIANCE, (odom.shape[0], 1, 1)) if a.noise == "reference" else None
        lC = np.tile(posegraph.REFERENCE_LOOP_COVARIANCE, (li.size, 1, 1)) if a.noise == "reference" else None

        def timed(g, call):
            call()                                               # warm: allocations
            wall, stages = [], []
            for _ in range(reps):
                g.set_prior(np.eye(4))                           # stage 1 runs again, as after a new closure
                t0 = time.perf_counter()
                r = call()
                wall.append((time.perf_counter() - t0) * 1e3)
                stages.append(g.stage_ms())
            return r, float(np.median(wall)), np.median(np.array(stages), axis=0)

        e = {"loops": int(li.size), "outliers": int(round(fraction * li.size)), "method": a.method, "noise": a.noise, "kernel": a.kernel, "kernel_k": a.kernel_k}
        plain = posegraph.PoseGraph(chain_lengths)
        plain.set_odometry(odom)
        plain.add_loops(li, lj, lZ)
        try:
            r, ms, st = timed(plain, plain.optimize)
            e["parent_optimize"] = {"wall_ms": ms, "iterations": r.iterations, "converged": r.converged, "ms_per_iteration": ms / r.iterations,
                                    "ms_per_iteration_without_stage1": (ms - float(st[0])) / r.iterations,
                                    "stages_ms": {k: float(v) for k, v in zip(STAGES, st)}}
        except Exception as err:                                 # a step that is not finite is a status, and a finding
            e["parent_optimize"] = {"error": str(err)}
        g = posegraph.PoseGraph(chain_lengths)
        g.set_odometry(odom)
        if oC is not None:
            g.set_odometry_noise(oC)
        g.add_loops(li, lj, lZ, lC)
        if a.kernel != "none":
            g.set_loop_kernel(a.kernel, a.kernel_k)
        if a.method == "lm":
            r, ms, st = timed(g, lambda: g.optimize(method="lm"))
            n, e["solves"], e["accepted"], e["lambda"] = r.solves, r.solves, r.accepted, r.lam
            e["cost_initial"], e["cost_final"] = r.cost_initial, r.cost_final
        else:
            r, ms, st = timed(g, g.optimize)
            n, e["solves"], e["accepted"] = r.iterations, r.iterations, r.iterations
            e["cost_initial"], e["cost_final"] = r.error_initial, r.error_final
        e.update({"wall_ms": ms, "converged": r.converged, "ms_per_solve": ms / n, "ms_per_solve_without_stage1": (ms - float(st[0])) / n,
                  "stages_ms": {k: float(v) for k, v in zip(STAGES, st)}, "separators": r.separators})
        if "error" not in e["parent_optimize"]:
            e["ms_per_solve_over_parent_ms_per_iteration"] = e["ms_per_solve_without_stage1"] / e["parent_optimize"]["ms_per_iteration_without_stage1"]
        w, _ = g.loop_state()
        e["loops_below_weight_0.1"] = int((w < 0.1).sum())
        if a.restatement:
            t0 = time.perf_counter()
            if a.method == "lm":
                want = RR.lm_optimize(*s, oC=oC, lC=None if lC is None else list(lC), kernel=kinds[a.kernel], k=a.kernel_k)
                e["restatement"] = {"solves": want.solves, "accepted": want.accepted, "converged": want.converged}
            else:
                want = RR.gn_optimize(*s, oC=oC, lC=None if lC is None else list(lC))
                e["restatement"] = {"solves": want.iterations, "accepted": want.iterations, "converged": want.converged}
            e["restatement"]["wall_ms"] = (time.perf_counter() - t0) * 1e3
            e["restatement"]["max_abs_T"] = float(np.abs(r.T - want.T).max())
        out["%g" % fraction] = e
        print("robust loops %d outliers %g: %.1f ms, %d solves (%d accepted), converged %s" % (li.size, fraction, ms, e["solves"], e["accepted"], r.converged),
              file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--method", choices=("gn", "lm"), help="adds the robust legs: the optimiser they run")
    ap.add_argument("--noise", choices=("none", "reference"), default="none", help="robust legs: the reference's loopNoise / odometryNoise on every factor")
    ap.add_argument("--kernel", choices=("none", "huber", "cauchy", "geman_mcclure"), default="none", help="robust legs: the kernel on the loops")
    ap.add_argument("--kernel-k", type=float, default=1.0)
    ap.add_argument("--outliers", type=float, nargs="*", default=[0.0, 0.1], help="robust legs: fractions of grossly wrong loops")
    ap.add_argument("--no-restatement", dest="restatement", action="store_false", help="robust legs: skip the one-thread restatement")
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
        if a.method:
            r["robust"] = robust_legs(a, scene, a.reps)
        out["scenes"][str(L)] = r
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
