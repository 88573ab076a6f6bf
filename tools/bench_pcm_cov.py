"""Pairwise consistency with covariances on the GPU (mr_slam_amd/pcm.py): for L = 256, 1024 and 4096 loops on the scenes of
tools/bench_pcm.py (two 2 000-pose trajectories) the time of add_loops in one call, of add_loops in 64 appends of L / 64, and of solve, in
mode NONE and in mode SPAN on the same scene and in the same run, each as wall-clock around the blocking call and as device time between
two events.  Every odometry step and every loop carries a random positive definite covariance around FIXED_COVARIANCE.  Prints ONE JSON
line and, with --out, writes it to a file.  Run on its own.

The NONE figures of this run are the baseline of the SPAN figures of this run; the ratio is reported as measured.  The second baseline is the
NumPy restatement (tests/golden/pcm_cov_restate.py, the direct covariance chain) on one CPU thread, timed on a sample of pairs (sweeps
included) and reported per pair, with the product for all L (L - 1) / 2 pairs marked as extrapolated.  The sample also checks the
distances of the kernels against the restatement.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

APPENDS = 64


def random_covariances(rng, n, lo, hi):
    """[n, 6, 6] positive definite, shaped like FIXED_COVARIANCE and scaled log-uniformly in [lo, hi]"""
    d = np.sqrt(np.array([1e-4, 1e-4, 1e-4, 1e-2, 1e-2, 1e-2]))
    G = rng.normal(size=(n, 6, 8))
    s = np.exp(rng.uniform(np.log(lo), np.log(hi), n))
    C = s[:, None, None] * (d[:, None] * (0.5 * np.eye(6) + G @ np.swapaxes(G, 1, 2) / 16.0) * d[None, :])
    return 0.5 * (C + np.swapaxes(C, 1, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", type=int, nargs="*", default=[256, 1024, 4096])
    ap.add_argument("--numpy-pairs", type=int, default=300, help="pairs the NumPy restatement is timed on")
    a = ap.parse_args()
    os.environ.setdefault("OMP_NUM_THREADS", "1")
    import torch
    import bench_pcm as B
    import pcm_cov_restate as RC
    from mr_slam_amd import pcm
    assert torch.cuda.is_available(), "needs a GPU (there is no CPU fallback)"
    torch.set_num_threads(1)

    def events():
        return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    thresholds = {"none": pcm.chi2_threshold(0.01), "span": pcm.chi2_upper(0.99)}
    out = {"metric": "pcm_cov", "poses_per_trajectory": B.POSES, "inlier_share": B.INLIERS, "thresholds": thresholds,
           "runs": "one run; medians of %d repetitions" % a.reps, "sizes": {}}
    for L in a.sizes:
        XA, XB, ia, kb, Z, n_in = B.make_scene(L)
        rng = np.random.default_rng(L)
        QA, QB = random_covariances(rng, B.POSES - 1, 0.05, 1.0), random_covariances(rng, B.POSES - 1, 0.05, 1.0)
        Cv = random_covariances(rng, L, 0.25, 16.0)
        r = {"loops": L, "inliers": n_in}
        for mode in ("none", "span"):
            g = pcm.PcmGraph(capacity=L, threshold=thresholds[mode])
            g.set_trajectories(XA, XB)
            t0 = time.perf_counter()
            g.set_covariances(mode, QA, QB)
            r[mode + "_set_covariances_wall_ms"] = (time.perf_counter() - t0) * 1e3
            cov = Cv if mode == "span" else None

            def once():
                g.clear()
                g.add_loops(ia, kb, Z, cov)

            def appended():
                g.clear()
                step = L // APPENDS
                for lo in range(0, L, step):
                    g.add_loops(ia[lo:lo + step], kb[lo:lo + step], Z[lo:lo + step], None if cov is None else cov[lo:lo + step])

            once()
            A_once = g.matrix()
            appended()
            assert np.array_equal(g.matrix(), A_once), "appending changed the matrix"
            r[mode + "_edges"] = int(A_once.sum() // 2)
            r[mode + "_add_loops_once_wall_ms"], r[mode + "_add_loops_once_events_ms"] = B._timed(once, a.reps, events)
            r[mode + "_add_loops_%d_appends_wall_ms" % APPENDS], r[mode + "_add_loops_%d_appends_events_ms" % APPENDS] = \
                B._timed(appended, max(3, a.reps // 4), events)
            once()
            clique, rejected = g.solve()
            r[mode + "_solve_wall_ms"], r[mode + "_solve_events_ms"] = B._timed(g.solve, a.reps, events)
            r.update({mode + "_rounds": g.rounds, mode + "_clique": int(clique.size)})
            if mode == "span":
                D = g.distances()
        for what in ("add_loops_once", "add_loops_%d_appends" % APPENDS, "solve"):
            r["span_over_none_%s_events" % what] = r["span_%s_events_ms" % what] / r["none_%s_events_ms" % what]

        # the NumPy restatement on one thread, on a sample of pairs
        u, v = np.triu_indices(L, 1)
        pick = rng.choice(u.size, min(a.numpy_pairs, u.size), replace=False)
        pairs = list(zip(u[pick].tolist(), v[pick].tolist()))
        t0 = time.perf_counter()
        Dn, _, _ = RC.evaluate("span", XA, XB, ia, kb, Z, Cv, QA, QB, pairs=pairs)
        ms = (time.perf_counter() - t0) * 1e3
        r["baseline_numpy_sample_pairs"] = len(pairs)
        r["baseline_numpy_ms_per_pair"] = ms / len(pairs)
        r["baseline_numpy_all_pairs_ms_extrapolated"] = ms / len(pairs) * u.size
        want = np.array([Dn[p] for p in pairs])
        got = np.array([D[p] for p in pairs])
        with np.errstate(invalid="ignore"):
            rel = np.abs(got - want) / np.abs(want)
        r["sample_largest_relative_deviation_of_d2"] = float(np.nanmax(rel))
        assert np.array_equal(np.isnan(got), np.isnan(want)), "NaN pattern differs from the restatement"
        out["sizes"][str(L)] = r
        print("L = %d done" % L, file=sys.stderr, flush=True)
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
