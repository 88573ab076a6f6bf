"""Pairwise consistency on the GPU (mr_slam_amd/pcm.py): for L = 256, 1024 and 4096 loops between two 2 000-pose trajectories (70 % inliers
with 2 cm / 0.3 degree noise, the rest random poses) the time of add_loops in one call, of add_loops in 64 appends of L / 64, and of solve,
each as wall-clock around the blocking call and as device time between two events on the stream the handle works on (upload, kernels and
read-backs of the call), plus the rounds solve took.  Prints ONE JSON line and, with --out, writes it to a file.  Run on its own.

Both baselines are measured in the same run, never taken from the new code:
  (a) the NumPy restatement (tests/golden/pcm_restate.py) on one CPU thread: the distances of all pairs (in blocks of pairs, so that
      L = 4096 fits in memory) and max_clique_heu on the resulting matrix;
  (b) the reference's own clique finder on the same graph, through the Matrix-Market file the reference writes, when
      `tools/make_pcm_golden.py --keep-binary` has built it on this machine (read-graph and clique times as the binary reports them);
      "not available" otherwise.
Every L also checks the results: the matrix against (a) outside a 1e-9 band around the threshold, the member list against (a) and (b).
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

SIZES = (256, 1024, 4096)
POSES, INLIERS, APPENDS = 2000, 0.7, 64
FMC_BINARY = os.path.join(ROOT, "build", "pcm_fmc_ref")


def _pose(rng, angle_sigma, t):
    w = rng.normal(0, angle_sigma, 3)
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + (np.sin(th) / th) * K + ((1 - np.cos(th)) / (th * th)) * (K @ K) if th > 0 else np.eye(3)
    T[:3, 3] = t
    return T


def make_scene(L, seed=0):
    """two trajectories chained from 1 m odometry steps with small turns, and L loops in the reference's order"""
    import pcm_restate as R
    from mr_slam_amd import pcm
    rng = np.random.default_rng(seed)
    XA, XB = (pcm.chain_odometry(np.stack([_pose(rng, 0.05, [1.0, 0.0, 0.0]) for _ in range(POSES - 1)])) for _ in range(2))
    G = _pose(rng, 0.5, rng.uniform(-20, 20, 3))
    keys = np.sort(rng.choice(POSES * POSES, L, replace=False))
    ia, kb = (keys // POSES).astype(np.int32), (keys % POSES).astype(np.int32)
    Z = np.empty((L, 4, 4))
    inlier = rng.random(L) < INLIERS
    for u in range(L):
        if inlier[u]:
            Z[u] = R.inverse(XA[ia[u]]) @ G @ XB[kb[u]] @ _pose(rng, np.deg2rad(0.3), rng.normal(0, 0.02, 3))
        else:
            Z[u] = _pose(rng, 1.5, rng.uniform(-30, 30, 3))
    return XA, XB, ia, kb, Z, int(inlier.sum())


def numpy_distances(XA, XB, ia, kb, Z, block=1 << 18):
    """pcm_restate's distance of every pair u < v, evaluated in blocks of pairs; mirrored, zero diagonal"""
    import pcm_restate as R
    L = ia.size
    D = np.zeros((L, L))
    u, v = np.triu_indices(L, 1)
    for lo in range(0, u.size, block):
        a, b = u[lo:lo + block], v[lo:lo + block]
        E = R.inverse(Z[a]) @ (((R.inverse(XA[ia[a]]) @ XA[ia[b]]) @ Z[b]) @ (R.inverse(XB[kb[b]]) @ XB[kb[a]]))
        xi = R.logmap(E)
        D[a, b] = np.sqrt(np.sum(xi * xi, 1))
    return D + D.T


def _timed(fn, reps, events):
    """(median wall ms, median ms between events) of a blocking call"""
    wall, dev = [], []
    for _ in range(reps):
        s, e = events()
        s.record()
        t0 = time.perf_counter()
        fn()
        wall.append((time.perf_counter() - t0) * 1e3)
        e.record()
        e.synchronize()
        dev.append(s.elapsed_time(e))
    return float(np.median(wall)), float(np.median(dev))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", type=int, nargs="*", default=list(SIZES))
    ap.add_argument("--fmc-max-loops", type=int, default=4096, help="skip the reference binary above this many loops")
    a = ap.parse_args()
    os.environ.setdefault("OMP_NUM_THREADS", "1")
    import torch
    import pcm_restate as R
    from mr_slam_amd import pcm
    assert torch.cuda.is_available(), "needs a GPU (there is no CPU fallback)"
    torch.set_num_threads(1)

    def events():
        return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    have_fmc = os.path.exists(FMC_BINARY)
    out = {"metric": "pcm", "poses_per_trajectory": POSES, "inlier_share": INLIERS, "p": 0.01, "threshold": pcm.chi2_threshold(0.01),
           "runs": "one run; medians of %d repetitions" % a.reps, "sizes": {}}
    for L in a.sizes:
        XA, XB, ia, kb, Z, n_in = make_scene(L)
        g = pcm.PcmGraph(capacity=L, p=0.01)
        g.set_trajectories(XA, XB)

        def once():
            g.clear()
            g.add_loops(ia, kb, Z)

        def appended():
            g.clear()
            step = L // APPENDS
            for lo in range(0, L, step):
                g.add_loops(ia[lo:lo + step], kb[lo:lo + step], Z[lo:lo + step])

        once()
        A_once = g.matrix()
        appended()
        assert np.array_equal(g.matrix(), A_once), "appending changed the matrix"
        r = {"loops": L, "inliers": n_in, "edges": int(A_once.sum() // 2)}
        r["add_loops_once_wall_ms"], r["add_loops_once_events_ms"] = _timed(once, a.reps, events)
        r["add_loops_%d_appends_wall_ms" % APPENDS], r["add_loops_%d_appends_events_ms" % APPENDS] = _timed(appended, max(3, a.reps // 4), events)
        once()
        clique, rejected = g.solve()
        r["solve_wall_ms"], r["solve_events_ms"] = _timed(g.solve, a.reps, events)
        r.update({"rounds": g.rounds, "clique": int(clique.size), "rejected": int(rejected)})

        # (a) the NumPy restatement, one thread
        t0 = time.perf_counter()
        D = numpy_distances(XA, XB, ia, kb, Z)
        A_np = R.consistency_matrix(D, g.threshold)
        r["baseline_numpy_matrix_ms"] = (time.perf_counter() - t0) * 1e3
        near = np.abs(D - g.threshold) <= 1e-9
        r["pairs_within_1e-9_of_threshold"] = int(near.sum() // 2)
        assert np.array_equal(A_once | near, A_np | near), "matrix mismatch"
        t0 = time.perf_counter()
        size, members = R.max_clique_heu(A_once)
        r["baseline_numpy_clique_ms"] = (time.perf_counter() - t0) * 1e3
        assert clique.tolist() == members, "clique mismatch"

        # (b) the reference's own clique finder on the same graph
        if have_fmc and L <= a.fmc_max_loops:
            import make_pcm_golden as M
            with tempfile.TemporaryDirectory() as d:
                fsize, fmembers, read_ms, clique_ms = M.run_fmc(FMC_BINARY, L, M.edges_of(A_once), d)
            assert fmembers.tolist() == clique.tolist() and fsize == clique.size, "the reference's clique finder disagrees"
            r["baseline_reference_fmc_read_graph_ms"], r["baseline_reference_fmc_clique_ms"] = read_ms, clique_ms
        else:
            r["baseline_reference_fmc_clique_ms"] = "not available"
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
