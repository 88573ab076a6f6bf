#!/usr/bin/env python3
"""Measures the batched point-to-point ICP (row G9) on one GPU and, in the same run, two baselines that are not the code under test:
the NumPy restatement on one thread (tests/golden/icp_restate.py, one pair) and the same pairs through GicpBatch.align (what the library
offered before).  Protocols: `forced` runs exactly --iters iterations per pair with the stopping rules disabled (max correspondence
distance 5 m, the GICP leg's value); `natural` runs the Mapping node's settings (global_manager.cpp:890-906).  Per-stage times come from
HIP events around each stage launched alone (mrs_gicp_batch_icp_profile); k_icp_sums is compared with the 8 TB/s HBM peak at its
algorithmic 36 B per source point.

    python tools/bench_icp.py --out profiles/icp_bench.json            # 256 pairs x 120 k points
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

HBM_PEAK = 8.0e12       # bytes / s, MI355X
SUMS_BYTES = 36         # float4 source point + int correspondence + gathered float4 target point


def make_pairs(n_pairs, points, seed=2000):
    """pairs shaped like bench.py's GICP leg: two synthetic scans, random rotations up to 5 degrees and translations up to 1 m, 2 cm noise"""
    from scipy.spatial.transform import Rotation as Rot
    from mr_slam_amd import synth
    rng = np.random.default_rng(seed)
    base = [synth.lidar_scan(500 + s, points, metric=True) for s in range(2)]
    srcs, tgts = [], []
    for i in range(n_pairs):
        p = base[i % 2].astype(np.float64)
        axis = rng.normal(size=3); axis /= np.linalg.norm(axis)
        Rm = Rot.from_rotvec(np.deg2rad(rng.uniform(0, 5)) * axis).as_matrix()
        t = rng.normal(size=3); t *= rng.uniform(0, 1) / np.linalg.norm(t)
        srcs.append((p + rng.normal(0, 0.02, p.shape)).astype(np.float32))
        tgts.append((p @ Rm.T + t + rng.normal(0, 0.02, p.shape)).astype(np.float32))
    return srcs, tgts


def timed(fn, sync):
    sync()
    t0 = time.perf_counter()
    out = fn()
    sync()
    return out, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--points", type=int, default=120000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import icp_restate as R
    from mr_slam_amd import gicp
    assert torch.cuda.is_available(), "needs a GPU (there is no CPU fallback)"
    sync = lambda: torch.cuda.synchronize(a.device)     # noqa: E731
    srcs, tgts = make_pairs(a.pairs, a.points)
    n_src = sum(s.shape[0] for s in srcs)
    res = {"pairs": a.pairs, "points_per_cloud": a.points, "device": torch.cuda.get_device_name(a.device)}

    w = gicp.GicpBatch(1, a.device)            # load the code objects before anything is timed
    w.set_sources([srcs[0][:4000]]); w.set_targets([tgts[0][:4000]]); w.align(); w.align_icp(); del w

    b = gicp.GicpBatch(a.pairs, a.device)
    _, t_set = timed(lambda: (b.set_sources(srcs), b.set_targets(tgts)), sync)
    forced = dict(force_iterations=a.iters, max_correspondence_distance=5.0)
    runs = []
    for _ in range(a.reps):
        (T, conv, its, state), t = timed(lambda: b.align_icp(**forced), sync)
        runs.append(t)
    assert (its == a.iters).all()
    t = float(np.median(runs))
    res["forced"] = {"iterations_per_pair": a.iters, "seconds": runs, "ms_per_iteration_whole_batch": 1e3 * t / a.iters,
                     "pair_iterations_per_s": a.pairs * a.iters / t, "nn_passes": b.nn_passes, "searched_fraction": b.searched_fraction}
    natural = dict(R.MAPPING_890)
    runs = []
    for _ in range(a.reps):
        (Tn, conv, its, state), t = timed(lambda: b.align_icp(**natural), sync)
        runs.append(t)
    t = float(np.median(runs))
    res["natural"] = {"settings": natural, "seconds": runs, "pairs_per_s": a.pairs / t, "iterations_mean": float(its.mean()),
                      "iterations_max": int(its.max()), "converged": int(conv.sum()),
                      "states": {R.STATES[s]: int((state == s).sum()) for s in np.unique(state)}}
    ms, cnt = b.icp_profile(np.stack([np.eye(4)] * a.pairs), reps=a.reps, max_correspondence_distance=5.0)
    sums_bps = SUMS_BYTES * n_src / (ms["icp_sums"] * 1e-3)
    res["stages_ms_per_iteration"] = dict(ms, **cnt, note="each stage launched alone between HIP events at the identity poses; the search is a "
                                          "full pass over every source point, later passes of an alignment certify most neighbours instead")
    res["icp_sums"] = {"bytes_per_point": SUMS_BYTES, "bytes_per_s": sums_bps, "share_of_8TBps": sums_bps / HBM_PEAK}
    res["set_clouds_s"] = t_set

    # baseline 1: the same pairs through GICP (k = 15, 5 m, forced iterations: bench.py's protocol); the first call computes the covariances
    g = gicp.GicpBatch(a.pairs, a.device)
    g.set_params(k_correspondences=15, max_correspondence_distance=5.0, force_iterations=a.iters)
    g.set_sources(srcs); g.set_targets(tgts)
    _, t_cold = timed(lambda: g.align(), sync)
    warm = [timed(lambda: g.align(), sync)[1] for _ in range(a.reps)]
    tw = float(np.median(warm))
    res["baseline_gicp_batch_align"] = {"first_call_with_covariances_s": t_cold, "warm_seconds": warm, "pair_iterations_per_s_warm": a.pairs * a.iters / tw,
                                        "pair_iterations_per_s_first_call": a.pairs * a.iters / t_cold}
    res["forced"]["speedup_over_gicp_first_call"] = t_cold / float(np.median(res["forced"]["seconds"]))
    res["forced"]["speedup_over_gicp_warm"] = tw / float(np.median(res["forced"]["seconds"]))
    del g, b

    # baseline 2: the restatement, one pair, one thread (kd-tree queries and NumPy sums)
    t0 = time.perf_counter()
    r = R.icp(srcs[0], tgts[0], **forced)
    t_cpu = time.perf_counter() - t0
    res["baseline_numpy_restatement_one_thread"] = {"pairs": 1, "seconds": t_cpu, "pair_iterations_per_s": a.iters / t_cpu,
                                                    "includes": "kd-tree build"}
    res["forced"]["speedup_over_numpy_one_thread"] = res["forced"]["pair_iterations_per_s"] / (a.iters / t_cpu)
    dt = np.linalg.norm(T[0, :3, 3] - r["T"][:3, 3])
    res["forced"]["pair0_translation_difference_to_restatement_m"] = float(dt)
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(line)


if __name__ == "__main__":
    main()
