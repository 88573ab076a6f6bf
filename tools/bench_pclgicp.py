#!/usr/bin/env python3
"""Measures the batched PCL-style GICP (row G11) on one GPU and, in the same run, two baselines that are not the code under test: the NumPy
restatement on one thread (tests/golden/pclgicp_restate.py, one pair) and the same pairs through GicpBatch.align with the same distance and
epsilons (what the library offered before).  Protocols: `forced` runs exactly --iters outer iterations per pair with the stopping rule
disabled (5 m threshold); `natural` runs the Mapping node's settings (global_manager.cpp:2422-2425).  Per-stage times come from HIP events
around each stage launched alone (mrs_gicp_batch_pcl_profile); k_pclgicp_sums is compared with the 8 TB/s HBM peak at its algorithmic 84 B
per correspondence.

    python tools/bench_pclgicp.py --out profiles/pclgicp_bench.json            # 256 pairs x 120 k points
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

HBM_PEAK = 8.0e12       # bytes / s, MI355X
SUMS_BYTES = 84         # float4 source point + int correspondence + gathered float4 target point + two normals of 3 doubles


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
    import pclgicp_restate as G
    from bench_icp import make_pairs, timed
    from mr_slam_amd import gicp
    assert torch.cuda.is_available(), "needs a GPU (there is no CPU fallback)"
    sync = lambda: torch.cuda.synchronize(a.device)     # noqa: E731
    srcs, tgts = make_pairs(a.pairs, a.points)
    res = {"pairs": a.pairs, "points_per_cloud": a.points, "device": torch.cuda.get_device_name(a.device)}

    w = gicp.GicpBatch(1, a.device)            # load the code objects before anything is timed
    w.set_sources([srcs[0][:4000]]); w.set_targets([tgts[0][:4000]]); w.align(); w.align_pcl(); del w

    forced = dict(force_iterations=a.iters, max_correspondence_distance=5.0)
    natural = dict(G.MAPPING_2422)
    b = gicp.GicpBatch(a.pairs, a.device)
    _, t_set = timed(lambda: (b.set_sources(srcs), b.set_targets(tgts)), sync)
    (Tn, conv, its, state), t_cold = timed(lambda: b.align_pcl(**natural), sync)      # the first call computes both clouds' covariances
    runs = []
    for _ in range(a.reps):
        (Tn, conv, its, state), t = timed(lambda: b.align_pcl(**natural), sync)
        runs.append(t)
    t = float(np.median(runs))
    res["natural"] = {"settings": natural, "first_call_with_covariances_s": t_cold, "warm_seconds": runs, "pairs_per_s_warm": a.pairs / t,
                      "pairs_per_s_first_call": a.pairs / t_cold, "iterations_mean": float(its.mean()), "iterations_max": int(its.max()),
                      "converged": int(conv.sum()), "states": {G.STATES[s]: int((state == s).sum()) for s in np.unique(state)},
                      "nn_passes": b.nn_passes, "searched_fraction": b.searched_fraction}
    runs = []
    for _ in range(a.reps):
        (T, fconv, fits, fstate), t = timed(lambda: b.align_pcl(**forced), sync)
        runs.append(t)
    assert (fits == a.iters).all()
    t = float(np.median(runs))
    res["forced"] = {"iterations_per_pair": a.iters, "warm_seconds": runs, "ms_per_iteration_whole_batch": 1e3 * t / a.iters,
                     "pair_iterations_per_s": a.pairs * a.iters / t, "nn_passes": b.nn_passes, "searched_fraction": b.searched_fraction}
    ms, cnt = b.pcl_profile(np.stack([np.eye(4)] * a.pairs), reps=a.reps, max_correspondence_distance=5.0)
    sums_bps = SUMS_BYTES * cnt["correspondences"] / (ms["pclgicp_sums"] * 1e-3)
    res["stages_ms_per_iteration"] = dict(ms, **cnt, note="each stage launched alone between HIP events at the identity poses; the search is a "
                                          "full pass over every source point, later passes of an alignment certify most neighbours instead")
    res["pclgicp_sums"] = {"bytes_per_correspondence": SUMS_BYTES, "bytes_per_s": sums_bps, "share_of_8TBps": sums_bps / HBM_PEAK}
    res["set_clouds_s"] = t_set
    del b

    # baseline (b): the same pairs through GicpBatch.align (fast_gicp's Gauss-Newton / LM) with the same k, distance and epsilons
    g = gicp.GicpBatch(a.pairs, a.device)
    g.set_params(k_correspondences=20, max_correspondence_distance=natural["max_correspondence_distance"], max_iterations=natural["max_iterations"],
                 rotation_epsilon=G.DEFAULTS["rotation_epsilon"], transformation_epsilon=natural["transformation_epsilon"])
    g.set_sources(srcs); g.set_targets(tgts)
    (Tg, gconv, gits), tg_cold = timed(lambda: g.align(), sync)
    warm = [timed(lambda: g.align(), sync)[1] for _ in range(a.reps)]
    tw = float(np.median(warm))
    res["baseline_gicp_batch_align"] = {"first_call_with_covariances_s": tg_cold, "warm_seconds": warm, "pairs_per_s_warm": a.pairs / tw,
                                        "pairs_per_s_first_call": a.pairs / tg_cold, "iterations_mean": float(gits.mean()),
                                        "converged": int(gconv.sum()),
                                        "largest_translation_difference_to_align_pcl_m": float(np.abs(Tg[:, :3, 3] - Tn[:, :3, 3]).max())}
    res["natural"]["time_relative_to_gicp_batch_align_warm"] = float(np.median(res["natural"]["warm_seconds"])) / tw
    res["natural"]["time_relative_to_gicp_batch_align_first_call"] = t_cold / tg_cold
    del g

    # baseline (a): the restatement, one pair, one thread (kd-tree queries, NumPy covariances and sums)
    t0 = time.perf_counter()
    cv = (G.covariances(srcs[0]), G.covariances(tgts[0]))
    t_cov = time.perf_counter() - t0
    t0 = time.perf_counter()
    r = G.gicp(srcs[0], tgts[0], covs=cv, **natural)
    t_cpu = time.perf_counter() - t0
    res["baseline_numpy_restatement_one_thread"] = {"pairs": 1, "covariances_s": t_cov, "align_s": t_cpu, "iterations": r["iterations"],
                                                    "pairs_per_s": 1.0 / (t_cov + t_cpu), "includes": "kd-tree builds"}
    res["natural"]["speedup_over_numpy_one_thread_first_call"] = res["natural"]["pairs_per_s_first_call"] * (t_cov + t_cpu)
    res["natural"]["pair0_translation_difference_to_restatement_m"] = float(np.linalg.norm(Tn[0, :3, 3] - r["T"][:3, 3]))
    res["natural"]["pair0_iterations"] = [int(its[0]), int(r["iterations"])]
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(line)


if __name__ == "__main__":
    main()
