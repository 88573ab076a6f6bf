#!/usr/bin/env python3
"""Measures the batched point-to-plane ICP (row G12) on one GPU and, in the same run, two baselines that are not the code under test:
point-to-point ICP (GicpBatch.align_icp, what the library offered before) on the same pairs, and the NumPy restatement on one thread
(tests/golden/icp_plane_restate.py, one pair).  Protocols as tools/bench_icp.py, whose pairs these are: `forced` runs exactly --iters
iterations per pair with the stopping rules disabled (max correspondence distance 5 m); `natural` runs the Mapping node's settings
(global_manager.cpp:890-906).  Per-stage times come from HIP events around each stage launched alone
(mrs_gicp_batch_icp_plane_profile); k_icp_plane_sums is compared with the 8 TB/s HBM peak at its algorithmic 52 B per source point.  The
normals of the targets (k = 15) are timed alone, and as the difference between the first alignment of a handle and a later one.

    python tools/bench_icp_plane.py --out profiles/icp_plane_bench.json            # 256 pairs x 120 k points
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
SUMS_BYTES = 52         # float4 source point + int correspondence + gathered float4 target point + gathered float4 normal


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
    import icp_plane_restate as PR
    import icp_restate as R
    from bench_icp import make_pairs, timed
    from mr_slam_amd import gicp
    assert torch.cuda.is_available(), "needs a GPU (there is no CPU fallback)"
    sync = lambda: torch.cuda.synchronize(a.device)     # noqa: E731
    srcs, tgts = make_pairs(a.pairs, a.points)
    n_src = sum(s.shape[0] for s in srcs)
    res = {"pairs": a.pairs, "points_per_cloud": a.points, "device": torch.cuda.get_device_name(a.device)}

    w = gicp.GicpBatch(1, a.device)            # load the code objects before anything is timed
    w.set_sources([srcs[0][:4000]]); w.set_targets([tgts[0][:4000]]); w.align_icp(); w.align_icp_plane(); del w

    b = gicp.GicpBatch(a.pairs, a.device)
    _, t_set = timed(lambda: (b.set_sources(srcs), b.set_targets(tgts)), sync)
    forced = dict(force_iterations=a.iters, max_correspondence_distance=5.0)
    (T, conv, its, state), t_first = timed(lambda: b.align_icp_plane(**forced), sync)      # computes the targets' normals
    runs = []
    for _ in range(a.reps):
        (T, conv, its, state), t = timed(lambda: b.align_icp_plane(**forced), sync)
        runs.append(t)
    assert (its == a.iters).all()
    t = float(np.median(runs))
    res["forced"] = {"iterations_per_pair": a.iters, "first_call_with_normals_s": t_first, "seconds": runs,
                     "ms_per_iteration_whole_batch": 1e3 * t / a.iters, "pair_iterations_per_s": a.pairs * a.iters / t,
                     "nn_passes": b.nn_passes, "searched_fraction": b.searched_fraction}
    natural = dict(R.MAPPING_890)
    runs = []
    for _ in range(a.reps):
        (Tn, conv, its, state), t = timed(lambda: b.align_icp_plane(**natural), sync)
        runs.append(t)
    t = float(np.median(runs))
    res["natural"] = {"settings": natural, "seconds": runs, "pairs_per_s": a.pairs / t, "iterations_mean": float(its.mean()),
                      "iterations_max": int(its.max()), "converged": int(conv.sum()), "searched_fraction": b.searched_fraction,
                      "states": {PR.STATES[s]: int((state == s).sum()) for s in np.unique(state)}}
    ms, cnt = b.icp_plane_profile(np.stack([np.eye(4)] * a.pairs), reps=a.reps, max_correspondence_distance=5.0)
    sums_bps = SUMS_BYTES * n_src / (ms["icp_plane_sums"] * 1e-3)
    res["stages_ms"] = dict(ms, **cnt, note="each stage launched alone between HIP events at the identity poses; the search is a full pass over "
                            "every source point, later passes of an alignment certify most neighbours instead; normals: selection + "
                            "k_normals_from_knn of all target clouds, k = 15, once per set of targets")
    res["icp_plane_sums"] = {"bytes_per_point": SUMS_BYTES, "bytes_per_s": sums_bps, "share_of_8TBps": sums_bps / HBM_PEAK}
    res["normals"] = {"k": 15, "clouds": a.pairs, "ms_alone": ms["normals"], "first_call_minus_later_call_s": t_first - float(np.median(res["forced"]["seconds"]))}
    res["set_clouds_s"] = t_set

    # baseline 1: the same pairs through point-to-point ICP on the same handle (no normals, 17 sums), same protocols
    runs = [timed(lambda: b.align_icp(**forced), sync)[1] for _ in range(a.reps)]
    tf = float(np.median(runs))
    nat = []
    for _ in range(a.reps):
        (Ti, ci, ii, si), t = timed(lambda: b.align_icp(**natural), sync)
        nat.append(t)
    tn = float(np.median(nat))
    res["baseline_align_icp"] = {"forced_seconds": runs, "forced_pair_iterations_per_s": a.pairs * a.iters / tf, "natural_seconds": nat,
                                 "natural_pairs_per_s": a.pairs / tn, "natural_iterations_mean": float(ii.mean()), "natural_converged": int(ci.sum()),
                                 "natural_states": {R.STATES[s]: int((si == s).sum()) for s in np.unique(si)}}
    res["forced"]["time_relative_to_align_icp"] = float(np.median(res["forced"]["seconds"])) / tf
    res["natural"]["speedup_over_align_icp"] = tn / float(np.median(res["natural"]["seconds"]))
    del b

    # baseline 2: the restatement, one pair, one thread (kd-tree queries, NumPy normals and sums)
    t0 = time.perf_counter()
    N = PR.normals(tgts[0], 15)["normals"]
    t_nrm = time.perf_counter() - t0
    t0 = time.perf_counter()
    r = PR.icp(srcs[0], tgts[0], N, **forced)
    t_cpu = time.perf_counter() - t0
    res["baseline_numpy_restatement_one_thread"] = {"pairs": 1, "normals_seconds": t_nrm, "seconds": t_cpu, "pair_iterations_per_s": a.iters / t_cpu,
                                                    "includes": "kd-tree build"}
    res["forced"]["speedup_over_numpy_one_thread"] = res["forced"]["pair_iterations_per_s"] / (a.iters / t_cpu)
    res["normals"]["speedup_over_numpy_one_thread"] = t_nrm * a.pairs / (ms["normals"] * 1e-3)
    res["forced"]["pair0_translation_difference_to_restatement_m"] = float(np.linalg.norm(T[0, :3, 3] - r["T"][:3, 3]))
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(line)


if __name__ == "__main__":
    main()
