"""M2DP on the GPU: descriptor throughput for a batch of 64 scans x 120 000 points (mrs_m2dp_batch, device events around a synchronised
window) and database query latency.  Prints ONE JSON line and, with --out, writes it to a file.  Run on its own (a fresh process).

  --ref-json FILE   merge a CPU figure measured elsewhere (the reference's own M2DP.py on one thread, see --time-reference) into the output
  --time-reference  no GPU: time the reference's Python (needs the reference tree and sklearn) on one scan of 120 000 points, one CPU
                    thread, and print that JSON

Kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of this script (profiles/m2dp_kernel_stats.md): tracing slows
the host, so the end-to-end figures here are taken with the profiler off.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCANS, POINTS, DISTINCT = 64, 120_000, 8
PAIRS_PER_SCAN = POINTS * 64               # (point, plane) pairs = LDS atomics of the signature kernel


def time_reference():
    os.environ["OMP_NUM_THREADS"] = os.environ["OPENBLAS_NUM_THREADS"] = os.environ["MKL_NUM_THREADS"] = "1"
    import importlib.util
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import ref_import
    from mr_slam_amd import synth
    spec = importlib.util.spec_from_file_location("ref_M2DP", os.path.join(ref_import.RING_ROS, "pr_methods", "M2DP.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    cloud = synth.lidar_scan(0, POINTS).astype(np.float64)
    ref.M2DP(cloud)
    ts = []
    for _ in range(5):
        t0 = time.perf_counter()
        ref.M2DP(cloud)
        ts.append(time.perf_counter() - t0)
    return {"reference_cpu_1thread_s_per_scan": float(np.median(ts)), "reference_points": POINTS,
            "reference_what": "RING_ros/pr_methods/M2DP.py on one CPU thread of the build container, median of 5"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--ref-json")
    ap.add_argument("--time-reference", action="store_true")
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    if a.time_reference:
        out = time_reference()
    else:
        import torch
        from mr_slam_amd import m2dp as M, synth
        assert torch.cuda.is_available(), "needs a GPU (there is no CPU fallback)"
        dev = "cuda:0"
        base = [synth.lidar_scan(s, POINTS) for s in range(DISTINCT)]
        pts = torch.from_numpy(np.concatenate(base * (SCANS // DISTINCT))).to(dev)          # float32 [64 x 120 000, 3]
        offs = torch.arange(SCANS + 1, dtype=torch.int64) * POINTS

        def run():
            return M.m2dp_batch(pts, offs)

        for _ in range(3):
            desc, _A = run()
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(a.reps):
            run()
        e.record()
        torch.cuda.synchronize()
        ms = s.elapsed_time(e) / a.reps
        out = {"metric": "m2dp", "scans": SCANS, "points_per_scan": POINTS, "input": "float32 [n, 3] resident in HBM",
               "batch_ms": ms, "scans_per_s": SCANS / (ms * 1e-3), "window_s": ms * a.reps * 1e-3,
               "lds_atomics_per_point": 64, "pairs_per_s": SCANS * PAIRS_PER_SCAN / (ms * 1e-3),
               "input_bytes_per_s": 4 * pts.numel() * pts.element_size() / (ms * 1e-3),       # three moment passes over the points + the histogram pass
               "note": "whole call: 3 moment passes, PCA, signature matrix, SVD; kernel times: profiles/m2dp_kernel_stats.md"}
        db = M.M2DPDatabase(0, capacity=16384)
        d = desc.cpu().numpy()
        rng = np.random.default_rng(0)
        for i in range(10000):
            db.append(np.abs(d[i % SCANS] + rng.normal(0, 1e-2, 192)))
        q = d[5].copy()
        for k in (1, 10):
            db.query(q, k)
            ts = []
            for _ in range(50):
                t0 = time.perf_counter()
                db.query(q, k)
                ts.append((time.perf_counter() - t0) * 1e3)
            out["query_k%d_n10000_ms" % k] = float(np.median(ts))
    if a.ref_json and os.path.exists(a.ref_json):
        out.update(json.load(open(a.ref_json)))
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
