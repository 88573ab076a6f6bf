"""Scan Context on the GPU: query latency of the loop database (k = 1, 10 at 10 000 and 50 000 entries), the exhaustive alignment sweep
(query_all) and descriptor + key throughput for batches of 1024 scans.  Prints ONE JSON line.  Run on its own (a fresh process)."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mr_slam_amd import bev, synth, scancontext as SC  # noqa: E402

PEAK, COPY = 8.0e12, 6.3e12          # HBM peak, measured copy rate (bytes / s)
ENTRY_BYTES = (256 + 120 * 120) * 4  # packed entry: header + descriptor


def median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def event_ms(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def main():
    dev = "cuda:0"
    scans = [synth.lidar_scan(s, 20000) for s in range(64)]
    xyz, offs = bev.pack_scans(scans, dev)
    base = SC.sc_descriptors(xyz, offs)                                  # [64, 120, 120]
    out = {"metric": "scancontext", "entry_bytes": ENTRY_BYTES}
    db = SC.ScanContextDatabase(0, capacity=50000)
    q = torch.roll(base[5], 17, dims=-1).contiguous()
    qh = q.cpu().numpy()
    for n in (10000, 50000):
        while len(db) < n:
            i = len(db)
            db.append(base[i % 64] * (1.0 + (i // 64) * 1e-4))
        torch.cuda.synchronize()
        print("entries", n, file=sys.stderr, flush=True)
        for k in (1, 10):
            db.query(qh, k)
            out[f"query_k{k}_n{n}_ms"] = median_ms(lambda: db.query(qh, k), 50)
        db.query_all(qh)
        t = median_ms(lambda: db.query_all(qh), 20)
        out[f"query_all_n{n}_ms"] = t
        out[f"query_all_n{n}_hbm_frac_peak"] = n * ENTRY_BYTES / (t * 1e-3) / PEAK
        out[f"query_all_n{n}_hbm_frac_copy"] = n * ENTRY_BYTES / (t * 1e-3) / COPY
    big = scans * 16                                                      # 1024 scans of 20 000 points
    xb, ob = bev.pack_scans(big, dev)
    t = event_ms(lambda: SC.keys(SC.sc_descriptors(xb, ob)), 10)
    out["desc_keys_batch1024_ms"] = t
    out["desc_keys_scans_per_s"] = 1024 / (t * 1e-3)
    # pairwise entry points: both sides packed per call, one Q per pair
    a = base.repeat(16, 1, 1)
    b = torch.roll(a, 9, dims=-1).contiguous()
    out["dist_align_pairs1024_ms"] = event_ms(lambda: SC.dist_align_sc(a, b, 0.1), 10)
    out["distance_sc_pairs1024_ms"] = event_ms(lambda: SC.distance_sc(a, b), 5)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
