"""Fast Histogram on the GPU: descriptor throughput for 1024 resident scans x 120 000 points (mrs_fh_batch, device events around a
synchronised window), the latency of one scan, and database query / distance latency at 10 000 entries.  Prints ONE JSON line and, with
--out, writes it to a file.  Run on its own (a fresh process).

Both baselines are measured in the same run, never taken from the new code:
  (a) the NumPy restatement (tests/golden/fasthist_restate.py) on one CPU thread, one scan of 120 000 points;
  (b) what a user of the library had on the device before: torch.linalg.norm + max + torch.bucketize + torch.bincount per scan (float64).

The share of the HBM peak counts 12 N bytes per scan ONCE: the bin pass reads the same points right after the range pass, and should find
them in L2 / MALL.  Kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of this script (profiles/fasthist_notes.md):
tracing slows the host, so the end-to-end figures here are taken with the profiler off.
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

SCANS, POINTS, DISTINCT, BINS, ENTRIES = 1024, 120_000, 8, 100, 10_000
HBM_PEAK = 8e12


def _median_ms(fn, reps, sync):
    fn()
    sync()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--scans", type=int, default=SCANS)
    a = ap.parse_args()
    os.environ.setdefault("OMP_NUM_THREADS", "1")
    import torch
    import fasthist_restate as R
    from mr_slam_amd import fasthist as F, synth
    from mr_slam_amd.compat import FastHistogram as D
    assert torch.cuda.is_available(), "needs a GPU (there is no CPU fallback)"
    dev = "cuda:0"
    sync = torch.cuda.synchronize
    scans = max(DISTINCT, a.scans // DISTINCT * DISTINCT)
    base = [synth.lidar_scan(s, POINTS) for s in range(DISTINCT)]
    pts = torch.from_numpy(np.concatenate(base)).to(dev).repeat(scans // DISTINCT, 1)       # float32 [scans x 120 000, 3]
    offs = torch.arange(scans + 1, dtype=torch.int64) * POINTS
    d_offs = offs.to(dev)
    out = {"metric": "fasthist", "scans": scans, "points_per_scan": POINTS, "bins": BINS, "input": "float32 [n, 3] resident in HBM"}

    # 1. the batch
    for _ in range(3):
        hist, counts, rng_, unb = F.range_histogram_batch(pts, (offs, d_offs), BINS)
    sync()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(5):
        F.range_histogram_batch(pts, (offs, d_offs), BINS)
    e.record()
    sync()
    reps = int(min(2000, max(a.reps, 1e3 / max(s.elapsed_time(e) / 5, 1e-3))))          # a timed window of about a second
    s.record()
    for _ in range(reps):
        F.range_histogram_batch(pts, (offs, d_offs), BINS)
    e.record()
    sync()
    ms = s.elapsed_time(e) / reps
    out.update({"batch_ms": ms, "ms_per_1024_scans": ms * 1024 / scans, "scans_per_s": scans / (ms * 1e-3), "window_s": ms * reps * 1e-3,
                "bytes_counted_per_scan": 12 * POINTS, "hbm_share_of_8TBps": 12.0 * POINTS * scans / (ms * 1e-3) / HBM_PEAK,
                "unbound_points": int(unb.sum())})
    want = R.range_histogram(base[3], BINS)
    assert np.array_equal(counts[3].cpu().numpy(), want.counts) and hist[3].cpu().numpy().tobytes() == want.hist.tobytes(), "result mismatch"

    # 2. one scan: resident cloud, whole call until the result is on the device; and the drop-in from a host array
    one, one_offs = pts[:POINTS], (offs[:2], d_offs[:2])
    out["one_scan_resident_ms"] = _median_ms(lambda: F.range_histogram_batch(one, one_offs, BINS), a.reps, sync)
    out["one_scan_host_dropin_ms"] = _median_ms(lambda: D.statisticsOnRange(base[0], BINS), a.reps, sync)

    # baselines, same run.  (a) NumPy restatement, one thread; (b) torch on the device, per scan
    out["baseline_numpy_restatement_1thread_ms_per_scan"] = _median_ms(lambda: R.range_histogram(base[0], BINS), 5, lambda: None)

    def torch_scan(k):
        p = pts[k * POINTS:(k + 1) * POINTS].to(torch.float64)
        d = torch.linalg.norm(p, dim=1)
        M = d.max()
        edges = torch.arange(1, BINS, device=dev, dtype=torch.float64) * (M / BINS)
        b = torch.bucketize(d, edges, right=True)
        b[(d <= 0) | (d >= M)] = BINS - 1
        return torch.bincount(b, minlength=BINS).to(torch.float64) / POINTS

    n_t = min(scans, 64)
    out["baseline_torch_ms_per_scan"] = _median_ms(lambda: [torch_scan(k) for k in range(n_t)], 5, sync) / n_t
    out["baseline_torch_what"] = "torch.linalg.norm + max + bucketize + bincount per scan in float64, %d scans back to back" % n_t

    # 3. the database at 10 000 entries
    h = hist.cpu().numpy()
    rng = np.random.default_rng(0)
    rows = np.abs(h[rng.integers(0, scans, ENTRIES)] + rng.normal(0, 1e-3, (ENTRIES, BINS)))
    db = F.FastHistogramDatabase(0, capacity=16384, bins=BINS)
    for r in rows:
        db.append(r)
    q, q_dev = h[5].copy(), hist[5].clone()
    assert db.distances(q).cpu().numpy().tobytes() == R.emd_all(q, rows).tobytes(), "distance mismatch"
    for k in (1, 10, 32):
        out["query_k%d_n%d_ms" % (k, ENTRIES)] = _median_ms(lambda: db.query(q, k), a.reps, lambda: None)
    out["query_k1_device_arg_n%d_ms" % ENTRIES] = _median_ms(lambda: db.query(q_dev, 1), a.reps, lambda: None)
    out["distances_n%d_ms" % ENTRIES] = _median_ms(lambda: db.distances(q_dev), a.reps, sync)
    out["baseline_numpy_emd_all_n%d_ms" % ENTRIES] = _median_ms(lambda: R.emd_all(q, rows), 5, lambda: None)
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
