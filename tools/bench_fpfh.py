"""FPFH on the GPU: ms per stage (radius count, radius fill, SPFH, FPFH of every point, ISS) between HIP events and whole blocking calls, for
one resident 120 000-point scan and for 64 resident scans.  Prints ONE JSON line and, with --out, writes it to a file.  Run on its own (a
fresh process).

Both baselines are measured in the same run, never taken from the new code:
  (a) sklearn KDTree(points, 4).query_radius on one CPU thread, one scan (what the reference's __main__ calls for its lists);
  (b) the NumPy restatement (tests/golden/fpfh_restate.py: SPFH and FPFH of every point, vectorised) on one CPU thread, on those lists.
The reference's own get_spfh / describe are Python calls per keypoint and per neighbour; they are not run here.

The scan is mr_slam_amd.synth.lidar_scan (normalised coordinates, |x| <= 1); the radius is chosen for rows of some tens of entries (the
row statistics are part of the output).  The normals are synthetic unit vectors: the stage times do not depend on their values.
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

SCANS, POINTS, DISTINCT, BINS, RADIUS, ISS_SALIENT = 64, 120_000, 8, 5, 0.004, 0.006


def _event_ms(fn, reps, torch):
    """median over `reps` of the time of one call between two events on the current stream"""
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e))
    return float(np.median(ts))


def _host_ms(fn, reps, sync):
    fn()
    sync()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def stages(F, _lib, torch, pts, nrm, offs, reps):
    """-> dict of stage times for the packed batch (pts, nrm, offs = (host, device))"""
    h_off, d_off = offs
    B, n = h_off.numel() - 1, pts.shape[0]
    lib, ctx, stream = _lib.load(), _lib.ctx(0), _lib.current_stream(0)
    row_start = torch.empty(n + 1, dtype=torch.int64, device=pts.device)
    total = np.zeros(1, np.int64)
    out = {}
    out["radius_count_ms"] = _event_ms(lambda: lib.mrs_radius_count(ctx, pts, 3, d_off, h_off, B, RADIUS, row_start, total, stream), reps, torch)
    index = torch.empty(int(total[0]), dtype=torch.int32, device=pts.device)
    out["radius_fill_ms"] = _event_ms(lambda: lib.mrs_radius_fill(ctx, pts, 3, d_off, h_off, B, RADIUS, row_start, int(total[0]), index, stream),
                                      reps, torch)
    rows = (row_start, index)
    lens = (row_start[1:] - row_start[:-1]).to(torch.float64)
    out.update({"row_entries": int(total[0]), "row_mean": float(lens.mean()), "row_median": float(lens.median()), "row_max": int(lens.max())})
    out["spfh_ms"] = _event_ms(lambda: F.spfh(pts, nrm, offs, rows, BINS), reps, torch)
    _, s = F.spfh(pts, nrm, offs, rows, BINS)
    out["fpfh_all_points_ms"] = _event_ms(lambda: F.describe(pts, offs, rows, s, BINS), reps, torch)
    out["whole_fpfh_call_blocking_ms"] = _host_ms(lambda: F.fpfh(pts, nrm, offs, RADIUS, BINS), reps, torch.cuda.synchronize)
    out["whole_iss_call_blocking_ms"] = _host_ms(lambda: F.iss_keypoints(pts, offs, ISS_SALIENT, RADIUS), max(1, reps // 2), torch.cuda.synchronize)
    kp, _ = F.iss_keypoints(pts, offs, ISS_SALIENT, RADIUS)
    out["iss_keypoints"] = int(sum(k.numel() for k in kp))
    out["fpfh_iss_keypoints_ms"] = _event_ms(lambda: F.describe(pts, offs, rows, s, BINS, kp), reps, torch)
    return out, rows, s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--scans", type=int, default=SCANS)
    ap.add_argument("--no-baselines", action="store_true")
    a = ap.parse_args()
    os.environ.setdefault("OMP_NUM_THREADS", "1")
    import torch
    import fpfh_restate as R
    from mr_slam_amd import _lib, fpfh as F, synth
    assert torch.cuda.is_available(), "needs a GPU (there is no CPU fallback)"
    dev = "cuda:0"
    scans = max(DISTINCT, a.scans // DISTINCT * DISTINCT)
    base = [synth.lidar_scan(s, POINTS)[:, :3].astype(np.float32) for s in range(DISTINCT)]
    normals = [b / np.maximum(np.linalg.norm(b, axis=1)[:, None], 1e-12) for b in base]
    out = {"metric": "fpfh", "points_per_scan": POINTS, "bins": BINS, "radius": RADIUS, "iss_salient_radius": ISS_SALIENT,
           "iss_non_max_radius": RADIUS, "input": "float32 [n, 3] points and normals resident in HBM", "reps_median_of": a.reps}

    one_pts, one_nrm = torch.from_numpy(base[0]).to(dev), torch.from_numpy(normals[0].astype(np.float32)).to(dev)
    one_off = torch.tensor([0, POINTS], dtype=torch.int64)
    one, rows, s = stages(F, _lib, torch, one_pts, one_nrm, (one_off, one_off.to(dev)), a.reps)
    out["one_scan"] = one

    pts = torch.from_numpy(np.concatenate(base)).to(dev).repeat(scans // DISTINCT, 1)
    nrm = torch.from_numpy(np.concatenate(normals).astype(np.float32)).to(dev).repeat(scans // DISTINCT, 1)
    offs = torch.arange(scans + 1, dtype=torch.int64) * POINTS
    many, rows_many, s_many = stages(F, _lib, torch, pts, nrm, (offs, offs.to(dev)), max(2, a.reps // 3))
    many["scans"] = scans
    many["whole_fpfh_call_ms_per_scan"] = many["whole_fpfh_call_blocking_ms"] / scans
    out["batch"] = many
    # a cloud gives the same bits alone and in the batch
    n_rows = int(rows[0][-1])
    out["batch_equals_single_bit_for_bit"] = bool(torch.equal(rows[1], rows_many[1][:n_rows]) and torch.equal(s, s_many[:POINTS]))

    if not a.no_baselines:
        from sklearn.neighbors import KDTree
        P = base[0].astype(np.float64)
        t0 = time.perf_counter()
        tree = KDTree(P, 4)
        t1 = time.perf_counter()
        lists = tree.query_radius(P, RADIUS)
        t2 = time.perf_counter()
        out["baseline_sklearn_kdtree_build_1thread_ms"] = (t1 - t0) * 1e3
        out["baseline_sklearn_query_radius_1thread_ms"] = (t2 - t1) * 1e3
        lists = [np.sort(l) for l in lists]
        t0 = time.perf_counter()
        counts, values = R.spfh(base[0], normals[0].astype(np.float32), lists, BINS)
        t1 = time.perf_counter()
        f = R.fpfh(base[0], lists, values)
        t2 = time.perf_counter()
        out["baseline_numpy_restatement_spfh_1thread_ms"] = (t1 - t0) * 1e3
        out["baseline_numpy_restatement_fpfh_1thread_ms"] = (t2 - t1) * 1e3
        got_rows = R.from_csr(rows[0].cpu().numpy(), rows[1].cpu().numpy())
        out["rows_equal_sklearn"] = all(np.array_equal(x[x != i], y) for i, (x, y) in enumerate(zip(lists, got_rows)))
        out["spfh_equal_restatement_bit_for_bit"] = bool(np.array_equal(s.cpu().numpy(), values))
        out["fpfh_equal_restatement_bit_for_bit"] = bool(np.array_equal(F.describe(one_pts, one_off, rows, s, BINS).cpu().numpy(), f))
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            json.dump(out, fo, indent=1)
            fo.write("\n")


if __name__ == "__main__":
    main()
