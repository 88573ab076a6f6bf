"""GICP submap assembly on the GPU (row G0): one batch of 256 loop candidates = 512 submaps (submap_size 1, leaf 0.2, crop 60) from a resident
store of 600 keyframes x 40 000 points.  Prints ONE JSON line and, with --out, writes it to a file.  Run on its own (a fresh process).

What is measured, all in this run:
  merge_nearest_ms        the whole call (host clock around it: the call ends in the handle's stream synchronisation), median after warm-up;
  steps_ms                the steps of the call between HIP events on the handle's stream (the library's MRS_SUBMAP_TIMING development
                          switch; a separate pass, not the calls timed above);
  fraction_of_hbm_peak    algorithmic bytes (16 B per segment point read, 16 B per voxel written) over merge_nearest_ms, over 8 TB/s;
  one_candidate_*         the same call for ONE candidate (2 submaps): the interactive case;
  handover_ms             merge_nearest for the query and the database side + GicpBatch.set_sources + set_targets;
  baseline (a)            the NumPy restatement (tests/golden/submap_restate.py) on one thread, per submap, over --baseline-submaps submaps;
  baseline (b)            what the library offered before: the restatement's merged clouds handed to GicpBatch.set_sources / set_targets as
                          host arrays (restatement time + upload time, per pair).
The baselines never use the new code.  --small shrinks everything (rehearsal; its numbers mean nothing).
"""
import argparse
import contextlib
import json
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

KEYFRAMES, POINTS, DISTINCT, CANDIDATES, SUBMAP_SIZE, LEAF, CROP = 600, 40_000, 8, 256, 1, 0.2, 60.0
HBM_PEAK = 8e12


def path_poses(n):
    """a gently turning path: 1 m per keyframe, 0.01 rad of yaw per keyframe"""
    import submap_restate as R
    poses, x, y = [], 0.0, 0.0
    for k in range(n):
        yaw = 0.01 * k
        poses.append(R.pose(yaw, (x, y, 0.0)))
        x, y = x + np.cos(yaw), y + np.sin(yaw)
    return poses


@contextlib.contextmanager
def captured_stderr():
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as f:
        os.dup2(f.fileno(), 2)
        box = {}
        try:
            yield box
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            f.seek(0)
            box["text"] = f.read().decode(errors="replace")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--baseline-submaps", type=int, default=16)
    ap.add_argument("--small", action="store_true")
    a = ap.parse_args()
    keyframes, points, candidates = (40, 4000, 8) if a.small else (KEYFRAMES, POINTS, CANDIDATES)

    import torch
    import submap_restate as R
    from mr_slam_amd import synth
    from mr_slam_amd.gicp import GicpBatch
    from mr_slam_amd.submap import KeyframeStore
    assert torch.cuda.is_available(), "needs a GPU (there is no CPU fallback)"

    base = [R.with_intensity(synth.lidar_scan(s, points, metric=True), s) for s in range(DISTINCT)]
    poses = path_poses(keyframes)
    clouds = [base[k % DISTINCT] for k in range(keyframes)]
    store = KeyframeStore(capacity_hint=keyframes * points)
    t0 = time.perf_counter()
    for c, p in zip(clouds, poses):
        store.append(c, p)
    append_ms = (time.perf_counter() - t0) * 1e3 / keyframes
    rng = np.random.default_rng(0)
    query_ids = rng.integers(1, keyframes - 1, candidates)
    db_ids = rng.integers(1, keyframes - 1, candidates)
    ids = np.concatenate([query_ids, db_ids])                   # 512 submaps in one call
    seg_points = sum(clouds[k].shape[0] for c in ids for k in R.nearest_keyframe_ids(int(c), SUBMAP_SIZE, keyframes))

    for _ in range(3):
        pts, offs = store.merge_nearest(ids, SUBMAP_SIZE, CROP, LEAF)
    ts = []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pts, offs = store.merge_nearest(ids, SUBMAP_SIZE, CROP, LEAF)
        ts.append((time.perf_counter() - t0) * 1e3)
    ms, merge_min, merge_max = float(np.median(ts)), float(min(ts)), float(max(ts))
    voxels = int(offs[-1])
    algorithmic_bytes = 16 * seg_points + 16 * voxels

    # the interactive case: ONE candidate = 2 submaps per call (the segmented sort gives a large segment to one workgroup)
    one = np.array([query_ids[0], db_ids[0]])
    for _ in range(3):
        store.merge_nearest(one, SUBMAP_SIZE, CROP, LEAF)
    ts1 = []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        store.merge_nearest(one, SUBMAP_SIZE, CROP, LEAF)
        ts1.append((time.perf_counter() - t0) * 1e3)
    one_ms = float(np.median(ts1))

    os.environ["MRS_DEV"], os.environ["MRS_SUBMAP_TIMING"] = "1", "1"
    with captured_stderr() as err:
        for _ in range(3):
            store.merge_nearest(ids, SUBMAP_SIZE, CROP, LEAF)
        for _ in range(3):
            store.merge_nearest(one, SUBMAP_SIZE, CROP, LEAF)
    del os.environ["MRS_SUBMAP_TIMING"], os.environ["MRS_DEV"]
    rows = [[float(v) for v in m] for m in re.findall(
        r"submap steps ms: cells\+grid (\S+) keys (\S+) sort (\S+) heads\+scan (\S+) means\+offsets (\S+)", err["text"])]
    names = ["cells_grid", "keys", "sort", "heads_scan", "means_offsets"]
    steps = dict(zip(names, np.median(np.array(rows[:3]), axis=0).tolist())) if len(rows) >= 3 else None
    steps_one = dict(zip(names, np.median(np.array(rows[3:]), axis=0).tolist())) if len(rows) >= 6 else None

    # the whole hand-over: both sides assembled, then set as the sources and targets of one batch
    batch = GicpBatch(candidates)

    def handover():
        batch.set_sources(store.merge_nearest(query_ids, SUBMAP_SIZE, CROP, LEAF))
        batch.set_targets(store.merge_nearest(db_ids, SUBMAP_SIZE, CROP, LEAF))
        torch.cuda.synchronize()

    handover()
    ts = []
    for _ in range(max(3, a.reps // 2)):
        t0 = time.perf_counter()
        handover()
        ts.append((time.perf_counter() - t0) * 1e3)
    handover_ms = float(np.median(ts))

    # baselines: restatement on one thread, and its clouds uploaded as host arrays
    nb = min(a.baseline_submaps, candidates)
    t0 = time.perf_counter()
    host_q = [R.merge_nearest(clouds, poses, int(c), SUBMAP_SIZE, CROP, LEAF).means.astype(np.float32) for c in query_ids[:nb]]
    host_d = [R.merge_nearest(clouds, poses, int(c), SUBMAP_SIZE, CROP, LEAF).means.astype(np.float32) for c in db_ids[:nb]]
    restate_ms_per_submap = (time.perf_counter() - t0) * 1e3 / (2 * nb)
    small = GicpBatch(nb)

    def upload():
        small.set_sources(host_q)
        small.set_targets(host_d)
        torch.cuda.synchronize()

    upload()
    ts = []
    for _ in range(5):
        t0 = time.perf_counter()
        upload()
        ts.append((time.perf_counter() - t0) * 1e3)
    upload_ms_per_pair = float(np.median(ts)) / nb
    same = all(np.array_equal(offs[b + 1] - offs[b], h.shape[0]) for b, h in enumerate(host_q))

    out = {"metric": "submap_assembly", "keyframes": keyframes, "points_per_keyframe": points, "submaps": int(ids.size),
           "submap_size": SUBMAP_SIZE, "leaf": LEAF, "crop": CROP, "segment_points": int(seg_points), "voxels_out": voxels,
           "append_ms_per_keyframe_host_float32x4": append_ms,
           "merge_nearest_ms": ms, "merge_nearest_ms_min": merge_min, "merge_nearest_ms_max": merge_max,
           "segment_points_per_s": seg_points / (ms * 1e-3), "algorithmic_bytes": int(algorithmic_bytes),
           "achieved_bytes_per_s": algorithmic_bytes / (ms * 1e-3), "fraction_of_hbm_peak": algorithmic_bytes / (ms * 1e-3) / HBM_PEAK,
           "steps_ms": steps, "one_candidate_2_submaps_ms": one_ms, "one_candidate_steps_ms": steps_one, "handover_ms": handover_ms, "handover_ms_per_candidate": handover_ms / candidates,
           "baseline_a_restatement_ms_per_submap": restate_ms_per_submap,
           "baseline_a_restatement_ms_per_batch": restate_ms_per_submap * ids.size,
           "baseline_b_upload_ms_per_pair": upload_ms_per_pair,
           "baseline_b_ms_per_candidate": 2 * restate_ms_per_submap + upload_ms_per_pair,
           "baseline_b_ms_per_batch": (2 * restate_ms_per_submap + upload_ms_per_pair) * candidates,
           "baseline_submaps_measured": 2 * nb, "voxel_counts_equal_restatement": bool(same),
           "note": "merge_nearest_ms: whole call, host clock, median of %d after 3 warm-up calls; steps: HIP events, separate pass" % a.reps}
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
