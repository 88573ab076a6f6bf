"""The merged global map composed on the GPU (row G8): 3 robots x 200 keyframes x 40 000 points in three keyframe stores, leaf 0.5.
Prints ONE JSON line and, with --out, writes it to a file.  Run on its own (a fresh process).

Three timed cases, each the whole call (host clock around it: the call ends in a stream synchronisation), median / min / max of --reps
calls after WARMUP warm-up calls; baseline (b) is timed in exactly the same way:
  rebuild_skip3   GlobalMap.rebuild with compose_keyframe_ids(200, 3) of every robot (composeGlobalMap after a pose-graph correction);
  rebuild_all     GlobalMap.rebuild with every keyframe (savingGlobalMap);
  add_one         GlobalMap.add of one new keyframe per robot onto rebuild_skip3's map (the incremental branch).
Also, all in this run:
  steps_ms        the steps of a call between HIP events (the library's MRS_DEV=1 MRS_MAP_TIMING=1 development switch; a separate pass);
  fraction_of_hbm_peak   algorithmic bytes (16 B per input point read, 16 B per voxel written) over the call's time, over 8 TB/s;
  baseline (a)    the NumPy restatement (tests/golden/globalmap_restate.py) on one thread, once per case;
  baseline (b)    what the library offered before: the same keyframes appended to ONE store and KeyframeStore.assemble called with one
                  submap, crop 3e38, the same leaf and the same transforms (cases rebuild_skip3 and rebuild_all; it cannot fold a map in).
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

ROBOTS, KEYFRAMES, POINTS, DISTINCT, LEAF, SKIP = 3, 200, 40_000, 8, 0.5, 3
HBM_PEAK = 8e12
WARMUP = 3
STEPS = ["bounds_grid", "keys", "sort", "heads_scan", "means_stitch"]


def robot_poses(r, n):
    """a gently turning path, 1 m and 0.01 rad per keyframe, robot r offset by 50 r metres"""
    import submap_restate as R
    poses, x, y = [], 0.0, 50.0 * r
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


def timed(fn, reps):
    import torch
    for _ in range(WARMUP):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts)), "calls": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--small", action="store_true")
    a = ap.parse_args()
    keyframes, points = (20, 4000) if a.small else (KEYFRAMES, POINTS)

    import torch
    import globalmap_restate as G
    import submap_restate as R
    from mr_slam_amd import synth
    from mr_slam_amd.globalmap import GlobalMap, compose_keyframe_ids, pose_product
    from mr_slam_amd.submap import KeyframeStore
    assert torch.cuda.is_available(), "needs a GPU (there is no CPU fallback)"

    def say(msg):
        print("[bench_globalmap] " + msg, file=sys.stderr, flush=True)

    base = [R.with_intensity(synth.lidar_scan(s, points, metric=True), s) for s in range(DISTINCT)]
    cloud = lambda r, k: base[(r * keyframes + k) % DISTINCT]                                           # noqa: E731
    correction = R.pose(0.001, (0.01, -0.02, 0.0))              # optMapTF; originMapTF is the keyframe's pose
    T = [[pose_product(correction, p) for p in robot_poses(r, keyframes)] for r in range(ROBOTS)]
    stores = [KeyframeStore(capacity_hint=keyframes * points) for _ in range(ROBOTS)]
    single = KeyframeStore(capacity_hint=ROBOTS * keyframes * points)                                    # baseline (b): everything in ONE store
    for r in range(ROBOTS):
        for k in range(keyframes):
            stores[r].append(cloud(r, k), T[r][k])
            single.append(cloud(r, k), T[r][k])
    say("stores filled")

    cases = {"rebuild_skip3": [(r, kid, T[r][tk]) for r in range(ROBOTS) for kid, tk in compose_keyframe_ids(keyframes, SKIP)],
             "rebuild_all": [(r, k, T[r][k]) for r in range(ROBOTS) for k in range(keyframes)],
             "add_one": [(r, keyframes - 1, T[r][keyframes - 1]) for r in range(ROBOTS)]}
    gm = GlobalMap(stores, leaf=LEAF)
    base_map = gm.rebuild(cases["rebuild_skip3"]).clone()

    def run(name):
        if name == "add_one":
            gm.points = base_map
            return gm.add(cases[name])
        return gm.rebuild(cases[name])

    out = {"metric": "global_map_compose", "robots": ROBOTS, "keyframes_per_robot": keyframes, "points_per_keyframe": points, "leaf": LEAF,
           "cases": {}}
    for name, segs in cases.items():
        n_prev = base_map.shape[0] if name == "add_one" else 0
        n_in = n_prev + len(segs) * points
        res = timed(lambda: run(name), a.reps)
        voxels = int(run(name).shape[0])
        nbytes = 16 * n_in + 16 * voxels
        res.update(input_points=n_in, previous_map_points=n_prev, voxels_out=voxels, algorithmic_bytes=nbytes,
                   input_points_per_s=n_in / (res["median_ms"] * 1e-3),
                   fraction_of_hbm_peak=nbytes / (res["median_ms"] * 1e-3) / HBM_PEAK)
        out["cases"][name] = res
        say("%s: %.3f ms (min %.3f max %.3f), %d points -> %d voxels" % (name, res["median_ms"], res["min_ms"], res["max_ms"], n_in, voxels))

    # the steps, in a pass of their own
    os.environ["MRS_DEV"], os.environ["MRS_MAP_TIMING"] = "1", "1"
    for name in cases:
        with captured_stderr() as err:
            for _ in range(3):
                run(name)
        rows = [[float(v) for v in m] for m in re.findall(
            r"map steps ms: bounds\+grid (\S+) keys (\S+) sort (\S+) heads\+scan (\S+) means\+stitch (\S+) points \d+ bits (\d+)", err["text"])]
        if rows:
            med = np.median(np.array(rows), axis=0).tolist()
            out["cases"][name]["steps_ms"] = dict(zip(STEPS, med[:5]))
            out["cases"][name]["sorted_key_bits"] = int(med[5])
    del os.environ["MRS_MAP_TIMING"], os.environ["MRS_DEV"]

    # baseline (b): one store, one submap, a crop that keeps everything
    for name in ("rebuild_skip3", "rebuild_all"):
        one = [[(r * keyframes + k, Tk) for r, k, Tk in cases[name]]]
        res = timed(lambda: single.assemble(one, crop=3e38, leaf=LEAF), a.reps)
        pts, _ = single.assemble(one, crop=3e38, leaf=LEAF)
        new = run(name)
        res["voxels_out"] = int(pts.shape[0])
        res["same_voxel_count"] = bool(pts.shape[0] == new.shape[0])
        res["largest_difference_of_means"] = float((pts - new).abs().max()) if pts.shape == new.shape else None
        c = out["cases"][name]
        c["baseline_b_assemble_one_submap"] = res
        c["not_slower_than_baseline_b"] = bool(c["median_ms"] <= res["median_ms"])
        say("%s baseline (b): %.3f ms (min %.3f max %.3f)" % (name, res["median_ms"], res["min_ms"], res["max_ms"]))
        del pts, new

    # baseline (a): the restatement on one thread, once per case
    host_prev = base_map.cpu().numpy()
    for name, segs in cases.items():
        host = [(cloud(r, k), Tk) for r, k, Tk in segs]
        t0 = time.perf_counter()
        want = G.compose(host, LEAF, prev=host_prev if name == "add_one" else None)
        ms = (time.perf_counter() - t0) * 1e3
        out["cases"][name]["baseline_a_restatement_ms"] = ms
        out["cases"][name]["baseline_a_voxels"] = int(want.keys.size)
        say("%s baseline (a): %.0f ms" % (name, ms))
        del want, host
    out["note"] = ("whole calls, host clock, median of %d after %d warm-up calls, baseline (b) likewise; baseline (a): one run; "
                   "steps: HIP events, separate pass" % (a.reps, WARMUP))
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
