"""Keyframe intake on the GPU (row G10): raw 120 000-point clouds through KeyframeStore.ingest / ingest_batch, leaf 0.3, z in [-1, 30],
intensity tag.  Prints ONE JSON line and, with --out, writes it to a file.  Run on its own (a fresh process).

Two timed shapes, each the whole call (host clock around it: the call ends in the handle's stream synchronisation), median / min / max of
--reps calls after WARMUP warm-up calls; baseline (b) is timed in exactly the same way:
  one_host_blob       one keyframe from a HOST blob in the pcl::PointXYZI layout (point_step 32): the Mapping callback's shape;
  batch_device_blob   BATCH such keyframes in one call from one DEVICE blob (a bag replay, several robots' callbacks).
Also, all in this run:
  steps_ms            the steps of a call between HIP events (the library's MRS_DEV=1 MRS_INTAKE_TIMING=1 development switch; a separate pass);
  fraction_of_hbm_peak  algorithmic bytes (point_step bytes read per raw point, 16 B written per survivor) over the call's time, over 8 TB/s;
  baseline (a)        the NumPy restatement (tests/golden/intake_restate.py) on one thread, once per distinct cloud;
  baseline (b)        what the library offered before, with calls that predate the intake only: append(raw) to a scratch store,
                      assemble([[(id, I)]], crop=3e38, leaf), a torch mask on z, an intensity fill, append into the real store.
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

POINTS, BATCH, DISTINCT, LEAF, Z_LIMITS, TAG, STEP = 120_000, 64, 8, 0.3, (-1.0, 30.0), 60.0, 32
HBM_PEAK = 8e12
WARMUP = 3
STEPS = ["upload", "bounds_grid", "keys", "sort", "means", "scan_scatter"]


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
    points, batch = (6000, 4) if a.small else (POINTS, BATCH)

    import torch
    import intake_restate as K
    import submap_restate as R
    from mr_slam_amd import synth
    from mr_slam_amd.submap import KeyframeStore
    assert torch.cuda.is_available(), "needs a GPU (there is no CPU fallback)"

    def say(msg):
        print("[bench_intake] " + msg, file=sys.stderr, flush=True)

    eye = np.eye(4, dtype=np.float32)
    base = []
    for s in range(DISTINCT):                                   # the sensor's frame: the generator's ground sits at z = 0
        c = R.with_intensity(synth.lidar_scan(s, points, metric=True), s)
        c[:, 2] -= np.float32(1.7)
        base.append(c)

    def wide(c):                                                # float32 [n, 8] with pcl::PointXYZI's layout
        w = np.zeros((c.shape[0], 8), np.float32)
        w[:, :3], w[:, 4] = c[:, :3], c[:, 3]
        return w

    calls = WARMUP + a.reps + 8
    host_one = wide(base[0])
    dev_batch = torch.from_numpy(np.concatenate([wide(base[k % DISTINCT]) for k in range(batch)])).cuda()
    dev_clouds = [dev_batch[k * points:(k + 1) * points] for k in range(batch)]
    offsets = np.arange(batch + 1, dtype=np.int64) * points
    poses = [eye] * batch
    shapes = {"one_host_blob": 1, "batch_device_blob": batch}
    new_store = {name: KeyframeStore(capacity_hint=calls * n * points) for name, n in shapes.items()}

    def run(name):
        if name == "one_host_blob":
            return new_store[name].ingest_batch([host_one], [eye], LEAF, Z_LIMITS, TAG)[1]
        return new_store[name].ingest_batch(dev_batch, poses, LEAF, Z_LIMITS, TAG, offsets=offsets)[1]

    out = {"metric": "keyframe_intake", "points_per_keyframe": points, "batch": batch, "leaf": LEAF, "z_limits": list(Z_LIMITS),
           "point_step": STEP, "shapes": {}}
    for name, n in shapes.items():
        res = timed(lambda: run(name), a.reps)
        survivors = int(run(name).sum())
        n_in = n * points
        nbytes = STEP * n_in + 16 * survivors
        res.update(raw_points=n_in, survivors=survivors, algorithmic_bytes=nbytes, raw_points_per_s=n_in / (res["median_ms"] * 1e-3),
                   fraction_of_hbm_peak=nbytes / (res["median_ms"] * 1e-3) / HBM_PEAK)
        out["shapes"][name] = res
        say("%s: %.3f ms (min %.3f max %.3f), %d points -> %d survivors" % (name, res["median_ms"], res["min_ms"], res["max_ms"], n_in, survivors))

    # the steps, in a pass of their own
    os.environ["MRS_DEV"], os.environ["MRS_INTAKE_TIMING"] = "1", "1"
    for name in shapes:
        with captured_stderr() as err:
            for _ in range(3):
                run(name)
        rows = [[float(v) for v in m] for m in re.findall(
            r"intake steps ms: upload (\S+) bounds\+grid (\S+) keys (\S+) sort (\S+) means (\S+) scan\+scatter (\S+) points \d+ bits (\d+)",
            err["text"])]
        if rows:
            med = np.median(np.array(rows), axis=0).tolist()
            out["shapes"][name]["steps_ms"] = dict(zip(STEPS, med[:6]))
            out["shapes"][name]["sorted_key_bits"] = int(med[6])
    del os.environ["MRS_INTAKE_TIMING"], os.environ["MRS_DEV"]

    # baseline (b): the detour through a scratch store, with calls that predate the intake only
    scratch = {name: KeyframeStore(capacity_hint=calls * n * points) for name, n in shapes.items()}
    real = {name: KeyframeStore(capacity_hint=calls * n * points) for name, n in shapes.items()}

    def detour(name):
        clouds = [host_one] if name == "one_host_blob" else dev_clouds
        ids = [scratch[name].append(c, eye) for c in clouds]
        pts, offs = scratch[name].assemble([[(k, eye)] for k in ids], crop=3e38, leaf=LEAF)
        total = 0
        for b in range(len(ids)):
            sub = pts[int(offs[b]):int(offs[b + 1])]
            sub = sub[(sub[:, 2] >= Z_LIMITS[0]) & (sub[:, 2] <= Z_LIMITS[1])]
            sub[:, 3] = TAG
            real[name].append(sub, eye)
            total += sub.shape[0]
        return total

    for name in shapes:
        res = timed(lambda: detour(name), a.reps)
        res["survivors"] = int(detour(name))
        c = out["shapes"][name]
        res["same_survivor_count"] = bool(res["survivors"] == c["survivors"])
        c["baseline_b_detour"] = res
        c["ratio_to_baseline_b"] = c["median_ms"] / res["median_ms"]
        c["not_slower_than_baseline_b"] = bool(c["median_ms"] <= res["median_ms"])
        say("%s baseline (b): %.3f ms (min %.3f max %.3f)" % (name, res["median_ms"], res["min_ms"], res["max_ms"]))

    # baseline (a): the restatement on one thread, once per distinct cloud
    ms = []
    for c in base[:min(DISTINCT, batch)]:
        t0 = time.perf_counter()
        K.ingest(c, LEAF, Z_LIMITS, TAG)
        ms.append((time.perf_counter() - t0) * 1e3)
    out["baseline_a_restatement_ms_per_keyframe"] = float(np.median(ms))
    say("baseline (a): %.0f ms per keyframe" % np.median(ms))
    out["note"] = ("whole calls, host clock, median of %d after %d warm-up calls, baseline (b) likewise; baseline (a): one run per cloud; "
                   "steps: HIP events, separate pass" % (a.reps, WARMUP))
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
