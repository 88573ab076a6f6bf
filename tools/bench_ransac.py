"""RANSAC pose from correspondences on the GPU: ms per whole blocking call and per stage (models, score, refit: between HIP events inside
mrs_ransac_pose_batch_profile), for 256 pairs and for 1 pair at M = 2 000 and M = 7 000 correspondences (7 000 is the ISS keypoint count
per scan of profiles/fpfh_notes.md), H = 4096 hypotheses.  Prints ONE JSON line and, with --out, writes it to a file.  Run on its own (a
fresh process).

Both baselines are measured in the same run, never taken from the new code:
  (a) the NumPy restatement (tests/golden/ransac_restate.py) on one CPU thread, one pair;
  (b) what a user had before: batched torch.linalg.svd for the models of the valid triples plus an [H_valid, M] distance matrix per pair on
      the device (the triples and their pre-rejection are taken from the restatement, outside the timed part).
The fp64 rate counts the 26 add / multiply / subtract operations of one residual (contraction is off, so none fuses) per (valid model,
correspondence) of the scoring stage against 256 CUs x 4 SIMDs x 64 lanes / 4 cycles x 2.4 GHz = 39.3e12 fp64 operations per second
(profiles/r03_ubench.md: every fp64 instruction occupies its SIMD for 4 cycles).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

H, D, INLIERS, NOISE = 4096, 0.3, 0.3, 0.05
RESIDUAL_OPS = 26
PEAK_FP64 = 256 * 4 * 64 / 4 * 2.4e9


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


def torch_baseline(torch, src, dst, idx_ok, d):
    """one pair: Kabsch of every valid triple by batched torch.linalg.svd, then the [H_valid, M] matrix of squared residuals, its
    counts and the argmax; fp64 on the device"""
    P, Q = src[:, :3].double(), dst[:, :3].double()
    a, b = P[idx_ok], Q[idx_ok]                                   # [V, 3, 3]
    ab, bb = a.mean(1, keepdim=True), b.mean(1, keepdim=True)
    Hm = (a - ab).transpose(1, 2) @ (b - bb)
    U, _, Vt = torch.linalg.svd(Hm)
    dsign = torch.sign(torch.linalg.det(Vt.transpose(1, 2) @ U.transpose(1, 2)))
    S = torch.diag_embed(torch.stack([torch.ones_like(dsign), torch.ones_like(dsign), dsign], 1))
    Rm = Vt.transpose(1, 2) @ S @ U.transpose(1, 2)
    t = bb.squeeze(1) - (Rm @ ab.transpose(1, 2)).squeeze(2)
    e = P[None] @ Rm.transpose(1, 2) + t[:, None] - Q[None]      # [V, M, 3]
    counts = ((e * e).sum(-1) <= d * d).sum(1)
    return int(counts.argmax()), int(counts.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-baselines", action="store_true")
    args = ap.parse_args()
    import torch
    import ransac_cases as K
    from mr_slam_amd import fpfh
    R = K.R
    assert torch.cuda.is_available(), "needs a GPU"
    out = dict(hypotheses=H, max_distance=D, inlier_share=INLIERS, reps=args.reps, peak_fp64_ops_per_s=PEAK_FP64, cases=[])
    for M in (2000, 7000):
        distinct = [K.make(1000 + i, M, inl=INLIERS, noise=NOISE)[:2] for i in range(8)]
        for pairs in (256, 1):
            src = torch.tensor(np.concatenate([distinct[i % 8][0] for i in range(pairs)])).to("cuda:0")
            dst = torch.tensor(np.concatenate([distinct[i % 8][1] for i in range(pairs)])).to("cuda:0")
            off = np.arange(pairs + 1, dtype=np.int64) * M
            offs = (torch.from_numpy(off), torch.from_numpy(off).to("cuda:0"))
            seeds = np.arange(pairs, dtype=np.uint64)
            call = lambda **kw: fpfh.ransac_pose(src, dst, offs, D, seeds=seeds, hypotheses=H, **kw)
            c = dict(pairs=pairs, correspondences=M)
            c["call_ms"] = _host_ms(call, args.reps, torch.cuda.synchronize)
            c["call_with_mask_ms"] = _host_ms(lambda: call(return_mask=True), args.reps, torch.cuda.synchronize)
            ms = np.median([call(profile=True)[-1] for _ in range(args.reps)], axis=0)
            c["models_ms"], c["score_ms"], c["refit_ms"] = (float(x) for x in ms)
            T, info = call()
            info = info.cpu().numpy()
            c["valid_models"] = int(info[:, 2].sum())
            c["inliers_mean"] = float(info[:, 0].mean())
            ops = RESIDUAL_OPS * float(info[:, 2].sum()) * M
            c["score_fp64_ops_per_s"] = ops / (c["score_ms"] * 1e-3) if c["score_ms"] > 0 else None
            c["score_share_of_fp64_peak"] = c["score_fp64_ops_per_s"] / PEAK_FP64 if c["score_ms"] > 0 else None
            out["cases"].append(c)
        if not args.no_baselines:
            s0, d0 = distinct[0]
            t0 = time.perf_counter()
            r = R.ransac(s0, d0, 0, D, hypotheses=H)
            b = dict(correspondences=M, numpy_restatement_one_pair_ms=(time.perf_counter() - t0) * 1e3)
            idx_ok = torch.from_numpy(r["idx"][r["ok"]]).to("cuda:0")
            ts, td = torch.tensor(s0).to("cuda:0"), torch.tensor(d0).to("cuda:0")
            got = torch_baseline(torch, ts, td, idx_ok, D)
            b["torch_svd_distance_matrix_one_pair_ms"] = _host_ms(lambda: torch_baseline(torch, ts, td, idx_ok, D), args.reps, torch.cuda.synchronize)
            b["torch_best_count"], b["restatement_best_count"] = got[1], int(r["counts"].max())
            b["valid_models"] = int(r["ok"].sum())
            out.setdefault("baselines", []).append(b)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
