#!/usr/bin/env python3
"""Fused descriptor kernel: variant 1 (raw sums parked in the output buffer, re-read, rewritten) against variant 2 (sinogram written once:
raw sums in registers through the march, transposed through the free tile): same bits, time per 1024 scans.  python tools/quick_fused_once.py [--chunks 16]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from mr_slam_amd import ring  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--chunks", type=int, default=16)
ap.add_argument("--batch", type=int, default=1024)
args = ap.parse_args()
dev = "cuda:0"
B, CH, N = args.batch, args.chunks, bench.N_POINTS
bench.make_shard(B, CH, 0, dev)
whole = bench.make_shard.whole
for nscan in (CH * B, CH * B - 1):
    offs = torch.arange(nscan + 1, dtype=torch.int64, device=dev) * N
    flat = whole[:CH].view(-1)[: nscan * 3 * N]
    plan = ring.ring_plan(0)

    def fused(out, raw=False):
        return ring.ring_descriptors_fused(flat, offs, raw=raw, normalized=True, out_norm=out)

    was = plan.get_option(plan.OPT_FUSED_VARIANT)
    plan.set_option(plan.OPT_FUSED_VARIANT, 1)
    _, raw_ref, ref = fused(None, raw=True)
    ref, raw_ref = ref.clone(), raw_ref.clone()
    buf = torch.empty_like(ref)
    for rep in range(3):
        for v in (1, 2):
            plan.set_option(plan.OPT_FUSED_VARIANT, v)
            buf.zero_()
            _, raw_got, got = fused(buf, raw=(rep == 0))
            torch.cuda.synchronize()
            same = bool(torch.equal(ref.view(torch.int32), got.view(torch.int32))) and (raw_got is None or bool(torch.equal(raw_got, raw_ref)))
            ms = bench.ev_ms(lambda: fused(buf), reps=5, warm=1)
            print({"scans": nscan, "variant": v, "bit_identical": same, "ms_per_1024": round(ms / nscan * 1024, 4)}, flush=True)
    plan.set_option(plan.OPT_FUSED_VARIANT, was)
