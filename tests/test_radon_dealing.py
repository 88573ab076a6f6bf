"""The conflict-aware dealing of Radon rays to lane slots (mr_slam_amd/csrc/radon_deal.hpp).

CPU: the routine, compiled with the host compiler, places every ray exactly once, keeps the orientations apart, is deterministic, and
reaches the modelled cost the unrefined numpy prototype reached (tools/radon_order_sim.py is the model; figures from the issue that
asked for the dealing: LDS-array cycles <= 140 434 with wave-steps <= 23 604 for the default 120 x 120 plan on a 120 x 120 image).
GPU: any table that holds every ray once gives the same sinogram bits, so the fused descriptor kernel must reproduce, for all three
OPT_FUSED_VARIANT values, the digests recorded from the commit before the dealing changed (tests/golden/radon_dealing_parent.json:
SHA-256 of the raw and the normalised sinograms of the scans of tests/test_fused_gpu.py, an odd batch).
"""
import ctypes as C
import hashlib
import importlib.util
import io
import json
import os
import subprocess
import sys
from contextlib import redirect_stdout

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "radon_dealing_parent.json")
WG = 1024
LDS_CYCLES_MAX, WAVE_STEPS_MAX = 140434, 23604

sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def deal(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("radon_deal") / "radon_deal.so")
    cmd = ["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "mr_slam_amd", "csrc"),
           os.path.join(ROOT, "tests", "cpp", "radon_deal_capi.cpp"), "-o", so]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lib = C.CDLL(so)
    lib.deal_rays_c.restype = C.c_int

    def run(t, stride):
        """t: ray table of tools/radon_lds_sim.ray_table -> slot table [per_lane, 16 waves, 64 lanes]"""
        import radon_lds_sim as sim
        rays = t["n"].size
        meta = (t["n"] | (t["ydom"].astype(np.int64) << 16)).astype(np.int32)
        base = (4 * np.where(t["ydom"], (t["major"] + sim.PAD) * stride, t["major"] + sim.PAD)).astype(np.int32)
        q, vm = t["q"].astype(np.float32), t["vm"].astype(np.float32)
        per_lane = (rays + WG - 1) // WG
        out = np.full(per_lane * WG, -7, dtype=np.int32)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        got = lib.deal_rays_c(ptr(meta), ptr(base), ptr(q), ptr(vm), rays, stride, WG, per_lane, ptr(out))
        assert got == out.size
        return out.reshape(per_lane, WG // 64, 64)
    return run


GEOMETRIES = {"default": dict(A=120, D=120, H=120, W=120), "90x100_on_100x120": dict(A=90, D=100, H=100, W=120),
              "under_1024_rays": dict(A=30, D=30, H=120, W=120)}


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_every_ray_once_orientations_apart_deterministic(deal, name):
    import radon_lds_sim as sim
    g = GEOMETRIES[name]
    t = sim.ray_table(**g)
    stride = (g["W"] + 2 * sim.PAD) | 1
    tab = deal(t, stride)
    rays = t["n"].size
    flat = tab.ravel()
    assert np.array_equal(np.sort(flat[flat >= 0]), np.arange(rays)), "a ray is missing or dealt twice"
    assert (flat[flat < 0] == -1).all() and (flat < 0).sum() == flat.size - rays
    mixed = 0
    for w in range(tab.shape[1]):
        idle_seen = np.zeros(64, dtype=bool)
        for k in range(tab.shape[0]):
            r = tab[k, w]
            assert not (idle_seen & (r >= 0)).any(), "an idle slot is followed by a ray in its lane"
            idle_seen |= r < 0
            live = r[r >= 0]
            live = live[t["n"][live] > 0]
            mixed += int(live.size > 0 and t["ydom"][live].min() != t["ydom"][live].max())
    assert mixed <= 1, "%d wave-rounds mix the two orientations" % mixed
    assert np.array_equal(tab, deal(t, stride)), "two calls gave different tables"


def test_model_cost_of_the_default_plan(deal):
    import radon_lds_sim as sim
    import radon_order_sim as model
    t = sim.ray_table()
    tab = deal(t, sim.STRIDE)
    waves = [[tab[k, w] for k in range(tab.shape[0]) if (tab[k, w] >= 0).any()] for w in range(tab.shape[1])]
    steps = sum(model.wave_cost(t, r)[0] for wl in waves for r in wl)
    with redirect_stdout(io.StringIO()) as line:
        valu, lds = model.evaluate(t, waves, "dealt by radon_deal.hpp")
    print(line.getvalue().strip())
    print("wave-steps", steps, "LDS cycles", lds, "VALU cycles", valu)
    simd = np.array([sum(model.wave_cost(t, r)[0] for w in range(s, 16, 4) for r in waves[w]) for s in range(4)])
    print("steps per SIMD", simd)
    assert lds <= LDS_CYCLES_MAX and steps <= WAVE_STEPS_MAX
    # dealing longest first to the least loaded wave leaves the waves, and so the SIMDs, within one wave-round (at most max n steps) of each other
    assert simd.max() - simd.min() <= int(t["n"].max()), "the four SIMDs do not carry equal step sums"


def fused_scans():
    """the scans of tests/test_fused_gpu.py::test_fused_equals_two_call_path_and_oracle (an odd batch)"""
    from mr_slam_amd import synth
    spec = importlib.util.spec_from_file_location("_fused_gpu_scans", os.path.join(ROOT, "tests", "test_fused_gpu.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    rng = np.random.default_rng(11)
    return [synth.lidar_scan(3, 20000), mod._adversarial_scan(rng, 4096), synth.uniform_scan(5, 12345),
            synth.lidar_scan(4, 8000), mod._adversarial_scan(rng, 1001)]


def fused_digests(dev="cuda:0"):
    """{variant: {"raw": sha256, "norm": sha256}} of ring_descriptors_fused over fused_scans()"""
    import torch
    from mr_slam_amd import bev, ring
    xyz, offs = bev.pack_scans(fused_scans(), dev)
    plan = ring.ring_plan(0)
    out = {}
    try:
        for variant in (0, 1, 2):
            plan.set_option(plan.OPT_FUSED_VARIANT, variant)
            _, raw, norm = ring.ring_descriptors_fused(xyz, offs)
            torch.cuda.synchronize()
            out[str(variant)] = {"raw": hashlib.sha256(raw.cpu().numpy().tobytes()).hexdigest(),
                                 "norm": hashlib.sha256(norm.cpu().numpy().tobytes()).hexdigest()}
    finally:
        plan.set_option(plan.OPT_FUSED_VARIANT, 2)
    return out


@pytest.mark.gpu
def test_fused_sinograms_bit_identical_to_the_previous_order():
    import torch
    assert torch.cuda.is_available()
    from mr_slam_amd import ring
    slots = ring.ring_plan(0).slot_rays()
    assert slots.size == 15 * WG and np.array_equal(np.sort(slots[slots >= 0]), np.arange(120 * 120))
    want = json.load(open(GOLDEN))["digests"]
    got = fused_digests()
    for variant in ("0", "1", "2"):
        for kind in ("raw", "norm"):
            assert got[variant][kind] == want[variant][kind], "variant %s: %s sinogram differs from the previous order's bits" % (variant, kind)
