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

    def images(t, stride, tab, nrm, drop=0):
        """slot table of run() -> the padded device images (int4 slots [n, 4], norms [n], rays [n]) of radon_deal::slot_images; drop > 0: hand
        over a table that many entries short and return what the routine answers"""
        import radon_lds_sim as sim
        rays = t["n"].size
        meta = (t["n"] | (t["ydom"].astype(np.int64) << 16)).astype(np.int32)
        base = (4 * np.where(t["ydom"], (t["major"] + sim.PAD) * stride, t["major"] + sim.PAD)).astype(np.int32)
        q, vm = t["q"].astype(np.float32), t["vm"].astype(np.float32)
        per_lane = tab.shape[0]
        flat = np.ascontiguousarray(tab.reshape(-1), dtype=np.int32)
        cap = 32 * WG                                          # guard cells behind the images: the routine must not write past its length
        slot = np.full((cap + 1, 4), -7, dtype=np.int32)
        out_nrm, out_ray = np.full(cap + 1, -7.0, dtype=np.float32), np.full(cap + 1, -7, dtype=np.int32)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        n = lib.slot_images_c(ptr(meta), ptr(base), ptr(q), ptr(vm), ptr(np.ascontiguousarray(nrm, dtype=np.float32)), rays, stride, WG, per_lane,
                              ptr(flat), flat.size - drop, cap, ptr(slot), ptr(out_nrm), ptr(out_ray))
        if drop:
            assert (slot == -7).all() and (out_ray == -7).all(), "a refused table was written out all the same"
            return n
        assert 0 < n <= cap, n
        assert (slot[n:] == -7).all() and (out_nrm[n:] == -7.0).all() and (out_ray[n:] == -7).all()
        return slot[:n], out_nrm[:n], out_ray[:n], (meta, base, q, vm)
    lib.slot_images_c.restype = C.c_int
    run.images = images
    return run


# ring.ring_plan(num_ring, num_sector) builds A = H = num_ring, D = W = num_sector: the grids tests/test_fused_gpu.py runs the fused kernel on,
# and the 64 x 64 image under the default rays whose raw sums do not fit the tile (the fall-back of OPT_FUSED_VARIANT 2)
GEOMETRIES = {"default": dict(A=120, D=120, H=120, W=120), "90x100_on_100x120": dict(A=90, D=100, H=100, W=120),
              "under_1024_rays": dict(A=30, D=30, H=120, W=120),
              "ring100x128": dict(A=100, D=128, H=100, W=128), "ring128x100": dict(A=128, D=100, H=128, W=100),
              "ring128x128": dict(A=128, D=128, H=128, W=128), "ring127x127": dict(A=127, D=127, H=127, W=127),
              "ring30x30": dict(A=30, D=30, H=30, W=30), "default_rays_on_64x64": dict(A=120, D=120, H=64, W=64)}
# lane slots per lane that the fused kernel's instantiation walks: k_bev_radon3<15, ...> for up to 15 rays per lane, <16, ...> for 16
# (mrs_ring_descriptors_batch, fused.hip), whatever ceil(rays / 1024) is
WALKED = {name: (16 if -(-g["A"] * g["D"] // WG) == 16 else 15) for name, g in GEOMETRIES.items()}


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


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_device_slot_tables_cover_every_slot_the_kernel_walks(deal, name):
    """The slot-table kernel reads table entry lane + k * 1024 for EVERY k below its template's rays per lane (15 or 16), also when the plan
    deals fewer rounds (13 for 100 x 128, 1 for 30 x 30): the device images must be that long, the entries behind the dealt ones idle
    (ray -1, norm 0, zero slot: the kernel's `ray >= 0` test skips them), the dealt ones unchanged."""
    import radon_lds_sim as sim
    g = GEOMETRIES[name]
    t = sim.ray_table(**g)
    stride = (g["W"] + 2 * sim.PAD) | 1
    tab = deal(t, stride)
    rays, per_lane = t["n"].size, tab.shape[0]
    assert per_lane == -(-rays // WG) <= 16
    nrm = (1.0 + np.arange(rays) / rays).astype(np.float32)            # any non-zero norms: a pad entry cannot be mistaken for a ray's
    slot, got_nrm, got_ray, (meta, base, q, vm) = deal.images(t, stride, tab, nrm)
    walked = WALKED[name]
    assert walked in (15, 16) and walked >= per_lane
    assert slot.shape == (walked * WG, 4) and got_nrm.shape == (walked * WG,) and got_ray.shape == (walked * WG,), \
        "the kernel walks %d slots per lane, the device tables hold %d" % (walked, got_ray.size // WG)
    dealt = per_lane * WG
    assert np.array_equal(got_ray[:dealt], tab.ravel()), "the dealt part differs from the slot table"
    assert (got_ray[dealt:] == -1).all() and (got_nrm[dealt:] == 0.0).all() and (slot[dealt:] == 0).all(), "a pad entry is not idle"
    live = got_ray >= 0
    assert np.array_equal(np.sort(got_ray[live]), np.arange(rays)), "a ray is missing or dealt twice"
    r = got_ray[live]
    want = np.stack([meta[r], base[r], q[r].view(np.int32), vm[r].view(np.int32)], axis=1)
    assert np.array_equal(slot[live], want) and np.array_equal(got_nrm[live], nrm[r])
    assert (slot[~live] == 0).all() and (got_nrm[~live] == 0.0).all()


def test_slot_table_of_the_wrong_length_is_refused(deal):
    """a table shorter than per_lane * 1024 is an error (no images), not something to pad over"""
    import radon_lds_sim as sim
    g = GEOMETRIES["ring30x30"]
    t = sim.ray_table(**g)
    stride = (g["W"] + 2 * sim.PAD) | 1
    tab = deal(t, stride)
    nrm = np.ones(t["n"].size, dtype=np.float32)
    assert deal.images(t, stride, tab, nrm, drop=1) == 0 and deal.images(t, stride, tab, nrm, drop=WG) == 0


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
    before = plan.get_option(plan.OPT_FUSED_VARIANT)
    try:
        for variant in (0, 1, 2):
            plan.set_option(plan.OPT_FUSED_VARIANT, variant)
            _, raw, norm = ring.ring_descriptors_fused(xyz, offs)
            torch.cuda.synchronize()
            out[str(variant)] = {"raw": hashlib.sha256(raw.cpu().numpy().tobytes()).hexdigest(),
                                 "norm": hashlib.sha256(norm.cpu().numpy().tobytes()).hexdigest()}
    finally:
        plan.set_option(plan.OPT_FUSED_VARIANT, before)
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
