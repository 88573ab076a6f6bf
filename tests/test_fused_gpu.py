"""GPU parity of the single-launch descriptor kernel (mrs_ring_descriptors_batch: Cartesian BEV rasterised into the Radon
kernel's LDS tile, sinogram, normalisation) against the two-call path and the oracle: the same bits."""
import contextlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    from mr_slam_amd import _lib
    _lib.load()
    return "cuda:0"


def _adversarial_scan(rng, n, n0=120, n1=120):
    """points on / next to the bin edges of an n0 x n1 grid, zeros, values past +-1, NaN / inf, negative z: everything the slow path exists for"""
    p = rng.uniform(-1.0, 1.0, size=(n, 3)).astype(np.float32)
    p[:, 2] = rng.uniform(-0.2, 1.0, size=n).astype(np.float32)
    k = n // 8
    j = rng.integers(0, n0 + 1, size=k)
    p[:k, 0] = (j / (n0 / 2.0) - 1.0).astype(np.float32)                                # exact bin edges in x
    edges_y = ((j % (n1 + 1)) / (n1 / 2.0) - 1.0).astype(np.float32)
    p[k:2 * k, 1] = np.nextafter(edges_y, np.float32(2.0))                             # one ulp past an edge in y
    p[2 * k:2 * k + 8, 0] = [0.0, 1.0, -1.0, 1.5, -3.0, np.nan, np.inf, -np.inf]
    p[2 * k + 8:2 * k + 16, 1] = [0.0, 1.0, -1.0, 1.5, -3.0, np.nan, np.inf, -np.inf]
    p[2 * k + 16:2 * k + 22, 2] = [0.0, 1.0, 1.5, np.nan, np.inf, 0.9999]
    return p


OPTIONS = ("OPT_FUSED_STAGGER_US", "OPT_FUSED_PREFETCH", "OPT_FUSED_GRID", "OPT_FUSED_VARIANT", "OPT_FUSED_SKIP")
DEFAULTS = dict(OPT_FUSED_STAGGER_US=70, OPT_FUSED_PREFETCH=2, OPT_FUSED_GRID=0, OPT_FUSED_VARIANT=2, OPT_FUSED_SKIP=0)   # include/mrslam_hip.h


def _options_of(plan):
    return {name: plan.get_option(getattr(plan, name)) for name in OPTIONS}


@contextlib.contextmanager
def _options(plan, **values):
    """set plan options (by their OPT_* names) for the block, then put back what the plan HAD, not what it is believed to default to"""
    before = _options_of(plan)
    try:
        for name, v in values.items():
            plan.set_option(getattr(plan, name), v)
        yield plan
    finally:
        for name, v in before.items():
            plan.set_option(getattr(plan, name), v)
        assert _options_of(plan) == before


def _both(xyz, offs, want_bev=True):
    from mr_slam_amd import ring
    a = ring.ring_descriptors(xyz, offs, want_bev=want_bev, fused=False)
    b = ring.ring_descriptors(xyz, offs, want_bev=want_bev, fused=True)
    return a, b


def _same(a, b):
    import torch
    for x, y in zip(a, b):
        assert (x is None) == (y is None)
        if x is not None:
            assert x.shape == y.shape
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), "fused kernel differs from the two-call path"


def test_fused_equals_two_call_path_and_oracle(dev, oracle):
    from mr_slam_amd import bev, synth
    rng = np.random.default_rng(11)
    scans = [synth.lidar_scan(3, 20000), _adversarial_scan(rng, 4096), synth.uniform_scan(5, 12345),    # 12345: planes not 16-byte aligned
             synth.lidar_scan(4, 8000), _adversarial_scan(rng, 1001)]                                    # odd batch: last pair half empty
    xyz, offs = bev.pack_scans(scans, dev)
    a, b = _both(xyz, offs)
    _same(a, b)
    ang = np.linspace(0, 2 * np.pi, 120).astype(np.float32)
    for i, s in enumerate(scans):
        want = oracle.bev_cart(synth.to_soa(s), 1, 1, 120, 120, 1).reshape(-1, 3)[:, 2].reshape(120, 120)
        assert np.array_equal(b[0][i].cpu().numpy(), want), "fused BEV image differs from the oracle"
        # the adversarial scans carry z = +inf (stored as the cell's maximum, like the reference does): inf * 0 weights -> NaN samples
        assert np.array_equal(b[1][i].cpu().numpy(), oracle.radon_parallel(want[None], ang, 120, 1.0)[0], equal_nan=True), \
            "fused sinogram differs from the oracle"


def test_fused_single_scan_and_outputs_optional(dev):
    import torch
    from mr_slam_amd import bev, ring, synth
    xyz, offs = bev.pack_scans([synth.lidar_scan(7, 30000)], dev)
    a, b = _both(xyz, offs)
    _same(a, b)
    _, _, n_only = ring.ring_descriptors_fused(xyz, offs, want_bev=False, raw=False, normalized=True)
    assert torch.equal(n_only, a[2])
    img_only, s_none, n_none = ring.ring_descriptors_fused(xyz, offs, want_bev=True, raw=False, normalized=False)
    assert s_none is None and n_none is None and torch.equal(img_only, a[0])


def test_fused_blank_scan_counts_as_degenerate(dev):
    import torch
    from mr_slam_amd import bev, ring, synth
    blank = np.zeros((500, 3), np.float32)
    blank[:, 2] = -0.5                                          # nothing above the ground: empty image, constant sinogram
    xyz, offs = bev.pack_scans([synth.lidar_scan(1, 5000), blank, synth.lidar_scan(2, 5000)], dev)
    plan = ring.ring_plan(0)
    plan.degenerate_count(reset=True)
    _, sino, norm = ring.ring_descriptors(xyz, offs, fused=True)
    assert plan.degenerate_count(reset=True) == 1
    assert float(sino[1].abs().max()) == 0.0 and float(norm[1].abs().max()) == 0.0
    assert torch.isfinite(norm).all()


@pytest.mark.parametrize("opts", [dict(), dict(stagger=70), dict(prefetch=4), dict(prefetch=6), dict(grid=7), dict(stagger=25, prefetch=4, grid=64),
                                  dict(variant=0), dict(variant=0, prefetch=4, grid=7), dict(variant=1, prefetch=6, grid=3),
                                  dict(variant=1), dict(variant=1, stagger=70), dict(variant=1, prefetch=4), dict(variant=1, prefetch=6),
                                  dict(variant=1, grid=7), dict(variant=1, stagger=25, prefetch=4, grid=64),
                                  dict(variant=2), dict(variant=2, prefetch=6, grid=3)])
def test_fused_persistent_rounds_and_tuning_knobs(dev, opts):
    """more pairs than workgroups (rounds handed out by the global counter), with every tuning knob -- incl. the lane <-> ray dealing
    (variant 2, the default: slot tables, raw sums kept in registers and parked in the tile the next round clears; variant 1: slot tables, raw
    sums parked in the output; variant 0: (angle, detector) order): same bits.  A case without `variant` runs the shipped default."""
    import torch
    from mr_slam_amd import bev, ring, synth
    base = [synth.lidar_scan(20 + s, 6000) for s in range(3)]
    rng = np.random.default_rng(5)
    scans = []
    for i in range(601):                                        # 301 pairs > 256 compute units, ragged sizes
        p = base[i % 3][: 6000 - 7 * (i % 11)].copy()
        th = rng.uniform(0, 2 * np.pi)
        c, s = np.float32(np.cos(th)), np.float32(np.sin(th))
        q = p.copy()
        q[:, 0] = c * p[:, 0] - s * p[:, 1]
        q[:, 1] = s * p[:, 0] + c * p[:, 1]
        scans.append(q)
    xyz, offs = bev.pack_scans(scans, dev)
    plan = ring.ring_plan(0)
    with _options(plan, OPT_FUSED_STAGGER_US=opts.get("stagger", 0), OPT_FUSED_PREFETCH=opts.get("prefetch", 2), OPT_FUSED_GRID=opts.get("grid", 0),
                  OPT_FUSED_VARIANT=opts.get("variant", DEFAULTS["OPT_FUSED_VARIANT"])):
        assert plan.get_option(plan.OPT_FUSED_VARIANT) == opts.get("variant", 2)
        a, b = _both(xyz, offs)
        _same(a, b)
        b2 = ring.ring_descriptors(xyz, offs, want_bev=True, fused=True)        # run to run: the same bits (order-free max, fixed sums)
        _same(b, b2)


def test_fused_rejects_what_it_cannot_do_with_mrs_error(dev):
    import ctypes as C
    import torch
    from mr_slam_amd import _lib, bev, ring, synth
    xyz, offs = bev.pack_scans([synth.lidar_scan(1, 2000)], dev)
    plan = ring.ring_plan(0)
    out = torch.empty((1, 120, 120), dtype=torch.float32, device=dev)
    lib = _lib.load()
    for cfg in (_lib.BevCfg(1, 1, 120, 120, 2, 1), _lib.BevCfg(1, 1, 100, 120, 1, 1)):      # two height layers; grid != the plan's image
        with pytest.raises(_lib.MrsError) as e:
            lib.mrs_ring_descriptors_batch(plan._h, xyz, offs, 1, C.byref(cfg), None, None, out, None)
        assert "unsupported" in str(e.value)
    before = _options_of(plan)
    with pytest.raises(_lib.MrsError):
        plan.set_option(plan.OPT_FUSED_PREFETCH, 3)
    with pytest.raises(_lib.MrsError):
        plan.set_option(99, 1)
    with pytest.raises(_lib.MrsError):
        plan.get_option(99)
    assert _options_of(plan) == before, "a refused option changed the plan"


def test_fresh_plan_reports_the_documented_defaults(dev):
    from mr_slam_amd import ring
    plan = ring.RadonPlan(120, np.linspace(0, 2 * np.pi, 120).astype(np.float32), 1.0, 120, 120)
    assert _options_of(plan) == DEFAULTS
    with _options(plan, OPT_FUSED_STAGGER_US=25, OPT_FUSED_PREFETCH=6, OPT_FUSED_GRID=3, OPT_FUSED_VARIANT=1, OPT_FUSED_SKIP=2):
        assert _options_of(plan) == dict(OPT_FUSED_STAGGER_US=25, OPT_FUSED_PREFETCH=6, OPT_FUSED_GRID=3, OPT_FUSED_VARIANT=1, OPT_FUSED_SKIP=2)
    assert _options_of(plan) == DEFAULTS


GRIDS = [(120, 120), (100, 128), (128, 100), (128, 128), (127, 127), (30, 30)]       # (num_ring, num_sector): 15, 13, 13, 16, 16 and 1 rays per lane
_grid_cache = {}


def _grid_case(n0, n1, dev, oracle):
    """five scans on an n0 x n1 grid (an odd batch: the last pair is half empty), the two-call path's results and the oracle's"""
    if (n0, n1) not in _grid_cache:
        from mr_slam_amd import bev, ring, synth
        rng = np.random.default_rng(11)
        scans = [synth.lidar_scan(3, 20000), _adversarial_scan(rng, 4096, n0, n1), synth.uniform_scan(5, 12345),      # 12345: planes not 16-byte aligned
                 synth.lidar_scan(4, 8000), _adversarial_scan(rng, 1001, n0, n1)]
        xyz, offs = bev.pack_scans(scans, dev)
        two_call = ring.ring_descriptors(xyz, offs, n0, n1, want_bev=True, fused=False)
        ang = np.linspace(0, 2 * np.pi, n0).astype(np.float32)
        want_bev = np.stack([oracle.bev_cart(synth.to_soa(s), 1, 1, n0, n1, 1).reshape(-1, 3)[:, 2].reshape(n0, n1) for s in scans])
        _grid_cache[(n0, n1)] = (xyz, offs, two_call, want_bev, oracle.radon_parallel(want_bev, ang, n1, 1.0))
    return _grid_cache[(n0, n1)]


@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("grid", [0, 2])
@pytest.mark.parametrize("n0,n1", GRIDS)
def test_fused_on_other_grids(dev, oracle, n0, n1, grid, variant):
    """every instantiation of the fused kernel (stride 125 / generic, 15 / 16 rays per lane, the three variants), in one round and -- two
    workgroups for three pairs -- with a second round: the two-call path's bits, the oracle's BEV bits and sinogram"""
    from mr_slam_amd import ring
    xyz, offs, two_call, want_bev, want_sino = _grid_case(n0, n1, dev, oracle)
    plan = ring.ring_plan(0, n0, n1)
    per_lane = -(-n0 * n1 // 1024)
    slots = plan.slot_rays()
    assert slots.size == per_lane * 1024 and np.array_equal(np.sort(slots[slots >= 0]), np.arange(n0 * n1)) and (slots[slots < 0] == -1).all()
    with _options(plan, OPT_FUSED_GRID=grid, OPT_FUSED_VARIANT=variant):
        got = ring.ring_descriptors(xyz, offs, n0, n1, want_bev=True, fused=True)
    _same(two_call, got)
    assert np.array_equal(got[0].cpu().numpy(), want_bev), "fused BEV image differs from the oracle"
    # the adversarial scans carry z = +inf (stored as the cell's maximum, like the reference does): inf * 0 weights -> NaN samples
    np.testing.assert_allclose(got[1].cpu().numpy(), want_sino, rtol=1e-6, atol=1e-6, equal_nan=True)


@pytest.mark.parametrize("variant", [2, 1, 0])
def test_fused_variant_2_falls_back_when_the_raw_sums_do_not_fit_the_tile(dev, variant):
    """120 x 120 rays over a 64 x 64 image: 2 x 14 400 raw sums (115 200 B) exceed the two-image tile (37 536 B), so variant 2 cannot park them
    there and runs the kernel of variant 1; all variants give the bits of mrs_bev_cart_batch + mrs_radon_forward"""
    import ctypes as C
    import torch
    from mr_slam_amd import _lib, bev, ring, synth
    rng = np.random.default_rng(12)
    scans = [synth.lidar_scan(5, 9000), _adversarial_scan(rng, 2048, 64, 64), synth.uniform_scan(6, 4097)]
    xyz, offs = bev.pack_scans(scans, dev)
    plan = ring.RadonPlan(120, np.linspace(0, 2 * np.pi, 120).astype(np.float32), 1.0, 64, 64)
    assert 2 * 120 * 120 * 4 > 2 * (64 + 4) * ((64 + 4) | 1) * 4
    assert _options_of(plan) == DEFAULTS and plan.slot_rays().size == 15 * 1024
    img = bev.cart_bev(xyz, offs, 1, 1, 64, 64, 1, layout=_lib.OUT_COMPACT).view(-1, 64, 64).contiguous()
    want_raw, want_norm = plan.forward(img, raw=True, normalized=True)
    got_img, got_raw, got_norm = (torch.empty_like(t) for t in (img, want_raw, want_norm))
    cfg = _lib.BevCfg(1, 1, 64, 64, 1, 1)
    with _options(plan, OPT_FUSED_VARIANT=variant):
        _lib.load().mrs_ring_descriptors_batch(plan._h, xyz, offs, 3, C.byref(cfg), got_img, got_raw, got_norm, _lib.current_stream(0))
        torch.cuda.synchronize()
    _same((img, want_raw, want_norm), (got_img, got_raw, got_norm))


def test_ring_descriptors_falls_back_only_when_the_choice_was_automatic(dev, monkeypatch):
    """150 x 150 has 22 rays per lane, more than the fused kernel holds: fused=True reports the refusal, the automatic choice takes the
    two-call path"""
    from mr_slam_amd import _lib, bev, ring, synth
    xyz, offs = bev.pack_scans([synth.lidar_scan(8, 7000), synth.uniform_scan(9, 3001), synth.lidar_scan(10, 5000)], dev)
    want = ring.ring_descriptors(xyz, offs, 150, 150, want_bev=True, fused=False)
    with pytest.raises(_lib.MrsError) as e:
        ring.ring_descriptors(xyz, offs, 150, 150, want_bev=True, fused=True)
    assert "unsupported" in str(e.value)
    monkeypatch.setattr(ring, "FUSED_MIN_BATCH", 1)
    _same(want, ring.ring_descriptors(xyz, offs, 150, 150, want_bev=True, fused=None))


def test_shared_plan_is_left_at_the_defaults(dev):
    """runs last in this module: every test above put back the options it changed, so the process-wide plan that the later GPU tests use
    is the configuration that ships"""
    from mr_slam_amd import ring
    assert _options_of(ring.ring_plan(0)) == DEFAULTS
    for n0, n1 in GRIDS:
        assert _options_of(ring.ring_plan(0, n0, n1)) == DEFAULTS
