"""GPU parity of the fused descriptor kernel's point streams (csrc/fused.hip: in a round with two scans each half of the workgroup
rasterises one of them; a round with one scan keeps the whole workgroup on it) against the two-call path (cart_bev + plan.forward):
BEV, raw sinogram and normalised sinogram, the same bits.

What the shapes are for.  A scan is read as float4 only if its three planes are 16-byte aligned, i.e. if it starts at a point index that
is a multiple of 4 AND its length is one; everything else takes the per-point loop.  A stage is 1024 quads x PF for a lone scan and
512 x PF per scan of a pair (PF = 1, 2, 3 for prefetch 2, 4, 6), so the lengths below sit on, one quad past and well off the stage sizes
of both groupings; `issue` packs the lengths back to back, which makes most of them start at a point index that is no multiple of 4."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OPTIONS = ("OPT_FUSED_STAGGER_US", "OPT_FUSED_PREFETCH", "OPT_FUSED_GRID", "OPT_FUSED_VARIANT", "OPT_FUSED_SKIP")

LENGTHS = [0, 3, 4, 5, 1023, 4096, 4100, 8199, 12291]

# name -> scan lengths, packed back to back in this order (scans 2k and 2k + 1 share a round)
CASES = {
    "issue": LENGTHS,                                                      # starts 0, 0, 3, 7, 12, 1035, ...: unaligned from the third scan on; odd batch
    "aligned": [4100, 4096, 4, 0, 4096, 4100, 2052, 6000, 12292],          # every scan float4-readable: full stages, ragged ends, both; odd batch
    "short_long": [4, 12292, 12292, 4, 0, 8200, 8200, 0],                  # the halves of a round finish far apart (aligned)
    "short_long_unaligned": [3, 12291, 12291, 5, 1023, 8199, 8199, 1023],
    "stage_edges": [2048, 2052, 6144, 6148, 12288, 12284, 8192, 2044],     # 512 / 1024 / 1536 quads per stage: on it, one quad past, one short
    "batch1": [4100], "batch2": [8199, 4096], "batch3": [4096, 1023, 4100], "batch7": [4100, 4, 12291, 3, 5, 4096, 8199],
}
CASES.update({"single_%d" % n: [n] for n in LENGTHS if n})                # each length alone at point 0 (an empty batch has no points to pass)


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    from mr_slam_amd import _lib
    _lib.load()
    return "cuda:0"


def _scan(rng, n):
    """n points over the grid, an eighth of them on bin edges, an eighth one ulp past one, a few outside the map or on the ground"""
    p = rng.uniform(-1.0, 1.0, size=(n, 3)).astype(np.float32)
    p[:, 2] = rng.uniform(-0.2, 1.0, size=n).astype(np.float32)
    k = n // 8
    j = rng.integers(0, 121, size=k)
    edges = (j / 60.0 - 1.0).astype(np.float32)
    p[:k, 0] = edges
    p[k:2 * k, 1] = np.nextafter(edges, np.float32(2.0))
    if n >= 64:
        p[2 * k:2 * k + 5, 0] = [0.0, 1.0, -1.0, 1.5, -3.0]
        p[2 * k + 5:2 * k + 10, 1] = [0.0, 1.0, -1.0, 1.5, -3.0]
        p[2 * k + 10:2 * k + 14, 2] = [0.0, 1.0, 1.5, 0.9999]
    return p


_cache = {}


def _case(name, dev):
    """the packed scans of a case and the two-call path's (BEV, raw, normalised), computed once"""
    if name not in _cache:
        from mr_slam_amd import bev, ring
        rng = np.random.default_rng(sorted(CASES).index(name) + 100)
        xyz, offs = bev.pack_scans([_scan(rng, n) for n in CASES[name]], dev)
        assert offs.cpu().tolist() == np.concatenate([[0], np.cumsum(CASES[name])]).tolist()
        _cache[name] = (xyz, offs, ring.ring_descriptors(xyz, offs, want_bev=True, fused=False))
    return _cache[name]


def _fused(plan, xyz, offs, **opts):
    from mr_slam_amd import ring
    before = {name: plan.get_option(getattr(plan, name)) for name in OPTIONS}
    try:
        for name, v in opts.items():
            plan.set_option(getattr(plan, name), v)
        return ring.ring_descriptors(xyz, offs, want_bev=True, fused=True)
    finally:
        for name, v in before.items():
            plan.set_option(getattr(plan, name), v)


def _same(want, got, what):
    import torch
    for name, x, y in zip(("BEV", "raw sinogram", "normalised sinogram"), want, got):
        assert x.shape == y.shape
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), "%s: %s differs from the two-call path" % (what, name)


@pytest.mark.parametrize("grid", [1, 2, 65535])      # one / two workgroups run every round (tickets from the global counter); one round per workgroup
@pytest.mark.parametrize("name", sorted(CASES))
def test_streams_equal_two_call_path(dev, name, grid):
    """every FUSED_VARIANT and every prefetch setting on the case's scans"""
    from mr_slam_amd import ring
    xyz, offs, want = _case(name, dev)
    plan = ring.ring_plan(0)
    for variant in (0, 1, 2):
        for prefetch in (2, 4, 6):
            got = _fused(plan, xyz, offs, OPT_FUSED_GRID=grid, OPT_FUSED_VARIANT=variant, OPT_FUSED_PREFETCH=prefetch, OPT_FUSED_STAGGER_US=0)
            _same(want, got, "%s grid %d variant %d prefetch %d" % (name, grid, variant, prefetch))


def test_staggered_start_and_default_grid(dev):
    """the shipped configuration (one workgroup per compute unit, every other one starting late) on more rounds than two workgroups: 9 scans, grid 2"""
    from mr_slam_amd import ring
    plan = ring.ring_plan(0)
    for name in ("issue", "aligned"):
        xyz, offs, want = _case(name, dev)
        _same(want, _fused(plan, xyz, offs), name + " defaults")
        _same(want, _fused(plan, xyz, offs, OPT_FUSED_GRID=2, OPT_FUSED_STAGGER_US=70), name + " grid 2 stagger 70")


@pytest.mark.parametrize("grid", [1, 65535])
@pytest.mark.parametrize("blank_at", [0, 1, 2, 3])
def test_blank_scan_inside_a_pair_counts_as_degenerate(dev, grid, blank_at):
    """a scan with nothing above the ground, as either half of a round: empty image, zero sinograms, one degenerate count, neighbours untouched"""
    import torch
    from mr_slam_amd import bev, ring
    rng = np.random.default_rng(7)
    scans = [_scan(rng, n) for n in (4100, 4096, 6000, 1023)]
    blank = np.zeros((2052, 3), np.float32)
    blank[:, 2] = -0.5
    scans[blank_at] = blank
    xyz, offs = bev.pack_scans(scans, dev)
    plan = ring.ring_plan(0)
    want = ring.ring_descriptors(xyz, offs, want_bev=True, fused=False)
    for variant in (0, 1, 2):
        plan.degenerate_count(reset=True)
        got = _fused(plan, xyz, offs, OPT_FUSED_GRID=grid, OPT_FUSED_VARIANT=variant)
        assert plan.degenerate_count(reset=True) == 1
        _same(want, got, "blank at %d grid %d variant %d" % (blank_at, grid, variant))
        assert float(got[0][blank_at].abs().max()) == 0.0 and float(got[1][blank_at].abs().max()) == 0.0 and float(got[2][blank_at].abs().max()) == 0.0
        assert torch.isfinite(got[2]).all()
    assert {name: plan.get_option(getattr(plan, name)) for name in OPTIONS} == \
        dict(OPT_FUSED_STAGGER_US=70, OPT_FUSED_PREFETCH=2, OPT_FUSED_GRID=0, OPT_FUSED_VARIANT=2, OPT_FUSED_SKIP=0)
