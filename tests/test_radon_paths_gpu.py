"""Every kernel path behind mrs_radon_forward, one geometry each, at a small and a large batch.

mrs_radon_forward (mr_slam_amd/csrc/radon.hip) picks its kernel by image size, ray count and batch size:
  image larger than the LDS                       -> k_radon_pad + k_radon_global (+ k_normalize)
  more than 16 rays per lane                      -> k_radon_big (+ k_normalize)
  batch <= 128                                    -> k_radon_split<125> / <0> (+ k_normalize)
  batch > 128, two images fit the LDS             -> k_radon2<15,125> / <15,0> / <16,0>
  batch > 128, one image fits the LDS, two do not -> k_radon<15,0> / <16,0>
All of them claim the oracle's operation order (raw sinogram) and one reduction order (normalised sinogram), so the same image gives
the same bits whichever kernel, batch slot or output combination computes it.  The rays per lane and row strides in GEOMETRIES are
ceil(A * D / 1024) and (W + 4) | 1; every plan's rays stay inside the 2-texel border (checked when the plan is created).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TWO_PI, HALF = "linspace(0, 2 pi, A)", "linspace(0, pi, A, endpoint=False)"
# name: A, D, H, W, spacing, angles, rays per lane (None: image not in the LDS), the plan has slot tables (two images fit the LDS, <= 16 rays per lane)
GEOMETRIES = {
    "control_120":         (120, 120, 120, 120, 1.0, TWO_PI, 15, True),     # split<125>        | k_radon2<15,125>
    "90x100_on_100x120":   (90, 100, 100, 120, 1.0, TWO_PI, 9, True),       # split<125>        | k_radon2<15,125>
    "100x128_on_100x128":  (100, 128, 100, 128, 1.0, TWO_PI, 13, True),     # split<0>          | k_radon2<15,0>; 204 rays miss the image
    "128x128_on_128x128":  (128, 128, 128, 128, 1.0, TWO_PI, 16, True),     # split<0>          | k_radon2<16,0>
    "30x30_on_30x30":      (30, 30, 30, 30, 1.0, TWO_PI, 1, True),          # split<0>          | k_radon2<15,0>; 900 rays: idle lanes
    "64x100_on_160x160":   (64, 100, 160, 160, 1.0, TWO_PI, 7, False),      # split<0>          | k_radon<15,0>: one image in the LDS, not two
    "64x256_on_160x160":   (64, 256, 160, 160, 1.0, TWO_PI, 16, False),     # split<0>          | k_radon<16,0>; 3404 rays miss the image
    "120x243_on_128x128":  (120, 243, 128, 128, 0.5, TWO_PI, 29, False),    # k_radon_big at both batch sizes
    "64x256_on_256x256":   (64, 256, 256, 256, 1.0, HALF, None, False),     # k_radon_pad + k_radon_global at both batch sizes
}
SMALL, LARGE = 3, 131        # both odd: the last workgroup of the two-image kernels is half empty; 131 > 128 leaves the latency path
ZERO = 2                     # index of the all-zero image among the five

# Geometries whose raw sinogram is asserted to equal the oracle's bit for bit, beyond the tolerance of test_radon_other_geometries.  radon.hip
# claims the oracle's operation order for every path, and on an MI355X all nine geometries gave the oracle's bits at both batch sizes
# (profiles/radon_paths_coverage.md keeps the record).  The test still prints, per geometry and batch, the largest distance in ulp.
BIT_EXACT = set(GEOMETRIES)


def _angles(kind, A):
    return (np.linspace(0, 2 * np.pi, A) if kind == TWO_PI else np.linspace(0, np.pi, A, endpoint=False)).astype(np.float32)


def _images(H, W):
    """the five distinct images: sparse positive (BEV-like), dense signed, all zero, one hot pixel in either far corner"""
    sparse = np.random.default_rng(101).uniform(0, 1, size=(H, W)).astype(np.float32)
    sparse[np.random.default_rng(102).uniform(0, 1, size=(H, W)) > 0.06] = 0.0
    dense = np.random.default_rng(103).standard_normal(size=(H, W)).astype(np.float32)
    first, last = np.zeros((H, W), np.float32), np.zeros((H, W), np.float32)
    first[0, 0] = 1.75
    last[H - 1, W - 1] = 1.75
    return np.stack([sparse, dense, np.zeros((H, W), np.float32), first, last])


def _ulps(a, b):
    """largest distance in units in the last place between two finite float32 arrays"""
    def key(x):
        i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return int(np.abs(key(a) - key(b)).max())


def _bits(x):
    return np.ascontiguousarray(x).view(np.int32)


@pytest.fixture(scope="module", params=list(GEOMETRIES))
def run(request, oracle):
    """one geometry: the five images, the oracle's sinograms of them and, for both batch sizes, what the three output combinations gave"""
    import torch
    assert torch.cuda.is_available()
    from mr_slam_amd import ring
    name = request.param
    A, D, H, W, spacing, kind, per_lane, slots = GEOMETRIES[name]
    ang = _angles(kind, A)
    imgs = _images(H, W)
    assert np.isfinite(imgs).all()
    plan = ring.RadonPlan(D, ang, spacing, H, W)
    out = dict(name=name, imgs=imgs, want=oracle.radon_parallel(imgs, ang, D, spacing), plan=plan, rays=A * D)
    for batch in (SMALL, LARGE):
        idx = np.arange(batch) % 5
        x = torch.from_numpy(imgs[idx]).to("cuda:0").contiguous()
        plan.degenerate_count(reset=True)
        raw, norm = plan.forward(x, raw=True, normalized=True)
        degenerate = plan.degenerate_count(reset=True)
        raw_only, none_n = plan.forward(x, raw=True, normalized=False)
        none_r, norm_only = plan.forward(x, raw=False, normalized=True)
        plan.degenerate_count(reset=True)
        assert none_n is None and none_r is None
        out[batch] = dict(idx=idx, raw=raw.cpu().numpy(), norm=norm.cpu().numpy(), degenerate=degenerate,
                          raw_only=raw_only.cpu().numpy(), norm_only=norm_only.cpu().numpy())
    return out


def test_geometry_keeps_its_dispatch_path(run):
    """what of the dispatch can be seen from outside: rays per lane, and the slot tables that only plans with two images in the LDS have"""
    A, D, H, W, spacing, kind, per_lane, slots = GEOMETRIES[run["name"]]
    stride = (W + 4) | 1
    lds = (H + 4) * stride * 4
    if per_lane is None:
        assert lds > 160 * 1024, "the image fits the LDS: not the global-memory path"
    else:
        assert lds <= 160 * 1024 and per_lane == -(-A * D // 1024)
        assert slots == (2 * lds + 1024 <= 160 * 1024 and per_lane <= 16)
    got = run["plan"].slot_rays()
    assert got.size == (per_lane * 1024 if slots else 0)
    if slots:
        assert np.array_equal(np.sort(got[got >= 0]), np.arange(A * D)) and (got[got < 0] == -1).all()


@pytest.mark.parametrize("batch", [SMALL, LARGE])
def test_raw_sinogram_equals_the_oracle(run, batch):
    r = run[batch]
    first = {int(i): int(np.flatnonzero(r["idx"] == i)[0]) for i in np.unique(r["idx"])}
    got = np.stack([r["raw"][first[i]] for i in sorted(first)])
    want = run["want"][sorted(first)]
    assert np.isfinite(got).all()
    equal = np.array_equal(_bits(got), _bits(want))
    print("%s batch %d: raw sinogram %s the oracle's bits, largest distance %d ulp, largest |difference| %.3g"
          % (run["name"], batch, "equals" if equal else "DIFFERS from", _ulps(got, want), float(np.abs(got - want).max())))
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-6)
    if run["name"] in BIT_EXACT:
        assert equal, "raw sinogram differs from the oracle's bits (largest distance %d ulp)" % _ulps(got, want)


@pytest.mark.parametrize("batch", [SMALL, LARGE])
def test_repeats_of_an_image_give_the_same_bits(run, batch):
    """slot A against slot B of an image pair, every workgroup against every other, and the half-empty last pair"""
    r = run[batch]
    for kind in ("raw", "norm"):
        for b, i in enumerate(r["idx"]):
            f = int(np.flatnonzero(r["idx"] == i)[0])
            assert np.array_equal(_bits(r[kind][b]), _bits(r[kind][f])), \
                "%s sinogram of batch entry %d differs from entry %d (the same image)" % (kind, b, f)


def test_large_batch_kernel_gives_the_small_batch_kernels_bits(run):
    for kind in ("raw", "norm"):
        assert np.array_equal(_bits(run[LARGE][kind][:SMALL]), _bits(run[SMALL][kind])), \
            "%s sinogram: batch %d and batch %d disagree on the same images" % (kind, LARGE, SMALL)


@pytest.mark.parametrize("batch", [SMALL, LARGE])
def test_single_output_calls_give_the_same_bits(run, batch):
    """raw only / normalised only: the branches that trace into a temporary buffer or skip the normalisation"""
    r = run[batch]
    assert np.array_equal(_bits(r["raw_only"]), _bits(r["raw"])), "raw-only call differs from the call with both outputs"
    assert np.array_equal(_bits(r["norm_only"]), _bits(r["norm"])), "normalised-only call differs from the call with both outputs"


@pytest.mark.parametrize("batch", [SMALL, LARGE])
def test_normalised_sinogram_and_degenerate_count(run, batch):
    """(S - mean) / std with the unbiased std, from the GPU's own raw sinogram in float64; a constant sinogram (blank image, or a hot
    pixel no ray meets) is written as zeros and counted.  Constant is decided from the GPU's own raw sinogram, which is what the kernel
    normalises; the oracle's sinogram has to class every image the same way."""
    r = run[batch]
    first = {int(i): int(np.flatnonzero(r["idx"] == i)[0]) for i in np.unique(r["idx"])}       # batch 3 holds only the first three images
    blank = {i: bool(r["raw"][f].min() == r["raw"][f].max()) for i, f in first.items()}
    assert blank == {i: bool(run["want"][i].min() == run["want"][i].max()) for i in first}, "GPU and oracle disagree on which sinograms are constant"
    assert blank[ZERO] and not blank[0] and not blank[1]
    for b, i in enumerate(r["idx"]):
        s = r["raw"][b].astype(np.float64)
        if blank[i]:
            assert not r["norm"][b].any(), "constant sinogram (batch entry %d) not normalised to zeros" % b
            continue
        want = (s - s.mean()) / s.std(ddof=1)
        np.testing.assert_allclose(r["norm"][b], want, rtol=2e-5, atol=2e-6)
    assert not r["raw"][r["idx"] == ZERO].any() and not r["norm"][r["idx"] == ZERO].any()
    assert r["degenerate"] == sum(blank[i] for i in r["idx"]), "degenerate count is not the number of blank images in the batch"


def test_plans_of_one_geometry_own_their_tables():
    """two plans of one small geometry (8 angles x 8 detectors on 8 x 8: slot tables) alive together, one destroyed before the other is
    read again: equal slot tables, every ray dealt once; a geometry with more than 16 rays per lane creates without slot tables"""
    import torch
    assert torch.cuda.is_available()
    from mr_slam_amd import ring
    ang = _angles(TWO_PI, 8)
    a, b = ring.RadonPlan(8, ang, 1.0, 8, 8), ring.RadonPlan(8, ang, 1.0, 8, 8)
    rays_a, rays_b = a.slot_rays(), b.slot_rays()
    assert rays_a.size == 1024 and np.array_equal(rays_a, rays_b)
    assert np.array_equal(np.sort(rays_a[rays_a >= 0]), np.arange(64)) and (rays_a[rays_a < 0] == -1).all()
    del a
    assert np.array_equal(b.slot_rays(), rays_b)
    x = torch.from_numpy(_images(8, 8)).to("cuda:0").contiguous()
    first = b.forward(x)[0].cpu().numpy()
    c = ring.RadonPlan(8, ang, 1.0, 8, 8)
    assert np.array_equal(_bits(c.forward(x)[0].cpu().numpy()), _bits(first))
    big = ring.RadonPlan(130, _angles(TWO_PI, 130), 1.0, 16, 16)            # 16 900 rays: 17 per lane
    assert big.slot_rays().size == 0
