"""The correlation and small-DFT entry points of csrc/ring.hip and csrc/fft2d.hip away from 120 x 120 and one candidate per workgroup:
every test compares with the float64 references of tests/corr_cases.py, the hand-written direct-sum kernels at the tolerance derived there,
the rocFFT-backed values at 4 x the error of the torch fp32 CPU restatement on the same input (and never looser than the earlier tests'
form).  tests/test_corr_cases_cpu.py shows that every planted peak is clear, so angles, shifts and argmaxima are compared exactly.
Each test prints its measured figures before it asserts (pytest -s)."""

import numpy as np
import pytest

import corr_cases as cc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    from mr_slam_amd import _lib
    _lib.load()
    return "cuda:0"


def _up(x, dev):
    import torch
    return torch.from_numpy(np.array(x)).to(dev)


def _within(got, ref, allow, what):
    """|got - ref| <= allow element by element (derived allowance); prints the largest fraction of the allowance used"""
    err = np.abs(np.asarray(got, ref.dtype) - ref)
    print("%s: max |err| / allow = %.3f, max |err| = %.3g" % (what, float((err / allow).max()), float(err.max())))
    assert (err <= allow).all(), (what, float((err / allow).max()))


def _check_sweep(out, q, db, planted, what):
    """all Q*N values of corr, dist and angle of a sweep against the float64 reference"""
    dist, ang, corr = (t.cpu().numpy() for t in out)
    Q, Cc, A, D = q.shape
    ref, allow = cc.ring_corr_ref(q, db)
    assert corr.shape == ref.shape
    _within(corr, ref, allow, what + " corr")
    rang, rdist, adist = cc.peak(ref, 0.15 * Cc * A * D, allow)
    _within(dist, rdist, adist, what + " dist")
    is_planted = np.zeros(ang.shape, bool)
    for i, j, k in planted:
        is_planted[i, j] = True
        assert ang[i, j] == rang[i, j] == (A // 2 if k == A // 2 else -k), (what, i, j, ang[i, j], rang[i, j])
    # elsewhere the peak may be shallow: the returned angle's reference value is the reference maximum to within twice the allowance
    assert (np.abs(ang) <= A // 2).all()
    at = np.take_along_axis(ref, (A // 2 - ang)[..., None].astype(np.int64), -1)[..., 0]
    short = (ref.max(-1) - at) / allow.max(-1)
    print("%s: angle agrees for %d of %d pairs; largest shortfall %.3f allowances" % (what, int((ang == rang).sum()), ang.size, float(short.max())))
    assert (short[~is_planted] <= 2.0).all() and (short[is_planted] == 0).all()


# -------------------------------------------------------------------------------------------------------------------------- k_ring_corr
@pytest.mark.parametrize("name", ["q1", "q5", "c2", "big"])
def test_sweep_with_several_candidates_per_workgroup(dev, name):
    """n_db > number of workgroups: the candidate loop re-zeroes s[] / part[], keeps the query tile for C == 1 (reloads it per channel for
    C == 2), and some workgroups do one candidate more than others (Q = 5: ceil(num_cu / 5) workgroups per query)."""
    import torch
    from mr_slam_amd import ring
    num_cu = torch.cuda.get_device_properties(0).multi_processor_count
    q, db, planted = cc.many_case(name, num_cu)
    tq, tdb = _up(q, dev), _up(db, dev)
    out = ring.corr_sweep(tq, tdb, want_corr=True)
    _check_sweep(out, q, db, planted, "many[%s] N=%d" % (name, db.shape[0]))
    # the pairwise form (one candidate per workgroup) gives the sweep's bits
    for i in range(q.shape[0]):
        dp, ap = ring.corr_pairs(tq[i:i + 1].expand(db.shape[0], -1, -1, -1).contiguous(), tdb)
        assert torch.equal(dp, out[0][i]) and torch.equal(ap, out[1][i]), (name, i)


@pytest.mark.parametrize("shape", cc.SWEEP_SHAPES)
def test_sweep_shapes(dev, shape):
    """D not a multiple of 64 (live mask), D > 128 (column chunks 2, 3), D <= 64 (no second chunk), A > 120 (second pass of shift blocks),
    A < 120 (idle waves), several channels; 120 x 120 as the control.  Q = 3, N = 6, planted rolls 0, 7, -11, A/2."""
    import torch
    from mr_slam_amd import ring
    q, db, planted = cc.sweep_case(shape)
    tq, tdb = _up(q, dev), _up(db, dev)
    out = ring.corr_sweep(tq, tdb, want_corr=True)
    _check_sweep(out, q, db, planted, "sweep%s" % (shape,))
    dp, ap = ring.corr_pairs(tq, tdb[[1, 4, 5]].contiguous())
    assert torch.equal(dp, out[0][[0, 1, 2], [1, 4, 5]]) and torch.equal(ap, out[1][[0, 1, 2], [1, 4, 5]])
    d2, a2 = ring.corr_sweep(tq, tdb)                                   # without the map: same numbers
    assert torch.equal(d2, out[0]) and torch.equal(a2, out[1])


@pytest.mark.parametrize("shape", cc.TIE_SHAPES)
def test_exact_tie_reports_the_first_maximum(dev, shape):
    """A query with period A/2 along the angle axis: s[n] and s[n + A/2] are the same fma chain over the same values, so the map's two
    halves are bitwise equal and the angle is that of the first maximum in shifted order (what torch.argmax returns in the reference)."""
    from mr_slam_amd import ring
    A = shape[1]
    x, y = cc.tie_case(shape)
    dist, ang, corr = (t.cpu().numpy() for t in ring.corr_sweep(_up(x, dev), _up(y, dev), want_corr=True))
    assert np.array_equal(corr[0, 0, :A // 2], corr[0, 0, A // 2:])
    ref, allow = cc.ring_corr_ref(x, y)
    _within(corr, ref, allow, "tie%s corr" % (shape,))
    m = int(np.argmax(ref[0, 0, :A // 2]))                              # the clear peak inside the first half
    assert int(ang[0, 0]) == A // 2 - m and m == int(np.argmax(corr[0, 0]))


def test_rejected_shapes_raise_and_leave_the_context_usable(dev):
    import torch
    from mr_slam_amd import _lib, ring
    q, db, _ = cc.sweep_case((1, 30, 34))
    tq, tdb = _up(q, dev), _up(db, dev)
    good = ring.corr_sweep(tq, tdb)
    _check_sweep(ring.corr_sweep(tq, tdb, want_corr=True), q, db, cc.sweep_case((1, 30, 34))[2], "before the rejections")

    def still_right():
        d, a = ring.corr_sweep(tq, tdb)
        assert torch.equal(d, good[0]) and torch.equal(a, good[1])

    for Cc, A, D in cc.REJECTED:
        z = torch.zeros((2, Cc, A, D), device=dev)
        with pytest.raises(_lib.MrsError):
            ring.corr_sweep(z[:1], z)
        still_right()
        with pytest.raises(_lib.MrsError):
            ring.corr_pairs(z, z)
        still_right()
    L, ctx, st = _lib.load(), _lib.ctx(0), _lib.current_stream(0)
    dist = torch.empty((3, 6), dtype=torch.float32, device=dev)
    ang = torch.empty((3, 6), dtype=torch.int32, device=dev)
    for nq, ndb, ch, A, D in ((0, 6, 1, 30, 34), (3, 0, 1, 30, 34), (3, 6, 0, 30, 34), (3, 6, 1, 0, 34), (3, 6, 1, 30, 0)):     # zero counts
        with pytest.raises(_lib.MrsError):
            L.mrs_ring_corr_sweep(ctx, tq, nq, tdb, ndb, ch, A, D, dist, ang, None, st)
        still_right()
    with pytest.raises(_lib.MrsError):
        L.mrs_ring_corr_pairs(ctx, tq, tdb, 0, 1, 30, 34, dist, ang, None, st)
    still_right()


# ----------------------------------------------------------------------------------------------------------------------------- small DFTs
@pytest.mark.parametrize("shape", cc.DFT_SHAPES)
def test_fft_angle_and_row_fft_shapes(dev, shape):
    """Odd A (Hermitian mirror, twiddle table after an odd-length tile), A = 2, D of every parity, sizes below one wave; batch of 3.  The
    whole complex [A][D] output is compared: row 0, the mirrored rows and row A/2 for even A."""
    from mr_slam_amd import ring
    x = cc.dft_case(shape)
    t = _up(x, dev)
    spec = ring.fft_angle(t).cpu().numpy()
    ref, allow = cc.dft_angle_ref(x)
    assert spec.shape == ref.shape == (3,) + shape
    _within(spec, ref, allow, "fft_angle%s" % (shape,))
    mag = ring.forward_row_fft(t).cpu().numpy()
    ref, allow = cc.dft_row_mag_ref(x)
    _within(mag, ref, allow, "forward_row_fft%s" % (shape,))


@pytest.mark.parametrize("case", cc.SPECTRA_CASES)
def test_corr_spectra_pairs(dev, case):
    """mrs_ring_corr_spectra with n_pairs = 4 on non-Hermitian complex spectra; the denominator has no channel factor."""
    import torch
    from mr_slam_amd import _lib, ring
    Cc, A, D = case
    a, b = cc.spectra_case(case)
    ta, tb = _up(a, dev), _up(b, dev)
    dist = torch.empty(4, dtype=torch.float32, device=dev)
    ang = torch.empty(4, dtype=torch.int32, device=dev)
    corr = torch.empty((4, A), dtype=torch.float32, device=dev)
    _lib.load().mrs_ring_corr_spectra(_lib.ctx(0), ta, tb, 4, Cc, A, D, dist, ang, corr, _lib.current_stream(0))
    ref, allow = cc.corr_spectra_ref(a, b)
    _within(corr.cpu().numpy(), ref, allow, "spectra%s corr" % (case,))
    rang, rdist, adist = cc.peak(ref, 0.15 * A * D, allow)
    _within(dist.cpu().numpy(), rdist, adist, "spectra%s dist" % (case,))
    assert np.array_equal(ang.cpu().numpy(), rang)
    d0, g0, c0 = ring.fast_corr(ta[0], tb[0], device=dev, want_corr=True)              # the drop-in's "full" branch == pair 0
    assert d0 == dist.cpu().numpy()[0] and g0 == rang[0] and np.array_equal(c0, corr[0].cpu().numpy())


def test_ringplusplus_fallback_shape(dev):
    """fast_corr_RINGplusplus away from 120 x 120: joint normalisation, then the sinogram-domain sweep with the channel factor."""
    from mr_slam_amd import ring
    Cc, A, D = cc.RINGPP_SHAPE
    a, b = cc.ringpp_case()
    na, nb = (ring.normalize(_up(v, dev)[None]).cpu().numpy() for v in (a, b))
    for got, raw in ((na, a), (nb, b)):                                               # the normalisation itself, at the earlier test's tolerance
        np.testing.assert_allclose(got[0], cc.normalize(raw), rtol=2e-5, atol=2e-6)
    d, g = ring.fast_corr_RINGplusplus(np.array(a), np.array(b), device=dev)
    ref, allow = cc.ring_corr_ref(na, nb)                                             # the correlation on the kernel's own normalised input
    rang, rdist, adist = cc.peak(ref[0, 0], 0.15 * Cc * A * D, allow[0, 0])
    _within(np.float32(d), rdist, adist, "ringpp dist")
    assert int(g) == rang == 13
    want = cc.peak(cc.ringpp_ref(a, b)[0], 0.15 * Cc * A * D)                         # and end to end
    assert int(g) == want[0] and abs(float(d) - want[1]) < 2e-5


@pytest.mark.parametrize("shape", cc.TRANSLATION_SHAPES)
def test_solve_translation_shapes(dev, shape):
    """W > 128 (third stride of lags), row counts that are no multiple of 16 waves, several channels: every row's shift exactly, the least
    squares against the float64 pseudo-inverse at test_solve_translation's tolerances."""
    from mr_slam_amd import ring
    q, p, planted = cc.translation_case(shape)
    x, y, err, sh = ring.solve_translation(np.array(q), np.array(p), 0.3, device=dev, want_shifts=True, least_squares=True)
    assert np.array_equal(sh, cc.row_shifts_ref(q, p)) and np.array_equal(sh, planted)
    wx, wy, wres = cc.lstsq_ref(sh, 0.3)
    print("solve_translation%s: dx %.2g dy %.2g dres %.2g" % (shape, abs(x[0] - wx), abs(y[0] - wy), abs(err - wres)))
    assert abs(x[0] - wx) < 1e-3 and abs(y[0] - wy) < 1e-3 and abs(err - wres) < 1e-2 * max(wres, 1.0)


# ------------------------------------------------------------------------------------------------------------------------- rocFFT-backed
def _fft_check(got, ref, oracle, what, rtol, atol):
    """relative L2 error of got <= 4 x that of the torch fp32 CPU restatement on the same input (cc.rel_l2: why L2), and element by
    element the earlier tests' form |got - ref| <= atol + rtol |ref|"""
    got, ref, oracle = np.asarray(got), np.asarray(ref), np.asarray(oracle)
    e_gpu, e_cpu = cc.rel_l2(got, ref), cc.rel_l2(oracle, ref)
    m_gpu, m_cpu = float(np.abs(got - ref).max()), float(np.abs(oracle - ref).max())
    print("%s: rel L2 gpu %.3g, torch fp32 %.3g, ratio %.2f (bar 4); max |err| gpu %.3g, torch fp32 %.3g, scale %.3g"
          % (what, e_gpu, e_cpu, e_gpu / e_cpu, m_gpu, m_cpu, float(np.abs(ref).max())))
    assert e_gpu <= 4.0 * e_cpu, (what, e_gpu, e_cpu)
    assert (np.abs(got - ref) <= atol + rtol * np.abs(ref)).all(), what


# Measured on an MI355X (rocFFT against the float64 reference; in brackets the torch fp32 CPU restatement on the same input), relative L2:
#   (H,R,S,col)       spectrum               signature              phase_corr map         largest single error, spectrum / map
#   (1,40,120,16)     1.22e-7 (1.03e-7)      1.03e-7 (6.86e-8)      9.42e-8 (5.61e-8)      1.12e-6 (1.64e-7) / 1.08e-6 (5.36e-7)
#   (3,32,32,16)      8.15e-8 (7.56e-8)      6.64e-8 (6.46e-8)      3.21e-9 (3.21e-9)      2.56e-7 (1.96e-7) / 8.16e-8 (8.16e-8)
#   (2,33,47,8)       1.70e-7 (9.52e-8)      8.86e-8 (5.40e-8)      1.38e-7 (1.33e-7)      3.83e-7 (2.44e-7) / 2.41e-6 (1.67e-6)
#   (1,41,120,16)     1.92e-7 (1.09e-7)      1.35e-7 (7.18e-8)      1.64e-7 (9.33e-8)      6.63e-7 (3.72e-7) / 2.60e-6 (7.63e-7)
#   (5,16,20,4)       7.14e-8 (6.62e-8)      4.18e-8 (3.83e-8)      6.79e-8 (6.44e-8)      3.00e-7 (2.95e-7) / 1.81e-6 (1.42e-6)
# i.e. at most 1.9 x the restatement (bar 4 x).  The largest single error of the (1,40,120,16) spectrum is its DC bin (10.8), 1.7 u of it: the
# two roundings of the ortho scaling, 6.8 x the restatement's largest error -- why the bar is on the L2 norm (corr_cases.rel_l2).
@pytest.mark.parametrize("case", cc.DISCO_CASES)
def test_disco_descriptor_and_phase_corr_shapes(dev, case):
    """Odd R / S (ceil(n/2) shifts), 2 col == R (crop at the edge), R S < 1024 (idle threads of the argmax), lengths rocFFT does not do by
    radix kernels (33, 41, 47); rolls planted along both axes."""
    from mr_slam_amd import disco
    from oracle import corr_oracle as K
    H, R, S, col = case
    bev = cc.disco_case(case)
    sig, spec = disco.disco_from_bev(_up(bev, dev), col)
    rsig, rspec = cc.disco_ref(bev, col)
    wsig, wspec = K.disco_forward(np.array(bev), col)
    assert tuple(sig.shape) == (5, 4 * col * col) and tuple(spec.shape) == (5, 1, R, S)
    scale = np.abs(rspec).max()
    _fft_check(spec.cpu().numpy(), rspec, wspec.numpy(), "disco%s spectrum" % (case,), 0.0, 2e-6 * scale + 1e-5)
    _fft_check(sig.cpu().numpy(), rsig, wsig, "disco%s signature" % (case,), 1e-4, 2e-5 * scale)
    # phase correlation on the reference's spectra (narrowed to complex64): the same input as the CPU margin test
    import torch
    s32 = cc.spectra_of_disco(case)
    ts = _up(s32, dev)
    ta = ts[:1].expand(5, -1, -1, -1).contiguous()
    yaw, corr = disco.phase_corr(ta, ts, num_sector=S, want_corr=True)
    rmap, rarg = cc.phase_corr_ref(np.repeat(s32[:1], 5, 0), s32)
    w = torch.from_numpy(np.array(s32))
    wmap = np.stack([K.phase_corr(w[:1], w[i:i + 1], S)[1][0] for i in range(5)])
    _fft_check(corr.cpu().numpy(), rmap, wmap, "phase_corr%s map" % (case,), 1e-4, 1e-4 * rmap.max())
    raw = corr.reshape(5, -1).argmax(1).cpu().numpy()
    assert np.array_equal(raw, rarg) and np.array_equal(yaw.cpu().numpy(), rarg % S)
    assert np.array_equal(rarg, [((R // 2 - dr) % R) * S + (S // 2 - ds) % S for dr, ds in cc.disco_rolls(R, S)])


@pytest.mark.parametrize("shape", cc.RELORI_SHAPES)
def test_calc_rel_ori_shapes(dev, shape):
    from mr_slam_amd import disco
    s = cc.relori_case(shape)
    a = np.stack([s[0]] * 3)
    got = disco.calc_rel_ori(_up(a, dev), _up(s, dev)).cpu().numpy()
    real, _ = cc.relori_ref(a, s)
    assert np.array_equal(got, cc.relori_angle(real)), (got, cc.relori_angle(real))
    got4 = disco.calc_rel_ori(_up(a[:, None], dev), _up(s[:, None], dev)).cpu().numpy()      # the [P,1,R,S] form
    assert np.array_equal(got4, got)


# Measured on an MI355X, relative L2 of the map (torch fp32 CPU restatement in brackets) and |-max| relative error:
#   (6,120,120) 8.86e-8 (1.51e-7), 8.5e-8    (1,48,80) 1.62e-7 (1.70e-7), 9.4e-8    (2,33,47) 2.05e-7 (1.32e-7), 1.6e-7    (3,16,20) 9.46e-8 (9.98e-8), 5.3e-8
@pytest.mark.parametrize("shape", cc.BEV_TRANSLATION_SHAPES)
def test_solve_translation_bev_shapes(dev, shape):
    """H != W, odd sizes, H W < 1024; planted (dy, dx); num_ring / num_sector passed through."""
    from mr_slam_amd import ring
    from oracle import corr_oracle as K
    Cc, H, W = shape
    a, b = cc.bev_translation_case(shape)
    y, x, neg, corr = ring.solve_translation_bev(_up(a, dev), _up(b, dev), want_corr=True, num_ring=H, num_sector=W)
    corr = corr.cpu().numpy()
    refs = [cc.bev_translation_ref(a[i], b[i], H, W) for i in range(a.shape[0])]
    ws = [K.solve_translation_bev(np.array(a[i]), np.array(b[i]), H, W) for i in range(a.shape[0])]
    rmap = np.stack([r[3] for r in refs])
    _fft_check(corr, rmap, np.stack([w[3] for w in ws]), "bev_translation%s map" % (shape,), 2e-4, 2e-4 * rmap.max())
    for i, (dy, dx) in enumerate(cc.bev_plants()):
        assert (y[i], x[i]) == refs[i][:2] == ((W // 2 - (W // 2 - dx) % W) + (H // 2 - W // 2), (H // 2 - dy) % H - W // 2), (i, y[i], x[i], refs[i][:2])
    # -max is one value of the map, whose accuracy the line above bounds: the earlier test's relative form
    rneg = np.array([r[2] for r in refs])
    print("bev_translation%s -max: max |gpu - ref| / |ref| = %.3g" % (shape, (np.abs(neg - rneg) / np.abs(rneg)).max()))
    assert (np.abs(neg - rneg) <= 2e-4 * np.abs(rneg)).all()
    y1, x1, n1 = ring.solve_translation_bev(_up(a[1], dev), _up(b[1], dev), num_ring=H, num_sector=W)
    assert (y1, x1, n1) == (y[1], x[1], neg[1])


@pytest.mark.parametrize("shape", cc.ROTATE_SHAPES)
def test_rotate_bev_shapes_and_several_angles_per_call(dev, shape):
    """H != W, odd sizes, and three images with three different angles in one call (img / imgs_per_angle picks the angle)."""
    from mr_slam_amd import ring
    from oracle import corr_oracle as K
    Cc, H, W = shape
    img = np.random.default_rng(1100 + H).uniform(size=(3, Cc, H, W)).astype(np.float32)
    got = ring.rotate_bev(_up(img, dev), list(cc.ROTATE_ANGLES)).cpu().numpy()
    for n, ang in enumerate(cc.ROTATE_ANGLES):
        want = K.rotate_nearest(img[n], ang * 180.0 / np.pi).numpy()
        bad = np.argwhere((got[n] != want).any(0))
        for yy, xx in bad:                    # only where the source coordinate sits on a texel boundary to float rounding
            assert cc.texel_distance(H, W, ang, yy, xx) < 2e-4, (shape, ang, yy, xx)
        assert len(bad) < 0.002 * H * W
        assert (got[n] != 0).any() and not np.array_equal(got[n], img[n])
    np.testing.assert_array_equal(ring.rotate_bev(_up(img, dev), [0.0, 0.0, 0.0]).cpu().numpy(), img)
    np.testing.assert_array_equal(ring.rotate_bev(_up(img[0], dev), 0.0).cpu().numpy(), img[0])
