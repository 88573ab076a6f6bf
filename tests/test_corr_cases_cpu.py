"""The float64 references of tests/corr_cases.py checked on the CPU: each agrees with the torch fp32 restatement of oracle/corr_oracle.py to
fp32 FFT accuracy, and every planted case of tests/test_corr_shapes_gpu.py has a peak that leads the runner-up by more than 10 x the allowance
-- the condition under which the GPU tests may compare every angle, shift and argmax exactly."""
import numpy as np
import pytest
import torch

import corr_cases as cc
from oracle import corr_oracle as K

FFT32 = 2e-5      # fp32 FFT accuracy relative to the largest value: three chained length-120 transforms at ~ u log2(N) each, summed over D columns


_w = np.array                               # a writable copy of a shared read-only input, for the restatements


def _t(x):
    return torch.from_numpy(np.array(x))     # a writable copy of a shared read-only input


def _close(got, want, rel=FFT32):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= rel * np.abs(want).max(), (np.abs(got - want).max(), np.abs(want).max())


@pytest.mark.parametrize("shape", [(1, 120, 120), (2, 30, 34), (3, 90, 20)])
def test_ring_references_agree_with_the_restatements(shape):
    C, A, D = shape
    q, db, _ = cc.sweep_case(shape)
    corr, allow = cc.ring_corr_ref(q[:2], db[:3])
    for i in range(2):
        a = torch.fft.fft2(_t(q[i]), dim=-2, norm="ortho")
        _close(a.numpy(), cc.dft_angle_ref(q[i])[0])
        for j in range(3):
            b = torch.fft.fft2(_t(db[j]), dim=-2, norm="ortho")
            wd, wa, wc = K.fast_corr(a, b, A, D)
            _close(wc, corr[i, j])
            sc, sa = cc.corr_spectra_ref(a.numpy()[None], b.numpy()[None])
            _close(wc, sc[0])
            ang, dist = cc.peak(sc[0], 0.15 * A * D)
            assert abs(float(wd) - dist) < FFT32 * max(1.0, abs(dist))
    # pairwise form == the diagonal of the sweep
    pc, pa = cc.ring_corr_ref(q[:2], db[:2], pairwise=True)
    assert np.array_equal(pc[:, 0], corr[[0, 1], [0, 1]]) and np.array_equal(pa[:, 0], allow[[0, 1], [0, 1]])
    # RING++ form: joint normalisation, channel factor in the denominator
    raw_a, raw_b = np.abs(q[0]) + 0.1, np.abs(db[1])
    wd, wa, wc = K.fast_corr_ringplusplus(raw_a, raw_b, A, D)
    rc, _ = cc.ringpp_ref(raw_a, raw_b)
    _close(wc, rc)
    ang, dist = cc.peak(rc, 0.15 * C * A * D)
    assert abs(float(wd) - dist) < FFT32 * max(1.0, abs(dist))
    # |DFT along the detector axis|
    _close(K.forward_row_fft(_w(q[0]))[0].numpy(), cc.dft_row_mag_ref(q[0])[0])


@pytest.mark.parametrize("shape", [(1, 120, 120), (2, 30, 34), (1, 17, 130)])
def test_translation_references_agree_with_the_restatements(shape):
    q, p, sh = cc.translation_case(shape)
    assert np.array_equal(K.row_shifts(_w(q), _w(p)).numpy(), cc.row_shifts_ref(q, p))
    x, y, res = cc.lstsq_ref(sh, 0.3)
    wx, wy, werr, wsh = K.solve_translation(_w(q), _w(p), 0.3, literal=False)
    assert abs(x - wx.item()) < 1e-4 and abs(y - wy.item()) < 1e-4 and abs(res - werr.item()) < 1e-4 * max(res, 1.0)


@pytest.mark.parametrize("shape", [(6, 120, 120), (2, 33, 47), (3, 16, 20)])
def test_bev_translation_and_rotation_references_agree_with_the_restatements(shape):
    C, H, W = shape
    a, b = cc.bev_translation_case(shape)
    for i in range(len(cc.bev_plants())):
        wy, wx, wneg, wmap = K.solve_translation_bev(_w(a[i]), _w(b[i]), H, W)
        y, x, neg, m = cc.bev_translation_ref(a[i], b[i], H, W)
        _close(wmap, m)
        assert (wy, wx) == (y, x) and abs(wneg - neg) < FFT32 * abs(neg)
    img = a[0]
    for ang in cc.ROTATE_ANGLES + (0.0, np.pi / 2):
        got, want = cc.rotate_ref(img, ang), K.rotate_nearest(_w(img), ang * 180.0 / np.pi).numpy()
        bad = np.argwhere((got != want).any(0))
        assert all(cc.texel_distance(H, W, ang, yy, xx) < 2e-4 for yy, xx in bad) and len(bad) < 0.002 * H * W
    assert np.array_equal(cc.rotate_ref(img, 0.0), img)


@pytest.mark.parametrize("case", [(1, 40, 120, 16), (2, 33, 47, 8), (5, 16, 20, 4)])
def test_disco_references_agree_with_the_restatements(case):
    bev = cc.disco_case(case)
    sig, spec = cc.disco_ref(bev, case[3])
    wsig, wspec = K.disco_forward(_w(bev), case[3])
    _close(wsig, sig)
    _close(wspec.numpy(), spec)
    s32 = _t(cc.spectra_of_disco(case))
    m, arg = cc.phase_corr_ref(s32[:1].expand(5, -1, -1, -1).numpy(), s32.numpy())
    for i in range(5):
        wy, wc = K.phase_corr(s32[:1], s32[i:i + 1], case[2])
        _close(wc[0], m[i])
        assert wy == arg[i] % case[2]


# ------------------------------------------------------------------------------------------------------------------------ peak margins
def _assert_margin(v, allow, what):
    lead, al = cc.margin(v, allow)
    assert lead > 10 * al, (what, lead, al)


@pytest.mark.parametrize("shape", cc.SWEEP_SHAPES)
def test_sweep_planted_pairs_have_a_clear_peak(shape):
    C, A, D = shape
    q, db, planted = cc.sweep_case(shape)
    corr, allow = cc.ring_corr_ref(q, db)
    for i, j, k in planted:
        _assert_margin(corr[i, j], allow[i, j], (shape, i, j))
        assert cc.peak(corr[i, j], 1.0)[0] == (A // 2 if k == A // 2 else -k)      # query rolled by +k <=> angle -k


@pytest.mark.parametrize("name", sorted(cc.MANY))
def test_many_candidate_planted_pairs_have_a_clear_peak(name):
    A = cc.MANY[name][1]
    q, db, planted = cc.many_case(name, cc.NOMINAL_CU)
    for i, j, k in planted:
        corr, allow = cc.ring_corr_ref(q[i:i + 1], db[j:j + 1])
        _assert_margin(corr[0, 0], allow[0, 0], (name, i, j))
        assert cc.peak(corr[0, 0], 1.0)[0] == (A // 2 if k == A // 2 else -k)


@pytest.mark.parametrize("shape", cc.TIE_SHAPES)
def test_tie_case_has_a_clear_peak_inside_each_half(shape):
    A = shape[1]
    x, y = cc.tie_case(shape)
    corr, allow = cc.ring_corr_ref(x, y)
    assert np.abs(corr[0, 0, :A // 2] - corr[0, 0, A // 2:]).max() < 1e-9
    _assert_margin(corr[0, 0, :A // 2], allow[0, 0], shape)


@pytest.mark.parametrize("case", cc.SPECTRA_CASES)
def test_spectra_pairs_have_a_clear_peak(case):
    A = case[1]
    a, b = cc.spectra_case(case)
    corr, allow = cc.corr_spectra_ref(a, b)
    for p, k in enumerate(cc.spectra_rolls(A)):
        _assert_margin(corr[p], allow[p], (case, p))
        assert cc.peak(corr[p], 1.0)[0] == (A // 2 if k == A // 2 else -k)


def test_ringpp_pair_has_a_clear_peak():
    corr, allow = cc.ringpp_ref(*cc.ringpp_case())
    _assert_margin(corr, allow, "ringpp")
    assert cc.peak(corr, 1.0)[0] == 13          # the SECOND argument is the rolled one


@pytest.mark.parametrize("shape", cc.TRANSLATION_SHAPES)
def test_every_translation_row_has_a_clear_peak(shape):
    q, p, sh = cc.translation_case(shape)
    corr, allow = cc.row_corr_ref(q, p)
    for i in range(shape[1]):
        _assert_margin(corr[i], allow[i], (shape, i))
    assert np.array_equal(cc.row_shifts_ref(q, p), sh)


@pytest.mark.parametrize("shape", cc.BEV_TRANSLATION_SHAPES)
def test_bev_translation_pairs_have_a_clear_peak(shape):
    C, H, W = shape
    a, b = cc.bev_translation_case(shape)
    for i, (dy, dx) in enumerate(cc.bev_plants()):
        y, x, neg, m = cc.bev_translation_ref(a[i], b[i], H, W)
        _assert_margin(m, cc.fft_allow(m, "bev_translation"), (shape, i))
        # a rolled by (dy, dx) along (H, W): the peak sits at row H/2 - dy, column W/2 - dx of the shifted map
        assert (x, y) == ((H // 2 - dy) % H - W // 2, H // 2 - (W // 2 - dx) % W)


@pytest.mark.parametrize("case", cc.DISCO_CASES)
def test_phase_corr_pairs_have_a_clear_peak(case):
    H, R, S, col = case
    s32 = _t(cc.spectra_of_disco(case))
    m, arg = cc.phase_corr_ref(s32[:1].expand(5, -1, -1, -1).numpy(), s32.numpy())
    for i, (dr, ds) in enumerate(cc.disco_rolls(R, S)):
        _assert_margin(m[i], cc.fft_allow(m[i], "phase_corr"), (case, i))
        assert arg[i] == ((R // 2 - dr) % R) * S + (S // 2 - ds) % S


@pytest.mark.parametrize("shape", cc.RELORI_SHAPES)
def test_relori_pairs_have_a_clear_peak(shape):
    s = cc.relori_case(shape)
    real, allow = cc.relori_ref(np.stack([s[0]] * 3), s)
    for i in range(3):
        _assert_margin(real[i], allow[i], (shape, i))
