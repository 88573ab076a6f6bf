"""k_ring_spec_corr_pairs loops over pairs (workgroup b: pairs b, b + grid, ...) and requests the next pair's columns while it
computes: launches long enough for several, ragged iterations per workgroup must give the bits of the two-step path
(half_spectrum_f16 + corr_pairs_fft on the gathered rows), with and without pairs that have no database row."""
import pytest

pytestmark = pytest.mark.gpu

N_DB = 64
N_LONG = 3 * 512 + 77          # three full rounds of 2 workgroups x 256 CUs and a ragged fourth
SIZES = (1, 2, 511, 512, 513, N_LONG)


class _Case:
    pass


@pytest.fixture(scope="module")
def case():
    """Inputs and the two-step reference, computed once and only read by the tests."""
    import torch
    assert torch.cuda.is_available()
    from mr_slam_amd import _lib, ring
    _lib.load()
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(9)
    n = N_LONG + N_DB
    imgs = torch.rand((n, 120, 120), device=dev, generator=g) * (torch.rand((n, 120, 120), device=dev, generator=g) < 0.3)
    _, norm = ring.ring_plan(0).forward(imgs, raw=False, normalized=True)
    c = _Case()
    c.dev = dev
    c.norm = norm[:N_LONG].contiguous()
    c.db = ring.half_spectrum(norm[N_LONG:].contiguous())
    c.db16 = torch.view_as_real(c.db).to(torch.float16)
    c.idx = torch.randint(0, N_DB, (N_LONG,), device=dev, generator=g, dtype=torch.int32)   # 1613 picks of 64 rows: repeats
    c.idx[5] = c.idx[4]
    c.rows = c.db[c.idx.long()].contiguous()
    c.spec, c.spec16 = ring.half_spectrum_f16(c.norm)
    c.dist, c.angle = ring.corr_pairs_fft(c.spec, c.rows)
    return c


def _launch_db(c, n, db, idx):
    import torch
    from mr_slam_amd import ring
    slot = torch.zeros((n, 61, 120), dtype=torch.complex64, device=c.dev)
    spec, spec16, d, a = ring.spectrum_corr_pairs_db(c.norm[:n], db, idx[:n].contiguous(), want_f16=True, spec_out=slot)
    assert spec.data_ptr() == slot.data_ptr()
    return spec, spec16, d, a


@pytest.mark.parametrize("n", SIZES)
def test_looped_launch_is_bitwise_the_two_step_path(case, n):
    import torch
    c = case
    spec, spec16, d, a = _launch_db(c, n, c.db, c.idx)
    assert torch.equal(spec, c.spec[:n]) and torch.equal(spec16, c.spec16[:n])
    assert torch.equal(d, c.dist[:n]) and torch.equal(a, c.angle[:n])


# pair 0; 612 = the middle one of workgroup 100's three pairs (100, 612, 1124); 1100 = the pair before workgroup 76's last
# (76, 588, 1100, 1612); 1611 / 1612 = the last two pairs of the ragged fourth round
@pytest.mark.parametrize("bad", [{0: -1, 612: N_DB, N_LONG - 1: -1},
                                 {0: N_DB, 612: -1, 1100: N_DB, N_LONG - 2: -1}])
def test_pairs_without_a_row_are_skipped_and_disturb_no_other_pair(case, bad):
    import torch
    c = case
    clean = _launch_db(c, N_LONG, c.db, c.idx)
    idx = c.idx.clone()
    for pair, row in bad.items():
        idx[pair] = row
    spec, spec16, d, a = _launch_db(c, N_LONG, c.db, idx)
    ok = torch.ones(N_LONG, dtype=torch.bool, device=c.dev)
    ok[list(bad)] = False
    assert torch.isinf(d[~ok]).all() and (d[~ok] > 0).all() and (a[~ok] == 0).all()
    assert torch.equal(spec, clean[0]) and torch.equal(spec16, clean[1])          # every spectrum is still written
    assert torch.equal(spec, c.spec) and torch.equal(spec16, c.spec16)
    assert torch.equal(d[ok], clean[2][ok]) and torch.equal(a[ok], clean[3][ok])


def test_fp16_database_long_launch_equals_single_iteration_slices(case):
    import torch
    c = case
    spec, spec16, d, a = _launch_db(c, N_LONG, c.db16, c.idx)
    ds, as_ = [], []
    for lo in range(0, N_LONG, 64):                      # 64 pairs: one iteration per workgroup
        hi = min(lo + 64, N_LONG)
        s1, s16, d1, a1 = _launch_db_slice(c, lo, hi)
        assert torch.equal(s1, spec[lo:hi]) and torch.equal(s16, spec16[lo:hi])
        ds.append(d1)
        as_.append(a1)
    d_slices, a_slices = torch.cat(ds), torch.cat(as_)
    assert torch.equal(d, d_slices) and torch.equal(a, a_slices)
    assert (d_slices - c.dist).abs().max() < 2e-3        # the replica bound of the existing fp16-database test
    assert torch.equal(spec, c.spec) and torch.equal(spec16, c.spec16)


def _launch_db_slice(c, lo, hi):
    from mr_slam_amd import ring
    return ring.spectrum_corr_pairs_db(c.norm[lo:hi], c.db16, c.idx[lo:hi].contiguous(), want_f16=True)


def test_identity_form_long_launch_is_bitwise_the_two_step_path(case):
    import torch
    from mr_slam_amd import ring
    c = case
    spec, spec16, d, a = ring.spectrum_corr_pairs(c.norm, c.rows, want_f16=True)
    assert torch.equal(spec, c.spec) and torch.equal(spec16, c.spec16)
    assert torch.equal(d, c.dist) and torch.equal(a, c.angle)


def test_long_launch_repeats_bit_for_bit(case):
    import torch
    c = case
    first = _launch_db(c, N_LONG, c.db, c.idx)
    second = _launch_db(c, N_LONG, c.db, c.idx)
    for x, y in zip(first, second):
        assert torch.equal(x, y)
