"""The kernels of csrc/preprocess.hip on small, edge and hostile inputs (tests/preprocess_cases.py), one test id per case and form.

What is asserted follows from the contract, not from the kernels' output: the single-scan voxel grid does the IEEE operations of
voxel_sequential in its order, so it equals it bit for bit; the batch form is held to batch_bound, derived from the launch code and checked
against the exact reference in tests/test_preprocess_cases_cpu.py; 1e-12 is the accuracy DESIGN.md states at lidar range; the approximate
grid and the crop are bit-exact restatements.  Refusals are error returns: the call raises, and the next call is right."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import preprocess_cases as PC  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    from mr_slam_amd import _lib
    _lib.load()
    return "cuda:0"


def _t(a, dev):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to(dev)       # a copy: the cases are read-only


def _same_bits(got, want, what=""):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    np.testing.assert_array_equal(got.view(u), want.view(u), err_msg=what)


@functools.lru_cache(maxsize=None)
def _exact(name):
    p, v = PC.voxel_cases()[name]
    return PC.voxel_exact(p, v)


def _lex(idx):
    return np.lexsort((idx[:, 2], idx[:, 1], idx[:, 0]))


def _same_voxels(out, p, v, em, ei, bound, what):
    """row j of the batch output lies in voxel ei[j]: the indices recomputed from the output means equal voxel_exact's, row by row.  A
    coordinate whose exact mean is within two bounds of a voxel face may legitimately land on either side and is left to the comparison of
    the means"""
    o = p.min(0) - v * 0.5
    got = np.floor((out - o) / v).astype(np.int64)
    inside = (em - o) - ei * v
    safe = (inside > 2 * bound) & (v - inside > 2 * bound)
    assert safe.any(), what
    wrong = np.flatnonzero(((got != ei) & safe).any(1))
    assert wrong.size == 0, "%s: wrong voxel in rows %s: got %s, want %s" % (what, wrong[:5], got[wrong[:5]].tolist(), ei[wrong[:5]].tolist())


def _batch(scans, v, dev, dtype="float64", stride=3):
    from mr_slam_amd import preprocess
    pts, offs = PC.pack(scans, dtype, stride)
    out, o = preprocess.voxel_down_sample_batch(_t(pts, dev), offs, v)
    return out.cpu().numpy(), o.cpu().numpy()


# ---- exact voxel grid ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(PC.voxel_cases()))
def test_voxel_single_scan(dev, name):
    """bit-equal to the sequential sums, sorted by (ix, iy, iz), and within 1e-12 m of the exactly rounded means at lidar range"""
    from mr_slam_amd import preprocess
    p, v = PC.voxel_cases()[name]
    got = preprocess.voxel_down_sample(_t(p, dev), v).cpu().numpy()
    want, widx = PC.voxel_sequential(p, v)
    assert (_lex(widx) == np.arange(len(widx))).all()                  # what it is compared with IS in (ix, iy, iz) order
    _same_bits(got, want, name)
    em, ei = _exact(name)
    err = float(np.abs(got - em[_lex(ei)]).max())
    print("%s: single-scan form off the exact means by %.3g m" % (name, err))
    if PC.at_lidar_range(p):
        assert err <= PC.ACCURACY


@pytest.mark.parametrize("name", list(PC.voxel_cases()))
def test_voxel_batch_of_one(dev, name):
    """the voxels of voxel_exact, ALL of them in order of first occurrence, means within the derived bound; exact offsets; the same bits twice"""
    p, v = PC.voxel_cases()[name]
    out, o = _batch((p,), v, dev)
    em, ei = _exact(name)
    np.testing.assert_array_equal(o, [0, em.shape[0]])
    assert out.shape == em.shape
    bound = PC.batch_bound(p, v)
    _same_voxels(out, p, v, em, ei, bound, name)                        # the voxel set, and every voxel in its place
    err = float(np.abs(out - em).max())                                 # row by row: the whole output order
    print("%s: batch form off the exact means by %.3g m, bound %.3g m" % (name, err, bound))
    assert err <= bound
    if PC.at_lidar_range(p):
        assert err <= PC.ACCURACY
    out2, o2 = _batch((p,), v, dev)
    _same_bits(out2, out, name)
    np.testing.assert_array_equal(o2, o)


@pytest.mark.parametrize("name", list(PC.voxel_batches()))
def test_voxel_batch(dev, name):
    scans, v = PC.voxel_batches()[name]
    longest = max(s.shape[0] for s in scans)
    out, o = _batch(scans, v, dev)
    both = [PC.voxel_exact(s, v) if s.shape[0] else (np.zeros((0, 3)), np.zeros((0, 3), np.int64)) for s in scans]
    refs = [m for m, _ in both]
    np.testing.assert_array_equal(o, np.concatenate([[0], np.cumsum([r.shape[0] for r in refs])]))
    assert out.shape[0] == o[-1]
    for b, (s, r) in enumerate(zip(scans, refs)):
        got = out[o[b]:o[b + 1]]
        if s.shape[0]:
            bound = PC.batch_bound(s, v, longest)
            _same_voxels(got, s, v, r, both[b][1], bound, "%s scan %d" % (name, b))
            assert np.abs(got - r).max() <= bound < PC.ACCURACY, (name, b)
        alone, oa = _batch((s,), v, dev)                                # the scan as a batch of one: the same bits
        _same_bits(alone, got, "%s scan %d" % (name, b))
        np.testing.assert_array_equal(oa, [0, r.shape[0]])
    out2, o2 = _batch(scans, v, dev)
    _same_bits(out2, out, name)
    np.testing.assert_array_equal(o2, o)


FORM_CLOUDS = ("runs_n257_v0.2", "faces_f32_v0.25", "shifted_f32")


@pytest.mark.parametrize("dtype,stride", [(d, s) for d in ("float32", "float64") for s in PC.STRIDES])
def test_voxel_input_forms(dev, dtype, stride):
    """the same float32 values as float32 or float64, rows of 3, 4 or 7 (NaN past xyz): the same bits as float32 rows of 3"""
    from mr_slam_amd import preprocess
    for name in FORM_CLOUDS:
        p, v = PC.voxel_cases()[name]
        f = PC.forms(p.astype(F32))
        p = f["float64", 3]                                            # the case's float32 values, widened
        offs = np.array([0, p.shape[0]], np.int64)
        base_s = preprocess.voxel_down_sample(_t(f["float32", 3], dev), v).cpu().numpy()
        base_b = preprocess.voxel_down_sample_batch(_t(f["float32", 3], dev), offs, v)[0].cpu().numpy()
        _same_bits(base_s, PC.voxel_sequential(p, v)[0], name)
        _same_bits(preprocess.voxel_down_sample(_t(f[dtype, stride], dev), v).cpu().numpy(), base_s, name)
        _same_bits(preprocess.voxel_down_sample_batch(_t(f[dtype, stride], dev), offs, v)[0].cpu().numpy(), base_b, name)


def _good_call_is_right(dev):
    from mr_slam_amd import preprocess
    p, v = PC.voxel_cases()["runs_n257_v0.2"]
    _same_bits(preprocess.voxel_down_sample(_t(p, dev), v).cpu().numpy(), PC.voxel_sequential(p, v)[0])
    out, o = _batch((p,), v, dev)
    em, _ = _exact("runs_n257_v0.2")
    np.testing.assert_array_equal(o, [0, em.shape[0]])
    assert np.abs(out - em).max() <= PC.batch_bound(p, v)


@pytest.mark.parametrize("form", ["single", "batch", "inside_batch"])
@pytest.mark.parametrize("name", list(PC.refused_cases()))
def test_voxel_refusals(dev, name, form):
    """an extent of 2^21 voxels, a NaN or an infinity: MrsError naming the count of rejected points, and the next call is right"""
    from mr_slam_amd import preprocess
    from mr_slam_amd._lib import MrsError
    p, v, count = PC.refused_cases()[name]
    with pytest.raises(MrsError, match=r"(^|\D)%d points are NaN or more than 2\^21 voxels" % count):
        if form == "single":
            preprocess.voxel_down_sample(_t(p, dev), v)
        elif form == "batch":
            _batch((p,), v, dev)
        else:
            good = PC.pattern_cloud("runs", 65, 0.2)
            _batch((good, np.zeros((0, 3)), p, good), v, dev)
    _good_call_is_right(dev)


# ---- approximate grid ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(PC.avg_cases()))
def test_approximate_grid(dev, oracle, name):
    """device float32, device float64 and pygicp.downsample: the sequential filter's values in its order, bit for bit"""
    from mr_slam_amd import preprocess
    from mr_slam_amd.compat import pygicp
    p, leaf = PC.avg_cases()[name]
    want = oracle.approx_voxel_grid(p, leaf)
    _same_bits(preprocess.approx_voxel_grid(_t(p.astype(F32), dev), leaf).cpu().numpy(), want, name + " float32")
    _same_bits(preprocess.approx_voxel_grid(_t(p, dev), leaf).cpu().numpy(), want, name + " float64")
    _same_bits(pygicp.downsample(p.copy(), leaf), want, name + " pygicp.downsample")


@pytest.mark.parametrize("dtype,stride", [(d, s) for d in ("float32", "float64") for s in PC.STRIDES])
def test_approximate_grid_input_forms(dev, oracle, dtype, stride):
    from mr_slam_amd import preprocess
    for name in ("evicting_n513_l0.2", "negative_n1025_l1", "on_leaf_n511_l0.2"):
        p, leaf = PC.avg_cases()[name]
        f = PC.forms(p.astype(F32))
        assert (f["float64", 3] == p).all()
        _same_bits(preprocess.approx_voxel_grid(_t(f[dtype, stride], dev), leaf).cpu().numpy(), oracle.approx_voxel_grid(p, leaf), name)


# ---- crop / scale ------------------------------------------------------------------------------------------------------------------------

def _crop(scans, dev, dtype, stride=3):
    from mr_slam_amd import preprocess
    pts, offs = PC.pack(scans, dtype, stride)
    xyz, o = preprocess.load_pc_infer_batch(_t(pts, dev), offs)
    return xyz.cpu().numpy(), o.cpu().numpy()


def _check_crop(scans, xyz, o, what):
    refs = [PC.crop_restate(s) if s.shape[0] else np.zeros((0, 3), F32) for s in scans]
    np.testing.assert_array_equal(o, np.concatenate([[0], np.cumsum([r.shape[0] for r in refs])]), err_msg=what)
    assert o.dtype == np.int64
    for b, r in enumerate(refs):
        nb = r.shape[0]
        _same_bits(xyz[3 * o[b]: 3 * o[b] + 3 * nb].reshape(3, nb).T, r, "%s scan %d" % (what, b))


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("name", list(PC.crop_batches()))
def test_crop_scale(dev, name, dtype):
    """SoA output and offsets of every scan equal util.py:91-112 bit for bit: thresholds, rounding casts, signed zero, subnormals, NaN, inf"""
    scans = PC.crop_batches()[name]
    xyz, o = _crop(scans, dev, dtype)
    _check_crop(scans, xyz, o, name)
    if name == "planted":
        assert o[1] == sum(k for _, _, k in PC.crop_plants())             # exactly the plants the contract keeps


@pytest.mark.parametrize("dtype,stride", [(d, s) for d in ("float32", "float64") for s in PC.STRIDES])
def test_crop_scale_input_forms(dev, dtype, stride):
    scans = tuple(s.astype(F32).astype(np.float64) for s in PC.crop_batches()["ends_1"])
    base, bo = _crop(scans, dev, "float32", 3)
    xyz, o = _crop(scans, dev, dtype, stride)
    np.testing.assert_array_equal(o, bo)
    _same_bits(xyz[: 3 * o[-1]], base[: 3 * bo[-1]])
    _check_crop(scans, xyz, o, "ends_1 %s stride %d" % (dtype, stride))


# ---- empty input ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_empty_input(dev, dtype):
    """a ROS callback can hand over an empty cloud: empty results and all-zero offsets, and the next call is right"""
    import torch
    from mr_slam_amd import preprocess
    from mr_slam_amd.compat import pygicp
    e = _t(np.zeros((0, 4), dtype), dev)
    for got in (preprocess.voxel_down_sample(e, 0.2), preprocess.approx_voxel_grid(e, 0.2)):
        assert got.shape == (0, 3) and got.dtype == torch.float64 and got.is_cuda
    assert pygicp.downsample(np.zeros((0, 3)), 0.2).shape == (0, 3)
    offs = np.array(PC.EMPTY_BATCH, np.int64)
    out, o = preprocess.voxel_down_sample_batch(e, offs, 0.2)
    assert out.shape == (0, 3) and out.dtype == torch.float64 and o.dtype == torch.int64 and o.is_cuda
    np.testing.assert_array_equal(o.cpu().numpy(), np.zeros(4, np.int64))
    xyz, o = preprocess.load_pc_infer_batch(e, offs)
    assert xyz.dtype == torch.float32 and xyz.is_cuda and o.dtype == torch.int64 and o.is_cuda
    assert xyz.shape == (3,) and not xyz.any()                          # the documented minimum buffer, zeroed
    np.testing.assert_array_equal(o.cpu().numpy(), np.zeros(4, np.int64))
    _good_call_is_right(dev)
