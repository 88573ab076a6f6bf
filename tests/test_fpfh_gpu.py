"""GPU suite for FPFH (fpfh.hip, mr_slam_amd.fpfh and the FPFH / ISS drop-ins) against tests/golden/ref_fpfh.npz, which the reference's own
get_spfh / describe produced, and against the NumPy restatement tests/golden/fpfh_restate.py, which tests/test_fpfh_cpu.py checks
against that fixture.

Radius rows, histogram counts, SPFH and FPFH (whose summation orders are fixed) are compared exactly; FPFH against the reference's recorded
vectors within the forward-error bound of np.dot's unknown order; ISS keypoints exactly on the margin-checked fixture scene."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import fpfh_restate as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _F():
    from mr_slam_amd import fpfh
    return fpfh


@pytest.fixture(scope="module")
def fx():
    return R.load()


def _pack(clouds, stride=3, cols=3):
    """packed device tensor [N, stride] of the clouds' first `cols` columns (columns past them hold something that must not matter) and
    host offsets"""
    offs = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int64)
    pts = np.full((int(offs[-1]), stride), 7.5, np.float32)
    if offs[-1]:
        pts[:, :cols] = np.concatenate([np.asarray(c, np.float32).reshape(-1, cols) for c in clouds if len(c)])
    return torch.from_numpy(pts).to(DEV), torch.from_numpy(offs)


def _rows(clouds, radius, stride=3):
    pts, offs = _pack(clouds, stride)
    rs, idx = _F().radius_neighbors(pts, offs, radius)
    torch.cuda.synchronize()
    assert rs.dtype == torch.int64 and idx.dtype == torch.int32 and rs.numel() == pts.shape[0] + 1
    return rs.cpu().numpy(), idx.cpu().numpy()


def _check_rows(clouds, radius, stride=3):
    rs, idx = _rows(clouds, radius, stride)
    want_rs, want_idx = R.batch_csr(clouds, radius)
    assert np.array_equal(rs, want_rs) and np.array_equal(idx, want_idx)
    return rs, idx


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- radius rows ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 257, 1500])
def test_rows_equal_brute_force(n):
    rng = np.random.default_rng(100 + n)
    cloud = (rng.random((n, 3)) * [1.0, 1.0, 0.5] - 0.25).astype(np.float32)
    radius = 0.12 if n == 1500 else 0.3
    rs, idx = _check_rows([cloud], radius)
    assert rs[-1] == len(idx) and (n < 63 or len(idx) > n)


def test_rows_longer_than_a_wave():
    """every point within r of every other: 200 rows of 199, ascending"""
    rng = np.random.default_rng(7)
    cloud = (rng.random((200, 3)) * 0.05 + 3.0).astype(np.float32)
    rs, idx = _check_rows([cloud], 0.1)
    assert np.array_equal(np.diff(rs), np.full(200, 199))
    assert np.array_equal(idx[:199], np.arange(1, 200))


def test_rows_isolated_coincident_and_hostile_points():
    """empty rows, coincident points (members of each other's rows, a point never of its own), a NaN and an infinite point (nobody's
    neighbours), negative coordinates, and a cloud 2 * 10^5 cells wide: the far cluster lies in the clamped last cell"""
    rng = np.random.default_rng(11)
    near = (rng.random((150, 3)) * 0.004 - 0.002).astype(np.float32)
    far = near[:100] + np.float32(200.0)
    lone = np.array([[50, 0, 0], [-50, 3, 1], [0, 80, -7]], np.float32)
    same = np.tile(np.array([[10.0, -10.0, 10.0]], np.float32), (3, 1))
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0]], np.float32)
    cloud = np.concatenate([near, lone, same, far, bad])
    rs, idx = _check_rows([cloud], 0.001)
    rows = R.from_csr(rs, idx)
    assert [len(rows[i]) for i in (150, 151, 152)] == [0, 0, 0]
    assert [rows[i].tolist() for i in (153, 154, 155)] == [[154, 155], [153, 155], [153, 154]]
    assert len(rows[-1]) == 0 and len(rows[-2]) == 0 and max(len(r) for r in rows[156:256]) > 0


def test_rows_ragged_batch_is_the_clouds_alone_and_repeatable():
    rng = np.random.default_rng(13)
    clouds = [(rng.random((n, 3)) * s).astype(np.float32) for n, s in ((300, 1.0), (0, 1.0), (77, 0.5))]
    rs, idx = _check_rows(clouds, 0.2, stride=4)
    again = _rows(clouds, 0.2, stride=4)
    assert _same_bits(rs, again[0]) and _same_bits(idx, again[1])
    a_rs, a_idx = _rows(clouds[:1], 0.2)
    c_rs, c_idx = _rows(clouds[2:], 0.2, stride=5)
    assert _same_bits(rs[:301], a_rs) and _same_bits(idx[:rs[300]], a_idx)
    assert _same_bits(rs[300:] - rs[300], c_rs) and _same_bits(idx[rs[300]:], c_idx)
    # an empty cloud last and first
    _check_rows([clouds[1], clouds[2], clouds[1]], 0.2)


def test_rows_bad_arguments():
    from mr_slam_amd import _lib
    pts, offs = _pack([np.zeros((4, 3), np.float32)])
    for radius in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(_lib.MrsError) as e:
            _F().radius_neighbors(pts, offs, radius)
        assert e.value.status == 1


# ---- SPFH and FPFH --------------------------------------------------------------------------------------------------------------------
def _spfh_from_lists(F, s, bins, lists=None):
    pts, offs = _pack([s["points"]])
    nrm, _ = _pack([s["normals"]])
    rs, idx = R.to_csr(s["lists"] if lists is None else lists)
    rows = (torch.from_numpy(rs).to(DEV), torch.from_numpy(idx).to(DEV))
    counts, values = F.spfh(pts, nrm, offs, rows, bins, from_neighbors=True)
    return pts, offs, rows, counts, values


def test_spfh_counts_equal_the_reference(fx):
    """through from_neighbors on the reference's own lists (sklearn's order, the point itself included): the counts exactly, and with them
    the values bit for bit (alpha and phi by the operation order, theta because no value lies within 1e-9 of an edge)"""
    scenes, runs = fx
    for r in runs:
        s, B, has = scenes[r["scene"]], r["bins"], r["has"]
        _, _, _, counts, values = _spfh_from_lists(_F(), s, B)
        counts, values = counts.cpu().numpy(), values.cpu().numpy()
        assert counts.dtype == np.int32 and np.array_equal(counts[has], r["counts"][has]), (r["scene"], B)
        assert _same_bits(values[has][:, :2 * B], r["spfh"][has][:, :2 * B]), (r["scene"], B)
        assert _same_bits(values[has], r["spfh"][has]), (r["scene"], B)
        assert not counts[~has].any() and not values[~has].any()


def test_fpfh_against_the_reference_and_the_restatement(fx):
    """the reference's recorded vectors within 4 (m + 3B + 8) 2^-53 per entry, zeros where it has zeros; the restatement bit for bit"""
    scenes, runs = fx
    F = _F()
    for r in runs:
        s, B = scenes[r["scene"]], r["bins"]
        lists = [np.unique(l) for l in s["lists"]]
        pts, offs, rows, _, values = _spfh_from_lists(F, s, B, lists)
        got = F.describe(pts, offs, rows, values, B, torch.from_numpy(s["keypoints"])).cpu().numpy()
        want = R.fpfh(s["points"], lists, values.cpu().numpy(), s["keypoints"])
        assert _same_bits(got, want), (r["scene"], B)
        m = np.array([len(lists[i]) - 1 for i in s["keypoints"]])
        err = np.abs(got - r["fpfh"])
        print("%s B = %d: largest relative error against the reference %.3g, bound %.3g" % (
            r["scene"], B, np.max(err / np.maximum(np.abs(r["fpfh"]), 1e-300)), R.fpfh_tolerance(m, B).min()))
        assert np.array_equal(got == 0, r["fpfh"] == 0), (r["scene"], B)
        assert (err <= R.fpfh_tolerance(m, B)[:, None] * np.abs(r["fpfh"])).all(), (r["scene"], B)


def _clusters():
    """clusters of 201, 66, 65, 64, 2 and 1 points, each within the radius of all of its own and far from the others: rows of 200, 65, 64,
    63, 1 and 0 entries"""
    rng = np.random.default_rng(21)
    parts = [(rng.random((n, 3)) * 0.05 + 2.0 * k).astype(np.float32) for k, n in enumerate((201, 66, 65, 64, 2, 1))]
    pts = np.concatenate(parts)
    nrm = rng.standard_normal(pts.shape)
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    order = rng.permutation(len(pts))
    return pts[order], nrm[order].astype(np.float32)


@pytest.mark.parametrize("bins", [1, 5, 11, 32])
def test_spfh_and_fpfh_on_library_rows_equal_the_restatement(bins):
    F = _F()
    cloud, normals = _clusters()
    other = R.scene(5, perturb=0.1)
    clouds, nrms = [cloud, other[0][:150]], [normals, other[1][:150]]
    pts, offs = _pack(clouds, stride=4)
    nrm, _ = _pack(nrms)
    f, s, counts, (rs, idx) = F.fpfh(pts, nrm, offs, 0.1, bins, return_parts=True)
    torch.cuda.synchronize()
    rs, idx = rs.cpu().numpy(), idx.cpu().numpy()
    assert sorted(set(np.diff(rs[:400]).tolist())) == [0, 1, 63, 64, 65, 200]
    assert f.dtype == torch.float64 and f.shape == (549, 3 * bins)
    for c, (lo, hi) in enumerate(((0, 399), (399, 549))):
        rows = R.from_csr(rs[lo:hi + 1] - rs[lo], idx[rs[lo]:rs[hi]])
        assert all(np.array_equal(a, b) for a, b in zip(rows, R.radius_rows(clouds[c], 0.1)))
        want_counts, want_s = R.spfh(clouds[c], nrms[c], rows, bins)
        assert np.array_equal(counts[lo:hi].cpu().numpy(), want_counts), (bins, c)
        assert _same_bits(s[lo:hi].cpu().numpy(), want_s), (bins, c)
        assert _same_bits(f[lo:hi].cpu().numpy(), R.fpfh(clouds[c], rows, want_s)), (bins, c)
    # keypoints: packed indices, or per-cloud lists of cloud-local ones; the second cloud alone gives the same bits
    kp = [torch.tensor([3, 0, 398]), torch.tensor([149, 7])]
    sub = F.fpfh(pts, nrm, offs, 0.1, bins, keypoints=kp)
    assert _same_bits(sub.cpu().numpy(), f[[3, 0, 398, 399 + 149, 399 + 7]].cpu().numpy())
    assert _same_bits(F.fpfh(pts, nrm, offs, 0.1, bins, keypoints=torch.tensor([402, 3])).cpu().numpy(), f[[402, 3]].cpu().numpy())
    p1, o1 = _pack(clouds[1:])
    n1, _ = _pack(nrms[1:])
    assert _same_bits(F.fpfh(p1, n1, o1, 0.1, bins).cpu().numpy(), f[399:].cpu().numpy())


def test_named_deviations():
    """a neighbour at distance 0 is skipped and not counted in k; a histogram without entries gives zeros; a keypoint without neighbours
    gives zeros; nothing is NaN"""
    F = _F()
    cloud = np.array([[0, 0, 0], [0, 0, 0], [1, 0, 0], [9, 9, 9], [20, 0, 0], [21, 0, 0]], np.float32)
    normals = np.array([[0, 0, 1], [0, 0, 1], [0, 1, 0], [1, 0, 0], [0, 0, 2], [0, 3, 0]], np.float32)
    pts, offs = _pack([cloud])
    nrm, _ = _pack([normals])
    f, s, counts, (rs, idx) = F.fpfh(pts, nrm, offs, 2.0, 5, return_parts=True)
    f, s, counts = f.cpu().numpy(), s.cpu().numpy(), counts.cpu().numpy()
    rows = R.from_csr(rs.cpu().numpy(), idx.cpu().numpy())
    assert [r.tolist() for r in rows] == [[1, 2], [0, 2], [0, 1], [], [5], [4]]
    want_counts, want_s = R.spfh(cloud, normals, rows, 5)
    assert np.array_equal(counts, want_counts) and _same_bits(s, want_s) and _same_bits(f, R.fpfh(cloud, rows, want_s))
    assert np.isfinite(s).all() and np.isfinite(f).all()
    assert counts[0].reshape(3, 5).sum(1).tolist() == [1, 1, 1] and _same_bits(f[0], f[1])      # the coincident twin is not counted
    assert not counts[3].any() and not s[3].any() and not f[3].any()                             # k = 0
    assert counts[4].reshape(3, 5).sum(1).tolist() == [0, 1, 1] and not s[4, :5].any()           # alpha = 6 is dropped: an empty third
    assert s[4, 5:].sum() == 2.0 and abs(np.linalg.norm(f[4]) - 1.0) < 1e-14


def test_from_neighbors_rejects_rows_outside_the_cloud():
    from mr_slam_amd import _lib
    F = _F()
    pts, offs = _pack([np.random.default_rng(3).random((10, 3)).astype(np.float32)])
    nrm, _ = _pack([np.tile(np.array([[0, 0, 1]], np.float32), (10, 1))])
    rs = torch.arange(0, 11, dtype=torch.int64, device=DEV)
    for bad in (10, -1):
        idx = torch.full((10,), bad, dtype=torch.int32, device=DEV)
        with pytest.raises(_lib.MrsError) as e:
            F.spfh(pts, nrm, offs, (rs, idx), 5, from_neighbors=True)
        assert e.value.status == 1
    counts, _ = F.spfh(pts, nrm, offs, (rs, torch.full((10,), 10, dtype=torch.int32, device=DEV)), 5)       # skipped, not read
    assert not counts.cpu().numpy().any()


# ---- ISS ------------------------------------------------------------------------------------------------------------------------------
def test_iss_equals_the_restatement(fx):
    scenes, _ = fx
    cloud = scenes["perturbed"]["points"]
    want_kp, want_sal, margin = R.iss(cloud, R.ISS_SALIENT, R.ISS_NONMAX)
    assert margin >= 1e-6
    junk = np.random.default_rng(2).random((40, 3)).astype(np.float32)
    pts, offs = _pack([junk, cloud], stride=4)
    kp, sal = _F().iss_keypoints(pts, offs, R.ISS_SALIENT, R.ISS_NONMAX)
    assert len(kp) == 2 and kp[1].dtype == torch.int64
    assert np.array_equal(kp[1].cpu().numpy(), want_kp)
    sal = sal.cpu().numpy()[40:]
    assert np.array_equal(sal > 0, want_sal > 0)
    assert (np.abs(sal - want_sal) <= 1e-9 * want_sal).all()
    j_kp, _, j_margin = R.iss(junk, R.ISS_SALIENT, R.ISS_NONMAX)
    assert j_margin < 1e-6 or np.array_equal(kp[0].cpu().numpy(), j_kp)


# a flat, elongated cluster of dyadic coordinates: every sum over 8 of them, their mean and every product of deviations is exact
_CLUSTER = np.array([[1, 0, 0], [2, 0.5, 0.25], [3, 0, 0.25], [4, 0.5, 0], [1.5, 1, 0.125], [2.5, 1, 0.375], [3.5, 0.25, 0.5],
                     [4.5, 0.75, 0.125]]) / 8.0


def test_iss_min_neighbors_boundary():
    """a cluster of 4 (min_neighbors - 1 members each: saliency 0) and one of 5 (exactly min_neighbors: salient); the 5 have one and the
    same member set, hence one saliency, and the lowest index is the keypoint"""
    cloud = np.concatenate([_CLUSTER[:4], _CLUSTER[:5] + [10.0, 0, 0]]).astype(np.float32)
    pts, offs = _pack([cloud])
    kp, sal = _F().iss_keypoints(pts, offs, 1.0, 1.0)
    sal = sal.cpu().numpy()
    want_kp, want_sal, _ = R.iss(cloud, 1.0, 1.0)
    assert want_kp.tolist() == [4] and kp[0].cpu().numpy().tolist() == [4]
    assert not sal[:4].any() and (sal[4:] > 0).all() and len(set(sal[4:].tolist())) == 1
    assert (np.abs(sal - want_sal) <= 1e-9 * want_sal).all()
    kp6, sal6 = _F().iss_keypoints(pts, offs, 1.0, 1.0, min_neighbors=6)
    assert kp6[0].numel() == 0 and not sal6.cpu().numpy().any()
    kp4, sal4 = _F().iss_keypoints(pts, offs, 1.0, 1.0, min_neighbors=4)
    assert kp4[0].cpu().numpy().tolist() == [0, 4] and (sal4.cpu().numpy() > 0).all()


def test_iss_tie_goes_to_the_lower_index():
    """a cluster and its mirror image (even and odd indices), far apart for the salient radius and inside one non-maximum radius: the
    mirrored points have equal saliencies (all arithmetic up to the eigenvalues is exact), and point 0 alone is kept"""
    left = _CLUSTER - [2.0, 0, 0]
    right = left * [-1.0, 1, 1]
    cloud = np.empty((16, 3), np.float32)
    cloud[0::2], cloud[1::2] = left, right
    pts, offs = _pack([cloud])
    kp, sal = _F().iss_keypoints(pts, offs, 0.75, 8.0)
    sal = sal.cpu().numpy()
    assert (sal > 0).all() and len(set(sal.tolist())) == 1
    assert kp[0].cpu().numpy().tolist() == [0]
    kp, _ = _F().iss_keypoints(pts, offs, 0.75, 0.75)           # each cluster for itself: its lowest index
    assert kp[0].cpu().numpy().tolist() == [0, 1]


# ---- drop-in and match ----------------------------------------------------------------------------------------------------------------
def test_dropin_and_match(fx):
    from mr_slam_amd import compat
    scenes, _ = fx
    s = scenes["perturbed"]
    F = _F()
    pts, offs = _pack([s["points"]])
    nrm, _ = _pack([s["normals"]])
    f, sp, _, _ = F.fpfh(pts, nrm, offs, s["radius"], 5, return_parts=True)
    f, sp = f.cpu().numpy(), sp.cpu().numpy()
    mine = ("FPFH", "ISS")
    saved = {k: sys.modules.pop(k) for k in mine if k in sys.modules}
    try:
        compat.install(fpfh=True)
        import FPFH
        import ISS
        FPFH.point_cloud_normals = s["normals"].astype(np.float64)
        cloud = s["points"].astype(np.float64)
        lists = np.empty(len(s["lists"]), object)
        lists[:] = s["lists"]
        for i in s["keypoints"][:4].tolist():
            d = FPFH.describe(cloud, lists, i, s["radius"], 5)
            assert d.dtype == np.float64 and d.shape == (15,) and _same_bits(d, f[i])
            assert _same_bits(FPFH.get_spfh(cloud, lists, i, s["radius"], 5), sp[i])
        state = FPFH._cache[4]
        FPFH.describe(cloud, lists, 0, s["radius"], 5)
        assert FPFH._cache[4] is state                           # one SPFH pass per (cloud, lists, normals, B) identity
        FPFH.get_spfh(cloud, lists, 0, s["radius"], 11)
        assert FPFH._cache[4] is not state
        want_kp, _, _ = R.iss(s["points"], R.ISS_SALIENT, R.ISS_NONMAX)
        got = ISS.iss(cloud, R.ISS_SALIENT, R.ISS_NONMAX)
        assert got.dtype == np.int64 and np.array_equal(got, want_kp)
    finally:
        for k in mine:
            sys.modules.pop(k, None)
        sys.modules.update(saved)
    d = np.unique(f[s["keypoints"]].astype(np.float32), axis=0)
    assert len(d) > 60
    index, dist2 = F.match(torch.from_numpy(d).to(DEV), torch.from_numpy(d).to(DEV), k=2)
    index, dist2 = index.cpu().numpy(), dist2.cpu().numpy()
    assert np.array_equal(index[:, 0], np.arange(len(d))) and not dist2[:, 0].any() and (dist2[:, 1] > 0).all()
