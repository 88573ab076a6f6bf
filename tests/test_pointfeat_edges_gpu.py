"""The RING++ point-feature front-end (mrs_pointfeat_batch -> k_knn_cov + k_feat_from_knn, mrs_pointfeat_from_neighbors) off its nominal
configuration: every k of tests/pointfeat_cases.K_LIST, degenerate clouds (plane, line, lattice, duplicates), clouds smaller than k, a
one-point cloud, a batch whose sizes straddle the kernels' block edges, and point strides 3 / 4 / 6.  Every row and every element is
compared; references and the derived eigenvalue allowance: tests/pointfeat_cases.py."""
import functools

import numpy as np
import pytest

import pointfeat_cases as PC

pytestmark = pytest.mark.gpu

WANT = ("knn", "eigens", "features", "planes")
CASES = PC.cases()
IDS = ["%s-k%d" % c for c in CASES]
CASES_COV = [c for c in CASES if PC.zoo()[c[0]].shape[0] >= 2]        # one point has no covariance: test_one_point_cloud
IDS_COV = ["%s-k%d" % c for c in CASES_COV]


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    from mr_slam_amd import _lib
    _lib.load()
    return "cuda:0"


def _front_end(clouds, k, stride=3):
    """one mrs_pointfeat_batch call over `clouds`: {output: numpy array}, and the offsets"""
    import torch
    from mr_slam_amd import pointfeat
    sizes = [c.shape[0] for c in clouds]
    pts = np.concatenate(clouds).astype(np.float32)
    if stride > 3:
        pts = np.concatenate([pts, np.full((pts.shape[0], stride - 3), 7.5e8, np.float32)], 1)      # whatever rides along must not matter
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    out = pointfeat.point_features(torch.from_numpy(np.ascontiguousarray(pts)).to("cuda:0"), offs, k, want=WANT)
    return {n: v.cpu().numpy() for n, v in out.items()}, offs


@functools.lru_cache(maxsize=None)
def _run(name, k):
    return _front_end([PC.zoo()[name]], k)[0]


def _bits(x):
    return np.ascontiguousarray(x).view(np.int32)


def _same_bits(a, b, what):
    for n in WANT:
        assert np.array_equal(_bits(a[n]), _bits(b[n])), (what, n)


def _cut(out, offs, b):
    """cloud b of a batched result, in the shape a call with that cloud alone returns"""
    lo, hi = int(offs[b]), int(offs[b + 1])
    return {"knn": out["knn"][lo:hi], "eigens": out["eigens"][lo:hi], "features": out["features"][lo:hi], "planes": out["planes"][9 * lo:9 * hi]}


def _d2(oracle, cloud, knn):
    I = np.eye(4)
    return np.stack([oracle.pair_d2(cloud, I, cloud, np.ascontiguousarray(knn[:, j])) for j in range(knn.shape[1])], 1)


@pytest.mark.parametrize("name,k", CASES, ids=IDS)
def test_knn_every_row_exact(dev, oracle, name, k):
    """Every index valid and distinct, self first, slots past min(k, n) at -1; the float32 distances of EVERY row, ascending, are the
    restatement's k smallest (the searches' own operation chain, oracle.pair_d2: index sets may differ only at exact ties, and then the
    distances still agree).  Self first: slot 0 holds a point with the query's own coordinates, and the query itself wherever no other
    point shares them (among exact duplicates the order is by index, like any other tie)."""
    pc = PC.zoo()[name]
    n, kk = pc.shape[0], min(k, pc.shape[0])
    knn = _run(name, k)["knn"]
    assert knn.shape == (n, k) and (knn[:, kk:] == -1).all() and (knn[:, :kk] >= 0).all() and (knn[:, :kk] < n).all()
    s = np.sort(knn[:, :kk], 1)
    assert (np.diff(s, axis=1) > 0).all()                                            # no point twice, in every row
    assert np.array_equal(_bits(pc[knn[:, 0]]), _bits(pc))
    _, first, counts = np.unique(pc, axis=0, return_inverse=True, return_counts=True)
    alone = counts[np.ravel(first)] == 1
    assert np.array_equal(knn[alone, 0], np.arange(n)[alone])
    d = _d2(oracle, pc, knn[:, :kk])
    want = np.sort(_d2(oracle, pc, oracle.knn(pc, kk)), 1)
    assert np.array_equal(d, want)


@pytest.mark.parametrize("name,k", CASES_COV, ids=IDS_COV)
def test_eigenvalues_every_element_within_the_allowance(dev, name, k):
    """float64 reference from the GPU's OWN neighbour indices (no mask of agreeing rows): every one of the 5 x n eigenvalues within one
    float32 rounding plus the fp64 term of tests/pointfeat_cases.py.  Measured on an MI355X: the largest error is 0.997 of the allowance (a
    float32 rounding that comes close to half a unit in the last place), as in the NumPy emulation of the arithmetic."""
    pc = PC.zoo()[name]
    n, kk = pc.shape[0], min(k, pc.shape[0])
    out = _run(name, k)
    share = PC.assert_eigens_within_allowance(pc, out["knn"][:, :kk], out["eigens"], "%s k=%d" % (name, k))
    print("%s k=%d: largest used share of the eigenvalue allowance %.3f" % (name, k, share))
    e = out["eigens"]
    assert (e[:, 0] >= e[:, 1]).all() and (e[:, 1] >= e[:, 2]).all() and (e[:, 3] >= e[:, 4]).all()
    if name == "duplicates":
        assert (e == 0).all()                                                        # zero covariance: exactly zero
    if name == "line":
        assert (e[:, [1, 2, 4]] == 0).all()


@pytest.mark.parametrize("name,k", CASES_COV, ids=IDS_COV)
def test_features_every_element_against_the_restatement(dev, name, k):
    """calculate_features on the GPU's own neighbours and eigenvalues: the class (finite, +inf, -inf, NaN) of every element identical, finite
    ones at rtol 5e-5 / atol 1e-6; the planes are the point and features C, O, E, L2, dZ, vZ, bit for bit."""
    from oracle import pointfeat_oracle as P
    pc = PC.zoo()[name]
    n, kk = pc.shape[0], min(k, pc.shape[0])
    out = _run(name, k)
    want = P.calculate_features(pc, out["knn"][:, :kk], out["eigens"])
    PC.assert_features_match(out["features"], want, "%s k=%d" % (name, k))
    pl = out["planes"].reshape(9, n)
    assert np.array_equal(_bits(pl[:3].T), _bits(pc))
    assert np.array_equal(_bits(pl[3:].T), _bits(out["features"][:, [0, 1, 3, 10, 11, 12]]))
    if name in ("plane", "duplicates", "line"):
        assert not np.isfinite(out["features"][:, [3, 8]]).any()                     # E_ and D_ of a zero eigenvalue


@pytest.mark.parametrize("n", [2, 3, 5, 29])
def test_cloud_smaller_than_k_equals_k_equal_n(dev, n):
    """2 <= n < k: every output is what the same call gives with k = n, bit for bit (the header's contract); knn slots past n stay -1"""
    pc = PC.zoo()["n%d" % n]
    big, own = _run("n%d" % n, PC.K_NOMINAL), _run("n%d" % n, n)
    for name in ("eigens", "features", "planes"):
        assert np.array_equal(_bits(big[name]), _bits(own[name])), name
    assert np.array_equal(big["knn"][:, :n], own["knn"]) and (big["knn"][:, n:] == -1).all()
    assert sorted(own["knn"][0].tolist()) == list(range(n)) and pc.shape[0] == n


def test_one_point_cloud(dev):
    """n = 1 must not fault: its knn row is [0, -1, ...], planes 0-2 hold the point, and it gives the same bits alone as inside a batch"""
    z = PC.zoo()
    alone = _run("n1", PC.K_NOMINAL)
    assert alone["knn"].tolist() == [[0] + [-1] * (PC.K_NOMINAL - 1)]
    assert np.array_equal(_bits(alone["planes"][:3]), _bits(z["n1"][0]))
    out, offs = _front_end([z["n5"], z["n1"], z["n31"]], PC.K_NOMINAL)
    _same_bits(_cut(out, offs, 1), alone, "n1 inside a batch")
    _same_bits(_cut(out, offs, 0), _run("n5", PC.K_NOMINAL), "n5 next to it")
    _same_bits(_cut(out, offs, 2), _run("n31", PC.K_NOMINAL), "n31 next to it")


def test_ragged_block_edge_batch_equals_each_cloud_alone(dev):
    """sizes 63 / 64 / 65 (the 64-point blocks of the neighbour lists), 255 / 257 (a workgroup), 1023 / 1025 (a tile) in one call"""
    clouds = PC.ragged()
    out, offs = _front_end(list(clouds), PC.K_NOMINAL)
    for b, pc in enumerate(clouds):
        _same_bits(_cut(out, offs, b), _front_end([pc], PC.K_NOMINAL)[0], "cloud %d of %d points" % (b, pc.shape[0]))


def test_point_stride_does_not_matter(dev):
    pc = PC.zoo()["lidar_metric"]
    base = _run("lidar_metric", PC.K_NOMINAL)
    for stride in (4, 6):
        _same_bits(_front_end([pc], PC.K_NOMINAL, stride)[0], base, "stride %d" % stride)


@pytest.mark.parametrize("k", [1, 7, 32])
def test_drop_in_extractor_any_k(dev, k):
    """voxelfeat.GPUFeatureExtractor (k_features_from_neighbors) with the caller's neighbours and eigenvalues against the restatement"""
    from mr_slam_amd.compat import voxelfeat
    from oracle import pointfeat_oracle as P
    pc = PC.zoo()["lidar_metric"]
    n = pc.shape[0]
    idx = PC.exact_knn(pc, k)
    eig = PC.eig_ref(pc, PC.exact_knn(pc, PC.K_NOMINAL)).astype(np.float32)
    fe = voxelfeat.GPUFeatureExtractor(pc.flatten(), n, 13, k, idx.flatten().astype(np.int32), eig.flatten())
    got = fe.get_features().reshape(n, 13)
    PC.assert_features_match(got, P.calculate_features(pc, idx, eig), "k=%d" % k, rtol=2e-5)


def test_drop_in_extractor_limits(dev):
    """k = 33 is refused (the kernel's neighbour array has 32 slots); n = 0 returns without touching the output"""
    import torch
    from mr_slam_amd import _lib
    from mr_slam_amd.compat import voxelfeat
    pc = PC.zoo()["n31"]
    with pytest.raises(_lib.MrsError):
        voxelfeat.GPUFeatureExtractor(pc.flatten(), 31, 13, 33, np.zeros(31 * 33, np.int32), np.ones(31 * 5, np.float32)).get_features()
    L = _lib.load()
    pts = torch.zeros(3, device=dev)
    knn = torch.zeros(7, dtype=torch.int32, device=dev)
    eig = torch.ones(5, device=dev)
    feat = torch.full((13,), -3.0, device=dev)
    L.mrs_pointfeat_from_neighbors(_lib.ctx(0), pts, 0, 7, knn, eig, feat, _lib.current_stream(0))
    torch.cuda.synchronize()
    assert (feat.cpu().numpy() == -3.0).all()
