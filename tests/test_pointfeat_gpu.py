"""GPU parity suite for the RING++ point-feature front-end (row N1) vs the numpy/scipy restatement."""
import numpy as np
import pytest

import pointfeat_cases as PC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    from mr_slam_amd import _lib
    _lib.load()
    return "cuda:0"


def _finite_close(a, b, rtol, atol):
    """the class (finite, +inf, -inf, NaN) of every element identical; the finite ones close"""
    PC.assert_features_match(a, b, rtol=rtol, atol=atol)


def test_feature_extractor_drop_in(dev):
    """voxelfeat.GPUFeatureExtractor with caller-supplied neighbours / eigenvalues (util.py:218-219)."""
    from mr_slam_amd import synth
    from mr_slam_amd.compat import voxelfeat
    from oracle import pointfeat_oracle as P
    pc = synth.lidar_scan(50, 8000)
    idx = P.knn_indices(pc, 30)
    eig = P.covariation_eigenvalue(pc, idx)
    fe = voxelfeat.GPUFeatureExtractor(pc.flatten(), pc.shape[0], 13, 30, idx.flatten().astype(np.int32), eig.flatten())
    got = fe.get_features().reshape(-1, 13)
    want = P.calculate_features(pc, idx, eig)
    _finite_close(got, want, rtol=2e-5, atol=1e-6)


def test_fused_knn_eigen_features(dev, oracle):
    import torch
    from mr_slam_amd import pointfeat, synth
    from oracle import pointfeat_oracle as P
    clouds = [synth.lidar_scan(51, 9000), synth.lidar_scan(52, 5001)]
    pts = torch.from_numpy(np.concatenate(clouds)).to(dev)
    offs = np.array([0, 9000, 14001], np.int64)
    out = pointfeat.point_features(pts, offs, 30, want=("knn", "eigens", "features", "planes"))
    knn, eig, feat = (out[n].cpu().numpy() for n in ("knn", "eigens", "features"))
    planes = out["planes"].cpu().numpy()
    for b, pc in enumerate(clouds):
        lo, hi = offs[b], offs[b + 1]
        n = hi - lo
        got = knn[lo:hi]
        # every row: valid, distinct, self first (the point itself wherever no other point shares its coordinates), and the float32 distances,
        # ascending, are those of the restatement's exact search (oracle.pair_d2: the searches' own operation chain) -- index sets may differ
        # only where the distances tie exactly
        assert (got >= 0).all() and (got < n).all() and (np.diff(np.sort(got, 1), axis=1) > 0).all()
        assert np.array_equal(pc[got[:, 0]], pc)
        _, inv, counts = np.unique(pc, axis=0, return_inverse=True, return_counts=True)
        alone = counts[np.ravel(inv)] == 1
        assert np.array_equal(got[alone, 0], np.arange(n)[alone])
        I = np.eye(4)
        dg = np.stack([oracle.pair_d2(pc, I, pc, np.ascontiguousarray(got[:, j])) for j in range(30)], 1)
        want_idx = oracle.knn(pc, 30)
        dw = np.stack([oracle.pair_d2(pc, I, pc, np.ascontiguousarray(want_idx[:, j])) for j in range(30)], 1)
        assert np.array_equal(dg, np.sort(dw, 1))
        # every eigenvalue against the float64 reference on the GPU's own neighbours, within the derived allowance (tests/pointfeat_cases.py)
        PC.assert_eigens_within_allowance(pc, got, eig[lo:hi], "cloud %d" % b)
        # features from the GPU's own neighbours / eigenvalues == restated formulas on the same inputs
        want = P.calculate_features(pc, knn[lo:hi], eig[lo:hi])
        _finite_close(feat[lo:hi], want, rtol=5e-5, atol=1e-6)
        pl = planes[9 * lo: 9 * hi].reshape(9, hi - lo)
        np.testing.assert_array_equal(pl[:3].T, pc)
        np.testing.assert_array_equal(pl[3:].T, feat[lo:hi][:, [0, 1, 3, 10, 11, 12]])


def test_generate_ringplusplus_end_to_end(dev, oracle):
    """util.py:204-250: front-end -> feature BEV -> Radon (6 channels) -> row-FFT magnitude."""
    from mr_slam_amd import ring, synth
    from oracle import corr_oracle as K
    from oracle import pointfeat_oracle as P
    pc = synth.lidar_scan(53, 12000)
    bev6, sino, tiring = ring.generate_RINGplusplus(pc)
    assert tuple(bev6.shape) == (6, 120, 120) and tuple(sino.shape) == (6, 120, 120)
    # rebuild with the restatements from the GPU's own features (feature parity is tested above)
    from mr_slam_amd import pointfeat
    import torch
    pts = torch.from_numpy(pc).to(dev)
    feat = pointfeat.point_features(pts, np.array([0, pc.shape[0]], np.int64), 30)["features"].cpu().numpy()
    planes = np.concatenate([pc.T, feat[:, [0, 1, 3, 10, 11, 12]].T]).astype(np.float32)
    want_bev = oracle.bev_feat(planes.reshape(-1), 9, 1, 1, 120, 120, 1).reshape(-1, 9)[:, 3:].T.reshape(6, 120, 120)
    np.testing.assert_array_equal(bev6.cpu().numpy(), want_bev)
    ang = np.linspace(0, 2 * np.pi, 120).astype(np.float32)
    want_sino = oracle.radon_parallel(want_bev, ang, 120, 1.0)
    np.testing.assert_allclose(sino.numpy(), want_sino, rtol=1e-6, atol=1e-6)
    want_t, _ = K.forward_row_fft(want_sino)
    np.testing.assert_allclose(tiring.numpy(), want_t.numpy(), rtol=1e-4, atol=1e-4 * want_t.numpy().max())


def test_cached_container_reuse_and_concurrent_callers(dev):
    """mrs_pointfeat_batch keeps its cloud container per context between calls (grow-only buffers) and hands a concurrent caller a temporary
    one: repeated calls with growing / shrinking clouds and two threads at once must return what a fresh call returns, bit for bit."""
    import threading
    import torch
    from mr_slam_amd import pointfeat, synth
    sizes = [3000, 9000, 1200, 9000, 6000]
    clouds = [synth.lidar_scan(60 + i, n) for i, n in enumerate(sizes)]

    def run(pc, stream=None):
        pts = torch.from_numpy(pc).to(dev)
        offs = np.array([0, pc.shape[0]], np.int64)
        if stream is None:
            out = pointfeat.point_features(pts, offs, 30, want=("knn", "features"))
        else:
            with torch.cuda.stream(stream):
                out = pointfeat.point_features(pts, offs, 30, want=("knn", "features"))
            stream.synchronize()
        return out["knn"].cpu().numpy(), out["features"].cpu().numpy()

    first = [run(pc) for pc in clouds]                 # one container (batch of 1), grown and re-used
    again = [run(pc) for pc in reversed(clouds)][::-1]
    for (k0, f0), (k1, f1) in zip(first, again):
        assert np.array_equal(k0, k1) and np.array_equal(f0.view(np.int32), f1.view(np.int32))
    res = [None] * len(clouds)

    def worker(i):
        res[i] = run(clouds[i], torch.cuda.Stream())
    for rep in range(3):
        ths = [threading.Thread(target=worker, args=(i,)) for i in range(len(clouds))]
        [t.start() for t in ths]
        [t.join() for t in ths]
        for (k0, f0), (k1, f1) in zip(first, res):
            assert np.array_equal(k0, k1) and np.array_equal(f0.view(np.int32), f1.view(np.int32))


def test_batched_clouds_in_chunks_equal_one_pass(dev):
    """A batch whose neighbour lists would not fit the scratch limit goes through the selection and the feature tail in chunks of clouds
    (1 GiB by default; the development switch MRS_FEAT_CHUNK_MB makes it small): ragged clouds, 1 / 2 / all clouds per chunk, same bits;
    and every cloud of the batch equals the same cloud processed alone."""
    import os
    import torch
    from mr_slam_amd import pointfeat, synth
    sizes = [5000, 1300, 64, 9000, 2500]
    clouds = [synth.lidar_scan(80 + i, n) for i, n in enumerate(sizes)]
    pts = torch.from_numpy(np.concatenate(clouds)).to(dev)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    want = ("knn", "eigens", "features", "planes")
    ref = {k: v.cpu().numpy() for k, v in pointfeat.point_features(pts, offs, 30, want=want).items()}
    old = {v: os.environ.get(v) for v in ("MRS_DEV", "MRS_FEAT_CHUNK_MB")}
    try:
        os.environ["MRS_DEV"] = "1"
        for mb in ("1", "2"):           # 9000 points x 30 neighbours = 1.1 MB: one cloud per chunk; two small ones together at 2 MB
            os.environ["MRS_FEAT_CHUNK_MB"] = mb
            got = pointfeat.point_features(pts, offs, 30, want=want)
            for k in want:
                assert np.array_equal(ref[k].view(np.int32), got[k].cpu().numpy().view(np.int32)), (mb, k)
    finally:
        for v, x in old.items():
            if x is None:
                os.environ.pop(v, None)
            else:
                os.environ[v] = x
    for i, pc in enumerate(clouds):
        one = pointfeat.point_features(torch.from_numpy(pc).to(dev), np.array([0, sizes[i]], np.int64), 30, want=("knn", "features"))
        assert np.array_equal(one["knn"].cpu().numpy(), ref["knn"][offs[i]:offs[i + 1]]), i
        assert np.array_equal(one["features"].cpu().numpy().view(np.int32), ref["features"][offs[i]:offs[i + 1]].view(np.int32)), i
