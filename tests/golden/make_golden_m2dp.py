"""Generates tests/golden/ref_m2dp.npz by RUNNING THE REFERENCE's own M2DP (RING_ros/pr_methods/M2DP.py, imported by path from the
reference tree; it needs sklearn) in the build container.

The input clouds are stored themselves (float32), not their seeds: the suite shifts every integer-seeded generator by MRS_FUZZ_SEED_OFFSET,
and a fixture keyed on seeds would stop matching its inputs.  The NCLT scan is read from tests/golden/nclt_scan.npz and not stored again.
Per case: the integer counts round(A n), the reference's descriptor as LAPACK returned it, sigma1 and sigma2 of A.

A candidate cloud is rejected (next seed) when the restatement (m2dp_restate.py) finds a (point, plane) pair within 1e-9 maxRho of a bin
edge -- so every stored case is an exact-match case by construction -- or when two consecutive covariance eigenvalues are closer than a
factor of 1.5 (the PCA axes would be ill conditioned).  One exception is structural: three points are coplanar with their centroid, so the
four planes of elevation 0 see the 3-point cloud exactly edge-on (m2dp_restate.EDGE_ON_ROWS) and its 12 pairs there sit ON a theta edge in
exact arithmetic; that case is accepted when every other plane is clear, and the tests compare those four rows by pair count only.
The NCLT scan is given, not drawn: it must be clear of bin edges, and its eigenvalue gap (1.49) is accepted as it is.

Run in the build container (needs the reference tree):  python tests/golden/make_golden_m2dp.py
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import m2dp_restate as R  # noqa: E402
import ref_import  # noqa: E402

GAUSS_SIZES = (3, 64, 1000, 4097)
LIDAR_POINTS = 20000
MAX_BYTES = 512 * 1024


def gaussian_cloud(seed, n):
    """anisotropic Gaussian with an offset mean, turned by a random rotation, float32"""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    scale = np.array([rng.uniform(20, 30), rng.uniform(8, 12), rng.uniform(1.5, 2.0)])
    return ((rng.normal(size=(n, 3)) * scale) @ q.T + rng.uniform(-15, 15, size=3)).astype(np.float32)


def acceptable(cloud, gap=1.5):
    w = R.pca(cloud)[2]
    if any(w[k] < gap * w[k + 1] for k in range(2)):
        return False
    rows = R.m2dp(cloud).uncertain_rows.copy()
    if cloud.shape[0] == 3:
        rows[list(R.EDGE_ON_ROWS)] = 0
    return not rows.any()


def first_acceptable(make, seed0):
    for seed in range(seed0, seed0 + 100):
        c = make(seed)
        if acceptable(c):
            return c, seed
    raise RuntimeError("no acceptable cloud in 100 seeds")


def main():
    from mr_slam_amd import synth
    spec = importlib.util.spec_from_file_location("ref_M2DP", os.path.join(ref_import.RING_ROS, "pr_methods", "M2DP.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    import sklearn

    cases = {}
    for n in GAUSS_SIZES:
        cases["gauss%d" % n], seed = first_acceptable(lambda s: gaussian_cloud(s, n), 1000 + n)
        print("gauss%d: seed %d" % (n, seed))
    cases["lidar"], seed = first_acceptable(lambda s: synth.lidar_scan(s, LIDAR_POINTS), 11)
    print("lidar: seed %d" % seed)
    nclt = np.load(os.path.join(HERE, "nclt_scan.npz"))["hits"]
    # a given scan, not a candidate: its two smaller eigenvalues are a factor 1.49 apart, which the tests' eigenvector demands still tolerate
    assert acceptable(nclt, gap=1.4), "the NCLT scan has a pair on a bin edge"
    cases["nclt"] = nclt

    rec = {"names": np.array(list(cases)), "numpy_version": np.array(np.__version__), "sklearn_version": np.array(sklearn.__version__)}
    for name, cloud in cases.items():
        n = cloud.shape[0]
        desc, A = ref.M2DP(cloud.astype(np.float64))
        counts = np.rint(A * n)
        assert np.abs(A * n - counts).max() < 1e-6 and counts.sum() == 64 * n
        s = np.linalg.svd(A, compute_uv=False)
        if name != "nclt":
            rec["cloud_" + name] = cloud
        rec["counts_" + name] = counts.astype(np.int32)
        rec["desc_" + name] = np.asarray(desc, np.float64)
        rec["sigma_" + name] = s[:2].astype(np.float64)
        print("%-10s n = %6d  sigma1 / (sigma1 - sigma2) = %.3f  sum(u0) = %+.3f" % (name, n, s[0] / (s[0] - s[1]), desc[:64].sum()))
    np.savez_compressed(R.FIXTURE, **rec)
    size = os.path.getsize(R.FIXTURE)
    print("%s: %d bytes" % (R.FIXTURE, size))
    assert size < MAX_BYTES, "shrink LIDAR_POINTS"


if __name__ == "__main__":
    main()
