"""Generates tests/golden/ref_fasthist.npz by RUNNING THE REFERENCE's own statisticsOnRange (RING_ros/pr_methods/FastHistogram.py, imported
by path from the reference tree; its matplotlib import is satisfied by an empty stand-in when matplotlib is absent) in the build container.

The input clouds are stored themselves (float32), not their seeds: the suite shifts every integer-seeded generator by MRS_FUZZ_SEED_OFFSET,
and a fixture keyed on seeds would stop matching its inputs (make_golden_m2dp.py has the same rule).  The NCLT scan is read from
tests/golden/nclt_scan.npz and not stored again.  Per case: the reference's float64 vector (b = 100) and the integer counts round(vector n).

A candidate cloud is rejected (next seed) when the restatement (fasthist_restate.py) reports unbound > 0: a point in the one-ulp gap above
the last edge makes the reference raise UnboundLocalError, so such a cloud has no reference result.  The cap is 0.  The fixed cases (edges,
grid, zeros, the NCLT scan) are given, not drawn: they must have unbound == 0 as they are.

Run in the build container (needs the reference tree):  python tests/golden/make_golden_fasthist.py
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import fasthist_restate as R  # noqa: E402
import ref_import  # noqa: E402

GAUSS_SIZES = (1, 2, 7, 100, 1000, 4097)
LIDAR_POINTS = 20000
BINS = 100
MAX_BYTES = 512 * 1024


def gaussian_cloud(seed, n):
    """anisotropic Gaussian with an offset mean, turned by a random rotation, float32"""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    scale = np.array([rng.uniform(20, 30), rng.uniform(8, 12), rng.uniform(1.5, 2.0)])
    return ((rng.normal(size=(n, 3)) * scale) @ q.T + rng.uniform(-15, 15, size=3)).astype(np.float32)


def acceptable(cloud):
    return R.range_histogram(cloud, BINS).unbound == 0


def first_acceptable(make, seed0):
    for seed in range(seed0, seed0 + 100):
        c = make(seed)
        if acceptable(c):
            return c, seed
    raise RuntimeError("no acceptable cloud in 100 seeds")


def reference_module():
    try:
        import matplotlib.pyplot  # noqa: F401
    except ImportError:                        # imported by the reference, never called on the path used here
        mpl = types.ModuleType("matplotlib")
        mpl.pyplot = types.ModuleType("matplotlib.pyplot")
        sys.modules.setdefault("matplotlib", mpl)
        sys.modules.setdefault("matplotlib.pyplot", mpl.pyplot)
    spec = importlib.util.spec_from_file_location("ref_FastHistogram", os.path.join(ref_import.RING_ROS, "pr_methods", "FastHistogram.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    return ref


def main():
    from mr_slam_amd import synth
    ref = reference_module()

    cases = {}
    for n in GAUSS_SIZES:
        cases["gauss%d" % n], seed = first_acceptable(lambda s: gaussian_cloud(s, n), 2000 + n)
        print("gauss%d: seed %d" % (n, seed))
    cases["lidar"], seed = first_acceptable(lambda s: synth.lidar_scan(s, LIDAR_POINTS), 11)
    print("lidar: seed %d" % seed)
    cases["nclt"] = np.load(os.path.join(HERE, "nclt_scan.npz"))["hits"]
    z = np.zeros(101, np.float32)
    cases["edges"] = np.stack([np.arange(101, dtype=np.float32), z, z], axis=1)                   # every point sits on an edge
    z = np.zeros(300, np.float32)
    cases["grid"] = np.stack([0.25 * np.arange(300, dtype=np.float32), z, z], axis=1)
    cases["zeros"] = np.zeros((5, 3), np.float32)
    for name in ("nclt", "edges", "grid", "zeros"):
        assert acceptable(cases[name]), "%s has a point above the last edge" % name

    rec = {"names": np.array(list(cases)), "numpy_version": np.array(np.__version__), "bins": np.array(BINS)}
    for name, cloud in cases.items():
        n = cloud.shape[0]
        vec = np.asarray(ref.statisticsOnRange(cloud.astype(np.float64), BINS), np.float64)
        counts = np.rint(vec * n)
        assert np.abs(vec * n - counts).max() < 1e-6 and counts.sum() == n
        if name != "nclt":
            rec["cloud_" + name] = cloud
        rec["hist_" + name] = vec
        rec["counts_" + name] = counts.astype(np.int32)
        r = R.range_histogram(cloud, BINS)
        same = np.array_equal(r.counts, counts) and r.hist.tobytes() == vec.tobytes()
        print("%-10s n = %6d  M = %.17g  restatement %s" % (name, n, r.M, "equal" if same else "DIFFERS"))
    np.savez_compressed(R.FIXTURE, **rec)
    size = os.path.getsize(R.FIXTURE)
    print("%s: %d bytes" % (R.FIXTURE, size))
    assert size < MAX_BYTES, "shrink LIDAR_POINTS"


if __name__ == "__main__":
    main()
