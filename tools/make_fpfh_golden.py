"""Writes tests/golden/ref_fpfh.npz: small seeded clouds and what the REFERENCE's own get_spfh / describe (LoopDetection/src/RING_ros/FPFH.py)
return for them.

FPFH.py cannot be imported (it needs open3d, an ISS module the reference does not ship, and a global that exists only under __main__), so
the two functions are lifted out of the file where it lies with `ast` at run time and given `np` and the `point_cloud_normals` global.  The
`np` they see records the arguments and results of np.histogram, which is how the reference's integer counts and its alpha / phi / theta
values are obtained.  The neighbour lists are sklearn's KDTree(points, 4).query_radius, as in the reference's __main__.  Only data is
stored: points, normals, the lists, keypoint ids and the reference's numbers.

A fixture is accepted only if (the tool tries the next seed otherwise)
  * every alpha, phi and theta lies at least 1e-9 from every bin edge, or exactly on the closed outer edge;
  * no pair of points has |d2 - r2| <= 1e-5 r2, for the FPFH radius and the two ISS radii;
  * every ratio test and every saliency comparison of the ISS restatement has a relative margin of at least 1e-6.

Run on a development machine that has the reference tree:  python tools/make_fpfh_golden.py
Not called by the build, the tests, the smoke run or any benchmark."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import fpfh_restate as R  # noqa: E402
import ref_import  # noqa: E402

FPFH_PY = os.path.join(ref_import.RING_ROS, "FPFH.py")
MAX_BYTES = 512 * 1024
EDGE_MARGIN, RADIUS_MARGIN, ISS_MARGIN = 1e-9, 1e-5, 1e-6


class RecordingNumpy:
    """numpy, with np.histogram's (values, range, counts) kept"""

    def __init__(self):
        self.log = []

    def __getattr__(self, name):
        return getattr(np, name)

    def histogram(self, a, bins=10, range=None, **kw):
        out = np.histogram(a, bins=bins, range=range, **kw)
        self.log.append((np.array(a, np.float64), range, out[0]))
        return out


def reference_run(points, normals, lists, keypoints, radius, bins):
    """-> has [n] (the point has a neighbour), counts int32 [n, 3 bins], spfh [n, 3 bins] (zeros where has is False), fpfh [K, 3 bins], the
    least edge distance of any alpha / phi / theta"""
    rec = RecordingNumpy()
    ns = ref_import.reference_modules.functions_of(FPFH_PY, ("get_spfh", "describe"),
                                                   {"np": rec, "point_cloud_normals": normals.astype(np.float64)})
    P = points.astype(np.float64)
    n = len(P)
    has = np.array([len(set(lists[i].tolist()) - {i}) > 0 for i in range(n)])
    counts, values = np.zeros((n, 3 * bins), np.int32), np.zeros((n, 3 * bins))
    margin = np.inf
    for i in np.nonzero(has)[0]:
        del rec.log[:]
        values[i] = ns["get_spfh"](P, lists, int(i), radius, bins)
        assert len(rec.log) == 3
        counts[i] = np.concatenate([c for _, _, c in rec.log])
        for v, (lo, hi), _ in rec.log:
            margin = min(margin, R.edge_margin(v, lo, hi, bins))
    out = np.stack([ns["describe"](P, lists, int(i), radius, bins) for i in keypoints])
    return has, counts, values, out, margin


def build(seed):
    """-> the fixture's arrays, or a string saying which condition this seed misses"""
    from sklearn.neighbors import KDTree
    rng = np.random.default_rng(seed + 1000)
    rec = {"seed": np.int64(seed), "radius": np.float64(R.RADIUS), "runs": np.array(["%s:%d" % r for r in R.RUNS])}
    scenes = {}
    for name in sorted({s for s, _ in R.RUNS}):
        pts, nrm = R.make_scene(name, seed)
        radius = R.RADIUS if name != "edge" else 0.6
        for r in (radius,) + ((R.ISS_SALIENT, R.ISS_NONMAX) if name == "perturbed" else ()):
            if R.radius_margin(pts, r) <= RADIUS_MARGIN:
                return "scene %s: a pair within %g of radius %g" % (name, RADIUS_MARGIN, r)
        lists = KDTree(pts.astype(np.float64), 4).query_radius(pts.astype(np.float64), radius)
        mine = R.radius_rows(pts, radius)
        for i in range(len(pts)):      # sklearn's lists hold the point itself; otherwise the brute-force rows
            assert sorted(set(lists[i].tolist()) - {i}) == mine[i].tolist(), (name, i)
        with_nb = np.array([i for i in range(len(pts)) if len(mine[i])])
        kp = np.sort(rng.choice(with_nb, min(R.N_KEYPOINTS, len(with_nb)), replace=False)).astype(np.int64)
        scenes[name] = (pts, nrm, lists, kp, radius)
        rs, idx = R.to_csr(lists)
        rec.update({"pts_" + name: pts, "nrm_" + name: nrm, "rs_" + name: rs, "idx_" + name: idx, "kp_" + name: kp,
                    "radius_" + name: np.float64(radius)})
    for k, (name, bins) in enumerate(R.RUNS):
        pts, nrm, lists, kp, radius = scenes[name]
        has, counts, values, out, margin = reference_run(pts, nrm, lists, kp, radius, bins)
        if margin < EDGE_MARGIN:
            return "run %s B = %d: a value %g from a bin edge" % (name, bins, margin)
        assert np.isfinite(values).all() and np.isfinite(out).all(), (name, bins)
        rec.update({"has_%d" % k: has, "counts_%d" % k: counts.astype(np.int16), "spfh_%d" % k: values, "fpfh_%d" % k: out})
        print("seed %d run %-9s B = %2d: least edge distance %.3g" % (seed, name, bins, margin))
    _, _, iss_margin = R.iss(scenes["perturbed"][0], R.ISS_SALIENT, R.ISS_NONMAX)
    if iss_margin < ISS_MARGIN:
        return "ISS: a decision with relative margin %g" % iss_margin
    print("seed %d ISS: least relative margin %.3g" % (seed, iss_margin))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=1, help="the first seed to try")
    ap.add_argument("--tries", type=int, default=50)
    args = ap.parse_args()
    if not os.path.isfile(FPFH_PY):
        raise RuntimeError("reference tree not present: " + FPFH_PY)
    for seed in range(args.seed, args.seed + args.tries):
        rec = build(seed)
        if isinstance(rec, dict):
            break
        print("seed %d rejected: %s" % (seed, rec))
    else:
        raise RuntimeError("no seed in the range gives an acceptable fixture")
    np.savez_compressed(R.FIXTURE, **rec)
    size = os.path.getsize(R.FIXTURE)
    print("%s: %d bytes" % (R.FIXTURE, size))
    assert size < MAX_BYTES


if __name__ == "__main__":
    main()
