"""Generates tests/golden/ref_scancontext_geom.npz by RUNNING THE REFERENCE's own Scan Context (RING_ros/pr_methods/ScanContext.py, imported
as pr_methods.ScanContext through tests/golden/ref_import.py) at geometries other than the node's 120 x 120:

  cfg.num_ring / cfg.num_sector are set per geometry (the functions read them at call time);
  search_ratio is passed explicitly (the default argument was bound at import).

Inputs are the seeded pairs of tests/sc_cases.py, rebuilt by the tests; the fixture holds results only: for every pair of the geometries
sc_cases.PINNED the ring and sector keys of both descriptors, the sector-key norm of every shift with fast_align_with_sectorkey's pick,
dist_direct_sc, dist_align_sc at every ratio of sc_cases.ratios(S), and distance_sc, plus the sum of each input (a guard against a
generator and a test that no longer build the same inputs).

Run in the build container (needs the reference tree):  python tests/golden/make_golden_scancontext_geom.py
"""
import importlib
import os
import sys

import numpy as np

os.environ.setdefault("MPLBACKEND", "Agg")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ref_import  # noqa: E402
import sc_cases  # noqa: E402

PATH = os.path.join(HERE, "ref_scancontext_geom.npz")


def tag(geom):
    return "%dx%d" % geom


def main():
    rec = {}
    with ref_import.reference_modules("oracle") as ref:
        ref.util
        sys.path.insert(0, ref_import.RING_ROS)
        try:
            SC = importlib.import_module("pr_methods.ScanContext")
        finally:
            sys.path.remove(ref_import.RING_ROS)
        cfg = SC.cfg
        saved = cfg.num_ring, cfg.num_sector
        try:
            for geom in sc_cases.PINNED:
                cfg.num_ring, cfg.num_sector = geom
                S = geom[1]
                names, a, b = sc_cases.batch(geom)
                rat = sc_cases.ratios(S)
                n = len(names)
                ring, sector = np.zeros((n, 2, geom[0])), np.zeros((n, 2, S))
                norms, sstar = np.zeros((n, S)), np.zeros(n, np.int32)
                direct, align, dsc = np.zeros(n), np.zeros((len(rat), n, 2)), np.zeros((n, 2))
                for p in range(n):
                    sc1, sc2 = np.array(a[p])[None], np.array(b[p])[None]                    # [1, R, S], as the node holds them
                    for side, d in enumerate((sc1, sc2)):
                        ring[p, side] = SC.make_ringkey(d)
                        sector[p, side] = SC.make_sectorkey(d)
                    norms[p] = [np.linalg.norm(sector[p, 0] - np.roll(sector[p, 1], s)) for s in range(S)]
                    _, sstar[p] = SC.fast_align_with_sectorkey(sector[p, 0], sector[p, 1])
                    direct[p] = SC.dist_direct_sc(sc1, sc2)
                    for q, (_, ratio) in enumerate(rat):
                        align[q, p] = SC.dist_align_sc(sc1, sc2, search_ratio=ratio)
                    dsc[p] = SC.distance_sc(sc1, sc2)
                    print(tag(geom), names[p], "align", align[:, p].tolist(), "distance_sc", dsc[p].tolist())
                t = tag(geom)
                rec[t + "/names"] = np.array(names)
                rec[t + "/ratios"] = np.array([r for _, r in rat])
                rec[t + "/input_sums"] = np.stack([a.astype(np.float64).sum((1, 2)), b.astype(np.float64).sum((1, 2))], 1)
                rec[t + "/ringkey"], rec[t + "/sectorkey"] = ring, sector
                rec[t + "/sector_norms"], rec[t + "/sector_shift"] = norms, sstar
                rec[t + "/dist_direct"], rec[t + "/dist_align"], rec[t + "/distance_sc"] = direct, align, dsc
        finally:
            cfg.num_ring, cfg.num_sector = saved
            for k in [k for k in sys.modules if k == "pr_methods" or k.startswith("pr_methods.")]:
                sys.modules.pop(k)
    np.savez_compressed(PATH, **rec)
    print(os.path.getsize(PATH), "bytes")


if __name__ == "__main__":
    main()
