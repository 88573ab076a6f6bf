"""Generates tests/golden/ref_scancontext.npz by RUNNING THE REFERENCE's own Scan Context in this container:

  RING_ros/pr_methods/ScanContext.py   make_ringkey, make_sectorkey, distance_sc, fast_align_with_sectorkey, dist_direct_sc,
                                       dist_align_sc (imported as pr_methods.ScanContext, with RING_ros/util.py and config.py)
  RING_ros/main_SC.py                  generate_scan_context (function extracted by ast: the module imports rospy); the candidate
                                       step of detect_loop_icp_SC (main_SC.py:159-170) replayed statement by statement

imported through tests/golden/ref_import.py (voxelocc is the oracle stand-in: the reference-built Cartesian rasteriser).

Inputs are deterministic and rebuilt by the tests: clouds A, B, C of make_golden_ref_corr.inputs(), synthetic scans
synth.lidar_scan(seed, 20000) for SYNTH_SEEDS; derived descriptors (rolled + noised, emptied columns, all zero) are stored.

Run in the build container (needs the reference tree):  python tests/golden/make_golden_scancontext.py
"""
import importlib
import os
import sys

import numpy as np

os.environ.setdefault("MPLBACKEND", "Agg")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ref_import  # noqa: E402
import make_golden_ref_corr  # noqa: E402

SYNTH_SEEDS = (11, 12, 13, 14)
ROLLS = (("A", 17, 1), ("A", -40, 2), ("B", 60, 3))     # (base, known shift, noise seed)
RATIOS = (0.1, 0.2, 1.0)
WMAX = 240                                               # the window never holds more than 2 * num_sector shifts
# robot, descriptor name: the three-robot callback sequence of the node replay
SEQUENCE = ((1, "S11"), (2, "S12"), (3, "A"), (1, "B"), (2, "C"), (3, "S13"), (1, "A_roll17"), (2, "S14"), (3, "B_roll60"),
            (1, "C_empty"), (2, "A_roll-40"), (3, "zero"))


def clouds():
    from mr_slam_amd import synth
    A, B, C = make_golden_ref_corr.inputs()
    out = {"A": A, "B": B, "C": C}
    for s in SYNTH_SEEDS:
        out[f"S{s}"] = synth.lidar_scan(s, 20000)
    return out


def main():
    rec = {}
    with ref_import.reference_modules("oracle") as ref:
        u = ref.util
        cfg = u.cfg
        sys.path.insert(0, ref_import.RING_ROS)
        try:
            SC = importlib.import_module("pr_methods.ScanContext")
        finally:
            sys.path.remove(ref_import.RING_ROS)
        ns = ref.functions_of(os.path.join(ref_import.RING_ROS, "main_SC.py"), ["generate_scan_context"],
                              {"voxelocc": sys.modules["voxelocc"], "np": np, "cfg": cfg})
        gen = ns["generate_scan_context"]
        import inspect
        rec["public_names"] = np.array(sorted(n for n, f in vars(SC).items() if inspect.isfunction(f) and f.__module__ == SC.__name__
                                              and not n.startswith("_")))
        # ------------------------------------------------------------------------------------------------ descriptors
        names, descs = [], []
        for name, pc in clouds().items():
            names.append(name)
            descs.append(gen(pc).astype(np.float32))                           # main_SC.py:57-69
        rec["n_cloud_descriptors"] = np.array([len(names)])
        base = dict(zip(names, descs))
        for b, k, seed in ROLLS:
            rng = np.random.default_rng(seed)
            d = np.roll(base[b], k, axis=-1)
            d = np.where(d > 0, np.clip(d + rng.normal(0, 0.01, d.shape), 1e-3, 1.0), 0).astype(np.float32)
            names.append(f"{b}_roll{k}")
            descs.append(d)
        e = base["C"].copy()
        e[..., 0:30] = 0
        e[..., 70:80] = 0
        names.append("C_empty"); descs.append(e)
        names.append("zero"); descs.append(np.zeros_like(descs[0]))
        D = np.stack(descs)                                                    # [D, 1, 120, 120]
        rec["names"] = np.array(names)
        rec["sc"] = D
        rec["ringkey"] = np.stack([SC.make_ringkey(d) for d in D])             # ScanContext.py:13-21
        rec["sectorkey"] = np.stack([SC.make_sectorkey(d) for d in D])         # ScanContext.py:23-31
        # ------------------------------------------------------------------------------------------------ pairs
        ix = {n: i for i, n in enumerate(names)}
        und = [("A", "B"), ("A", "C"), ("A", "A_roll17"), ("A", "A_roll-40"), ("B", "B_roll60"), ("S11", "S12"), ("C", "C_empty"),
               ("zero", "A"), ("zero", "zero"), ("A", "A"), ("S13", "C_empty")]
        pairs = []
        for a, b in und:
            pairs.append((ix[a], ix[b]))
            if a != b:
                pairs.append((ix[b], ix[a]))
        P = np.array(pairs, np.int32)
        rec["pairs"] = P
        ns_norms = np.zeros((len(P), cfg.num_sector))
        sstar = np.zeros(len(P), np.int32)
        align = np.zeros((len(RATIOS), len(P), 2))
        wstart = np.zeros((len(RATIOS), len(P)), np.int32)
        wd = np.full((len(RATIOS), len(P), WMAX), np.nan)
        dsc = np.zeros((len(P), 2))
        direct = np.zeros(len(P))
        for p, (i, j) in enumerate(P):
            sc1, sc2 = D[i], D[j]
            k1, k2 = SC.make_sectorkey(sc1), SC.make_sectorkey(sc2)
            ns_norms[p] = [np.linalg.norm(k1 - np.roll(k2, s)) for s in range(cfg.num_sector)]   # fast_align_with_sectorkey's scores
            _, sstar[p] = SC.fast_align_with_sectorkey(k1, k2)
            direct[p] = SC.dist_direct_sc(sc1, sc2)
            for q, ratio in enumerate(RATIOS):
                dist, shift = SC.dist_align_sc(sc1, sc2, search_ratio=ratio)   # ScanContext.py:128-142
                align[q, p] = (dist, shift)
                r = round(0.5 * ratio * cfg.num_sector)
                win = range(max(-cfg.num_sector, sstar[p] - r), min(cfg.num_sector, sstar[p] + r + 1))
                wstart[q, p] = win[0]
                for w, s in enumerate(win):
                    wd[q, p, w] = SC.dist_direct_sc(sc1, np.roll(sc2, s, axis=-1))
            dist, yaw = SC.distance_sc(sc1, sc2)                               # ScanContext.py:34-69
            dsc[p] = (dist, yaw)
            print(names[i], names[j], "align", align[:, p].tolist(), "distance_sc", dsc[p].tolist())
        rec["ratios"] = np.array(RATIOS)
        rec["sector_norms"] = ns_norms
        rec["sector_shift"] = sstar
        rec["dist_align"] = align
        rec["window_start"] = wstart
        rec["window_dists"] = wd
        rec["distance_sc"] = dsc
        rec["dist_direct"] = direct
        # ------------------------------------------------------------------------------ node replay, main_SC.py:159-170
        from sklearn.neighbors import KDTree
        SCs = {1: [], 2: [], 3: []}
        RK = {1: [], 2: [], 3: []}
        rows = []
        for step, (robot, name) in enumerate(SEQUENCE):
            SC_current = D[ix[name]]
            Ringkey_current = SC.make_ringkey(SC_current)
            SCs[robot].append(SC_current)
            RK[robot].append(Ringkey_current)
            for cand in (1, 2, 3):
                if cand == robot or len(RK[cand]) < 1:
                    continue
                num_candidates = 1
                kdtree_pc = KDTree(np.array(RK[cand]))
                dists_pc, idxs_pc = kdtree_pc.query(np.array([Ringkey_current]), k=num_candidates)
                idx_sc = idxs_pc[0][0]
                SC_candidate = SCs[cand][idx_sc]
                dist_pc, yaw_pc = SC.dist_align_sc(SC_candidate, SC_current, search_ratio=0.1)
                rows.append((step, robot, cand, int(idx_sc), float(dists_pc[0][0]), float(dist_pc), int(yaw_pc)))
        rec["sequence"] = np.array([(r, ix[n]) for r, n in SEQUENCE], np.int32)
        rec["replay"] = np.array(rows)
        print("replay", rows)
        for k in [k for k in sys.modules if k == "pr_methods" or k.startswith("pr_methods.")]:
            sys.modules.pop(k)
    path = os.path.join(HERE, "ref_scancontext.npz")
    np.savez_compressed(path, **rec)
    print(os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
