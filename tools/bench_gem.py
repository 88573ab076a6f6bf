"""The global elevation map on the GPU (mr_slam_amd/gem.py): 3 robots x 100 submaps x 40 000 cells (200 x 200 cells of 0.2 m), submap centres
on a 10 x 10 lattice 8 m apart, so that a submap overlaps its 8 lattice neighbours inside the 15 m radius.  Measured per robot store:
`update_global` as wall-clock around the blocking call and its steps between HIP events (MRS_DEV=1 MRS_GEM_TIMING=1: move, key range, keys,
sort, heads + gather, fuse); then `compose_robots` over the three stores with and without merge_cells, and `costmap` at 2000 x 2000 over the
composed cloud on the device.  Prints ONE JSON line and, with --out, writes it to a file.  Run on its own.

Both baselines are measured in the same run, never taken from the new code:
  (a) the NumPy restatement (tests/golden/gem_restate.py, the vectorised one) on one CPU thread, `update_global` of robot 0; its result is
      also compared with the GPU's, bit for bit;
  (b) what a user of the library had before: torch on the device -- one matmul per moved submap, torch.unique for the first record of a cell,
      torch.searchsorted for the join of a pair, the rule in float64 -- the same pairs in the same order, `update_global` of robot 0.
"""
import argparse
import json
import os
import sys
import tempfile
import time

os.environ.setdefault("OMP_NUM_THREADS", "1")
os.environ["MRS_DEV"] = "1"
os.environ["MRS_GEM_TIMING"] = "1"

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

ROBOTS, SIDE, CELLS_SIDE, RES, SPACING = 3, 10, 200, 0.2, 8.0


def pose(yaw, tx, ty, tz):
    c, s = np.cos(yaw), np.sin(yaw)
    return np.array([[c, -s, 0, tx], [s, c, 0, ty], [0, 0, 1, tz], [0, 0, 0, 1]], np.float32)


def make_robot(R, robot, side, cells_side):
    """-> (clouds, poses, centres, opt poses)"""
    rng = np.random.default_rng(100 + robot)
    n = cells_side * cells_side
    ix, iy = np.divmod(np.arange(n), cells_side)
    clouds, poses, centres, opt = [], [], [], []
    for k in range(side * side):
        cx, cy = SPACING * (k // side) + 3.0 * robot, SPACING * (k % side)
        c = R.cells(n)
        c["x"] = (cx + (ix - cells_side / 2 + rng.uniform(0.2, 0.8, n)) * RES).astype(np.float32)
        c["y"] = (cy + (iy - cells_side / 2 + rng.uniform(0.2, 0.8, n)) * RES).astype(np.float32)
        c["z"] = rng.uniform(-1, 2, n).astype(np.float32)
        c["var"] = rng.uniform(0.05, 0.9, n).astype(np.float32)
        c["r"], c["g"], c["b"] = rng.integers(0, 256, (3, n))
        c["frontier"] = rng.integers(0, 2, n)
        c["intensity"] = rng.uniform(0, 100, n).astype(np.float32)
        c["travers"] = rng.uniform(0, 1, n).astype(np.float32)
        clouds.append(c)
        poses.append(pose(0.002 * k, cx, cy, 0.1))
        centres.append((cx, cy))
        opt.append(pose(0.002 * k + rng.uniform(-0.002, 0.002), cx + rng.uniform(-0.05, 0.05), cy + rng.uniform(-0.05, 0.05), 0.1 + rng.uniform(-0.02, 0.02)))
    return clouds, np.stack(poses), centres, np.stack(opt)


def fill(store, clouds, poses, centres):
    for c, p, xy in zip(clouds, poses, centres):
        store.append_cells(c)
        store.close_submap(p, xy)
    return store


class Stderr:
    """the lines the library writes to file descriptor 2 while the block runs"""

    def __enter__(self):
        self.tmp = tempfile.TemporaryFile()
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode(errors="replace")
        self.tmp.close()


def steps_of(text):
    for line in text.splitlines():
        if "gem update steps ms:" in line:
            w = line.split("ms:")[1].split()
            f = dict(zip(w[::2], w[1::2]))                                # the line is "name value" pairs; read by name
            counts = {"records": int(f.pop("records")), "sort_bits": int(f.pop("bits")), "fuse_launches": int(f.pop("launches"))}
            return {k: float(v) for k, v in f.items()} | counts
    return None


def torch_update(torch, clouds, poses, centres, opt, radius=15.0, min_neighbours=3):
    """baseline (b): columns per submap as device tensors; returns the number of fused cells"""
    dev = "cuda:0"
    subs = [{f: torch.from_numpy(np.ascontiguousarray(c[f])).to(dev) for f in c.dtype.names} for c in clouds]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    K = len(subs)
    P, O = torch.from_numpy(poses).to(dev), torch.from_numpy(opt).to(dev)
    for i in range(1, K):
        T = O[i] @ torch.linalg.inv(P[i])
        s = subs[i]
        xyz = torch.stack([s["x"], s["y"], s["z"], torch.ones_like(s["x"])], 1) @ T.T
        s["x"], s["y"], s["z"] = xyz[:, 0].contiguous(), xyz[:, 1].contiguous(), xyz[:, 2].contiguous()
    C = torch.tensor(centres, dtype=torch.float32)
    d2 = ((C[:, None] - C[None]) ** 2).sum(-1)
    keys = []
    for s in subs:                                                        # canonical form: first record per key, key order, snapped
        kx, ky = torch.ceil(s["x"].double() / RES).long(), torch.ceil(s["y"].double() / RES).long()
        p = ((kx + (1 << 23)) << 24) | (ky + (1 << 23))
        u, inv = torch.unique(p, return_inverse=True)
        first = torch.full((u.numel(),), p.numel(), dtype=torch.long, device=dev).scatter_reduce(0, inv, torch.arange(p.numel(), device=dev), "amin")
        for f in s:
            s[f] = s[f][first]
        s["x"] = ((u >> 24) - (1 << 23)).double().mul(RES).sub(RES / 2).float()
        s["y"] = ((u & 0xFFFFFF) - (1 << 23)).double().mul(RES).sub(RES / 2).float()
        keys.append(u)
    matched = 0
    for i in range(K):
        near = [j for j in torch.argsort(d2[i], stable=True).tolist() if j != i and d2[i, j] <= radius * radius]
        if len(near) + 1 < min_neighbours:
            continue
        old = subs[i]
        for j in near:
            new = subs[j]
            at = torch.searchsorted(keys[j], keys[i]).clamp_(max=keys[j].numel() - 1)
            hit = (keys[j][at] == keys[i]) & (old["var"] > 0) & (old["var"] < 1)
            io, jn = torch.nonzero(hit).squeeze(1), at[hit]
            vo2, vn2 = old["var"][io].double() ** 2, new["var"][jn].double() ** 2
            z = ((vn2 * old["z"][io].double() + vo2 * new["z"][jn].double()) / (vo2 + vn2)).float()
            var = (vo2 * vn2 / (vo2 + vn2)).float()
            fr = ((old["frontier"][io] != 0) & (new["frontier"][jn] != 0)).int()
            for f in ("r", "g", "b", "intensity", "travers"):
                old[f][io] = new[f][jn]
            old["z"][io], new["z"][jn], old["var"][io], new["var"][jn], old["frontier"][io], new["frontier"][jn] = z, z, var, var, fr, fr
            matched += io.numel()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, matched


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--side", type=int, default=SIDE, help="submaps per robot = side^2")
    ap.add_argument("--cells-side", type=int, default=CELLS_SIDE, help="cells per submap = cells_side^2")
    ap.add_argument("--costmap-size", type=int, default=2000)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs cuda:0"
    import gem_restate as R
    from mr_slam_amd import gem

    res = dict(tool="bench_gem", device=torch.cuda.get_device_name(0), robots=ROBOTS, submaps_per_robot=a.side ** 2, cells_per_submap=a.cells_side ** 2,
               resolution=RES, centre_spacing_m=SPACING, runs=1)
    robots = [make_robot(R, r, a.side, a.cells_side) for r in range(ROBOTS)]
    stores, upd = [], []
    for clouds, poses, centres, opt in robots:
        t0 = time.perf_counter()
        st = fill(gem.ElevationSubmaps(RES), clouds, poses, centres)
        t_fill = (time.perf_counter() - t0) * 1e3
        with Stderr() as err:
            t0 = time.perf_counter()
            matched = st.update_global(opt)
            ms = (time.perf_counter() - t0) * 1e3
        upd.append(dict(fill_ms=round(t_fill, 2), update_global_ms=round(ms, 3), steps_ms=steps_of(err.text), matched=matched, dropped=st.dropped,
                        cells_after=st.n_cells))
        stores.append(st)
    res["gpu_update_global"] = upd

    clouds, poses, centres, opt = robots[0]
    ref = fill(R.Vectorised(RES), clouds, poses, centres)
    t0 = time.perf_counter()
    ref.update_global(opt)
    res["numpy_update_global_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    res["gpu_equals_numpy_bit_for_bit"] = bool(R.same(stores[0].compose(), ref.compose()) and ref.matched == upd[0]["matched"])
    ms, matched = torch_update(torch, clouds, poses, centres, opt)
    res["torch_update_global_ms"] = round(ms, 1)
    res["torch_matched"] = matched

    identity = [np.tile(np.eye(4, dtype=np.float32), (len(s), 1, 1)) for s in stores]
    for merge in (False, True):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = gem.compose_robots(stores, identity, merge_cells=merge, device=True)
        torch.cuda.synchronize()
        res["compose_robots_merge_ms" if merge else "compose_robots_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        res["compose_robots_merge_cells" if merge else "compose_robots_cells"] = int(out.shape[0])
        if not merge:
            cloud = out
    lo = float(min(c[0] for c in robots[0][2])) - 25.0
    size = a.costmap_size
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    grid = gem.costmap(cloud, (lo, lo), (size, size), RES, travers_thresh=0.5, device=True)
    torch.cuda.synchronize()
    res["costmap_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    res["costmap_size"] = size
    res["costmap_known_cells"] = int((grid != 255).sum())
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
