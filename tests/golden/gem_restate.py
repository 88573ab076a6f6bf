"""Two independent NumPy restatements of the global elevation map contract (the kernels are mr_slam_amd/csrc/gem.hip).

`Literal` follows the cited C++ statement by statement with a Python dict where the reference has a std::unordered_map
(elevation_mapping/src/ElevationMapping.cpp:762-811, :827-959, :1183-1239; global_manager.cpp:2133-2152; pointMap_layer.cpp:100-135).
`Vectorised` is the algorithm the kernels use: sort, first occurrence, searchsorted join.  They share the record type, the two neighbour
parameters and nothing else.  Every float32 step is one NumPy float32 operation in the order the library (built with -ffp-contract=off)
takes it; the fusion rules and the keys are in double, as there.

Where the contract fixes what the reference leaves to a library (PCL's radius search and transformPointCloud, grid_map, costmap_2d, the
iteration order of unordered_map) both restatements follow the contract:
  * the open submap and a closed submap list their cells in ascending order of first insertion; a rebuilt (canonical) submap lists them
    in ascending (kx, ky);
  * elevation == -10 is tested when a submap is put into canonical form, before its cells are fused; the reference tests it after
    (localHashtoPointCloud).  The two differ only where a moved or fused elevation is exactly -10, which no case here has
    (tests/test_gem_cpu.py asserts the margin);
  * a record without a key (non-finite x or y, |k| >= 2^23) is dropped and counted, where the reference would hash it.
"""
import numpy as np

CELL = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("var", "<f4"), ("r", "<i4"), ("g", "<i4"), ("b", "<i4"), ("frontier", "<i4"),
                 ("intensity", "<f4"), ("travers", "<f4")])
WEIGHTED, AS_WRITTEN = 0, 1
KEY_BOUND = 1 << 23
F = np.float32


def cells(n=0, **cols):
    """n records (z = 0, var = 0.5 unless given), columns from keyword arrays"""
    a = np.zeros(n, CELL)
    a["var"] = 0.5
    for k, v in cols.items():
        a[k] = v
    return a


def bits(a):
    """the 32-bit words of records, [n, 10] uint32: what 'bit for bit' compares"""
    return np.ascontiguousarray(a).view(np.uint32).reshape(-1, 10)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def key_of(v, res):
    """ceil((double)v / res) as an int, or None for a non-finite v or a key outside |k| < 2^23"""
    c = np.ceil(np.float64(v) / res)
    if not (c > -KEY_BOUND and c < KEY_BOUND):
        return None
    return int(c)


def centre_of(k, res):
    return F(float(k) * res - res / 2.0)


def fuse_zvar(rule, zo, vo, zn, vn):
    """double arithmetic on Python floats, stored to float32"""
    zo, vo, zn, vn = float(zo), float(vo), float(zn), float(vn)
    vo2, vn2 = vo * vo, vn * vn
    with np.errstate(all="ignore"):
        vo2, vn2, zo, zn = np.float64(vo2), np.float64(vn2), np.float64(zo), np.float64(zn)     # float64 scalars: x / 0 is inf, not an exception
        if rule == AS_WRITTEN:
            return F(((vn2 * zo) + ((vo2 * zn) / vo2)) + vn2), F(((vo2 * vn2) / vo2) + vn2)
        s = vo2 + vn2
        return F(((vn2 * zo) + (vo2 * zn)) / s), F((vo2 * vn2) / s)


def leaves_window(px, py, elevation, cx, cy, dx, dy, length, resolution):
    """ElevationMapping.cpp:770-779 as written, in float32"""
    px, py, elevation, cx, cy, dx, dy = F(px), F(py), F(elevation), F(cx), F(cy), F(dx), F(dy)
    half = F(length) * F(resolution) / F(2)
    if not elevation != F(-10):
        return False
    xl, xh, yl, yh = cx - half, cx + half, cy - half, cy + half
    return bool(((px < xl or py < yl) and (dx > 0 and dy > 0)) or ((px > xh or py > yh) and (dx < 0 and dy < 0))
                or ((px < xl or py > yh) and (dx > 0 and dy < 0)) or ((px > xh or py < yl) and (dx < 0 and dy > 0))
                or ((px < xl) and (dx > 0 and dy == 0)) or ((px > xh) and (dx < 0 and dy == 0))
                or ((py < yl) and (dy > 0 and dx == 0)) or ((py > yh) and (dy < 0 and dx == 0)))


def cell_cost(z, travers, travers_thresh, z_thresh):
    known = F(z) != F(-10) and F(z) != F(10) and F(travers) != F(-10)
    hit = float(travers) < travers_thresh if z_thresh is None else float(z) > z_thresh
    return 254 if known and hit else 0


# ---------------------------------------------------------------------------------------------------------------------------------------
# literal
# ---------------------------------------------------------------------------------------------------------------------------------------

def _correction_literal(opt, pose):
    """T = opt * inverse(pose) in float32; inverse = (R^T, -(R^T t)); every sum left to right"""
    opt, pose = np.asarray(opt, F), np.asarray(pose, F)
    inv = np.zeros((4, 4), F)
    for r in range(3):
        for c in range(3):
            inv[r, c] = pose[c, r]
        inv[r, 3] = -((pose[0, r] * pose[0, 3] + pose[1, r] * pose[1, 3]) + pose[2, r] * pose[2, 3])
    inv[3, 3] = 1
    T = np.zeros((4, 4), F)
    for r in range(3):
        for c in range(4):
            T[r, c] = ((opt[r, 0] * inv[0, c] + opt[r, 1] * inv[1, c]) + opt[r, 2] * inv[2, c]) + opt[r, 3] * inv[3, c]
    T[3, 3] = 1
    return T


def _move_literal(cloud, T):
    out = cloud.copy()
    T = np.asarray(T, F)
    with np.errstate(all="ignore"):
        for n in range(cloud.size):
            x, y, z = cloud["x"][n], cloud["y"][n], cloud["z"][n]
            out["x"][n] = ((T[0, 0] * x + T[0, 1] * y) + T[0, 2] * z) + T[0, 3]
            out["y"][n] = ((T[1, 0] * x + T[1, 1] * y) + T[1, 2] * z) + T[1, 3]
            out["z"][n] = ((T[2, 0] * x + T[2, 1] * y) + T[2, 2] * z) + T[2, 3]
    return out


class Literal:
    def __init__(self, resolution=0.2, rule=WEIGHTED, radius=15.0, min_neighbours=3):
        self.res, self.rule, self.radius, self.min_neighbours = float(resolution), rule, F(radius), min_neighbours
        self.open = {}                      # (x bits, y bits) -> record; a dict keeps a replaced key at its first place
        self.subs, self.poses, self.centres = [], [], []
        self.dropped = self.matched = 0

    # :762-811
    def append_cells(self, cloud):
        w = bits(cloud)
        for n in range(cloud.size):
            self.open[(int(w[n, 0]), int(w[n, 1]))] = cloud[n].copy()

    def append_leaving(self, cloud, current_xy, shift_xy, length, resolution):
        keep = [n for n in range(cloud.size) if leaves_window(cloud["x"][n], cloud["y"][n], cloud["z"][n], current_xy[0], current_xy[1],
                                                             shift_xy[0], shift_xy[1], length, resolution)]
        self.append_cells(cloud[keep])

    # :682-685 with localHashtoPointCloud :1183-1203
    def close_submap(self, pose, centre):
        out = [r for r in self.open.values() if r["z"] != F(-10)]
        self.subs.append(np.array(out, CELL) if out else np.zeros(0, CELL))
        self.poses.append(np.array(pose, F).reshape(4, 4))
        self.centres.append(np.array(centre, F).reshape(2))
        self.open = {}

    # pointCloudtoHash :1226-1239: insert keeps the first record of a key
    def _to_hash(self, cloud):
        out = {}
        for n in range(cloud.size):
            kx, ky = key_of(cloud["x"][n], self.res), key_of(cloud["y"][n], self.res)
            if kx is None or ky is None:
                self.dropped += 1
                continue
            if (kx, ky) in out:
                continue
            rec = cloud[n].copy()
            rec["x"], rec["y"] = centre_of(kx, self.res), centre_of(ky, self.res)
            out[(kx, ky)] = rec
        return {k: v for k, v in out.items() if v["z"] != F(-10)}       # :1187, applied before the cells are fused (see the module text)

    @staticmethod
    def _to_cloud(h):
        return np.array([h[k] for k in sorted(h)], CELL) if h else np.zeros(0, CELL)

    def _fuse_pair(self, j, i):
        """:899-941 with new = submap j, old = submap i"""
        out_new, out_old = self._to_hash(self.subs[j]), self._to_hash(self.subs[i])
        for key in list(out_new):                                  # every key once: erase / insert does not revisit one
            new, got = out_new[key], out_old.get(key)
            if got is not None and got["var"] > 0 and got["var"] < 1:
                self.matched += 1
                tmp = new.copy()
                tmp["z"], tmp["var"] = fuse_zvar(self.rule, got["z"], got["var"], new["z"], new["var"])
                tmp["frontier"] = 1 if (got["frontier"] and new["frontier"]) else 0
                out_new[key] = tmp
                out_old[key] = tmp.copy()
        self.subs[j], self.subs[i] = self._to_cloud(out_new), self._to_cloud(out_old)

    # :827-959
    def update_global(self, opt):
        self.dropped = self.matched = 0
        K = min(len(opt), len(self.subs))
        for i in range(1, K):
            T = _correction_literal(opt[i], self.poses[i])
            self.subs[i] = _move_literal(self.subs[i], T)
            self.poses[i] = np.array(opt[i], F).reshape(4, 4)
        r2 = self.radius * self.radius
        for i in range(K):
            found = []
            for j in range(K):
                dx, dy = self.centres[j][0] - self.centres[i][0], self.centres[j][1] - self.centres[i][1]
                d2 = dx * dx + dy * dy
                if j != i and d2 <= r2:
                    found.append((d2, j))
            idx = [i] + [j for _, j in sorted(found)]
            if len(idx) >= self.min_neighbours:
                for j in idx[1:]:
                    self._fuse_pair(j, i)
        return self.matched

    def compose(self):
        return np.concatenate(self.subs) if self.subs else np.zeros(0, CELL)


def compose_robots_literal(stores, poses, local_maps=None, refs=None, merge_cells=False, rule=WEIGHTED, resolution=0.2):
    """global_manager.cpp:2133-2152, :2287: (robot, submap) order, the local maps last; merge_cells: a left-to-right fold per key"""
    parts = [_move_literal(s.subs[j], poses[r][j]) for r, s in enumerate(stores) for j in range(len(s.subs))]
    if local_maps is not None:
        parts += [_move_literal(np.asarray(m, CELL), refs[r]) for r, m in enumerate(local_maps)]
    cat = np.concatenate(parts) if parts else np.zeros(0, CELL)
    if not merge_cells:
        return cat, 0
    grid, dropped = {}, 0
    for n in range(cat.size):
        kx, ky = key_of(cat["x"][n], resolution), key_of(cat["y"][n], resolution)
        if kx is None or ky is None:
            dropped += 1
            continue
        run = grid.get((kx, ky))
        if run is None:
            run = cat[n].copy()
            run["x"], run["y"] = centre_of(kx, resolution), centre_of(ky, resolution)
            grid[(kx, ky)] = run
        elif run["var"] > 0 and run["var"] < 1:
            new = cat[n]
            z, var = fuse_zvar(rule, run["z"], run["var"], new["z"], new["var"])
            frontier = 1 if (run["frontier"] and new["frontier"]) else 0
            for f in ("r", "g", "b", "intensity", "travers"):
                run[f] = new[f]
            run["z"], run["var"], run["frontier"] = z, var, frontier
    return Literal._to_cloud(grid), dropped


def costmap_literal(cloud, origin_xy, size_xy, resolution, travers_thresh=None, z_thresh=None):
    """pointMap_layer.cpp:100-135 with costmap_2d's worldToMap restated"""
    ox, oy, (sx, sy), res = float(origin_xy[0]), float(origin_xy[1]), size_xy, float(resolution)
    grid = np.full((sy, sx), 255, np.uint8)
    for n in range(cloud.size):
        px, py = float(cloud["x"][n]), float(cloud["y"][n])
        if px != px or py != py:
            continue
        if px < ox or py < oy:
            continue
        fx, fy = (px - ox) / res, (py - oy) / res
        if not (fx < sx and fy < sy):
            continue
        grid[int(fy), int(fx)] = cell_cost(cloud["z"][n], cloud["travers"][n], travers_thresh, z_thresh)
    return grid


# ---------------------------------------------------------------------------------------------------------------------------------------
# vectorised: the kernels' algorithm
# ---------------------------------------------------------------------------------------------------------------------------------------

def _keys_vec(cloud, res):
    """-> (valid [n], kx, ky int64)"""
    with np.errstate(all="ignore"):
        cx, cy = np.ceil(cloud["x"].astype(np.float64) / res), np.ceil(cloud["y"].astype(np.float64) / res)
        ok = (cx > -KEY_BOUND) & (cx < KEY_BOUND) & (cy > -KEY_BOUND) & (cy < KEY_BOUND)
    kx, ky = np.where(ok, cx, 0).astype(np.int64), np.where(ok, cy, 0).astype(np.int64)
    return ok, kx, ky


def _pack(kx, ky):
    return ((kx + KEY_BOUND) << 24) | (ky + KEY_BOUND)


def _fuse_vec(rule, zo, vo, zn, vn):
    zo, vo, zn, vn = (a.astype(np.float64) for a in (zo, vo, zn, vn))
    vo2, vn2 = vo * vo, vn * vn
    with np.errstate(all="ignore"):
        if rule == AS_WRITTEN:
            return (((vn2 * zo) + ((vo2 * zn) / vo2)) + vn2).astype(F), (((vo2 * vn2) / vo2) + vn2).astype(F)
        s = vo2 + vn2
        return (((vn2 * zo) + (vo2 * zn)) / s).astype(F), ((vo2 * vn2) / s).astype(F)


def _move_vec(cloud, T):
    T = np.asarray(T, F).reshape(4, 4)
    out = cloud.copy()
    x, y, z = cloud["x"], cloud["y"], cloud["z"]
    with np.errstate(all="ignore"):
        for r, f in enumerate(("x", "y", "z")):
            out[f] = ((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3]
    return out


def _correction_vec(opt, pose):
    opt, pose = np.asarray(opt, F).reshape(4, 4), np.asarray(pose, F).reshape(4, 4)
    Rt, t = pose[:3, :3].T, pose[:3, 3]
    inv = np.zeros((4, 4), F)
    inv[:3, :3] = Rt
    inv[:3, 3] = -((Rt[:, 0] * t[0] + Rt[:, 1] * t[1]) + Rt[:, 2] * t[2])
    inv[3, 3] = 1
    T = np.zeros((4, 4), F)
    T[:3] = ((opt[:3, 0:1] * inv[0] + opt[:3, 1:2] * inv[1]) + opt[:3, 2:3] * inv[2]) + opt[:3, 3:4] * inv[3]
    T[3, 3] = 1
    return T


class Vectorised:
    def __init__(self, resolution=0.2, rule=WEIGHTED, radius=15.0, min_neighbours=3):
        self.res, self.rule, self.radius, self.min_neighbours = float(resolution), rule, F(radius), min_neighbours
        self.open = np.zeros(0, CELL)
        self.subs, self.poses, self.centres = [], [], []
        self.dropped = self.matched = 0

    def append_cells(self, cloud):
        self.open = np.concatenate([self.open, np.asarray(cloud, CELL).reshape(-1)])

    def append_leaving(self, cloud, current_xy, shift_xy, length, resolution):
        px, py, z = cloud["x"], cloud["y"], cloud["z"]
        cx, cy, dx, dy = F(current_xy[0]), F(current_xy[1]), F(shift_xy[0]), F(shift_xy[1])
        half = F(length) * F(resolution) / F(2)
        xl, xh, yl, yh = px < cx - half, px > cx + half, py < cy - half, py > cy + half
        m = (((xl | yl) & bool(dx > 0 and dy > 0)) | ((xh | yh) & bool(dx < 0 and dy < 0)) | ((xl | yh) & bool(dx > 0 and dy < 0))
             | ((xh | yl) & bool(dx < 0 and dy > 0)) | (xl & bool(dx > 0 and dy == 0)) | (xh & bool(dx < 0 and dy == 0))
             | (yl & bool(dy > 0 and dx == 0)) | (yh & bool(dy < 0 and dx == 0)))
        self.append_cells(cloud[m & (z != F(-10))])

    def close_submap(self, pose, centre):
        n = self.open.size
        w = bits(self.open)
        key = (w[:, 0].astype(np.uint64) << np.uint64(32)) | w[:, 1].astype(np.uint64)
        order = np.argsort(key, kind="stable")
        ks = key[order]
        head = np.ones(n, bool)
        head[1:] = ks[1:] != ks[:-1]
        tail = np.ones(n, bool)
        tail[:-1] = head[1:]
        first, last = order[head], order[tail]                     # per run: the first insertion and the last writer
        keep = self.open["z"][last] != F(-10)
        by_first = np.argsort(first[keep], kind="stable")
        self.subs.append(self.open[last[keep][by_first]].copy())
        self.poses.append(np.array(pose, F).reshape(4, 4))
        self.centres.append(np.array(centre, F).reshape(2))
        self.open = np.zeros(0, CELL)

    def _canonical(self, cloud):
        """-> (cloud in canonical form, its packed keys ascending)"""
        ok, kx, ky = _keys_vec(cloud, self.res)
        self.dropped += int((~ok).sum())
        cloud, kx, ky = cloud[ok], kx[ok], ky[ok]
        order = np.lexsort((ky, kx))                               # stable: the first record of a cell stays first
        p = _pack(kx, ky)[order]
        head = np.ones(p.size, bool)
        head[1:] = p[1:] != p[:-1]
        sel = order[head]
        sel = sel[cloud["z"][sel] != F(-10)]
        out = cloud[sel].copy()
        out["x"] = (kx[sel].astype(np.float64) * self.res - self.res / 2.0).astype(F)
        out["y"] = (ky[sel].astype(np.float64) * self.res - self.res / 2.0).astype(F)
        return out, _pack(kx[sel], ky[sel])

    def update_global(self, opt):
        self.dropped = self.matched = 0
        K = min(len(opt), len(self.subs))
        for i in range(1, K):
            self.subs[i] = _move_vec(self.subs[i], _correction_vec(opt[i], self.poses[i]))
            self.poses[i] = np.array(opt[i], F).reshape(4, 4)
        if K == 0:
            return 0
        C = np.array(self.centres[:K], F).reshape(K, 2)
        dx, dy = C[None, :, 0] - C[:, None, 0], C[None, :, 1] - C[:, None, 1]
        d2 = dx * dx + dy * dy                                     # [i, j], float32
        lists = []
        for i in range(K):
            near = np.flatnonzero((d2[i] <= self.radius * self.radius) & (np.arange(K) != i))
            near = near[np.lexsort((near, d2[i][near]))]
            if near.size + 1 >= self.min_neighbours:
                lists.append((i, near))
        part = sorted({i for i, _ in lists} | {int(j) for _, near in lists for j in near})
        keys = {}
        for s in part:                                             # the one chain: everything that takes part, once
            self.subs[s], keys[s] = self._canonical(self.subs[s])
        for i, near in lists:
            old = self.subs[i]
            for j in near:
                new = self.subs[int(j)]
                at = np.searchsorted(keys[int(j)], keys[i])
                at[at == keys[int(j)].size] = 0
                hit = (keys[int(j)][at] == keys[i]) if keys[int(j)].size else np.zeros(keys[i].size, bool)
                with np.errstate(invalid="ignore"):
                    hit &= (old["var"] > 0) & (old["var"] < 1)
                io, jn = np.flatnonzero(hit), at[hit]
                fused = new[jn].copy()
                fused["z"], fused["var"] = _fuse_vec(self.rule, old["z"][io], old["var"][io], new["z"][jn], new["var"][jn])
                fused["frontier"] = ((old["frontier"][io] != 0) & (new["frontier"][jn] != 0)).astype(np.int32)
                old[io], new[jn] = fused, fused
                self.matched += io.size
        return self.matched

    def compose(self):
        return np.concatenate(self.subs) if self.subs else np.zeros(0, CELL)


def compose_robots_vec(stores, poses, local_maps=None, refs=None, merge_cells=False, rule=WEIGHTED, resolution=0.2):
    parts = [_move_vec(s.subs[j], poses[r][j]) for r, s in enumerate(stores) for j in range(len(s.subs))]
    if local_maps is not None:
        parts += [_move_vec(np.asarray(m, CELL), refs[r]) for r, m in enumerate(local_maps)]
    cat = np.concatenate(parts) if parts else np.zeros(0, CELL)
    if not merge_cells:
        return cat, 0
    ok, kx, ky = _keys_vec(cat, resolution)
    dropped = int((~ok).sum())
    cat, p = cat[ok], _pack(kx[ok], ky[ok])
    order = np.argsort(p, kind="stable")
    ps = p[order]
    head = np.ones(ps.size, bool)
    head[1:] = ps[1:] != ps[:-1]
    starts = np.flatnonzero(head)
    lens = np.diff(np.append(starts, ps.size))
    run = cat[order[starts]].copy()
    for step in range(1, int(lens.max()) if lens.size else 0):     # fold position `step` of every run that long into the running record
        live = np.flatnonzero(lens > step)
        with np.errstate(invalid="ignore"):
            live = live[(run["var"][live] > 0) & (run["var"][live] < 1)]
        new = cat[order[starts[live] + step]]
        z, var = _fuse_vec(rule, run["z"][live], run["var"][live], new["z"], new["var"])
        frontier = ((run["frontier"][live] != 0) & (new["frontier"] != 0)).astype(np.int32)
        for f in ("r", "g", "b", "intensity", "travers"):
            run[f][live] = new[f]
        run["z"][live], run["var"][live], run["frontier"][live] = z, var, frontier
    k = ps[starts]
    run["x"] = (((k >> 24) - KEY_BOUND).astype(np.float64) * resolution - resolution / 2.0).astype(F)
    run["y"] = (((k & 0xFFFFFF) - KEY_BOUND).astype(np.float64) * resolution - resolution / 2.0).astype(F)
    return run, dropped


def costmap_vec(cloud, origin_xy, size_xy, resolution, travers_thresh=None, z_thresh=None):
    ox, oy, (sx, sy), res = float(origin_xy[0]), float(origin_xy[1]), size_xy, float(resolution)
    px, py = cloud["x"].astype(np.float64), cloud["y"].astype(np.float64)
    with np.errstate(invalid="ignore"):
        fx, fy = (px - ox) / res, (py - oy) / res
        ok = ~np.isnan(px) & ~np.isnan(py) & ~(px < ox) & ~(py < oy) & (fx < sx) & (fy < sy)
        z, tr = cloud["z"], cloud["travers"]
        hit = (tr.astype(np.float64) < travers_thresh) if z_thresh is None else (z.astype(np.float64) > z_thresh)
    cost = np.where((z != F(-10)) & (z != F(10)) & (tr != F(-10)) & hit, 254, 0).astype(np.uint8)
    word = (np.arange(1, cloud.size + 1, dtype=np.int64) << 8) | cost          # the scatter's (input index, cost) word; the maximum wins
    cell = fy[ok].astype(np.int64) * sx + fx[ok].astype(np.int64)
    best = np.zeros(sx * sy, np.int64)
    np.maximum.at(best, cell, word[ok])
    return np.where(best > 0, best & 0xFF, 255).astype(np.uint8).reshape(sy, sx)
