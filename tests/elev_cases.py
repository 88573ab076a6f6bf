"""Small deterministic elevation-mapping scenarios (row N3), one stage at a time.  tests/test_elevation_stages_gpu.py runs them on
the HIP library against the sequential restatement (oracle/elev_oracle.cpp) with the map state copied from the GPU, and
tests/test_oracle_elev.py replays them on the restatement against the reference's gpu_process.cu built for the host.

A map object `m` below is anything with the methods of mr_slam_amd.elevation.ElevationMap (pyoracle.ElevMap / RefElevMap too).
Grid index = window index (0 = the +x / +y edge), storage index = grid index rotated by `start` (what Fuse takes).
"""
import numpy as np

F = np.float32
RV = np.diag([1e-4, 1e-4, 4e-4]).astype(F)
BSKEW = [[0, -0.2, 0.1], [0.2, 0, -0.05], [-0.1, 0.05, 0]]
SENSOR = (-2.0, 3.0, 0.02, 0.003, 0.01, [0.0, 0.0, 1.0], RV, np.eye(3), [0.0, 0.0, 1.0], BSKEW)
LAYERS = ("lowest", "elevation", "variance", "intensity", "traver")


# ------------------------------------------------------------------------------------------------ geometry helpers
def transform(k, tz=0.0, origin=(0.0, 0.0)):
    """sensor -> world: a rotation by k * 90 degrees about z (entries exactly 0 / +-1), a height offset and the sensor's world
    position; with the sensor at the world origin x_ts / y_ts are exactly the planned world coordinates"""
    T = np.eye(4, dtype=F)
    T[:2, :2] = ([[1, 0], [0, 1]], [[0, -1], [1, 0]], [[-1, 0], [0, -1]], [[0, 1], [-1, 0]])[k]
    T[:3, 3] = origin[0], origin[1], tz
    return T


def to_sensor(k, wx, wy, origin=(0.0, 0.0)):
    """the sensor-frame point that transform(k, origin=origin) maps onto the world point (wx, wy) (exactly, for origin 0)"""
    wx, wy = np.asarray(wx, F) - F(origin[0]), np.asarray(wy, F) - F(origin[1])
    return ((wx, wy), (wy, -wx), (-wx, -wy), (-wy, wx))[k]


def passes_filter(xs, ys):
    """the reference's point filter (gpu_process.cu:394-397) in the sensor frame: only points behind the robot survive"""
    return ~(((np.abs(xs) < 1.5) & (np.abs(ys) < 1.5)) | ((ys > -1) & (ys < 1)) | (ys > 0))


def rotation_for(wx, wy, origin=(0.0, 0.0)):
    """per world point, the first of the four sensor headings under which it survives the filter (-1: none)"""
    wx, wy = np.asarray(wx, F), np.asarray(wy, F)
    k = np.full(wx.shape, -1)
    for r in (3, 2, 1, 0):
        k[passes_filter(*to_sensor(r, wx, wy, origin))] = r
    return k


def cell_centre(L, res, central, i):
    """world coordinate of the centre of grid row / column i along one axis (i may lie outside 0 .. L-1)"""
    off = (L // 2 - np.asarray(i) - 0.5) if L % 2 == 0 else (L // 2 - np.asarray(i))
    return (np.float64(central) + off * np.float64(res)).astype(F)


def storage_index(L, start, gx, gy):
    return ((np.asarray(gx) + int(start[0])) % L) * L + (np.asarray(gy) + int(start[1])) % L


def process(m, xs, ys, zs, T):
    return m.process_points(xs, ys, zs, T, *SENSOR)


def observe(m, wx, wy, wz, origin=(0.0, 0.0)):
    """Process world points from a sensor at `origin` through as many of the four headings as needed (one Process_points call
    per heading, in heading order).  Returns the per-call outputs and the concatenated (map_index, z_ts, var) for fuse()."""
    k = rotation_for(wx, wy, origin)
    assert (k >= 0).all(), "a point lies in the 1.5 m box around the sensor, which the filter always rejects"
    outs = []
    for r in range(4):
        sel = k == r
        if sel.any():
            xs, ys = to_sensor(r, np.asarray(wx, F)[sel], np.asarray(wy, F)[sel], origin)
            outs.append(process(m, xs, ys, np.asarray(wz, F)[sel], transform(r, 0.0, origin)))
    cat = {key: np.concatenate([o[key] for o in outs]) for key in ("map_index", "z_ts", "var")}
    return outs, cat


def layers(m):
    return [m.layer(w) for w in range(5)]


def colours_for(rng, n):
    """non-zero colours and intensities (every point coloured)"""
    return rng.integers(1, 256, n), rng.integers(1, 256, n), rng.integers(1, 256, n), rng.uniform(0.1, 1, n).astype(F)


# ------------------------------------------------------------------------------------------------ Move
MOVE_RES = 0.5


def move_shifts(L):
    """single-axis cell shifts: inside the map, a whole map length, and far beyond, both signs"""
    return [0, 1, -1, L - 1, -(L - 1), L, -L, L + 1, -(L + 1), 2 * L + 3, -(2 * L + 3), -50 * L]


def planted(L, step=0):
    """one point per cell, distinct heights / variances / colours: (index, cr, cg, cb, inten, h, v)"""
    n = L * L
    i = np.arange(n)
    h = (0.25 + 0.001 * ((i * 37 + 11 * step) % 997) + 0.5 * step).astype(F)
    v = (0.01 + 0.0001 * (i % 13)).astype(F)
    return i.astype(np.int32), 1 + (i + step) % 255, 1 + (2 * i + step) % 255, 1 + (3 * i + step) % 255, (0.1 + (i % 9) / 10).astype(F), h, v


def fill_all(m, L, step=0):
    p = planted(L, step)
    m.fuse(*p)
    return p


def refill_empty(m, L, elevation, step):
    """plant new points in the empty cells only: first hits, so the cell takes exactly the planted height"""
    p = planted(L, step)
    sel = elevation == -10
    if sel.any():
        m.fuse(*[a[sel] for a in p])
    return p, sel


def walk_shifts(L, seed, steps=40):
    """random cell shifts in -(L-1) .. L-1 on both axes at once; asserts that `start` wraps round at least three times per axis"""
    rng = np.random.default_rng(seed)
    s = rng.integers(-(L - 1), L, (steps, 2))
    s[::7] = 0, 3          # some single-axis steps too
    start, wraps = np.zeros(2, int), np.zeros(2, int)
    for d in s:
        wraps += (start - d < 0) | (start - d >= L)
        start = (start - d) % L
    assert (wraps >= 3).all()
    return s


def survivors(L, elevation, start, cells, new_start):
    """Independent of any Move code: the elevation layer (storage layout) after a shift of `cells` (2 ints, |.| < L): the cell
    at a world position keeps its height when that position lay in the old window and lies in the new one, everything else is
    empty.  Grid row i of a window centred on cell c looks at world cell c - i (+ a constant)."""
    old = elevation.reshape(L, L)
    new = np.full((L, L), -10, F)
    g = np.arange(L)
    for a in g:
        for b in g:
            oa, ob = a - cells[0], b - cells[1]      # new centre c + d, new row a:  (c + d) - a = c - oa
            if 0 <= oa < L and 0 <= ob < L:
                new[(a + new_start[0]) % L, (b + new_start[1]) % L] = old[(oa + start[0]) % L, (ob + start[1]) % L]
    return new.reshape(-1)


def run_move_single(m, L, axis, cells):
    """fill, features (so that traver is set), one Move; returns the Move outputs and the five layers"""
    m.move([0, 0, 1.0])
    fill_all(m, L)
    m.map_feature()
    pos = [0.0, 0.0, 1.25]
    pos[axis] = MOVE_RES * cells
    return [("move", m.move(pos)), ("layers", layers(m)), ("feature", m.map_feature())]


def run_move_walk(m, L, seed):
    out = []
    c, _ = m.frame()
    for step, d in enumerate(walk_shifts(L, seed)):
        refill_empty(m, L, m.layer(1), step)
        m.map_feature()
        c = np.asarray(c, np.float64) + d * MOVE_RES
        mv = m.move([c[0], c[1], 1.0 + 0.01 * step])
        c = mv[0]
        out += [("move", mv), ("layers", layers(m))]
    return out


# ------------------------------------------------------------------------------------------------ Process_points
POINTS_RES = 0.2
FAR = (-1234.6, 987.4)


def points_setup(m, far):
    """leave the map at the origin, or carry it to about FAR (loop-closure shift, defined for any distance) and then Move it by
    (+7, -5) cells so that `start` is wrapped on both axes"""
    if far:
        m.map_closeloop(FAR, 0.0)
        c, _ = m.frame()
        return m.move([c[0] + 7 * POINTS_RES, c[1] - 5 * POINTS_RES, 0.9])
    return m.move([0.0, 0.0, 0.9])


def _index_of(oracle, L, frame, k, u, v):
    m = oracle.ElevMap(L, POINTS_RES)
    m.set_frame(frame[0], frame[1], 0.9)
    xs, ys = to_sensor(k, u, v)
    return process(m, xs, ys, np.zeros(xs.size, F), transform(k, 0.9, frame[0]))["map_index"]


def border_points(oracle, L, frame, k, axis, fixed):
    """Points one float either side of every cell border along `axis` (the other coordinate fixed), the two map edges
    included, and one more float out on each side: found by bisecting the restatement's own index arithmetic between the
    centres of neighbouring cells.  Coordinates are offsets from the map centre, where the sensor stands (see points_calls): the
    floats meant are those of the sensor-frame input, which the four headings only copy or negate.  (For even L the index truncates towards zero, so grid cell 0 is two cells wide and the map
    edge lies a cell further out: the search starts two cells outside and keeps the pairs that do differ.)
    Returns (wx, wy) and the number of borders, L + 1; four points per border, in border order."""
    i = np.arange(-2, L + 1)
    lo, hi = cell_centre(L, POINTS_RES, 0.0, i), cell_centre(L, POINTS_RES, 0.0, i + 1)

    def idx(p):
        other = np.full(p.size, fixed, F)
        return _index_of(oracle, L, frame, k, *((p, other) if axis == 0 else (other, p)))
    differ = idx(lo) != idx(hi)
    lo, hi = lo[differ], hi[differ]
    assert lo.size == L + 1
    want = idx(lo)
    for _ in range(64):
        mid = ((lo.astype(np.float64) + hi) / 2).astype(F)
        done = (mid == lo) | (mid == hi)
        if done.all():
            break
        same = idx(mid) == want
        lo = np.where(same & ~done, mid, lo)
        hi = np.where(~same & ~done, mid, hi)
    assert done.all() and (np.nextafter(lo, hi) == hi).all() and (idx(hi) != want).all()
    p = np.stack([np.nextafter(lo, 2 * lo - hi), lo, hi, np.nextafter(hi, 2 * hi - lo)], 1).reshape(-1).astype(F)
    o = np.full(p.size, fixed, F)
    return ((p, o) if axis == 0 else (o, p)), lo.size


def points_calls(oracle, L, far):
    """[(name, x, y, z, T)] in the sensor frame, for a map after points_setup(m, far).  The sensor stands at the map centre
    (T's translation), 0.9 m up, under one of the four headings; the scenario is laid out in offsets from that centre, which a
    heading only copies or negates into sensor coordinates.  A heading sees one half plane (the filter keeps y <= -1 only)."""
    scratch = oracle.ElevMap(L, POINTS_RES)
    points_setup(scratch, far)
    frame = scratch.frame()
    cx = cy = 0.0
    res = POINTS_RES
    rng = np.random.default_rng(100 * L + far)
    half = (L / 2 + 1.5) * res
    pose = iter([0, 1, 2, 3] * 25)
    calls = []

    def world_call(name, wx, wy, wz, k):
        xs, ys = to_sensor(k, wx, wy)
        calls.append((name, xs.copy(), ys.copy(), np.asarray(wz, F), transform(k, 0.9, frame[0])))

    def cloud(n):
        wx = (cx + rng.uniform(-half, half, n)).astype(F)
        wy = (cy + rng.uniform(-half, half, n)).astype(F)
        return wx, wy, rng.uniform(-1.2, -0.2, n).astype(F)

    one = (cell_centre(L, res, cx, 3), cell_centre(L, res, cy, L - 4))        # a corner region heading 0 sees
    world_call("n1", [one[0]], [one[1]], [-0.5], 0)
    for n in (255, 256, 257):
        world_call("n%d" % n, *cloud(n), next(pose))
    calls.append(("rejected", rng.uniform(-5, 5, 300).astype(F), rng.uniform(0.1, 5, 300).astype(F), rng.uniform(-1, 0, 300).astype(F),
                  transform(0, 0.9)))
    wx, wy, wz = cloud(6000)
    gx, gy = rng.integers(2, 5, 500), rng.integers(L - 6, L - 3, 500)               # 500 points crowd a 3 x 3 block of cells:
    wx[:500] = cell_centre(L, res, cx, gx) + rng.uniform(-0.05, 0.05, 500).astype(F)  # the sequential `lowest` rule sees heights
    wy[:500] = cell_centre(L, res, cy, gy) + rng.uniform(-0.05, 0.05, 500).astype(F)  # that fall, then rise
    wz[:500] = (-0.3 - 0.9 * np.abs(np.linspace(-1, 1, 500)) + rng.normal(0, 0.05, 500)).astype(F)
    world_call("n6000", wx, wy, wz, 0)
    world_call("n7", *cloud(7), 0)
    g = np.arange(L)
    for side, rows in enumerate(((0, -1, -2), (L - 1, L, L + 1))):                  # edge cells, one and two cells beyond; four sides
        across = np.concatenate([np.full(L, a) for a in rows])
        along = np.tile(g, 3)
        ez = rng.uniform(-1, 0, across.size).astype(F)
        world_call("edge_x%d" % side, cell_centre(L, res, cx, across), cell_centre(L, res, cy, along), ez, (1, 3)[side])
        world_call("edge_y%d" % side, cell_centre(L, res, cx, along), cell_centre(L, res, cy, across), ez, (2, 0)[side])
    kx, ky = 0, 1
    (bx, by), nb = border_points(oracle, L, frame, kx, 0, cell_centre(L, res, cy, L - 10))
    world_call("border_x", bx, by, np.full(bx.size, -0.4, F), kx)
    (bx, by), _ = border_points(oracle, L, frame, ky, 1, cell_centre(L, res, cx, 8))
    world_call("border_y", bx, by, np.full(bx.size, -0.4, F), ky)
    return calls


def run_points(m, far, calls):
    out = [("move", points_setup(m, far))]
    for name, xs, ys, zs, T in calls:
        out += [(name, process(m, xs, ys, zs, T)), (name + ".lowest", m.layer(0))]
    return out


# ------------------------------------------------------------------------------------------------ Fuse
def fuse_hand_case(L=8):
    """One cell (19) walked through every branch of the per-cell rule, its points interleaved with those of other cells and
    with ignored indices.  Rows: (index, R, G, B, intensity, height, variance)."""
    c, cells = 19, L * L
    rows = [
        (c, 10, 20, 30, 0.5, 1.0, 0.01),          # first hit
        (20, 1, 2, 3, 0.1, 0.3, 0.02),            # another cell in between
        (c, 11, 21, 31, 0.6, 1.2, 0.02),          # inlier (distance 2 sigma): blend, takes the colour
        (-1, 99, 99, 99, 0.9, 9.0, 0.01),         # index -1: ignored
        (c, 12, 22, 32, 0.7, 3.0, 0.015),         # higher outlier: replaces
        (cells, 98, 98, 98, 0.9, 9.0, 0.01),      # index L*L: ignored
        (c, 13, 23, 33, 0.8, 0.5, 0.01),          # lower outlier: ignored, colour not taken
        (c, 14, 24, 34, 0.9, -1.0, 0.01),         # height -1 with a valid index: skipped
        (20, 4, 5, 6, 0.2, 0.35, 0.02),
        (c, 0, 25, 35, 0.95, 3.05, 0.02),         # inlier with one zero colour channel: height taken, colour kept
        (c, 16, 26, 36, 0.0, 2.95, 0.02),         # inlier with zero intensity: height taken, colour kept
        (c, 17, 0, 37, 0.3, 9.0, 0.03),           # higher outlier, uncoloured: replaces, colour kept
        (c, 18, 28, 0, 0.3, 8.9, 0.03),           # inlier, uncoloured
        (63, 7, 8, 9, 0.4, -1.0, 0.01),           # a cell whose only point is skipped stays empty
        (0, 5, 5, 5, 0.0, 0.7, 0.00001),          # uncoloured first hit, variance below the floor
    ]
    a = np.array(rows, np.float64)
    return (a[:, 0].astype(np.int32), a[:, 1].astype(np.int32), a[:, 2].astype(np.int32), a[:, 3].astype(np.int32),
            a[:, 4].astype(F), a[:, 5].astype(F), a[:, 6].astype(F))


def fuse_crowded(seed, L=8, n=3000):
    """3000 points in cell 27 of an otherwise sparse map, interleaved with 200 points over the other cells"""
    rng = np.random.default_rng(seed)
    idx = np.full(n + 200, 27, np.int32)
    other = rng.choice(n + 200, 200, replace=False)
    idx[other] = rng.integers(0, L * L, 200)
    h = rng.normal(1.0, 0.05, n + 200).astype(F)
    v = rng.uniform(0.005, 0.02, n + 200).astype(F)
    cr, cg, cb, it = colours_for(rng, n + 200)
    dull = rng.random(n + 200) < 0.2
    cr[dull] = 0
    return idx, cr.astype(np.int32), cg.astype(np.int32), cb.astype(np.int32), it, h, v


def fuse_call_sets():
    """{name: [fuse call, ...]}; between the first and the second call of a set the tests run mapvar_update(2e-4)"""
    hand, crowd = fuse_hand_case(), fuse_crowded(1)
    perm = np.random.default_rng(2).permutation(crowd[0].size)
    return {"hand": [hand], "hand twice": [hand, hand], "crowded": [crowd], "permuted": [tuple(a[perm] for a in crowd)],
            "n1": [tuple(a[:1] for a in hand)], "crowded then hand": [crowd, hand]}


def fuse_numpy(L, state, call):
    """The per-cell rule of G_fuse read sequentially in float32 numpy.  state = [elevation, variance, intensity, R, G, B]
    (changed in place); returns how often the higher- and the lower-outlier branch were taken."""
    e, v, it, r, g, b = state
    hi = lo = 0
    for c, pr, pg, pb, pi, h, hv in zip(*call):
        if c < 0 or c >= L * L or h == F(-1):
            continue
        take = True
        if e[c] == F(-10):
            e[c], v[c] = h, hv
        elif np.abs(h - e[c]) / np.sqrt(v[c]) > F(5):
            take = e[c] < h
            hi, lo = hi + take, lo + (not take)
            if take:
                e[c], v[c] = h, hv
        else:
            e[c], v[c] = (v[c] * h + hv * e[c]) / (v[c] + hv), (hv * v[c]) / (hv + v[c])
        if take and pr != 0 and pg != 0 and pb != 0 and pi != F(0):
            it[c], r[c], g[c], b[c] = pi, pr, pg, pb
    v[v.astype(np.float64) < 0.0001] = F(0.0001)
    return hi, lo


def empty_state(L):
    n = L * L
    return [np.full(n, -10, F), np.full(n, -10, F), np.zeros(n, F), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)]


def fused_state(m):
    """[elevation, variance, intensity, R, G, B] of a map (colours through map_feature)"""
    f = m.map_feature()
    return [m.layer(1), m.layer(2), m.layer(3), f["colorR"], f["colorG"], f["colorB"]]


# ------------------------------------------------------------------------------------------------ Map_feature
FEATURE_RES = 0.2


def feature_scene(L, start):
    """(fuse arguments, filled-cell count per 5 x 5 window) of a scene laid out in grid coordinates, L >= 20: rolling terrain
    over grid rows 0-7 (its windows are cut by three map edges), an isolated 7-cell and an isolated 8-cell patch (3 x 3 blocks
    with 2 / 1 cells missing: every cell of a patch sees exactly the patch, the `pn > 7` threshold from both sides), a full
    3 x 3 block in one far corner and a 7-cell patch in the other."""
    rng = np.random.default_rng(7 * L + int(start[0]) + 3 * int(start[1]))
    filled = np.zeros((L, L), bool)
    filled[0:8, :] = True
    blk = np.ones((3, 3), bool)
    seven, eight = blk.copy(), blk.copy()
    seven[0, 0] = seven[2, 1] = False
    eight[1, 2] = False
    filled[11:14, 2:5] = seven
    filled[11:14, 10:13] = eight
    filled[L - 3:, L - 3:] = blk
    filled[L - 3:, 0:3] = seven
    gx, gy = np.nonzero(filled)
    h = (0.3 * np.sin(0.9 * gx * FEATURE_RES * 5) + 0.2 * np.cos(0.7 * gy * FEATURE_RES * 5) + rng.normal(0, 0.03, gx.size)).astype(F)
    pn = np.zeros((L, L), int)
    for a in range(L):
        for b in range(L):
            pn[a, b] = filled[max(a - 2, 0):a + 3, max(b - 2, 0):b + 3].sum() if filled[a, b] else 0
    assert (pn == 7).sum() >= 14 and (pn == 8).sum() >= 8 and (pn == 9).sum() >= 9
    idx = storage_index(L, start, gx, gy).astype(np.int32)
    cr, cg, cb, it = colours_for(rng, gx.size)
    v = rng.uniform(0.001, 0.01, gx.size).astype(F)
    order = rng.permutation(gx.size)
    call = tuple(a[order] for a in (idx, cr, cg, cb, it, h, v))
    pn_storage = np.zeros(L * L, int)
    pn_storage[idx] = pn[gx, gy]
    return call, pn_storage


# Worst |slope - float64 eigen answer| of the reference host build (float Jacobi, stops at an off-diagonal of 0.01) over the interior
# cells of the four planes below: 3.731e-3 rad, measured by tests/test_oracle_elev.py (which asserts it); rounded up.
PLANE_SLOPE_REF_DEVIATION = 3.74e-3
PLANE_TILTS = ((0.0, 0.0), (0.15, 20.0), (0.3, 115.0), (0.5, 250.0))       # (tilt in rad, direction of steepest ascent in degrees)


def plane_scene(L, tilt, direction):
    """every cell at z = a x + b y over the kernel's own cell coordinates (storage index * resolution, start = 0)"""
    a, b = np.tan(tilt) * np.cos(np.radians(direction)), np.tan(tilt) * np.sin(np.radians(direction))
    i = np.arange(L * L)
    x, y = (i // L) * F(FEATURE_RES), (i % L) * F(FEATURE_RES)
    h = (a * x.astype(np.float64) + b * y.astype(np.float64)).astype(F)
    return (i.astype(np.int32), i % 200 + 1, i % 100 + 1, i % 50 + 1, np.full(i.size, 0.5, F), h, np.full(i.size, 0.01, F)), (a, b)


def plane_slopes_f64(L, elevation):
    """slope = angle between the smallest-eigenvalue direction of the 5 x 5 patch's covariance and z, in float64, for the
    interior cells (rows / columns 2 .. L-3); same patch points as the kernel: (index * resolution, height)"""
    E = elevation.reshape(L, L).astype(np.float64)
    out = np.zeros((L - 4, L - 4))
    for a in range(2, L - 2):
        for b in range(2, L - 2):
            gx, gy = np.meshgrid(np.arange(a - 2, a + 3), np.arange(b - 2, b + 3), indexing="ij")
            P = np.stack([gx.reshape(-1) * np.float64(F(FEATURE_RES)), gy.reshape(-1) * np.float64(F(FEATURE_RES)), E[a - 2:a + 3, b - 2:b + 3].reshape(-1)], 1)
            P = P - P.mean(0)
            w, V = np.linalg.eigh(P.T @ P)
            out[a - 2, b - 2] = np.arccos(min(1.0, abs(V[2, 0])))
    return out


def interior(L, layer):
    return layer.reshape(L, L)[2:L - 2, 2:L - 2]


def run_features(m, L, wrapped):
    mv = m.move([3 * FEATURE_RES, -6 * FEATURE_RES, 1.0] if wrapped else [0.0, 0.0, 1.0])
    call, _ = feature_scene(L, mv[1])
    m.fuse(*call)
    m.mapvar_update(1e-4)
    return [("move", mv), ("feature", m.map_feature()), ("layers", layers(m))]


def run_plane(m, L, tilt, direction):
    m.fuse(*plane_scene(L, tilt, direction)[0])
    return m.map_feature()


# ------------------------------------------------------------------------------------------------ Raytracing
RAY_RES = 0.5
RAY_STARTS = {"zero": (0, 0), "wrap_x": (3, 0), "wrap_y": (0, -4), "wrap_xy": (-5, 2)}     # the first Move, in cells


def ray_scene(L, central):
    """World points of one frame around a robot at the map centre (grid cell r = (L-1)//2 on both axes), sensor 1 m up:
    flat ground wherever the sensor can see (everything outside the 1.5 m box, i.e. 3 cells), except beyond a wall 7 rows out;
    the wall (1.5 m high, nothing observed behind it: it must stay); single cells hanging 0.8 m up with ground seen behind
    them, in all four quadrants, on the four exact diagonals, and on the robot's own row and column (where the reference
    returns early and keeps them).  Returns (wx, wy, wz, {name: [(gx, gy)]})."""
    r = (L - 1) // 2
    rng = np.random.default_rng(L)
    quad = [(sa * a, sb * b) for sa in (1, -1) for sb in (1, -1) for a, b in ((4, 2), (2, 5), (5, 3), (3, 5))]
    diag = [(s * d, t * d) for s in (1, -1) for t in (1, -1) for d in (4, 5)]
    axis = [(0, 4), (0, -5), (-4, 0), (5, 0)]
    floating = {"quadrant": [(r + a, r + b) for a, b in quad], "diagonal": [(r + a, r + b) for a, b in diag],
                "axis": [(r + a, r + b) for a, b in axis]}
    wall = [(r + 7, r + b) for b in range(-6, 7)]
    hanging = set(sum(floating.values(), []))
    px, py, pz = [], [], []
    for a in range(L):
        for b in range(L):
            if max(abs(a - r), abs(b - r)) <= 3 or a >= r + 7:
                continue
            if (a, b) in hanging:
                px.append(a); py.append(b); pz.append(0.8)
            else:
                for _ in range(2):
                    px.append(a); py.append(b); pz.append(rng.uniform(-0.03, 0.03))
    for a, b in wall:
        for z in (1.5, 1.45, 1.55):
            px.append(a); py.append(b); pz.append(z)
    px, py = np.array(px), np.array(py)
    jitter = rng.uniform(-0.1, 0.1, (2, px.size))
    wx = cell_centre(L, RAY_RES, central[0], px) + jitter[0].astype(F)
    wy = cell_centre(L, RAY_RES, central[1], py) + jitter[1].astype(F)
    order = rng.permutation(px.size)
    return wx[order], wy[order], np.array(pz, F)[order], dict(floating, wall=wall)


def ray_prepare(m, L, start_name):
    """bring a map to the state Raytracing starts from; returns (sensor_z, scene cells, frame)"""
    d = RAY_STARTS[start_name]
    mv = m.move([d[0] * RAY_RES, d[1] * RAY_RES, 1.0])
    m.raytracing()                                   # on the empty map: only sets `lowest` to its "nothing seen" value 10
    wx, wy, wz, cells = ray_scene(L, mv[0])
    rng = np.random.default_rng(5)
    _, cat = observe(m, wx, wy, wz, origin=mv[0])
    m.fuse(cat["map_index"], *colours_for(rng, wx.size), cat["z_ts"], cat["var"])
    m.mapvar_update(1e-4)
    m.map_feature()
    return 1.0, cells, (mv[0], mv[1])


def run_ray(m, L, start_name):
    _, cells, frame = ray_prepare(m, L, start_name)
    before = layers(m)
    m.raytracing()
    return before, layers(m), cells, frame


def ray_outcome(before, after, obstacle=0.6):
    """(obstacle mask, cleared mask) in storage layout, from the five layers before and after Raytracing"""
    obstacle_cells = (before[4] < obstacle) & (before[1] != -10)
    return obstacle_cells, obstacle_cells & (after[1] == -10)


# ------------------------------------------------------------------------------------------------ two maps
def small_frame(m, rng, k, pose, n=1500):
    """one frame of a session, every stage once; returns everything the frame produced"""
    pose[:2] += rng.uniform(-0.5, 0.7, 2).astype(F)
    out = [m.move(pose)]
    x = rng.uniform(-6, 6, n).astype(F)
    y = rng.uniform(-7, 2, n).astype(F)
    z = (0.15 * np.sin(0.8 * x) + 0.1 * np.cos(1.1 * y) - 0.6 + rng.normal(0, 0.02, n)).astype(F)
    yaw = 0.1 * k
    T = np.eye(4, dtype=F)
    T[:2, :2] = [[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]]
    T[:3, 3] = [pose[0], pose[1], 0.9]
    res = process(m, x, y, z, T)
    out.append(res)
    m.fuse(res["map_index"], *colours_for(rng, n), res["z_ts"], res["var"])
    m.mapvar_update(1e-4)
    out.append(m.map_feature())
    m.raytracing()
    out.append(layers(m))
    if k == 1:
        out.append(m.map_optmove(pose[:2] + F(0.33), 0.05))
    if k == 2:
        m.map_closeloop(pose[:2] - F(0.41), -0.02)
    out.append(m.frame())
    return out


def flatten(out):
    """every array of a nested result, in order"""
    if isinstance(out, dict):
        return [a for k in sorted(out) for a in flatten(out[k])]
    if isinstance(out, (list, tuple)):
        return [a for o in out for a in flatten(o)]
    return [np.asarray(out)]
