"""Inputs, references and the derived allowance shared by tests/test_preprocess_cases_cpu.py (the cases are what they claim, the references
agree with each other, an integer emulation of the batch arithmetic stays inside the allowance) and tests/test_preprocess_edges_gpu.py (the
comparisons with the kernels of csrc/preprocess.hip).  No test functions and no GPU import here.  Everything is computed once per process
and shared read-only (functools.lru_cache).

Structure (sizes, run layouts, planted thresholds, bucket collisions) is built WITHOUT random numbers, so MRS_FUZZ_SEED_OFFSET, which shifts
integer seeds, cannot dissolve it; only the lidar filler of `shifted` / `negative_coords` comes from integer seeds.  No cloud exceeds 4 100
points except the two headroom cases.

The references:
  voxel_exact       the contract: index = floor((p - (min - v/2)) / v) in double, mean = the exactly rounded mean (rational arithmetic), voxels
                    in order of first occurrence
  voxel_sequential  stable sort by (ix, iy, iz), sums in input order from 0.0, one division: the IEEE operations of k_voxel_means in its
                    order (the library is built with -ffp-contract=off), so the single-scan form is compared with it BIT FOR BIT
  batch_bound       the allowance of the hash-grid batch form against voxel_exact, DERIVED from the launch code (see its docstring)
  batch_emulate     the batch arithmetic in integers (llrint offsets, Python-int sums, the emit expression)
  crop_restate      util.py:91-112 in numpy float32
  the approximate grid is judged by oracle.approx_voxel_grid, itself checked on these cases against the closed form of
  tests/test_oracle_voxel.py.  Its inputs keep |coordinate / leaf| < 2^20 and are finite: beyond that pcl::ApproximateVoxelGrid casts an
  out-of-range float to int, which is undefined behaviour in the reference filter itself, so there is nothing to compare with.
"""
import functools
import math
from fractions import Fraction

import numpy as np

VOXELS = (0.2, 0.25)
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1025)
PATTERNS = ("one_voxel", "alternating", "distinct", "runs")
LEAVES = (0.2, 1.0)
AVG_SIZES = (1, 2, 511, 512, 513, 1025)
AVG_PATTERNS = ("own_bucket", "evicting", "one_voxel", "negative", "on_leaf", "f64_values")
SHIFT = (1000.0, -2000.0, 50.0)                 # the translation of tests/pointfeat_cases.py: about 2.2 km
SHIFTED_HALF_WIDTH = 40.0                       # the filler of `shifted` is cut to |y| < 40 before the shift
STRIDES = (3, 4, 7)
ACCURACY = 1e-12                                # the project's stated accuracy of the centroids
EXTENT = 1 << 21                                # voxel indices per axis
WAVE = 64
F32 = np.float32


def _ro(x):
    x.setflags(write=False)
    return x


# ---- voxel grid: inputs ------------------------------------------------------------------------------------------------------------------

ANCHOR = np.array([-3.7, 1.3, -0.9])            # the minimum bound of every structured cloud: it sits at the centre of voxel (0, 0, 0)


def _in_voxel(idx, i, v):
    """a point of voxel idx (per axis >= 0): 0.5 to 0.82 of a voxel above the voxel's lower face, far from both faces in float32 too; point 0
    is the anchor itself"""
    i = np.asarray(i)
    d = np.stack([(i * 7) % 5, (i * 3) % 5, i % 5], -1) * 0.08
    return ANCHOR + (np.asarray(idx, np.float64) + d) * v


def run_lengths(n):
    """1, 2, ..., 6, 1, 2, ... cut off at n points.  A cycle holds 21 points and a wave 64 = 3 x 21 + 1: point 63 is a single-point run on
    lane 63.  The cycle restarts once there, so point 64 is a single-point run on lane 0 and point 127 another on lane 63; from then on the
    layout drifts by a lane per wave: a run from lane 0 (128-129), runs that straddle a wave edge (191-192) and a workgroup edge, longer runs
    that end on lane 63.  tests/test_preprocess_cases_cpu.py checks the positions"""
    out, pos, k = [], 0, 1
    while pos < n:
        out.append(min(k, n - pos))
        pos += k
        k = 1 if pos == 64 else k % 6 + 1
    return out


def run_ids(n):
    """run number of each of n points"""
    return np.repeat(np.arange(len(run_lengths(n))), run_lengths(n))


def pattern_voxels(pattern, n):
    """voxel index [n,3] of each point of a structured cloud"""
    i = np.arange(n)
    if pattern == "one_voxel":
        return np.zeros((n, 3), np.int64)
    if pattern == "alternating":
        return np.where((i % 2 == 0)[:, None], np.array([0, 0, 0]), np.array([3, 1, 2]))
    if pattern == "distinct":
        return np.stack([i % 11, (i // 11) % 11, i // 121], -1)
    if pattern == "runs":                       # seven voxels in turn: neighbouring runs differ, and every voxel is met again by later runs
        a = run_ids(n) % 7
        return np.stack([a, (2 * a) % 3, a % 2], -1)
    raise KeyError(pattern)


@functools.lru_cache(maxsize=None)
def pattern_cloud(pattern, n, v):
    return _ro(_in_voxel(pattern_voxels(pattern, n), np.arange(n), v))


@functools.lru_cache(maxsize=None)
def faces(v):
    """the anchor, then on each axis in turn the faces ANCHOR + (k + 0.5) v as computed in double, with the neighbouring double on each side"""
    rows = [ANCHOR.copy()]
    for a in range(3):
        for k in range(13):
            f = ANCHOR[a] + (k + 0.5) * v
            for x in (np.nextafter(f, -np.inf), f, np.nextafter(f, np.inf)):
                p = ANCHOR + np.array([0.3, 0.3, 0.3]) * v
                p[a] = x
                rows.append(p)
    return _ro(np.array(rows))


@functools.lru_cache(maxsize=None)
def _lidar(seed, n):
    from mr_slam_amd import synth
    return _ro(np.ascontiguousarray(synth.lidar_scan(seed, n, metric=True), np.float64))


@functools.lru_cache(maxsize=None)
def substep():
    """voxel 0.25, coordinates below 0.25: the anchor at 0 and one point alone in voxel (1, 1, 1) whose offset from the voxel's lower corner is
    (K + 115/128) steps of the 2^-48 m fixed-point grid.  Round-to-nearest leaves 13/128 of a step, truncation 115/128: with coordinates this
    small the double roundings of the allowance are far below a step, so this case tells the two apart"""
    step = 2.0 ** -48
    x = 0.125 + (14073748835532 + 115 / 128) * step          # 0.125 + ~0.05: exact in double (multiples of 2^-55 below 0.25)
    assert 0.17 < x < 0.18 and (x - 0.125) / step % 1 == 115 / 128
    return _ro(np.array([[0.0, 0.0, 0.0], [x, x, x]]))


@functools.lru_cache(maxsize=None)
def headroom(n):
    """voxel 0.25: one point at the minimum bound (the centre of voxel (0, 0, 0)), n - 1 at the last double below the voxel's upper corner on
    all three axes: every offset fills the whole 2^bits range (0.25 is a power of two) and all of them meet in one sum"""
    lo = np.array([3.125, -1.875, 0.125])
    hi = np.nextafter(lo + 0.125, -np.inf)
    p = np.tile(hi, (n, 1))
    p[0] = lo
    return _ro(p)


def _extent(delta, axis):
    """good points about the anchor and one point `delta` voxels further along `axis` than the anchor"""
    p = _in_voxel(pattern_voxels("distinct", 6), np.arange(6), 0.2)
    far = ANCHOR + np.array([0.1, 0.1, 0.1])
    far[axis] = ANCHOR[axis] + (delta + 0.2) * 0.2
    return np.concatenate([p[:3], far[None], p[3:]])


@functools.lru_cache(maxsize=None)
def voxel_cases():
    """{name: (float64 [n,3], voxel)}: the clouds that both forms of the exact voxel grid accept"""
    z = {}
    for v in VOXELS:
        for pat in PATTERNS:
            for n in SIZES:
                z["%s_n%d_v%g" % (pat, n, v)] = (pattern_cloud(pat, n, v), v)
        z["faces_v%g" % v] = (faces(v), v)
        z["faces_f32_v%g" % v] = (_ro(faces(v).astype(F32).astype(np.float64)), v)
    small = _lidar(411, 1500)
    small = _ro(small[np.abs(small[:, 1]) < SHIFTED_HALF_WIDTH])     # whatever the seed: |y - 2000| stays below 2048, one binade of ulps
    z["shifted"] = (_ro(small + np.asarray(SHIFT)), 0.2)
    z["shifted_f32"] = (_ro((small.astype(F32) + np.asarray(SHIFT, F32)).astype(np.float64)), 0.2)
    z["negative_coords"] = (_ro(_lidar(412, 1500) - np.array([200.0, 200.0, 50.0])), 0.2)
    for a, ax in enumerate("xyz"):
        z["extent_ok_" + ax] = (_ro(_extent(EXTENT - 1, a)), 0.2)
    z["substep"] = (substep(), 0.25)
    z["headroom_2p17"] = (headroom(1 << 17), 0.25)
    z["headroom_2p17_plus1"] = (headroom((1 << 17) + 1), 0.25)
    return z


LIDAR_RANGE = 128.0                             # |coordinate| below this: where DESIGN.md states 1e-12


def at_lidar_range(p):
    return float(np.abs(p).max()) < LIDAR_RANGE


@functools.lru_cache(maxsize=None)
def refused_cases():
    """{name: (float64 [n,3], voxel, rejected count)}: clouds that both forms must refuse with MrsError, naming the count.  The count follows
    from the contract: the minimum bound ignores NaN (fmin), and a point is rejected when its index on some axis is NaN or outside [0, 2^21).
    A coordinate of -inf is the minimum bound itself, so every point of that cloud is rejected"""
    z = {}
    for a, ax in enumerate("xyz"):
        z["extent_bad_" + ax] = (_ro(_extent(EXTENT, a)), 0.2, 1)
    good = _in_voxel(pattern_voxels("distinct", 70), np.arange(70), 0.2)
    for name, val, cnt in (("nan_point", np.nan, 1), ("inf_point", np.inf, 1), ("neg_inf_point", -np.inf, 70)):
        for a, ax in enumerate("xyz"):
            p = good.copy()
            p[37, a] = val
            z["%s_%s" % (name, ax)] = (_ro(p), 0.2, cnt)
    return z


def rejected_count(p, v):
    """the contract's count of points a call must refuse (0 = accepted)"""
    with np.errstate(invalid="ignore"):
        mn = np.fmin.reduce(p, 0)
        f = np.floor((p - (mn - v * 0.5)) / v)
        return int((~((f >= 0) & (f < EXTENT))).any(1).sum())


@functools.lru_cache(maxsize=None)
def voxel_batches():
    """{name: (tuple of float64 [n_b,3] scans, voxel)}"""
    E = _ro(np.zeros((0, 3)))
    c = lambda pat, n, v=0.2: pattern_cloud(pat, n, v)
    z = {
        "empties": ((E, c("runs", 65), E, E, c("alternating", 64), c("distinct", 63), E), 0.2),
        "only_empty_but_one": ((E, E, c("one_voxel", 2), E), 0.2),
        "ones": (tuple(_ro(c("distinct", 8)[i:i + 1] * (1 + i)) for i in range(6)) + (c("distinct", 2),), 0.2),
        "b1": ((c("runs", 257, 0.25),), 0.25),
        "b65_tiny": (tuple(_ro(c("distinct", 9)[: i % 5] + 0.37 * i) for i in range(65)), 0.2),
        "patterns": ((c("runs", 1025), c("one_voxel", 257), c("alternating", 255), c("distinct", 1025), faces(0.2)), 0.2),
        "patterns_v0.25": ((c("distinct", 256, 0.25), c("runs", 255, 0.25), faces(0.25), substep()), 0.25),
    }
    return z


EMPTY_BATCH = (0, 0, 0, 0)                      # raw offsets of a batch with total 0: three empty scans


def forms(p32):
    """{(dtype, stride): array [n, stride]} of the same float32 values: the columns past xyz hold NaN, which no kernel may read as a coordinate"""
    p32 = np.asarray(p32, F32)
    out = {}
    for dt in ("float32", "float64"):
        for s in STRIDES:
            a = np.full((p32.shape[0], s), np.nan, dt)
            a[:, :3] = p32
            out[dt, s] = a
    return out


# ---- voxel grid: references ----------------------------------------------------------------------------------------------------------------

def voxel_indices(p, v):
    p = np.asarray(p, np.float64)
    return np.floor((p - (p.min(0) - v * 0.5)) / v).astype(np.int64)


def _exact_mean(col):
    u, c = np.unique(col, return_counts=True)
    s = sum((Fraction(float(x)) * int(k) for x, k in zip(u, c)), Fraction(0))
    return float(s / int(c.sum()))               # float(Fraction) rounds once, correctly


def voxel_exact(p, v):
    """(means float64 [m,3], indices int64 [m,3]) in order of first occurrence"""
    p = np.asarray(p, np.float64)
    idx = voxel_indices(p, v)
    uniq, first, inv = np.unique(idx, axis=0, return_index=True, return_inverse=True)
    inv = inv.reshape(-1)
    order = np.argsort(first, kind="stable")
    means = np.empty((len(uniq), 3))
    members = np.argsort(inv, kind="stable")
    bounds = np.r_[0, np.cumsum(np.bincount(inv, minlength=len(uniq)))]
    for g in range(len(uniq)):
        rows = p[members[bounds[g]:bounds[g + 1]]]
        means[g] = [_exact_mean(rows[:, a]) for a in range(3)]
    return means[order], uniq[order]


def voxel_sequential(p, v):
    """(means float64 [m,3], indices int64 [m,3]) sorted by (ix, iy, iz): the _np_voxel_down_sample of tests/test_preprocess_gpu.py"""
    p = np.asarray(p, np.float64)
    idx = voxel_indices(p, v)
    order = np.lexsort((idx[:, 2], idx[:, 1], idx[:, 0]))
    idx, ps = idx[order], p[order]
    head = np.ones(len(p), bool)
    head[1:] = (idx[1:] != idx[:-1]).any(1)
    seg = np.cumsum(head) - 1
    out = np.zeros((seg[-1] + 1, 3))
    np.add.at(out, seg, ps)                     # unbuffered: one addition per point, in input order within a voxel
    return out / np.bincount(seg)[:, None], idx[head]


def batch_bits(longest):
    """the fixed-point bits voxel_downsample_batch_impl gives a batch whose longest scan has `longest` points"""
    pbits = 1
    while pbits < 31 and (1 << pbits) < longest:
        pbits += 1
    return 46 if pbits <= 17 else 62 - pbits


def batch_step(v, longest):
    """one step of the fixed-point grid, in metres: 1 / scale"""
    return 2.0 ** (math.ceil(math.log2(v)) - batch_bits(longest))


def batch_bound(p, v, longest=None):
    """|batch form - voxel_exact| per coordinate, from the code of k_vox_insert / k_vox_emit, not from their output.

    A voxel's lower corner C = o + f v is one double, computed by the same expression in both kernels, and x = C + (x - C) holds exactly in
    the reals, so only the offsets carry error:
      llrint((x - C) scale)       at most half a step of 1 / scale = 2^(ceil(log2 v) - bits) per point, hence per mean; the multiplication
                                  by a power of two is exact and the integer sum is exact
      x - C                       one rounding
      (double)sum, / scale, / c   two roundings (the scale is a power of two)
      C + mean offset             one rounding
    Each of the four is at most HALF an ulp of the largest magnitude involved (coordinates, corners, one voxel); they are charged a whole ulp
    each, which also pays for the half ulp of the correctly rounded reference"""
    p = np.asarray(p, np.float64)
    longest = p.shape[0] if longest is None else longest
    big = max(float(np.abs(p).max()), float(np.abs(p.min(0) - v * 0.5).max()), v)
    return 0.5 * batch_step(v, longest) + 4 * float(np.spacing(big))


def _wrap64(s):
    return (s + (1 << 63)) % (1 << 64) - (1 << 63)


def batch_emulate(p, v, longest=None, bits=None, mutate=None):
    """(means float64 [m,3] in order of first occurrence, largest bit length of a sum).  The sums are Python ints; the emit takes them modulo
    2^64 as the 64-bit atomics would, so a sum of 64 bits or more shows as a wrong mean as well.  `bits` overrides the launch code's choice and
    `mutate` in ("float32_offset", "truncate") alters one step: the mutations tests/test_preprocess_cases_cpu.py needs the cases to catch"""
    p = np.asarray(p, np.float64)
    longest = p.shape[0] if longest is None else longest
    bits = batch_bits(longest) if bits is None else bits
    scale = math.ldexp(1.0, bits - math.ceil(math.log2(v)))
    o = p.min(0) - 0.5 * v
    f = np.floor((p - o) / v)
    corner = o + f * v
    off = p - corner
    if mutate == "float32_offset":
        off = off.astype(F32).astype(np.float64)
    q = (np.trunc if mutate == "truncate" else np.rint)(off * scale)
    sums, count, corners = {}, {}, {}
    for i, key in enumerate(map(tuple, f.astype(np.int64))):
        s = sums.setdefault(key, [0, 0, 0])
        for a in range(3):
            s[a] += int(q[i, a])
        count[key] = count.get(key, 0) + 1
        corners.setdefault(key, corner[i])
    means = np.array([[corners[k][a] + (float(_wrap64(sums[k][a])) / scale) / float(count[k]) for a in range(3)] for k in sums])
    width = max(abs(x).bit_length() for s in sums.values() for x in s)
    return means, width


# ---- approximate grid ----------------------------------------------------------------------------------------------------------------------

def avg_hash(vox):
    """bucket of pcl::ApproximateVoxelGrid's 512-entry history for voxel indices [n,3]"""
    vox = np.asarray(vox, np.int64)
    return (vox[:, 0] * 7171 + vox[:, 1] * 3079 + vox[:, 2] * 4231) & 511


def avg_voxels(p, leaf):
    """the filter's voxel indices: floor(float32 point x float32 inverse leaf)"""
    return np.floor(np.asarray(p, F32) * (F32(1) / F32(leaf))).astype(np.int64)


@functools.lru_cache(maxsize=None)
def avg_cloud(pattern, n, leaf):
    """float64 [n,3].  All but `f64_values` hold float32 values"""
    i = np.arange(n)
    frac = np.stack([0.3 + 0.05 * (i % 7), 0.4 + 0.05 * (i % 5), 0.5 + 0.05 * (i % 3)], -1)      # 0.3 .. 0.65 of a leaf inside the voxel
    if pattern == "own_bucket":                  # 7171 is odd: ix -> 7171 ix mod 512 is a bijection of 0 .. 511
        vox = np.stack([i % 512, 0 * i, 0 * i], -1)
    elif pattern == "evicting":                  # 7171 x 512 = 0 mod 512: both voxels live in bucket 0
        vox = np.stack([(i % 2) * 512, 0 * i, 0 * i], -1)
    elif pattern == "one_voxel":
        vox = np.tile([2, -3, 1], (n, 1))
    elif pattern == "negative":                  # floor differs from truncation; the hash is negative before the mask
        vox = np.stack([-1 - (i // 3) % 9, -1 - (i // 2) % 4, -1 - i % 3], -1)
        frac = np.where((i % 5 == 0)[:, None], 0.95, frac)     # -0.05 leaf: floor -1, truncation 0
    elif pattern == "on_leaf":                   # exact multiples of the leaf, as float32 has them
        vox = np.stack([i % 17 - 8, (i // 2) % 9 - 4, (i // 3) % 5 - 2], -1)
        frac = np.zeros((n, 3))
    elif pattern == "f64_values":                # doubles that are not float32 values: the kernel's cast must round as numpy's does
        vox = np.stack([(i // 4) % 23 - 11, (i // 2) % 7, i % 3 - 1], -1)
        return _ro((vox + frac) * leaf + 1e-9 * (1 + i % 13)[:, None])
    else:
        raise KeyError(pattern)
    return _ro(((vox + frac) * leaf).astype(F32).astype(np.float64))


@functools.lru_cache(maxsize=None)
def avg_cases():
    """{name: (float64 [n,3], leaf)}"""
    return {"%s_n%d_l%g" % (pat, n, leaf): (avg_cloud(pat, n, leaf), leaf) for leaf in LEAVES for pat in AVG_PATTERNS for n in AVG_SIZES}


# ---- crop / scale ------------------------------------------------------------------------------------------------------------------------

def crop_restate(pc):
    """util.py:91-112: float32 [m,3]"""
    pc = np.array(pc, dtype=F32)
    keep = (np.abs(pc[:, 0]) < 70.) & (np.abs(pc[:, 1]) < 70.) & (pc[:, 2] < 30.) & (pc[:, 2] > 0.)
    h = pc[keep][:, :3].copy()
    h[:, 0] = h[:, 0] / 70.
    h[:, 1] = h[:, 1] / 70.
    h[:, 2] = h[:, 2] / 30.
    return h


GOOD = (1.5, -2.5, 3.5)
TINY = float(np.nextafter(F32(0), F32(1)))      # the smallest float32 subnormal


def _nb32(x):
    x = F32(x)
    return float(np.nextafter(x, F32(-np.inf))), float(x), float(np.nextafter(x, F32(np.inf)))


@functools.lru_cache(maxsize=None)
def crop_plants():
    """[(name, (x, y, z) doubles, kept)]: every threshold of every axis, exactly and at the float32 neighbour on each side, the doubles that
    round onto a threshold, signed zero, subnormals and non-finite values.  `kept` is what the contract says of the float32 cast"""
    rows = []

    def plant(name, axis, value, kept):
        p = list(GOOD)
        p[axis] = value
        rows.append((name, tuple(p), kept))

    for a, ax in ((0, "x"), (1, "y")):
        for sgn, sn in ((1.0, "+"), (-1.0, "-")):
            lo, at, hi = _nb32(70.0)
            plant("%s%s70_inside" % (ax, sn), a, sgn * lo, True)
            plant("%s%s70_exact" % (ax, sn), a, sgn * at, False)
            plant("%s%s70_outside" % (ax, sn), a, sgn * hi, False)
            # float32 spacing below 70 is 2^-17 = 7.6e-6: a double closer than half of it rounds ONTO 70 and is dropped
            plant("%s%s70_rounds_on" % (ax, sn), a, sgn * (70.0 - 3.0e-6), False)
            plant("%s%s70_rounds_in" % (ax, sn), a, sgn * (70.0 - 4.5e-6), True)
        plant("%s_zero" % ax, a, 0.0, True)
        plant("%s_negzero" % ax, a, -0.0, True)
    lo, at, hi = _nb32(30.0)
    plant("z30_inside", 2, lo, True)
    plant("z30_exact", 2, at, False)
    plant("z30_outside", 2, hi, False)
    plant("z30_rounds_on", 2, 30.0 - 0.9e-6, False)      # spacing below 30 is 2^-19 = 1.9e-6
    plant("z30_rounds_in", 2, 30.0 - 1.2e-6, True)
    plant("z0_exact", 2, 0.0, False)
    plant("z0_negzero", 2, -0.0, False)
    plant("z0_subnormal", 2, TINY, True)
    plant("z0_neg_subnormal", 2, -TINY, False)
    plant("z0_double_1e-50", 2, 1e-50, False)            # casts to 0.0f
    plant("z0_smallest_normal", 2, float(np.finfo(F32).tiny), True)
    for a, ax in enumerate("xyz"):
        for name, val in (("nan", np.nan), ("+inf", np.inf), ("-inf", -np.inf)):
            plant("%s_%s" % (ax, name), a, val, False)
    return tuple(rows)


@functools.lru_cache(maxsize=None)
def crop_planted_block():
    return _ro(np.array([p for _, p, _ in crop_plants()], np.float64))


def _kept_scan(n):
    i = np.arange(n)
    return np.stack([-60.0 + 0.11 * i, 55.0 - 0.07 * i, 0.5 + 0.02 * (i % 1000)], -1)


def _dropped_scan(n):
    p = _kept_scan(n)
    p[np.arange(n), np.arange(n) % 3] = np.array([75.0, -71.0, -0.5])[np.arange(n) % 3]
    return p


@functools.lru_cache(maxsize=None)
def crop_batches():
    """{name: tuple of float64 [n_b,3] scans}"""
    E = np.zeros((0, 3))
    K, D, M = _kept_scan(300), _dropped_scan(257), crop_planted_block()
    z = {"planted": (M,), "b1_all_dropped": (_dropped_scan(65),)}
    kinds = (K, D, E)
    for r in range(3):                           # each of kept / dropped / empty at the start, in the middle and at the end
        z["ends_%d" % r] = (kinds[r], M, K, D, E, E, M, kinds[(r + 1) % 3])
    for B in (255, 256, 257):                    # batch + 1 offsets straddle the 256 threads of k_out_offsets
        scans = []
        for b in range(B):
            n = (b * 5 + b // 7) % 4
            p = _kept_scan(3)[:n] + 0.01 * b
            if n and b % 3 == 0:
                p[0, 2] = -1.0
            scans.append(p)
        z["b%d_tiny" % B] = tuple(scans)
    return {k: tuple(_ro(np.array(s, np.float64)) for s in v) for k, v in z.items()}


def pack(scans, dtype="float64", stride=3):
    """(points [N, stride] with NaN past xyz, raw offsets int64 [B+1])"""
    offs = np.concatenate([[0], np.cumsum([s.shape[0] for s in scans])]).astype(np.int64)
    pts = np.full((int(offs[-1]), stride), np.nan, dtype)
    if offs[-1]:
        pts[:, :3] = np.concatenate(scans)
    return pts, offs
