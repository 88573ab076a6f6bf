"""Scan Context inputs, expected values and the comparison rule shared by tests/test_sc_cases_cpu.py (the conditions the cases must meet,
checked on the restatement alone) and tests/test_sc_shapes_gpu.py (the comparisons with the kernels of csrc/scancontext.hip).  No test
functions here.  Everything is seeded, built once per process (functools.lru_cache) and shared read-only.

Expected values come from tests/golden/sc_restate.py, the fp64 restatement of the reference's ScanContext.py, which the CPU tests pin to
fixtures the reference itself wrote (ref_scancontext.npz at 120 x 120, ref_scancontext_geom.npz at five other geometries).

The comparison rule is that of the existing Scan Context tests (tests/test_scancontext_gpu.py::_check_align), with its tolerances:
  dist    within 1e-5: the kernel and the reference both work in float32
  shift   exact where both stages have a clear winner: the smallest sector-key norm leads by more than 1e-6 relative and the smallest
          window dist by more than 1e-5, or the minimum is an exact tie, which goes to its first occurrence
  else    the dist at the GPU's shift equals the restated dist at that shift within 1e-5 (the weaker branch)
Two kinds of case never compare the shift (never_exact):
  R = 1   every engaged column's cosine is 1 up to float32 rounding, so every window dist is 0 up to rounding: an exact tie in fp64 is
          none in float32
  Z vs A  the sector keys of the zero descriptor are 0, so every shift's score is the norm of the same numbers in another order: equal
          in exact arithmetic, and apart by the rounding of whichever order an implementation sums in.  No s* is determined.
Outside those, at most MAX_WEAK of the (geometry, pair, ratio) cases may take the weaker branch; test_sc_cases_cpu.py asserts it.
"""
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.join(HERE, "golden") not in sys.path:
    sys.path.insert(0, os.path.join(HERE, "golden"))
import sc_restate as R  # noqa: E402

TOL_DIST, TOL_KEY, REL_NORM, ABS_NORM = 1e-5, 1e-6, 1e-9, 1e-12        # the existing Scan Context tests' tolerances
MAX_WEAK = 0.05

# (num_ring, num_sector)
GEOMETRIES = [(1, 1), (2, 1), (128, 1),            # smallest shapes
              (1, 128),                            # one row: every engaged column's cosine is 1
              (2, 2), (5, 10),                     # small, general
              (7, 50),                             # odd R, a radius tie (0.1 x 50)
              (20, 60),                            # the paper's geometry, a radius tie (0.15 x 60)
              (3, 63), (64, 64), (127, 65),        # the wave edge in S; uneven halves 64 + 63
              (33, 90),                            # a radius tie (0.1 x 90)
              (119, 120), (121, 120),              # just off the R = 120 template
              (120, 60), (120, 128),               # the R = 120 template with S != 120
              (128, 128)]                          # largest: 80 KiB of dynamic LDS, 256 window sums at the widest window
PINNED = [(7, 50), (20, 60), (33, 90), (5, 10), (127, 65)]       # the geometries of ref_scancontext_geom.npz

# (search_ratio, num_sector, the reference's round(0.5 * ratio * S), what rounding the float32 ratio gives): every product is x.5 in double
RADIUS_TABLE = [(0.1, 10, 0, 1), (0.1, 50, 2, 3), (0.1, 90, 4, 5), (0.15, 60, 4, 5), (0.2, 25, 2, 3), (0.3, 70, 10, 11), (0.7, 50, 18, 17),
                (0.075, 120, 4, 5), (0.225, 120, 14, 13)]

PAIR_NAMES = ["roll3", "roll-2", "noisy1", "noisy_half", "other0", "other1", "ZZ", "ZA", "AZ", "AA", "tiny", "period"]
NEVER_EXACT_PAIRS = ("ZA",)
KNOWN_SSTAR = {"roll3": lambda S: 3 % S, "roll-2": lambda S: (S - 2) % S, "ZZ": lambda S: 0, "AZ": lambda S: 0, "AA": lambda S: 0,
               "period": lambda S: 0}          # pairs whose pre-alignment is planted (exact ties included): the window is known in closed form
TINY = 1e-25                                   # its square underflows to 0 in float32


def ratios(S):
    """(label, search_ratio): 0 -> the window {s*}; radius 8 and 16 -> 17 and 33 shifts, one past a chunk of 16 and one past two; 4.0 ->
    the radius is clamped and the window clipped to all of [-S, S)"""
    return [("0", 0.0), ("0.1", 0.1), ("0.15", 0.15), ("0.3", 0.3), ("r8", 16.0 / S), ("r16", 32.0 / S), ("1", 1.0), ("4", 4.0)]


def radius(ratio, S):
    return round(0.5 * ratio * S)


def window(sstar, ratio, S):
    """the reference's shift_idx_search_space"""
    r = radius(ratio, S)
    return range(max(-S, sstar - r), min(S, sstar + r + 1))


def _ro(x):
    x.setflags(write=False)
    return x


def descriptor(rng, R_, S):
    """sparse positive float32 [R, S], about half the cells zero"""
    return (rng.random((R_, S)) * (rng.random((R_, S)) > 0.5)).astype(np.float32)


def noisy(rng, d):
    """tests/golden/make_golden_scancontext.py's noise: on the occupied cells only, clipped to [1e-3, 1]"""
    return np.where(d > 0, np.clip(d + rng.normal(0, 0.01, d.shape), 1e-3, 1.0), 0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def pairs(geom):
    """{name: (sc1, sc2)} float32 [R, S] of one geometry; `period` only for even S"""
    R_, S = geom
    rng = np.random.default_rng([2024, R_, S])
    base = [descriptor(rng, R_, S) for _ in range(9)]
    A = base[0]
    Z = np.zeros_like(A)
    out = {"roll3": (np.roll(base[1], 3 % S, axis=-1), base[1]),               # sc1 = roll(sc2, k): s* = k, dist 0 there
           "roll-2": (np.roll(base[2], (S - 2) % S, axis=-1), base[2]),        # the window runs into S and is clipped
           "noisy1": (noisy(rng, np.roll(base[3], 1 % S, axis=-1)), base[3]),
           "noisy_half": (noisy(rng, np.roll(base[4], S // 2, axis=-1)), base[4]),
           "other0": (base[5], base[6]), "other1": (base[7], base[8]),
           "ZZ": (Z, Z), "ZA": (Z, A), "AZ": (A, Z), "AA": (A, A)}
    # columns of 1e-25 on both sides: empty to the float32 norm the reference takes, not to an fp64 one
    t2 = base[5].copy()
    t1 = noisy(rng, np.roll(t2, 2 % S, axis=-1))
    t2[:, sorted({0, S // 3, S - 1})] = TINY
    t1[:, sorted({1 % S, S // 2})] = TINY
    out["tiny"] = (t1, t2)
    if S % 2 == 0:
        half = descriptor(rng, R_, S // 2)
        P = np.concatenate([half, half], axis=1)
        assert np.array_equal(P[:, :S // 2], P[:, S // 2:])
        out["period"] = (P, P)                  # sector keys of period S / 2: shifts 0 and S / 2 tie exactly, 0 must win
    return {k: (_ro(a), _ro(b)) for k, (a, b) in out.items()}


def pair_names(geom):
    return [n for n in PAIR_NAMES if n in pairs(geom)]


def batch(geom):
    """(names, sc1 [n, R, S], sc2 [n, R, S]) of every pair of a geometry, in PAIR_NAMES order"""
    names = pair_names(geom)
    P = pairs(geom)
    return names, np.stack([P[n][0] for n in names]), np.stack([P[n][1] for n in names])


class Align:
    """what the restatement gives for dist_align_sc(sc1, sc2, ratio)"""
    __slots__ = ("dist", "shift", "start", "wd", "nrm", "ratio")

    def __init__(self, sc1, sc2, ratio):
        self.dist, self.shift, self.start, self.wd, self.nrm = R.dist_align(sc1, sc2, ratio)
        self.ratio = ratio


@functools.lru_cache(maxsize=None)
def expected(geom):
    """{pair name: {"direct": dist, "distance": (dist, yaw), "align": {ratio label: Align}}}"""
    out = {}
    for name, (a, b) in pairs(geom).items():
        out[name] = {"direct": float(R.window_dists(a, b, [0])[0]), "distance": R.distance_sc(a, b),
                     "align": {lab: Align(a, b, r) for lab, r in ratios(geom[1])}}
    return out


def never_exact(geom, name):
    return geom[0] == 1 or name in NEVER_EXACT_PAIRS


def exact_shift(exp):
    """the condition of _check_align's strong branch"""
    return bool(R.clear_winner(exp.nrm, int(np.argmin(exp.nrm)), rel=1e-6) and R.clear_winner(exp.wd, int(np.argmin(exp.wd)), abs_=TOL_DIST))


def check_align(gpu_dist, gpu_shift, sc1, sc2, exp, exact_allowed=True):
    """tests/test_scancontext_gpu.py::_check_align against an Align; -> whether the shift was compared exactly"""
    S = sc1.shape[-1]
    assert abs(gpu_dist - exp.dist) < TOL_DIST, (gpu_dist, exp.dist)
    assert -S <= gpu_shift < S, gpu_shift
    if exact_allowed and exact_shift(exp):
        assert gpu_shift == exp.shift, (gpu_shift, exp.shift)
        return True
    assert abs(gpu_dist - R.window_dists(sc1, sc2, [gpu_shift])[0]) < TOL_DIST, (gpu_dist, gpu_shift)
    return False


# ------------------------------------------------------------------------------------------------------------------------ sector keys
KEY_LENGTHS = [1, 2, 63, 64, 65, 127, 128]


@functools.lru_cache(maxsize=None)
def key_pairs(length):
    """(names, key1 [n, len], key2 [n, len]) float32: random and unrelated; a noisy roll; constant keys (every shift scores 0: shift 0);
    keys of period len / 2 for even len (shifts 0 and len / 2 score exactly 0: shift 0)"""
    rng = np.random.default_rng([77, length])
    a, b = rng.random(length).astype(np.float32), rng.random(length).astype(np.float32)
    c = rng.random(length).astype(np.float32)
    names, k1, k2 = ["random", "rolled", "constant"], [a, (np.roll(c, 5 % length) + rng.normal(0, 1e-3, length)).astype(np.float32),
                                                       np.full(length, 0.375, np.float32)], [b, c, np.full(length, 0.375, np.float32)]
    if length % 2 == 0:
        h = rng.random(length // 2).astype(np.float32)
        names.append("period"); k1.append(np.concatenate([h, h])); k2.append(np.concatenate([h, h]))
    return names, _ro(np.stack(k1)), _ro(np.stack(k2))


# ------------------------------------------------------------------------------------------------- more pairs than workgroups, (7, 50)
MANY_GEOM = (7, 50)
MANY_RATIO = 0.1                                # the radius tie of that geometry
MANY_BASE = PAIR_NAMES[:6]


def many_pair(i):
    """pair i: the six seeded pairs in turn, sc2 rolled by i // 6 sectors (so the expected shift moves with i)"""
    a, b = pairs(MANY_GEOM)[MANY_BASE[i % 6]]
    return a, np.roll(b, (i // 6) % MANY_GEOM[1], axis=-1)


@functools.lru_cache(maxsize=None)
def many_expected(which, roll):
    a, b = many_pair(which + 6 * roll)
    return Align(a, b, MANY_RATIO)


# ------------------------------------------------------------------------------------------------------------- the 120 x 120 database
DB_STAGES = (1, 255, 256, 257, 513)             # the edges of the nearest-key sweep's 256-entry chunk and of its merge
DB_KS = (1, 10, 64)
DB_DUPLICATE = (40, 300)                        # entry 300 is entry 40 again: their key distances tie, the lower index comes first
DB_RATIO = 0.1


@functools.lru_cache(maxsize=None)
def _db_distinct():
    """64 distinct descriptors derived from the 120 x 120 fixture's non-zero ones (rolled, re-weighted), like the existing tests' _distinct"""
    g = R.load()
    base = [d[0] for d in g["sc"] if d.any()]
    out = []
    for i in range(64):
        d = np.roll(base[i % len(base)], (7 * i) % 120, axis=-1)
        out.append((d * (1.0 + 0.05 * (i // len(base)))).astype(np.float32))
    return _ro(np.stack(out))


def db_entry(e):
    if e == DB_DUPLICATE[1]:
        e = DB_DUPLICATE[0]
    return (_db_distinct()[e % 64] * np.float32(1.0 + 0.01 * (e // 64))).astype(np.float32)


def db_queries():
    """{name: descriptor}: a stored entry (key distance 0), the duplicated entry (an exact tie of two key distances at 0, from 301
    entries on), a fixture descriptor that is not stored, and the zero descriptor"""
    g = R.load()
    names = list(g["names"])
    return {"stored": db_entry(0), "duplicate": db_entry(DB_DUPLICATE[0]), "S12": g["sc"][names.index("S12")][0],
            "zero": np.zeros((120, 120), np.float32)}


@functools.lru_cache(maxsize=None)
def db_expected(e, qname):
    return Align(db_entry(e), db_queries()[qname], DB_RATIO)
