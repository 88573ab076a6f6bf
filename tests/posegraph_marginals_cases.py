"""Cases for the tests of the pose-graph optimiser's marginal covariances (test_posegraph_marginals_cpu.py, test_posegraph_marginals_gpu.py,
test_posegraph_marginals_adapter.py), and per case the bound of the comparison against the restatement
(tests/golden/posegraph_marginals_restate.py), computed once per process on the CPU from the restatement alone and never written to.

A case is a scene of posegraph_cases.py (unit model, Gauss-Newton) or a case of posegraph_robust_cases.py (covariances, a kernel on the
loops, the optimiser it is meant for).  Beyond those: panel scenes whose reduced order 6 E, at an unbounded segment length, lies one block
below, at and one block above one and two widths of the tile of the reduced system's inverse (MRS_PGO_MARGINAL_TILE); the dense
Cholesky's panel width is covered by the panel scenes of posegraph_cases.py.

The bound of a case is FACTOR times the spread between the restatement's two exact routes to the inverse (numpy.linalg.inv, and a Cholesky
factorisation of the system in reverse pose order) at the restatement's own result, in the measure max |a - b| / max |b| over the whole
inverse.  The spread is taken as at least SPREAD_FLOOR: on the smallest scenes the two routes agree to the last bits by chance, which says
nothing about a third elimination order.  FACTOR = 100 covers that third order (segments, then panels) on systems of condition 1e7 to
1e10."""
import collections
import functools

import numpy as np

import posegraph_cases as PC
import posegraph_robust_cases as RC
import posegraph_marginals_restate as MR  # noqa: E402  (posegraph_cases puts tests/golden on the path)

R, RR = PC.R, RC.RR
FACTOR, SPREAD_FLOOR = 100.0, 1e-12
SEGMENT_LENGTHS = PC.SEGMENT_LENGTHS
Case = collections.namedtuple("Case", "name scene oC lC kernel k method max_solves")


def tile_separator_counts():
    """E such that 6 E lies one block below, at and one block above one and two widths of the inverse's tile"""
    tile = PC.header_int("MRS_PGO_MARGINAL_TILE")
    out = set()
    for w in (1, 2):
        if (w * tile) % 6 == 0:
            out.update(w * tile // 6 + d for d in (-1, 0, 1))
        else:
            out.update((w * tile // 6, w * tile // 6 + 1))
    return sorted(e for e in out if e >= 1)


# a scene that breaks a condition of test_posegraph_marginals_cpu.py gets another seed here, never a skip
_TILE_SEEDS = {10: 50, 11: 51}
TILE_NAMES = tuple("panel_E%d" % e for e in tile_separator_counts())
PLAIN_NAMES = tuple(n for n in PC.NAMES if sum(PC.scene(n).chain_lengths) >= 2) + ("quirks_prior",) + tuple(n for n in TILE_NAMES if n not in PC.NAMES)
GN_NAMES = RC.GN_NAMES
LM_NAMES = ("outliers_geman_mcclure", "outliers_cauchy", "outliers_huber")      # the last at its BOUNDED_SOLVES: whatever result stands
NAMES = PLAIN_NAMES + GN_NAMES + LM_NAMES


@functools.lru_cache(maxsize=None)
def case(name):
    if name in GN_NAMES or name in LM_NAMES:
        c = RC.case(name)
        return Case(name, c.scene, c.oC, c.lC, c.kernel, c.k, "lm" if name in LM_NAMES else "gn", c.max_solves)
    if name == "quirks_prior":
        s = PC.with_prior()
    elif name in PC.NAMES:
        s = PC.scene(name)
    else:
        e = int(name[7:])
        s = PC._panel_scene(e, _TILE_SEEDS.get(e, 40 + e))
    return Case(name, s, None, None, RR.NONE, 1.0, "gn", None)


def _args(c):
    s = c.scene
    return s.chain_lengths, s.odom, s.li, s.lj, s.lZ


@functools.lru_cache(maxsize=None)
def expected_result(name):
    """(T, T0, w) of the restatement: the result, the stage-1 poses, the loops' weights at the result"""
    c = case(name)
    s = c.scene
    if name in LM_NAMES:
        r = RC.expected_lm(name)
        T, w = r.T, r.weights
    elif name in GN_NAMES:
        T, w = RC.expected_gn(name).T, np.ones(s.li.size)
    elif name in PC.NAMES or name == "quirks_prior":
        T, w = PC.expected(name).T, np.ones(s.li.size)
    else:
        T, w = R.optimize(*_args(c), prior=s.prior).T, np.ones(s.li.size)
    T0, _ = PC.expected_initial(name) if name in PC.NAMES or name == "quirks_prior" else R.initialize(*_args(c), prior=s.prior)
    return T, T0, w


def information_matrix(name, T, T0, w):
    c = case(name)
    return MR.information_matrix(T, T0, *_args(c), oC=c.oC, lC=c.lC, w=w)


@functools.lru_cache(maxsize=None)
def routes(name):
    """(H, the inverse by numpy.linalg.inv, the inverse by the reversed Cholesky) at the restatement's own result"""
    H = information_matrix(name, *expected_result(name))
    return H, MR.inverse_direct(H), MR.inverse_cholesky_reversed(H)


@functools.lru_cache(maxsize=None)
def two_route_spread(name):
    _, a, b = routes(name)
    return MR.spread(b, a)


def bound(name):
    return FACTOR * max(two_route_spread(name), SPREAD_FLOOR)


def reference(name, T, T0, w):
    """Sigma [6 N]^2 of the optimiser's tangent, pose 0 included as zeros, from results of the handle under test"""
    return MR.with_held_pose(MR.inverse_direct(information_matrix(name, T, T0, w)))
