"""Scenes for the pose-graph tests of per-factor noise, Levenberg-Marquardt step control and robust loop kernels
(test_posegraph_robust_cpu.py, test_posegraph_robust_gpu.py, test_posegraph_robust_adapter.py), and the restatement's results on them
(tests/golden/posegraph_robust_restate.py), computed once per process and never written to.

A case is a scene of posegraph_cases.py plus covariances (`oC` per odometry factor or None, `lC` a list with a covariance or None per
loop), a kernel on the loops and the optimiser it is meant for.  The sizes are the smallest at which each mechanism can go wrong."""
import collections
import functools

import numpy as np

import posegraph_cases as PC
import posegraph_robust_restate as RR  # noqa: E402  (posegraph_cases puts tests/golden on the path)

R = PC.R
Case = collections.namedtuple("Case", "name scene oC lC kernel k methods max_solves", defaults=(None,))
KERNEL_NAMES = {RR.NONE: None, RR.HUBER: "huber", RR.CAUCHY: "cauchy", RR.GEMAN_MCCLURE: "geman_mcclure"}
REFERENCE_LOOP_COVARIANCE = np.diag([1e-1, 1e-1, 1e-1, 1e-2, 1e-2, 1e-2])        # global_manager.cpp:103-109
REFERENCE_ODOMETRY_COVARIANCE = np.eye(6)
UNIT_COVARIANCE = np.diag([1.0, 1.0, 1.0, 0.99, 0.99, 0.99])                     # 0.99 + 0.01 == 1.0 in fp64: every weight is exactly 1
assert 0.99 + 0.01 == 1.0


def covariance(rng, anisotropy=1.0):
    """a full symmetric positive definite 6 x 6: rotation variances of 0.003 .. 0.1, a translation block with off-diagonal terms whose
    axes differ by up to `anisotropy` orders of magnitude"""
    A = rng.normal(0, 1, (6, 6))
    Q, _ = np.linalg.qr(A)
    s = np.concatenate([10.0 ** rng.uniform(-2.5, -1, 3), 10.0 ** rng.uniform(-2 - anisotropy, -2 + anisotropy, 3)])
    C = np.zeros((6, 6))
    Qr, _ = np.linalg.qr(rng.normal(0, 1, (3, 3)))
    Qt, _ = np.linalg.qr(rng.normal(0, 1, (3, 3)))
    C[:3, :3] = Qr @ np.diag(s[:3]) @ Qr.T
    C[3:, 3:] = Qt @ np.diag(s[3:]) @ Qt.T
    C[:3, 3:] = 0.01 * Q[:3, :3] * np.sqrt(s[:3, None] * s[None, 3:])           # ignored by the conversion, as the reference ignores it
    C[3:, :3] = C[:3, 3:].T
    return 0.5 * (C + C.T)


def _covs(seed, n, anisotropy=1.0):
    rng = np.random.default_rng(seed)
    return np.array([covariance(rng, anisotropy) for _ in range(n)]).reshape(n, 6, 6)


def _base():
    """3 x 30 poses with 12 loops"""
    return PC.make("r3x30", 77, (30, 30, 30), PC._random_loops(7, (30, 30, 30), 8, 4))


# a scene that breaks a condition of test_posegraph_robust_cpu.py gets another seed or loop here, never a skip
INCONSISTENT_LOOP, INCONSISTENT_SEED = 4, 3
OUTLIER_LOOPS = (9, 10, 11)
# kernel, k and the seed of the outliers' draws.  Geman-McClure and Cauchy (with a k small enough to redescend) take the outliers' weights
# to zero and converge.  Huber cannot reject 5 m outliers at the reference's noise (a loop's information is 50 times an odometry factor's,
# so k r stays below what the chains would pay); what is left is the large-residual problem, which no seed, k in 0.1 .. 10 or milder outlier
# brought to max|delta| < 1e-9 within 500 solves.  That case runs BOUNDED_SOLVES solves: it checks the arithmetic, not the convergence.
OUTLIER_KERNELS = {"huber": (RR.HUBER, 1.345, 4), "cauchy": (RR.CAUCHY, 0.3, 3), "geman_mcclure": (RR.GEMAN_MCCLURE, 1.0, 4)}
BOUNDED_SOLVES = 20


def _perturbed(s, loops, sigma_t, sigma_r, seed):
    """the loops named, right-multiplied by pose(N(0, sigma_r, 3), N(0, sigma_t, 3)) drawn in list order; sigma_r = 0 draws no rotation"""
    rng = np.random.default_rng(seed)
    lZ = s.lZ.copy()
    for u in loops:
        rv = rng.normal(0, sigma_r, 3) if sigma_r else np.zeros(3)
        lZ[u] = lZ[u] @ PC.pose(rv, rng.normal(0, sigma_t, 3))
    return s._replace(lZ=lZ)


@functools.lru_cache(maxsize=None)
def case(name):
    none = RR.NONE
    if name == "r3x2_noisy":                                     # 3 chains x 2 poses, 3 noisy loops, noisy odometry
        s = PC.scene("r3x2")
        return Case(name, s, _covs(1, 3), list(_covs(2, 3)), none, 1.0, ("gn", "lm"))
    if name == "chain70":                                        # a cut pose (segment lengths 1, 3, 64) carries weighted factors
        s = PC.make(name, 73, (70,), [(3, 40), (20, 68), (0, 33)])
        return Case(name, s, _covs(3, 69), list(_covs(4, 3)), none, 1.0, ("gn", "lm"))
    if name == "roles":
        # noisy loops onto pose 0 as i and as j, loops given with i > j (the first pose's Rhat is used), the same pair twice with
        # different covariances
        s = PC.scene("quirks")
        lC = list(_covs(5, s.li.size))
        assert (s.li[0], s.lj[0]) == (s.li[2], s.lj[2]) and not np.allclose(lC[0], lC[2])
        return Case(name, s, _covs(13, s.odom.shape[0]), lC, none, 1.0, ("gn", "lm"))
    if name == "anisotropic":                                    # translation axes three orders apart, off-diagonal terms, any yaw
        s = PC.make(name, 81, (12, 10), [(2, 17), (9, 13), (0, 11)])
        return Case(name, s, _covs(6, 20, 1.5), list(_covs(7, 3, 1.5)), none, 1.0, ("gn", "lm"))
    if name == "mixed":                                          # only some factors carry noise
        s = PC.scene("r3x64")
        lC = [c if u % 2 == 0 else None for u, c in enumerate(_covs(8, s.li.size))]
        return Case(name, s, None, lC, none, 1.0, ("gn", "lm"))
    if name == "mixed_odometry":                                 # noisy odometry, unit loops
        s = PC.scene("r3x64")
        return Case(name, s, _covs(9, s.odom.shape[0]), None, none, 1.0, ("gn",))
    if name == "inconsistent":                                   # one loop 0.3 m off: full Gauss-Newton steps do not converge
        return Case(name, _perturbed(_base(), (INCONSISTENT_LOOP,), 0.3, 0.0, INCONSISTENT_SEED), None, None, none, 1.0, ("lm",))
    if name.startswith("outliers_"):                             # three gross outliers, the reference's noise, a kernel
        kind, k, seed = OUTLIER_KERNELS[name[9:]]
        s = _perturbed(_base(), OUTLIER_LOOPS, 5.0, 0.5, seed)
        oC = np.tile(REFERENCE_ODOMETRY_COVARIANCE, (s.odom.shape[0], 1, 1))
        return Case(name, s, oC, [REFERENCE_LOOP_COVARIANCE] * s.li.size, kind, k, ("lm",), BOUNDED_SOLVES if kind == RR.HUBER else None)
    if name in ("r3x2", "quirks"):                               # step control alone
        return Case(name, PC.scene(name), None, None, none, 1.0, ("lm",))
    raise KeyError(name)


NAMES = ("r3x2_noisy", "chain70", "roles", "anisotropic", "mixed", "mixed_odometry", "inconsistent", "outliers_huber", "outliers_cauchy",
         "outliers_geman_mcclure", "r3x2", "quirks")
LM_NAMES = tuple(n for n in NAMES if "lm" in case(n).methods)
GN_NAMES = tuple(n for n in NAMES if "gn" in case(n).methods)


def _args(c):
    s = c.scene
    return s.chain_lengths, s.odom, s.li, s.lj, s.lZ


@functools.lru_cache(maxsize=None)
def expected_lm(name, order=None, max_solves=None):
    c = case(name)
    max_solves = max_solves or c.max_solves or RR.MAX_SOLVES_DEFAULT
    return RR.lm_optimize(*_args(c), prior=c.scene.prior, oC=c.oC, lC=c.lC, kernel=c.kernel, k=c.k, order=order, max_solves=max_solves)


@functools.lru_cache(maxsize=None)
def expected_gn(name, order=None):
    c = case(name)
    return RR.gn_optimize(*_args(c), prior=c.scene.prior, oC=c.oC, lC=c.lC, order=order)
