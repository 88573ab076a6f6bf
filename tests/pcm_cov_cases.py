"""Inputs shared by the tests of pairwise consistency with covariances (test_pcm_cov_cpu.py, test_pcm_cov_gpu.py, test_pcm_cov_adapter.py):
the two-robot scenes with odometry and loop covariances and the restatement's results for them (tests/golden/pcm_cov_restate.py: the direct
covariance chain), computed once per process and never written to."""
import functools

import numpy as np

import pcm_cases as PC

import pcm_cov_restate as RC  # noqa: E402  (pcm_cases puts tests/golden on the path)

R = PC.R
N_POSES = 40
SIZES = PC.SIZES                     # (1, 2, 63, 64, 65, 129)
MODES = ("span", "reference")
THRESHOLDS = (16.812, 7.840)         # chi2_upper(0.99) and chi2_threshold(0.75)
INLIER_SHARE = 0.6

# Relative tolerance on d2 and on Sigma_E (largest entry difference over the largest entry).  Measured, not chosen: the largest relative
# deviation of the g++ build of pcm_cov.hpp (world-frame prefixes) from the direct-chain restatement over scene(L) for L in SIZES and both
# modes was 2.154e-12, rounded up to 2.2e-12 (d2: 2.154e-12, Sigma_E: 2.8e-14; test_pcm_cov_cpu.py prints and re-checks it), times 4 for
# another order of fp64 sums on the device.  d2 deviates more than Sigma_E because of xi, not of the covariance: the two builds take the
# cycle pose in another order of products, which moves xi by up to 2.7e-13 in absolute terms (poses lie up to 100 m from the origin), and
# an inlier pair has an xi of a few centimetres and milliradians.
MEASURED_REL = 2.2e-12
TOL_REL = 4 * MEASURED_REL
MARGIN_REL = 10 * TOL_REL            # no d2 of a test scene lies within MARGIN_REL * threshold of a threshold (test_pcm_cov_cpu.py checks that)
# The cancellation scene (400 poses, 33 loops, SPAN): the prefix difference W_j - W_i cancels there.  Measured the same way: 6.415e-12 (d2; Sigma_E:
# 7.2e-13), rounded up to 6.5e-12.
LONG_MEASURED_REL = 6.5e-12
LONG_TOL_REL = 4 * LONG_MEASURED_REL
LONG_MARGIN_REL = 10 * LONG_TOL_REL
LONG_SKIP_CAP = 0.02                 # the share of pairs of that scene that may lie inside its margin
# xi = Logmap of the cycle pose, absolute: one rounding (2.2e-16) of poses up to 200 m from the origin (chain 40 m, frame offset 50 m, outliers
# 30 m), about 20 operations deep, times 1 / sin^2 theta <= 50 for rotations below 3 rad (pcm_cases.scene) = 4e-11, rounded up
XI_TOL = 1e-10


def random_covariance(rng, lo, hi):
    """a random positive definite 6x6 shaped like FIXED_COVARIANCE: D^1/2 s (I / 2 + G G^T / 16) D^1/2 with G 6x8 normal, so that the
    middle factor has eigenvalues of about 0.5 to 2, and a log-uniform scale s in [lo, hi]"""
    G = rng.normal(size=(6, 8))
    d = np.sqrt(np.diag(RC.FIXED_COVARIANCE))
    s = np.exp(rng.uniform(np.log(lo), np.log(hi)))
    C = s * (d[:, None] * (0.5 * np.eye(6) + G @ G.T / 16.0) * d[None, :])
    return 0.5 * (C + C.T)


def chain(rng, n):
    """n poses from the identity with steps of about 1 m / 0.05 rad"""
    X = np.empty((n, 4, 4))
    X[0] = np.eye(4)
    for m in range(n - 1):
        a = rng.normal(size=3)
        step = PC.pose(a / np.linalg.norm(a) * rng.uniform(0.025, 0.075), np.array([1.0, 0, 0]) + rng.normal(0, 0.1, 3))
        X[m + 1] = X[m] @ step
    return X


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def scene(L, seed=0, n_poses=N_POSES):
    """(XA, XB, QA, QB, ia, kb, Z, C, inlier): two chains, a random positive definite covariance per odometry step (0.05 to 1 x
    FIXED_COVARIANCE) and per loop (0.25 to 16 x), L loops in the reference's vertex order with distinct key pairs.  An inlier measures
    XA_i^-1 G XB_k with noise drawn from its own covariance, an outlier is a random pose.  Rotations stay small (steps 0.075 rad about
    random axes, G 0.25, outliers 0.85) so that every cycle pose turns by less than 3 rad, for the reason pcm_cases.scene gives;
    test_pcm_cov_cpu.py asserts it."""
    rng = np.random.default_rng(7000 * L + seed + 17 * n_poses)
    XA, XB = chain(rng, n_poses), chain(rng, n_poses)
    QA = np.stack([random_covariance(rng, 0.05, 1.0) for _ in range(n_poses - 1)])
    QB = np.stack([random_covariance(rng, 0.05, 1.0) for _ in range(n_poses - 1)])
    G = PC.random_pose(rng, 50.0, 0.25)
    keys = np.sort(rng.choice(n_poses * n_poses, L, replace=False))
    ia, kb = (keys // n_poses).astype(np.int32), (keys % n_poses).astype(np.int32)
    Z, C, inlier = np.empty((L, 4, 4)), np.empty((L, 6, 6)), np.zeros(L, bool)
    for u in range(L):
        C[u] = random_covariance(rng, 0.25, 16.0)
        if rng.random() < INLIER_SHARE:
            xi = np.linalg.cholesky(C[u]) @ rng.normal(size=6)
            Z[u] = R.inverse(XA[ia[u]]) @ G @ XB[kb[u]] @ PC.pose(xi[:3], xi[3:])
            inlier[u] = True
        else:
            Z[u] = PC.random_pose(rng, 30.0, 0.85)
    return _freeze(XA, XB, QA, QB, ia, kb, Z, C, inlier)


@functools.lru_cache(maxsize=None)
def long_scene():
    """the cancellation scene: 400 poses per chain, 33 loops"""
    return scene(33, seed=3, n_poses=400)


@functools.lru_cache(maxsize=None)
def special_scene():
    """six loops, not in the reference's order, whose pairs take the edges of the span arithmetic:
    (1, 2) the same poses on both sides (zero spans), (4, 5) i > j with k < l (backward on A, forward on B and the reverse),
    (0, 3) the first and the last pose of both trajectories"""
    XA, XB, QA, QB, _, _, _, _, _ = scene(2, seed=9)
    rng = np.random.default_rng(99)
    n = XA.shape[0]
    ia = np.array([0, 5, 5, n - 1, 20, 10], np.int32)
    kb = np.array([0, 7, 7, n - 1, 3, 30], np.int32)
    G = PC.random_pose(rng, 50.0, 0.25)
    C = np.stack([random_covariance(rng, 0.25, 16.0) for _ in range(6)])
    Z = np.empty((6, 4, 4))
    for u in range(6):
        xi = np.linalg.cholesky(C[u]) @ rng.normal(size=6)
        Z[u] = R.inverse(XA[ia[u]]) @ G @ XB[kb[u]] @ PC.pose(xi[:3], xi[3:])
    return _freeze(XA, XB, QA, QB, ia, kb, Z, C, np.ones(6, bool))


SPECIAL_PAIRS = ((1, 2), (4, 5), (0, 3), (0, 1), (3, 5))


def _expected(sc, mode, first=None):
    XA, XB, QA, QB, ia, kb, Z, C, _ = sc
    return _freeze(*RC.evaluate(mode, XA, XB, ia, kb, Z, C, QA, QB, first))


@functools.lru_cache(maxsize=None)
def expected(L, mode, seed=0):
    """the restatement's (D [L, L] of d2, XI [L, L, 6], SE [L, L, 6, 6]) of scene(L, seed), read-only"""
    return _expected(scene(L, seed), mode)


@functools.lru_cache(maxsize=None)
def expected_long():
    return _expected(long_scene(), "span")


@functools.lru_cache(maxsize=None)
def expected_special(mode):
    return _expected(special_scene(), mode)


def rel_sigma(got, want):
    """largest entry difference over the largest entry, per matrix: [..., 6, 6] -> [...]"""
    return np.abs(got - want).max((-1, -2)) / np.abs(want).max((-1, -2))


def rel_d(got, want):
    """|got - want| / want where want is a number and not 0; 0 where both are NaN or both 0; inf where only one is a number"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    out = np.zeros(want.shape)
    both = np.isfinite(got) & np.isfinite(want)
    nz = both & (want != 0)
    out[nz] = np.abs(got[nz] - want[nz]) / np.abs(want[nz])
    out[both & (want == 0) & (got != 0)] = np.inf
    out[np.isfinite(got) != np.isfinite(want)] = np.inf
    return out


def in_margin(D, thresholds, margin_rel):
    """bool [L, L]: the pairs whose d2 lies within margin_rel * threshold of one of the thresholds"""
    out = np.zeros(D.shape, bool)
    with np.errstate(invalid="ignore"):
        for t in thresholds:
            out |= np.abs(D - t) <= margin_rel * t
    np.fill_diagonal(out, False)
    return out
