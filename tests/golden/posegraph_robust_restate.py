"""NumPy / scipy restatement of the pose-graph contract's second half: per-factor noise converted as
evaluation_utils::convertToChordalNoise converts it (evaluation_utils.cpp:333-366), Levenberg-Marquardt step control, and robust kernels on
the loop factors.  Test infrastructure only, built on posegraph_restate.py; everything is float64.

A covariance is 6 x 6 in gtsam's Pose3 order (rotation xyz, translation xyz).  `oC` is None or one covariance per odometry factor; `lC` is
None or one entry per loop, each a covariance or None.  A factor without one keeps the unit model."""
import collections
import os
import sys

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import posegraph_restate as R  # noqa: E402

NONE, HUBER, CAUCHY, GEMAN_MCCLURE = 0, 1, 2, 3
TRANSLATION_FLOOR = 0.01                 # evaluation_utils.cpp:361
LAMBDA_INITIAL, LAMBDA_MIN, LAMBDA_MAX = 1e-5, 1e-12, 1e12
PRED_FLOOR = 1e-10                       # a step whose predicted decrease is below PRED_FLOOR * cost is accepted
EPS_DEFAULT, MAX_SOLVES_DEFAULT = R.EPS_DEFAULT, 200

ResultLM = collections.namedtuple("ResultLM", "T solves accepted converged max_delta cost_initial cost_final lam weights r2 log")
Solve = collections.namedtuple("Solve", "lam cost cost_new pred rho accepted max_delta")


def chordal_information(C, Rhat):
    """the 12 x 12 information of a chordal factor from a Pose3 covariance: 1 / max(C00, C11, C22) on the nine rotation rows,
    Rhat (C[3:, 3:] + 0.01 I)^-1 Rhat^T on the translation rows; the rotation-translation blocks of C are ignored"""
    C = np.asarray(C, np.float64).reshape(6, 6)
    L = np.zeros((12, 12))
    L[:9, :9] = np.eye(9) / max(C[0, 0], C[1, 1], C[2, 2])
    L[9:, 9:] = Rhat @ np.linalg.inv(C[3:, 3:] + TRANSLATION_FLOOR * np.eye(3)) @ Rhat.T
    return L


def covariances(n_odometry, n_loops, oC=None, lC=None):
    """one entry per factor, a 6 x 6 array or None"""
    out = [None] * n_odometry if oC is None else [c for c in np.asarray(oC, np.float64).reshape(n_odometry, 6, 6)]
    return out + ([None] * n_loops if lC is None else [None if c is None else np.asarray(c, np.float64).reshape(6, 6) for c in lC])


def information(T0, fi, covs):
    """Lam [F, 12, 12]: Rhat is the stage-1 rotation of the factor's first pose, fixed for the whole optimisation"""
    Lam = np.tile(np.eye(12), (fi.size, 1, 1))
    for f, c in enumerate(covs):
        if c is not None:
            Lam[f] = chordal_information(c, T0[fi[f], :3, :3])
    return Lam


def kernel_weight(kind, k, r):
    r = np.asarray(r, np.float64)
    if kind == NONE:
        return np.ones_like(r)
    if kind == HUBER:
        return np.where(r <= k, 1.0, k / np.maximum(r, 1e-300))
    s = k * k / (k * k + r * r)
    return s if kind == CAUCHY else s * s


def kernel_cost(kind, k, r):
    r = np.asarray(r, np.float64)
    if kind == NONE:
        return 0.5 * r * r
    if kind == HUBER:
        return np.where(r <= k, 0.5 * r * r, k * (r - 0.5 * k))
    if kind == CAUCHY:
        return 0.5 * k * k * np.log1p(r * r / (k * k))
    return 0.5 * k * k * r * r / (k * k + r * r)


def squared_residuals(T, fi, fj, fZ, Lam):
    """e^T Lam e per factor"""
    e, _, _ = R._linearize(T, fi, fj, fZ)
    return np.einsum("fk,fkl,fl->f", e, Lam, e)


def cost(T, fi, fj, fZ, Lam, n_odometry, kind=NONE, k=1.0):
    """sum 0.5 r^2 over the odometry factors plus sum rho(r) over the loops"""
    if fi.size == 0:
        return 0.0
    r2 = squared_residuals(T, fi, fj, fZ, Lam)
    return float(0.5 * r2[:n_odometry].sum() + kernel_cost(kind, k, np.sqrt(r2[n_odometry:])).sum())


def blocks(T, fi, fj, fZ, Lam):
    """per factor: e, Hi^T Lam Hi, Hi^T Lam Hj, Hj^T Lam Hj, -Hi^T Lam e, -Hj^T Lam e"""
    e, Hi, Hj = R._linearize(T, fi, fj, fZ)
    LHi, LHj = Lam @ Hi, Lam @ Hj
    Le = np.einsum("fkl,fl->fk", Lam, e)
    tr = lambda A, B: np.einsum("fka,fkb->fab", A, B)
    return e, tr(Hi, LHi), tr(Hi, LHj), tr(Hj, LHj), -np.einsum("fka,fk->fa", Hi, Le), -np.einsum("fka,fk->fa", Hj, Le)


def system(T, fi, fj, fZ, Lam):
    """(H sparse [6 (N - 1)]^2, g): pose 0 held"""
    N = T.shape[0]
    _, Hii, Hij, Hjj, gi, gj = blocks(T, fi, fj, fZ, Lam)
    a = np.arange(6)
    rows, cols, vals = [], [], []
    for p, q, B in ((fi, fi, Hii), (fi, fj, Hij), (fj, fi, Hij.transpose(0, 2, 1)), (fj, fj, Hjj)):
        rows.append((6 * p[:, None, None] + a[None, :, None] + 0 * a[None, None, :]).reshape(-1))
        cols.append((6 * q[:, None, None] + 0 * a[None, :, None] + a[None, None, :]).reshape(-1))
        vals.append(B.reshape(-1))
    H = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(6 * N, 6 * N)).tocsc()[6:, 6:]
    g = np.zeros((N, 6))
    np.add.at(g, fi, gi)
    np.add.at(g, fj, gj)
    return H.tocsc(), g.reshape(-1)[6:]


def _setup(chain_lengths, odom, li, lj, lZ, prior, oC, lC, order):
    fi, fj, fZ = R.factors(chain_lengths, odom, li, lj, lZ)
    if not R.connected(chain_lengths, li, lj):
        raise ValueError("a chain is not connected to chain 0")
    T, _ = R.initialize(chain_lengths, odom, li, lj, lZ, prior, order)       # stage 1 is not weighted (evaluation_utils.cpp:284)
    n_odometry = fi.size - np.asarray(li).size
    Lam = information(T, fi, covariances(n_odometry, np.asarray(li).size, oC, lC))
    return fi, fj, fZ, T, n_odometry, Lam


def gn_optimize(chain_lengths, odom, li, lj, lZ, prior=None, oC=None, lC=None, eps=EPS_DEFAULT, max_iterations=200, order=None):
    """posegraph_restate.optimize with the factors' information: full Gauss-Newton steps -> posegraph_restate.Result"""
    fi, fj, fZ, T, n_odometry, Lam = _setup(chain_lengths, odom, li, lj, lZ, prior, oC, lC, order)
    N = T.shape[0]
    e0 = cost(T, fi, fj, fZ, Lam, n_odometry)
    its, conv, md, deltas = 0, False, 0.0, []
    while its < max_iterations:
        d = np.zeros((N, 6))
        if N > 1:
            H, g = system(T, fi, fj, fZ, Lam)
            d[1:] = R._solve(H, g, order).reshape(N - 1, 6)
        T = R.retract(T, d)
        md = float(np.abs(d).max())
        deltas.append(md)
        its += 1
        if md < eps:
            conv = True
            break
    return R.Result(T, its, conv, md, e0, cost(T, fi, fj, fZ, Lam, n_odometry), deltas)


def lm_optimize(chain_lengths, odom, li, lj, lZ, prior=None, oC=None, lC=None, kernel=NONE, k=1.0, eps=EPS_DEFAULT, max_solves=MAX_SOLVES_DEFAULT,
                order=None):
    """Levenberg-Marquardt on the chordal factors -> ResultLM.
    Solve 1 is the Gauss-Newton step (lambda = 0, kernel weights 1), accepted whatever it does to the cost: the linear solve for the
    translations from t = 0.  Later solves: (H + lambda diag H) delta = g with lambda from LAMBDA_INITIAL, the loops' blocks scaled by the
    kernel's weight at the current poses; pred = 0.5 delta^T (lambda diag(H) delta + g); rho = (c - c_new) / pred, or 1 where
    pred <= PRED_FLOOR c (the cost resolves neither the decision nor the gain of such a step); accepted iff c_new <= c or
    pred <= PRED_FLOOR c; then lambda *= max(1/3, 1 - (2 rho - 1)^3) and nu = 2, else lambda *= nu, nu *= 2 and the poses are restored;
    lambda stays in [LAMBDA_MIN, LAMBDA_MAX].  Stops at an accepted step with max|delta| < eps or after max_solves solves."""
    fi, fj, fZ, T, n_odometry, Lam = _setup(chain_lengths, odom, li, lj, lZ, prior, oC, lC, order)
    N, F = T.shape[0], fi.size
    total = lambda X: cost(X, fi, fj, fZ, Lam, n_odometry, kernel, k)

    def weights(X):
        w = np.ones(F)
        if F:
            w[n_odometry:] = kernel_weight(kernel, k, np.sqrt(squared_residuals(X, fi, fj, fZ, Lam)[n_odometry:]))
        return w

    c0 = c = total(T)
    lam, nu = LAMBDA_INITIAL, 2.0
    solves = accepted = 0
    conv, md, log = False, 0.0, []
    while solves < max_solves:
        first = solves == 0
        lam_k = 0.0 if first else lam
        d = np.zeros((N, 6))
        pred = 0.0
        if N > 1:
            w = np.ones(F) if first else weights(T)
            H, g = system(T, fi, fj, fZ, Lam * w[:, None, None])
            dg = H.diagonal()
            x = R._solve((H + sp.diags(lam_k * dg)).tocsc(), g, order)
            d[1:] = x.reshape(N - 1, 6)
            pred = 0.5 * float(x @ (lam_k * dg * x + g))
        Tn = R.retract(T, d)
        cn = total(Tn)
        step = float(np.abs(d).max())
        solves += 1
        below = pred <= PRED_FLOOR * c                           # the cost cannot resolve this step: neither the decision nor the gain
        rho = 1.0 if below else (c - cn) / pred
        ok = first or cn <= c or below
        log.append(Solve(lam_k, c, cn, pred, rho, ok, step))
        if ok:
            T, c, md = Tn, cn, step
            accepted += 1
            if not first:
                q = 2.0 * rho - 1.0
                fac = 1.0 - q * q * q
                if not fac > 1.0 / 3.0:                          # a rho that is not a number too
                    fac = 1.0 / 3.0
                lam, nu = min(max(lam * fac, LAMBDA_MIN), LAMBDA_MAX), 2.0
            if md < eps:
                conv = True
                break
        else:
            lam, nu = min(max(lam * nu, LAMBDA_MIN), LAMBDA_MAX), 2.0 * nu
    r2 = squared_residuals(T, fi, fj, fZ, Lam)[n_odometry:] if F else np.zeros(0)
    return ResultLM(T, solves, accepted, conv, md, c0, c, lam, kernel_weight(kernel, k, np.sqrt(r2)), r2, log)


def decision_margins(log):
    """per solve after the first: (pred / (PRED_FLOOR c), |c_new - c| / c): a decision can flip only when the first is within a factor 10
    of 1 while the second is below 1e-12"""
    return [(s.pred / (PRED_FLOOR * s.cost) if s.cost > 0 else np.inf, abs(s.cost_new - s.cost) / s.cost if s.cost > 0 else np.inf) for s in log[1:]]
