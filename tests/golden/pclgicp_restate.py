"""NumPy restatement of the PCL-style GICP contract: pcl::GeneralizedIterativeClosestPoint as the
PCL_GICP branch of GlobalManager::select_registration_method configures it (global_manager.cpp:2419-2426).  PCL is not part of the reference
tree, so this restates the DEFINITION, not PCL's text, and parity with PCL is unpinned.  Test infrastructure: the product never imports it.

Per outer iteration: exact 1-NN of the float32-transformed source points (icp_restate.correspondences), kept where d^2 < max^2; the
Mahalanobis matrices (C_B + R0 C_A R0^T)^-1 frozen at the iteration's rotation; a BFGS over (t~, roll, pitch, yaw) about the pivot with the
contract's own backtracking line search; the pose rebuilt from the six parameters; PCL's stopping rule on the scaled entry-wise change.
mode "sums" (the defining one) evaluates f and its gradient through the 74 sums, mode "points" point by point, as PCL does."""
import numpy as np
from scipy.spatial import cKDTree

import icp_restate as I

STATES = I.STATES
NOT_CONVERGED, ITERATIONS, TRANSFORM, NO_CORRESPONDENCES = I.NOT_CONVERGED, I.ITERATIONS, I.TRANSFORM, I.NO_CORRESPONDENCES
ENDS = ("GRADIENT", "LIMIT", "NO_PROGRESS")
GRADIENT, LIMIT, NO_PROGRESS = range(3)
DEFAULTS = dict(max_iterations=200, max_inner_iterations=20, force_iterations=0, max_correspondence_distance=5.0, rotation_epsilon=2e-3,
                transformation_epsilon=5e-4, gradient_tolerance=1e-2)
# global_manager.cpp:2422-2425 with icp_iters = 50 (setEuclideanFitnessEpsilon is accepted and unused)
MAPPING_2422 = dict(max_correspondence_distance=100.0, max_iterations=50, transformation_epsilon=1e-3)
SYM = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))          # xx xy xz yy yz zz
SYM_OF = np.array([[0, 1, 2], [1, 3, 4], [2, 4, 5]])


# ---- covariances: the handle's (k nearest neighbours, the point itself included; C = I - 0.999 n n^T with n the normal) -------------------
def normals(P, k=20):
    P = I._f32(P).astype(np.float64)
    kk = min(k, P.shape[0])
    _, idx = cKDTree(P).query(P, k=kk)
    d = P[idx.reshape(P.shape[0], kk)] - P[:, None, :]
    m = d.mean(1)
    cov = np.einsum("nki,nkj->nij", d, d) / kk - m[:, :, None] * m[:, None, :]
    _, v = np.linalg.eigh(cov)
    return v[:, :, 0]


def cov_from_normals(n):
    return np.eye(3)[None] - 0.999 * n[:, :, None] * n[:, None, :]


def covariances(P, k=20):
    return cov_from_normals(normals(P, k))


def pivot(B):
    """the float32 midpoint of the target's bounding box"""
    B = I._f32(B)
    return (np.float32(0.5) * (B.min(0) + B.max(0))).astype(np.float64)


# ---- steps 3 and 4 ---------------------------------------------------------------------------------------------------------------------------
def inv3_sym(a):
    """cofactor inverse of [m,3,3] matrices (the kernels' expressions); (inverse, det != 0)"""
    a = a.reshape(-1, 9)
    c0 = a[:, 4] * a[:, 8] - a[:, 5] * a[:, 7]
    c1 = a[:, 5] * a[:, 6] - a[:, 3] * a[:, 8]
    c2 = a[:, 3] * a[:, 7] - a[:, 4] * a[:, 6]
    det = a[:, 0] * c0 + a[:, 1] * c1 + a[:, 2] * c2
    ok = det != 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        i = 1.0 / det
        r = np.stack([c0 * i, (a[:, 2] * a[:, 7] - a[:, 1] * a[:, 8]) * i, (a[:, 1] * a[:, 5] - a[:, 2] * a[:, 4]) * i,
                      c1 * i, (a[:, 0] * a[:, 8] - a[:, 2] * a[:, 6]) * i, (a[:, 2] * a[:, 3] - a[:, 0] * a[:, 5]) * i,
                      c2 * i, (a[:, 1] * a[:, 6] - a[:, 0] * a[:, 7]) * i, (a[:, 0] * a[:, 4] - a[:, 1] * a[:, 3]) * i], 1)
    return r.reshape(-1, 3, 3), ok


def frozen_terms(A, B, X, corr, CA, CB, c):
    """per kept correspondence: p = A_i - c, q = B_j - c, M as its six entries xx xy xz yy yz zz (a failed inverse drops the correspondence)"""
    keep = corr >= 0
    R0 = np.asarray(X, np.float64)[:3, :3]
    M, ok = inv3_sym(CB[corr[keep]] + R0 @ CA[keep] @ R0.T)
    p = (I._f32(A)[keep].astype(np.float64) - c)[ok]
    q = (I._f32(B)[corr[keep]].astype(np.float64) - c)[ok]
    M = M[ok]
    return p, q, np.stack([M[:, r, cc] for r, cc in SYM], 1)


def sums74(p, q, M6):
    M = M6[:, SYM_OF]
    Mq = np.einsum("nij,nj->ni", M, q)
    s = np.zeros(74)
    s[0] = p.shape[0]
    s[1:7] = M6.sum(0)
    s[7:10] = Mq.sum(0)
    s[10] = (q * Mq).sum()
    for a in range(3):
        s[11 + 6 * a:17 + 6 * a] = (p[:, a, None] * M6).sum(0)
        s[29 + 3 * a:32 + 3 * a] = (p[:, a, None] * Mq).sum(0)
    for k, (a, b) in enumerate(SYM):
        s[38 + 6 * k:44 + 6 * k] = ((p[:, a] * p[:, b])[:, None] * M6).sum(0)
    return s


# ---- step 5 -----------------------------------------------------------------------------------------------------------------------------------
def rotation(x):
    """R = Rz(psi) Ry(theta) Rx(phi) and its three partial derivatives"""
    cf, sf, ct, st, cp, sp = np.cos(x[3]), np.sin(x[3]), np.cos(x[4]), np.sin(x[4]), np.cos(x[5]), np.sin(x[5])
    R = np.array([[cp * ct, cp * st * sf - sp * cf, cp * st * cf + sp * sf],
                  [sp * ct, sp * st * sf + cp * cf, sp * st * cf - cp * sf],
                  [-st, ct * sf, ct * cf]])
    dphi = np.array([[0, cp * st * cf + sp * sf, -cp * st * sf + sp * cf],
                     [0, sp * st * cf - cp * sf, -sp * st * sf - cp * cf],
                     [0, ct * cf, -ct * sf]])
    dth = np.array([[-cp * st, cp * ct * sf, cp * ct * cf],
                    [-sp * st, sp * ct * sf, sp * ct * cf],
                    [-ct, -st * sf, -st * cf]])
    dpsi = np.array([[-sp * ct, -sp * st * sf - cp * cf, -sp * st * cf + cp * sf],
                     [cp * ct, cp * st * sf - sp * cf, cp * st * cf + sp * sf],
                     [0, 0, 0]])
    return R, (dphi, dth, dpsi)


def objective_sums(s, x):
    """f and its gradient through the quadratic form"""
    x = np.asarray(x, np.float64)
    R, dR = rotation(x)
    t, n = x[:3], s[0]
    sym = lambda m6: m6[SYM_OF]
    S, v, kq = sym(s[1:7]), s[7:10], s[10]
    P = [sym(s[11 + 6 * a:17 + 6 * a]) for a in range(3)]
    w = [s[29 + 3 * a:32 + 3 * a] for a in range(3)]
    Q = [[sym(s[38 + 6 * SYM_OF[a, b]:44 + 6 * SYM_OF[a, b]]) for b in range(3)] for a in range(3)]
    col = [R[:, a] for a in range(3)]
    St = S @ t
    val = t @ (St - 2 * v) + kq
    Bt = np.zeros(3)
    gr = []
    for a in range(3):
        Aa = sum(Q[a][b] @ col[b] for b in range(3))
        Ca = P[a] @ t
        Bt = Bt + P[a] @ col[a]
        val += col[a] @ (Aa + 2 * Ca - 2 * w[a])
        gr.append(Aa + Ca - w[a])
    g = np.empty(6)
    g[:3] = 2.0 / n * (St + Bt - v)
    for k in range(3):
        g[3 + k] = 2.0 / n * sum(gr[a] @ dR[k][:, a] for a in range(3))
    return val / n, g


def objective_points(p, q, M6, x):
    """f and its gradient point by point (what PCL's OptimizationFunctorWithIndices evaluates)"""
    x = np.asarray(x, np.float64)
    R, dR = rotation(x)
    M = M6[:, SYM_OF]
    r = p @ R.T + x[:3] - q
    Mr = np.einsum("nij,nj->ni", M, r)
    n = p.shape[0]
    g = np.empty(6)
    g[:3] = 2.0 / n * Mr.sum(0)
    for k in range(3):
        g[3 + k] = 2.0 / n * (Mr * (p @ dR[k].T)).sum()
    return (r * Mr).sum() / n, g


def bfgs(fun, x0, gradient_tolerance=1e-2, max_inner_iterations=20, decisions=None):
    """the contract's inner minimisation: (x, iterations counted, ending).  decisions (a list, optional) receives (kind, value, threshold)
    of every test taken: "gradient" (|g| against the tolerance), "armijo" (f(x + a d) against f + 0.01 a g.d), "curvature"
    (s.y against 1e-12 |s| |y|); and, as a second view of the Armijo test, "armijo_decrease" (the decrease f - f(x + a d) against the required
    decrease -0.01 a g.d)."""
    note = decisions.append if decisions is not None else (lambda _: None)
    x = np.array(x0, np.float64)
    H = np.eye(6)
    f, g = fun(x)
    scaled = False
    k = 0
    while k < max_inner_iterations:
        gnorm = np.sqrt(g @ g)
        note(("gradient", gnorm, gradient_tolerance))
        if gnorm < gradient_tolerance:
            return x, k, GRADIENT
        d = -(H @ g)
        gd = g @ d
        if not gd < 0.0:
            H = np.eye(6)
            d = -g
            gd = -(g @ g)
        alpha = 0.01 / gnorm if (k == 0 and 0.01 / gnorm < 1.0) else 1.0
        accepted = False
        for _ in range(30):
            xn = x + alpha * d
            fn, gn = fun(xn)
            note(("armijo", fn, f + 0.01 * alpha * gd))
            note(("armijo_decrease", f - fn, -0.01 * alpha * gd))
            if fn <= f + 0.01 * alpha * gd:
                accepted = True
                break
            alpha *= 0.5
        k += 1
        if not accepted:
            return x, k, NO_PROGRESS
        s, y = xn - x, gn - g
        sy, yy = s @ y, y @ y
        note(("curvature", sy, 1e-12 * np.sqrt(s @ s) * np.sqrt(yy)))
        if sy > 1e-12 * np.sqrt(s @ s) * np.sqrt(yy):
            if not scaled:
                scaled = True
                H = np.eye(6) * (sy / yy)
            rho = 1.0 / sy
            Hy = H @ y
            H = H - rho * (np.outer(s, Hy) + np.outer(Hy, s)) + (rho * rho * (y @ Hy) + rho) * np.outer(s, s)
        x, f, g = xn, fn, gn
    return x, k, LIMIT


def params_from_pose(X, c):
    R, t = X[:3, :3], X[:3, 3]
    x = np.empty(6)
    x[:3] = t + R @ c - c
    x[3] = np.arctan2(R[2, 1], R[2, 2])
    x[4] = np.arcsin(np.clip(-R[2, 0], -1.0, 1.0))
    x[5] = np.arctan2(R[1, 0], R[0, 0])
    return x


def pose_from_params(x, c):
    X = np.eye(4)
    X[:3, :3] = rotation(x)[0]
    X[:3, 3] = x[:3] - X[:3, :3] @ c + c
    return X


def delta_of(Xn, X, rotation_epsilon, transformation_epsilon):
    d = np.abs(Xn[:3] - X[:3])
    return max(d[:, :3].max() / rotation_epsilon, d[:, 3].max() / transformation_epsilon)


def iterate(A, B, X, corr, CA, CB, c, p, mode="sums", decisions=None):
    """steps 3-6 with given correspondences, rotating about c: (sums, next pose, inner iterations, ending), or None below 4 correspondences"""
    pp, q, M6 = frozen_terms(A, B, X, corr, CA, CB, c)
    if pp.shape[0] < 4:
        return None
    s = sums74(pp, q, M6)
    fun = (lambda x: objective_sums(s, x)) if mode == "sums" else (lambda x: objective_points(pp, q, M6, x))
    x, k, end = bfgs(fun, params_from_pose(X, c), p["gradient_tolerance"], p["max_inner_iterations"], decisions)
    return s, pose_from_params(x, c), k, end


def step(A, B, X, covs=None, tgt=None, corr=None, mode="sums", k=20, **params):
    """one outer iteration at pose X: dict(corr, d2, sums [74] (zeros below 4), next, inner, end, decisions).  corr: use these correspondences instead
    of searching (the kernel's own, for comparisons that must not depend on float ties)"""
    p = dict(DEFAULTS); p.update(params)
    X = np.asarray(X, np.float64)
    CA, CB = covs if covs is not None else (covariances(A, k), covariances(B, k))
    d2 = None
    if corr is None:
        corr, d2 = I.correspondences(A, tgt or I.Target(B), X, p["max_correspondence_distance"])
    decisions = []
    r = iterate(A, B, X, np.asarray(corr), CA, CB, pivot(B), p, mode, decisions)
    if r is None:
        return dict(corr=corr, d2=d2, sums=np.zeros(74), next=X.copy(), inner=0, end=0, decisions=decisions)
    return dict(corr=corr, d2=d2, sums=r[0], next=r[1], inner=r[2], end=r[3], decisions=decisions)


def gicp(A, B, guess=None, covs=None, mode="sums", k=20, pivot_at=None, **params):
    """pivot_at: rotate about this point instead of the pivot (the design note's comparison with PCL's rotation about the origin).
    Returns dict(T: X narrowed to float32, X, converged, iterations, state, trace: [(delta, n, inner iterations, ending)] per outer
    iteration, decisions: [(kind, value, threshold)] of every inner test)."""
    p = dict(DEFAULTS)
    assert set(params) <= set(p), params
    p.update(params)
    tgt = I.Target(B)
    CA, CB = covs if covs is not None else (covariances(A, k), covariances(B, k))
    c = pivot(B) if pivot_at is None else np.asarray(pivot_at, np.float64)
    X = (np.eye(4) if guess is None else np.asarray(guess, np.float64)).astype(np.float32).astype(np.float64)
    it, state, conv, trace, decisions = 0, NOT_CONVERGED, False, [], []
    limit = p["force_iterations"] if p["force_iterations"] > 0 else p["max_iterations"]
    while it < limit:
        corr, _ = I.correspondences(A, tgt, X, p["max_correspondence_distance"])
        r = iterate(A, B, X, corr, CA, CB, c, p, mode, decisions)
        if r is None:
            state = NO_CORRESPONDENCES
            break
        s, Xn, inner, end = r
        it += 1
        delta = delta_of(Xn, X, p["rotation_epsilon"], p["transformation_epsilon"])
        X = Xn
        trace.append((delta, int(s[0]), inner, end))
        if p["force_iterations"] > 0:
            continue
        if it >= p["max_iterations"]:
            state, conv = ITERATIONS, True
            break
        if delta < 1.0:
            state, conv = TRANSFORM, True
            break
    return dict(T=X.astype(np.float32).astype(np.float64), X=X, converged=conv, iterations=it, state=state, trace=trace, decisions=decisions)


def outer_margin(trace):
    """the smallest factor (>= 1) by which an outer delta of the trace lies from 1"""
    with np.errstate(divide="ignore"):
        return min((max(d, 1.0 / d) if d > 0 else np.inf) for d, *_ in trace)


def inner_margin(decisions):
    """the smallest relative distance |value - threshold| / |threshold| of an inner decision of the run: gradient, Armijo (f(x + a d)
    against f + 0.01 a g.d) and curvature tests"""
    return min((abs(v - t) / abs(t) if t != 0 else np.inf) for k, v, t in decisions if k != "armijo_decrease")


def decrease_margin(decisions):
    """the Armijo tests seen as decrease against required decrease: the smallest relative distance of the two"""
    return min((abs(v - t) / abs(t) if t != 0 else np.inf) for k, v, t in decisions if k == "armijo_decrease")


fitness = I.fitness
