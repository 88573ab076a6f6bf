"""NumPy restatement of the point-to-plane ICP contract: pcl::NormalEstimation with setKSearch /
setViewPoint as GlobalManager::addNormal drives it (global_manager.cpp:2679-2693), and pcl::IterativeClosestPointWithNormals with
TransformationEstimationPointToPlaneLLS and DefaultConvergenceCriteria.  PCL is not part of the reference tree, so this restates the
DEFINITION, not PCL's text, and parity with PCL is unpinned.  Test infrastructure: the product never imports it.

The shared steps (correspondences, the pose update, the stopping rules, the fitness score) are icp_restate's; this file adds the normals
(contract A) and steps 2-4 of contract B."""
import numpy as np
from scipy.spatial import cKDTree

import icp_restate as R

DEGENERATE = 6
STATES = R.STATES + ("DEGENERATE",)
PIVOT = 1e-10
DEFAULTS = dict(R.DEFAULTS, normal_k=15, viewpoint=(0.0, 0.0, 0.0))


def neighbours(P, k):
    """Contract A step 1: (idx [n, min(k, n)] in (float32 distance, index) order, tie [n] bool).  The float64 tree proposes one more than
    needed, the searches' float32 distance chain decides.  tie: the last neighbour kept and the first one left out are at exactly the same
    float distance -- the kernel may keep either (it breaks ties by its own storage order)."""
    P = R._f32(P)
    n = P.shape[0]
    kk = min(k, n)
    m = min(kk + 1, n)
    _, idx = cKDTree(P.astype(np.float64)).query(P.astype(np.float64), k=m)
    idx = idx.reshape(n, m)
    d = R.d2_f32(P[:, None, :], P[idx])
    order = np.lexsort((idx, d), axis=1)
    idx = np.take_along_axis(idx, order, 1)
    d = np.take_along_axis(d, order, 1)
    tie = d[:, kk - 1] == d[:, kk] if m > kk else np.zeros(n, bool)
    return idx[:, :kk], tie


def normals(P, k=15, viewpoint=(0.0, 0.0, 0.0)):
    """Contract A: dict(normals [n, 4] float32 (unit normal, curvature), lam [n, 3] ascending eigenvalues, cov [n, 3, 3], toward [n]
    |nrm . (v - p)| / |v - p|, tie [n], contains_self [n])"""
    P32 = R._f32(P)
    n = P32.shape[0]
    out = np.full((n, 4), np.nan, np.float32)
    lam = np.full((n, 3), np.nan)
    toward = np.full(n, np.nan)
    C = np.full((n, 3, 3), np.nan)
    if n == 0:
        return dict(normals=out, lam=lam, cov=C, toward=toward, tie=np.zeros(0, bool), contains_self=np.zeros(0, bool))
    idx, tie = neighbours(P32, k)
    self_in = (idx == np.arange(n)[:, None]).any(1)
    if idx.shape[1] >= 3:
        q = P32.astype(np.float64)[idx]                              # [n, cnt, 3]
        c = q - q.mean(1, keepdims=True)
        C = np.einsum("nki,nkj->nij", c, c) / idx.shape[1]
        w, v = np.linalg.eigh(C)
        nrm = v[:, :, 0]
        to_v = np.asarray(viewpoint, np.float64) - P32.astype(np.float64)
        dot = (nrm * to_v).sum(1)
        nrm = np.where((dot < 0)[:, None], -nrm, nrm)
        tr = w.sum(1)
        with np.errstate(invalid="ignore", divide="ignore"):
            curv = np.where(tr > 0, w[:, 0] / tr, 0.0)
            toward = np.abs(dot) / np.linalg.norm(to_v, axis=1)
        out = np.concatenate([nrm, curv[:, None]], 1).astype(np.float32)
        lam = w
    return dict(normals=out, lam=lam, cov=C, toward=toward, tie=tie, contains_self=self_in)


def kept(N, corr):
    """step 2: correspondences whose target normal is finite"""
    N = np.asarray(N)
    ok = corr >= 0
    ok[ok] = np.isfinite(N[corr[ok], :3]).all(1)
    return ok


def sums29(A, B, N, X, corr):
    """step 3: n, the upper triangle of sum a a^T (row-major), sum a r, sum |d - s|^2 over the kept correspondences; s = X A_i in float64"""
    keep = kept(N, corr)
    s = R._f32(A)[keep].astype(np.float64) @ X[:3, :3].T + X[:3, 3]
    d = R._f32(B)[corr[keep]].astype(np.float64)
    nrm = np.asarray(N, np.float32)[corr[keep], :3].astype(np.float64)
    a = np.concatenate([np.cross(s, nrm), nrm], 1)
    r = (nrm * (d - s)).sum(1)
    M = a.T @ a
    return np.concatenate([[float(keep.sum())], M[np.triu_indices(6)], a.T @ r, [((d - s) ** 2).sum()]])


def unpack(s):
    M = np.zeros((6, 6))
    M[np.triu_indices(6)] = s[1:22]
    return M + np.triu(M, 1).T, s[22:28]


def solve(s):
    """step 4: x = (alpha, beta, gamma, tx, ty, tz) or None when the scaled system has a Cholesky pivot <= 1e-10 or a diagonal entry <= 0"""
    M, g = unpack(np.asarray(s, np.float64))
    dg = np.diag(M)
    if not (np.isfinite(dg).all() and (dg > 0).all()):
        return None
    sc = 1.0 / np.sqrt(dg)
    Mt = M * sc[:, None] * sc[None, :]
    try:
        L = np.linalg.cholesky(Mt)
    except np.linalg.LinAlgError:
        return None
    if not (np.diag(L) ** 2 > PIVOT).all():
        return None
    return sc * np.linalg.solve(Mt, sc * g)


def delta(x):
    """pcl's constructTransformationMatrix: Rz(gamma) Ry(beta) Rx(alpha), t"""
    ca, sa, cb, sb, cg, sg = np.cos(x[0]), np.sin(x[0]), np.cos(x[1]), np.sin(x[1]), np.cos(x[2]), np.sin(x[2])
    Rx = np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]])
    Ry = np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]])
    Rz = np.array([[cg, -sg, 0], [sg, cg, 0], [0, 0, 1]])
    D = np.eye(4)
    D[:3, :3] = Rz @ Ry @ Rx
    D[:3, 3] = x[3:6]
    return D


def fit(s):
    """(delta, state): the increment, or the identity and NO_CORRESPONDENCES / DEGENERATE"""
    if s[0] < 3:
        return np.eye(4), R.NO_CORRESPONDENCES
    x = solve(s)
    if x is None:
        return np.eye(4), DEGENERATE
    return delta(x), R.NOT_CONVERGED


def step(A, B, N, X, max_corr, tgt=None):
    """steps 1-4 once at pose X: (corr, d2, sums [29], delta [4,4], state: 5, 6 or 0)"""
    tgt = tgt or R.Target(B)
    X = np.asarray(X, np.float64)
    corr, d2 = R.correspondences(A, tgt, X, max_corr)
    s = sums29(A, B, N, X, corr)
    D, state = fit(s)
    return corr, d2, s, D, state


def icp(A, B, N=None, guess=None, **params):
    """N: the target's normals [n, >= 3] (None: computed with normal_k and viewpoint).  Returns what icp_restate.icp returns."""
    p = dict(DEFAULTS)
    assert set(params) <= set(p), params
    p.update(params)
    if N is None:
        N = normals(B, p["normal_k"], p["viewpoint"])["normals"]
    tgt = R.Target(B)
    X = (np.eye(4) if guess is None else np.asarray(guess, np.float64)).astype(np.float32).astype(np.float64)
    prev, it, state, conv, trace = R.DBL_MAX, 0, R.NOT_CONVERGED, False, []
    limit = p["force_iterations"] if p["force_iterations"] > 0 else p["max_iterations"]
    while it < limit:
        corr, _ = R.correspondences(A, tgt, X, p["max_correspondence_distance"])
        s = sums29(A, B, N, X, corr)
        D, end = fit(s)
        if end != R.NOT_CONVERGED:
            state = end
            break
        X = D @ X
        it += 1
        mse = s[28] / s[0]
        cos, t2, d_abs, rel = R.criteria(D, mse, prev)
        trace.append((cos, t2, mse, rel, int(s[0])))
        if p["force_iterations"] > 0:
            continue
        state = R.converged(it, cos, t2, d_abs, rel, p["max_iterations"], p["transformation_epsilon"], p["rotation_epsilon"],
                            p["euclidean_fitness_epsilon"])
        if state != R.NOT_CONVERGED:
            conv = True
            break
        prev = mse
    return dict(T=X.astype(np.float32).astype(np.float64), X=X, converged=conv, iterations=it, state=state, trace=trace)
