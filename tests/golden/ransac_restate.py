"""NumPy restatement of the RANSAC pose from correspondences.  open3d's
registration_ransac_based_on_feature_matching is not in the reference tree, so parity is unpinned: the contract is the definition and this
file states it a second time, independently of mr_slam_amd/csrc/ransac_model.hpp.

Where bits matter (the draw, the pre-rejection, the residuals) every expression is written in the contract's operation order on float64
arrays -- NumPy's elementwise operations are single correctly rounded operations -- with no np.dot / norm / einsum.  The rigid fit is
Kabsch through np.linalg.svd on the centred points; the device's Jacobi fit agrees with it to rounding, which is why the suites compare
T within 1e-9 and first check that no residual lies within 1e-9 d^2 of d^2 (margin())."""
import numpy as np

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
DEFAULTS = dict(hypotheses=4096, refine_iters=3, edge_similarity=0.9, min_sin2=1e-6)


def mix(z):
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draw(seed, h, M):
    """three distinct indices in [0, M), M >= 3"""
    r = [mix(seed + (3 * h + t + 1) * GOLDEN) for t in range(3)]
    i0 = r[0] % M
    i1 = r[1] % (M - 1)
    i1 += i1 >= i0
    lo, hi = min(i0, i1), max(i0, i1)
    i2 = r[2] % (M - 2)
    i2 += i2 >= lo
    i2 += i2 >= hi
    return i0, i1, i2


def draws(seed, H, M):
    return np.array([draw(seed, h, M) for h in range(H)], np.int64).reshape(H, 3)


def widen(x):
    """[M, stride >= 3] float32 -> [M, 3] float64"""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 2 and x.shape[1] >= 3
    return x[:, :3].astype(np.float64)


def live(P, Q):
    return np.isfinite(P).all(1) & np.isfinite(Q).all(1)


def norm2(d):
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _spread(e1, e2, min_sin2):
    cx = e1[..., 1] * e2[..., 2] - e1[..., 2] * e2[..., 1]
    cy = e1[..., 2] * e2[..., 0] - e1[..., 0] * e2[..., 2]
    cz = e1[..., 0] * e2[..., 1] - e1[..., 1] * e2[..., 0]
    c2 = (cx * cx + cy * cy) + cz * cz
    return ~(c2 <= min_sin2 * (norm2(e1) * norm2(e2)))


def triples_ok(P, Q, idx, edge_similarity, min_sin2):
    """the pre-rejection verdict of every triple idx [H, 3] over the widened correspondences P -> Q"""
    with np.errstate(invalid="ignore", over="ignore"):
        p, q = P[idx], Q[idx]                                   # [H, 3, 3]
        ok = np.isfinite(p).all((1, 2)) & np.isfinite(q).all((1, 2))
        s2 = np.float64(edge_similarity) * np.float64(edge_similarity)
        for a, b in ((0, 1), (0, 2), (1, 2)):
            dp, dq = norm2(p[:, b] - p[:, a]), norm2(q[:, b] - q[:, a])
            ok &= (dp > 0) & (dq > 0) & (dp >= s2 * dq) & (dq >= s2 * dp)
        ok &= _spread(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0], np.float64(min_sin2))
        ok &= _spread(q[:, 1] - q[:, 0], q[:, 2] - q[:, 0], np.float64(min_sin2))
    return ok


def kabsch(a, b):
    """4x4 D = [R t; 0 1] with the proper rotation that minimises sum |R a + t - b|^2"""
    ab, bb = a.mean(0), b.mean(0)
    H = (a - ab).T @ (b - bb)
    if not np.isfinite(H).all() or not H.any():
        R = np.eye(3)
    else:
        U, _, Vt = np.linalg.svd(H)
        d = 1.0 if np.linalg.det(Vt.T @ U.T) >= 0 else -1.0
        R = Vt.T @ np.diag([1.0, 1.0, d]) @ U.T
    D = np.eye(4)
    D[:3, :3] = R
    D[:3, 3] = bb - R @ ab
    return D


def residual2(D, P, Q):
    with np.errstate(invalid="ignore", over="ignore"):
        e = [(((D[r, 0] * P[:, 0] + D[r, 1] * P[:, 1]) + D[r, 2] * P[:, 2]) + D[r, 3]) - Q[:, r] for r in range(3)]
        return (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]


def ransac(src, dst, seed, max_distance, hypotheses=4096, refine_iters=3, edge_similarity=0.9, min_sin2=1e-6):
    """one pair.  -> dict: T [4, 4], info int32 [4] = {inliers, best_h, valid, refits_done}, mask uint8 [M], and for the tests: margin (the
    smallest |e2 - d^2| / d^2 over every valid hypothesis and refit step), counts (the score of every valid hypothesis, -1 for the
    rejected), hist (|S_j| of every iterate)."""
    P, Q = widen(src), widen(dst)
    M, H = P.shape[0], int(hypotheses)
    d2 = np.float64(max_distance) * np.float64(max_distance)
    out = dict(T=np.eye(4), info=np.array([0, -1, 0, 0], np.int32), mask=np.zeros(M, np.uint8), margin=np.inf,
               counts=np.full(H, -1, np.int64), hist=[], models={})
    if M < 3:
        return out
    alive = live(P, Q)
    idx = draws(int(seed), H, M)
    ok = triples_ok(P, Q, idx, edge_similarity, min_sin2)
    out["idx"], out["ok"] = idx, ok
    out["info"][2] = int(ok.sum())
    if not ok.any():
        return out

    def inliers(D):
        e2 = residual2(D, P, Q)
        with np.errstate(invalid="ignore"):
            m = alive & (e2 <= d2)
            out["margin"] = min(out["margin"], float(np.abs(e2[alive] - d2).min() / d2)) if alive.any() else out["margin"]
        return m

    best = (-1, -1)
    for h in np.nonzero(ok)[0]:
        D = kabsch(P[idx[h]], Q[idx[h]])
        out["models"][int(h)] = D
        c = int(inliers(D).sum())
        out["counts"][h] = c
        if c > best[0]:                                          # ties stay with the lowest h
            best = (c, int(h))
    T = out["models"][best[1]]
    S = inliers(T)
    hist, done = [int(S.sum())], 0
    pick = (hist[0], T, S)
    for j in range(1, int(refine_iters) + 1):
        if S.sum() < 3:
            break
        Tj = kabsch(P[S], Q[S])
        Sj = inliers(Tj)
        done = j
        hist.append(int(Sj.sum()))
        if hist[-1] > pick[0]:                                   # ties stay with the lowest j
            pick = (hist[-1], Tj, Sj)
        same = np.array_equal(Sj, S)
        S = Sj
        if same:
            break
    out.update(T=pick[1], mask=pick[2].astype(np.uint8), hist=hist)
    out["info"][:] = [pick[0], best[1], int(ok.sum()), done]
    return out


def ransac_batch(src, dst, offsets, seeds, max_distance, **kw):
    res = [ransac(src[offsets[i]:offsets[i + 1]], dst[offsets[i]:offsets[i + 1]], seeds[i], max_distance, **kw) for i in range(len(offsets) - 1)]
    return (np.stack([r["T"] for r in res]), np.stack([r["info"] for r in res]),
            np.concatenate([r["mask"] for r in res]) if res else np.zeros(0, np.uint8), res)
