"""NumPy restatement of the point-to-point ICP contract: pcl::IterativeClosestPoint with
TransformationEstimationSVD and DefaultConvergenceCriteria (max_iterations_similar_transforms = 0), as the Mapping node configures it at
global_manager.cpp:890-906 and :2427-2434.  PCL is not part of the reference tree, so this restates the DEFINITION, not PCL's text, and parity
with PCL is unpinned.  Test infrastructure: the product never imports it.

Per iteration: exact 1-NN of the float32-transformed source points (the searches' own float operation chain, ties to the smaller index),
kept where d^2 < max^2; 17 sums in float64 with the float64 pose applied to the float32 points; Umeyama without scale; X <- D X; PCL's stopping
rules in PCL's order."""
import numpy as np
from scipy.spatial import cKDTree

DBL_MAX = np.finfo(np.float64).max
STATES = ("NOT_CONVERGED", "ITERATIONS", "TRANSFORM", "ABS_MSE", "REL_MSE", "NO_CORRESPONDENCES")
NOT_CONVERGED, ITERATIONS, TRANSFORM, ABS_MSE, REL_MSE, NO_CORRESPONDENCES = range(6)
DEFAULTS = dict(max_iterations=10, force_iterations=0, max_correspondence_distance=np.sqrt(DBL_MAX), transformation_epsilon=0.0,
                rotation_epsilon=0.0, euclidean_fitness_epsilon=-DBL_MAX)
MAPPING_890 = dict(max_correspondence_distance=2.0, max_iterations=50, transformation_epsilon=1e-3, euclidean_fitness_epsilon=1e-3)


def _f32(a):
    return np.ascontiguousarray(np.asarray(a)[:, :3], dtype=np.float32)


def transform_f32(T, A):
    """the searches' chain: pose narrowed to float32, q = T0 x + T1 y + T2 z + T3 with one rounding per operation, left to right"""
    Tf = np.asarray(T, np.float64).astype(np.float32)
    A = _f32(A)
    return np.stack([Tf[r, 0] * A[:, 0] + Tf[r, 1] * A[:, 1] + Tf[r, 2] * A[:, 2] + Tf[r, 3] for r in range(3)], 1)


def d2_f32(q, b):
    """fma(dz, dz, fma(dy, dy, dx * dx)) in float32 (products of two float32 are exact in float64)"""
    d = (q - b).astype(np.float32)
    s = (d[..., 0] * d[..., 0]).astype(np.float32)
    for c in (1, 2):
        s = (d[..., c].astype(np.float64) * d[..., c].astype(np.float64) + s.astype(np.float64)).astype(np.float32)
    return s


class Target:
    def __init__(self, B):
        self.B = _f32(B)
        self.tree = cKDTree(self.B.astype(np.float64))

    def nearest(self, q):
        """exact nearest neighbour under the float32 distance chain: the float64 tree proposes, the chain decides (ties: smaller index)"""
        k = min(4, self.B.shape[0])
        _, idx = self.tree.query(q.astype(np.float64), k=k)
        idx = idx.reshape(q.shape[0], k)
        d = d2_f32(q[:, None, :], self.B[idx])
        order = np.lexsort((idx, d), axis=1)[:, 0]
        rows = np.arange(q.shape[0])
        return idx[rows, order].astype(np.int64), d[rows, order]


def correspondences(A, tgt, X, max_corr):
    """step 1: (corr [n] int, -1 where rejected; d2 float32 of the nearest neighbour)"""
    j, d = tgt.nearest(transform_f32(X, A))
    max2 = np.inf if max_corr >= 1e150 else float(max_corr) * float(max_corr)
    return np.where(d.astype(np.float64) < max2, j, -1), d


def sums17(A, B, X, corr):
    """step 3: n, sum a, sum b, sum a b^T (row-major), sum |b - a|^2 over the kept correspondences, a = X A_i in float64"""
    keep = corr >= 0
    a = _f32(A)[keep].astype(np.float64) @ X[:3, :3].T + X[:3, 3]
    b = _f32(B)[corr[keep]].astype(np.float64)
    return np.concatenate([[float(keep.sum())], a.sum(0), b.sum(0), (a.T @ b).reshape(-1), [((b - a) ** 2).sum()]]), a, b


def rigid_fit(a, b):
    """step 4 on the point sets themselves (centred: no cancellation): D = [R t] with R = V diag(1, 1, det(V U^T)) U^T"""
    abar, bbar = a.mean(0), b.mean(0)
    H = (a - abar).T @ (b - bbar)
    U, _, Vt = np.linalg.svd(H)
    V = Vt.T
    R = V @ np.diag([1.0, 1.0, np.sign(np.linalg.det(V @ U.T)) or 1.0]) @ U.T
    D = np.eye(4)
    D[:3, :3] = R
    D[:3, 3] = bbar - R @ abar
    return D


def rotation_threshold(rotation_epsilon, transformation_epsilon):
    return rotation_epsilon if rotation_epsilon > 0 else 1.0 - transformation_epsilon


def criteria(D, mse, prev_mse):
    """the values step 6 compares: cosine of the increment's angle, squared translation, |mse - prev|, relative change"""
    cos = 0.5 * (np.trace(D[:3, :3]) - 1.0)
    t2 = float(D[:3, 3] @ D[:3, 3])
    d = abs(mse - prev_mse)
    return cos, t2, d, d / prev_mse


def converged(it, cos, t2, d_abs, rel, max_iterations, transformation_epsilon, rotation_epsilon, euclidean_fitness_epsilon):
    """step 6: the state that ends the pair after iteration `it` (counted from 1), or NOT_CONVERGED; PCL's order"""
    if it >= max_iterations:
        return ITERATIONS
    if cos >= rotation_threshold(rotation_epsilon, transformation_epsilon) and t2 <= transformation_epsilon:
        return TRANSFORM
    if d_abs < 1e-12:
        return ABS_MSE
    if rel < euclidean_fitness_epsilon:
        return REL_MSE
    return NOT_CONVERGED


def step(A, B, X, max_corr, tgt=None):
    """steps 1-4 once at pose X: (corr, d2, sums [17], delta [4,4]; identity below 3 correspondences)"""
    tgt = tgt or Target(B)
    X = np.asarray(X, np.float64)
    corr, d2 = correspondences(A, tgt, X, max_corr)
    s, a, b = sums17(A, B, X, corr)
    return corr, d2, s, (rigid_fit(a, b) if s[0] >= 3 else np.eye(4))


def icp(A, B, guess=None, **params):
    """Returns dict(T: X narrowed to float32, X: float64 pose, converged, iterations, state, trace: [(cos, t2, mse, rel, n)] per iteration)."""
    p = dict(DEFAULTS)
    assert set(params) <= set(p), params
    p.update(params)
    tgt = Target(B)
    X = (np.eye(4) if guess is None else np.asarray(guess, np.float64)).astype(np.float32).astype(np.float64)
    prev, it, state, conv, trace = DBL_MAX, 0, NOT_CONVERGED, False, []
    limit = p["force_iterations"] if p["force_iterations"] > 0 else p["max_iterations"]
    while it < limit:
        corr, _ = correspondences(A, tgt, X, p["max_correspondence_distance"])
        s, a, b = sums17(A, B, X, corr)
        if s[0] < 3:
            state = NO_CORRESPONDENCES
            break
        D = rigid_fit(a, b)
        X = D @ X
        it += 1
        mse = s[16] / s[0]
        cos, t2, d_abs, rel = criteria(D, mse, prev)
        trace.append((cos, t2, mse, rel, int(s[0])))
        if p["force_iterations"] > 0:
            continue
        state = converged(it, cos, t2, d_abs, rel, p["max_iterations"], p["transformation_epsilon"], p["rotation_epsilon"],
                          p["euclidean_fitness_epsilon"])
        if state != NOT_CONVERGED:
            conv = True
            break
        prev = mse
    return dict(T=X.astype(np.float32).astype(np.float64), X=X, converged=conv, iterations=it, state=state, trace=trace)


def margins(trace, **params):
    """For every iteration of a trace: how far (as a factor >= 1) each criterion value lies from its threshold -- 1 - cos against
    1 - rotation threshold, |t|^2 against transformation_epsilon, |mse - prev| against 1e-12, the relative change against
    euclidean_fitness_epsilon.  A fixture is only used for a natural-stopping comparison if every factor is at least 1.25."""
    p = dict(DEFAULTS)
    p.update(params)

    def factor(v, thr):
        if thr <= 0 or v <= 0:
            return np.inf           # a threshold that can never be met, or a value that is exactly on the far side
        with np.errstate(over="ignore"):
            return max(v / thr, thr / v)
    out, prev = [], DBL_MAX
    for cos, t2, mse, rel, _ in trace:
        out.append((factor(1.0 - cos, 1.0 - rotation_threshold(p["rotation_epsilon"], p["transformation_epsilon"])),
                    factor(t2, p["transformation_epsilon"]), factor(abs(mse - prev), 1e-12), factor(rel, p["euclidean_fitness_epsilon"])))
        prev = mse
    return out


def fitness(A, B, T, max_range, tgt=None):
    """getFitnessScore: mean squared nearest-neighbour distance over d^2 <= max_range at the float32 pose (DBL_MAX when empty)"""
    tgt = tgt or Target(B)
    _, d = tgt.nearest(transform_f32(T, A))
    d = d.astype(np.float64)
    keep = d <= max_range
    return float(d[keep].mean()) if keep.any() else DBL_MAX
