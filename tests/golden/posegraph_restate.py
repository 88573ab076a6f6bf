"""NumPy / scipy restatement of the pose-graph contract: chordal relaxation for the rotations, then Gauss-Newton on
BetweenChordalFactor errors (Mapping/src/global_manager: evaluation_utils.cpp:273-329, between_chordal_factor.h:97-144).  Test
infrastructure only: the definition the GPU path (mr_slam_amd/csrc/posegraph.hip) is compared with.  Everything is float64.

Poses are numbered chain after chain; factor f < N - nr is the odometry factor of a consecutive pair, the loop factors follow in the order
given.  A factor (i, j, Z) measures the pose of j in the frame of i."""
import collections

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spl

EPS_DEFAULT, MAX_ITERATIONS_DEFAULT = 1e-9, 200
SMALL_ANGLE = 1e-4                       # below it Exp uses the series of sin(t)/t and (1 - cos t)/t^2

Result = collections.namedtuple("Result", "T iterations converged max_delta error_initial error_final deltas")


def skew(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


# skewSymmetric(-1, 0, 0), (0, -1, 0), (0, 0, -1) (between_chordal_factor.h:100-102)
S = np.stack([skew(-np.eye(3)[k]) for k in range(3)])


def exp_so3(w):
    """Rodrigues: I + a W + b W^2, a = sin t / t, b = (1 - cos t) / t^2, by their series below SMALL_ANGLE"""
    w = np.asarray(w, np.float64)
    t2 = float(w @ w)
    t = np.sqrt(t2)
    if t < SMALL_ANGLE:
        a, b = 1.0 - t2 / 6.0, 0.5 - t2 / 24.0
    else:
        a, b = np.sin(t) / t, (1.0 - np.cos(t)) / t2
    W = skew(w)
    return np.eye(3) + a * W + b * (W @ W)


def retract(T, delta):
    """retractPose3Global (evaluation_utils.cpp:89-99) with Exp for Rot3::retract: R <- R Exp(delta[0:3]), t <- t + delta[3:6]"""
    out = np.array(T, np.float64, copy=True)
    for p in range(out.shape[0]):
        out[p, :3, :3] = T[p, :3, :3] @ exp_so3(delta[p, :3])
        out[p, :3, 3] = T[p, :3, 3] + delta[p, 3:]
    return out


def factor_error(Ti, Tj, Z):
    """the 12-vector of between_chordal_factor.h:104-122: the columns of Ri Rij - Rj, then tj - ti - Ri tij"""
    E = Ti[:3, :3] @ Z[:3, :3] - Tj[:3, :3]
    return np.concatenate([E.T.reshape(9), Tj[:3, 3] - Ti[:3, 3] - Ti[:3, :3] @ Z[:3, 3]])


def factor_jacobians(Ti, Tj, Z):
    """Hi, Hj [12, 6] of between_chordal_factor.h:127-139"""
    Ri, Rj, Rij, tij = Ti[:3, :3], Tj[:3, :3], Z[:3, :3], Z[:3, 3]
    Hi, Hj = np.zeros((12, 6)), np.zeros((12, 6))
    for k in range(3):
        Hi[3 * k:3 * k + 3, :3] = Ri @ Rij @ S[k] @ Rij.T
        Hj[3 * k:3 * k + 3, :3] = -Rj @ S[k]
    Hi[9:, :3] = Ri @ skew(tij)
    Hi[9:, 3:] = -np.eye(3)
    Hj[9:, 3:] = np.eye(3)
    return Hi, Hj


def _linearize(T, fi, fj, fZ):
    """all factors at once -> e [F, 12], Hi [F, 12, 6], Hj [F, 12, 6]; the same arithmetic as factor_error / factor_jacobians"""
    F = fi.size
    Ri, Rj, Rij, tij = T[fi, :3, :3], T[fj, :3, :3], fZ[:, :3, :3], fZ[:, :3, 3]
    RiRij = Ri @ Rij
    E = RiRij - Rj
    e = np.concatenate([E.transpose(0, 2, 1).reshape(F, 9), T[fj, :3, 3] - T[fi, :3, 3] - np.einsum("fab,fb->fa", Ri, tij)], axis=1)
    Hi, Hj = np.zeros((F, 12, 6)), np.zeros((F, 12, 6))
    RijT = Rij.transpose(0, 2, 1)
    for k in range(3):
        Hi[:, 3 * k:3 * k + 3, :3] = RiRij @ S[k] @ RijT
        Hj[:, 3 * k:3 * k + 3, :3] = -Rj @ S[k]
    K = np.zeros((F, 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -tij[:, 2], tij[:, 1], tij[:, 2], -tij[:, 0], -tij[:, 1], tij[:, 0]
    Hi[:, 9:, :3] = Ri @ K
    Hi[:, 9:, 3:] = -np.eye(3)
    Hj[:, 9:, 3:] = np.eye(3)
    return e, Hi, Hj


def total_error(T, fi, fj, fZ):
    """0.5 sum |e|^2 over the odometry and loop factors: the reference's "Initial Error" / "GN Error" (global_manager.cpp:1339, 1355)"""
    if fi.size == 0:
        return 0.0
    e, _, _ = _linearize(T, fi, fj, fZ)
    return 0.5 * float((e * e).sum())


def chain_starts(chain_lengths):
    n = np.asarray(chain_lengths, np.int64).reshape(-1)
    return np.concatenate([[0], np.cumsum(n)])


def factors(chain_lengths, odom, li, lj, lZ):
    """(fi, fj, fZ): the odometry factors chain after chain, then the loops"""
    st = chain_starts(chain_lengths)
    oi = np.concatenate([np.arange(st[r], st[r + 1] - 1) for r in range(st.size - 1)] + [np.zeros(0, np.int64)]).astype(np.int64)
    odom = np.asarray(odom, np.float64).reshape(-1, 4, 4)
    assert odom.shape[0] == oi.size, (odom.shape, oi.size)
    li, lj = np.asarray(li, np.int64).reshape(-1), np.asarray(lj, np.int64).reshape(-1)
    lZ = np.asarray(lZ, np.float64).reshape(-1, 4, 4)
    return np.concatenate([oi, li]), np.concatenate([oi + 1, lj]), np.concatenate([odom, lZ])


def connected(chain_lengths, li, lj):
    """every chain reaches chain 0 through loop factors"""
    st = chain_starts(chain_lengths)
    nr = st.size - 1
    chain_of = lambda p: int(np.searchsorted(st, p, side="right") - 1)
    seen, todo = {0}, [0]
    adj = collections.defaultdict(set)
    for a, b in zip(np.asarray(li).reshape(-1), np.asarray(lj).reshape(-1)):
        ca, cb = chain_of(a), chain_of(b)
        adj[ca].add(cb)
        adj[cb].add(ca)
    while todo:
        for c in adj[todo.pop()]:
            if c not in seen:
                seen.add(c)
                todo.append(c)
    return len(seen) == nr


def _solve(H, g, order):
    """order None: sparse LU; else a dense Cholesky of the system permuted by the seed `order`"""
    if order is None:
        return spl.spsolve(H.tocsc(), g)
    n = H.shape[0]
    perm = np.random.default_rng(order).permutation(n)
    A = H.toarray()[np.ix_(perm, perm)]
    L = np.linalg.cholesky(A)
    import scipy.linalg as sl
    y = sl.solve_triangular(L, g[perm], lower=True)
    x = sl.solve_triangular(L.T, y, lower=False)
    out = np.empty_like(x)
    out[perm] = x
    return out


def relaxed_rotations(N, fi, fj, fZ, prior=None, order=None):
    """stage 1 before the projection (evaluation_utils.cpp:176-213): X [N, 3, 3], the rows are the three solved vectors.  Node N is the
    anchor; the prior on pose 0 is the between factor anchor -> pose 0 with the prior's rotation."""
    Rp = np.eye(3) if prior is None else np.asarray(prior, np.float64)[:3, :3]
    ai = np.concatenate([fi, [N]])
    aj = np.concatenate([fj, [0]])
    aR = np.concatenate([fZ[:, :3, :3], Rp[None]])
    F, n = ai.size, N + 1
    # residual Rij x_j - x_i per row of the rotations: rows 3 f .. 3 f + 2 of A
    rows, cols, vals = [], [], []
    for a in range(3):
        rows.append(3 * np.arange(F) + a)
        cols.append(3 * ai + a)
        vals.append(-np.ones(F))
        for b in range(3):
            rows.append(3 * np.arange(F) + a)
            cols.append(3 * aj + b)
            vals.append(aR[:, a, b])
    for a in range(3):                                           # the anchor's prior: x_a - e_k
        rows.append(np.array([3 * F + a]))
        cols.append(np.array([3 * N + a]))
        vals.append(np.ones(1))
    A = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(3 * F + 3, 3 * n)).tocsr()
    H = (A.T @ A).tocsc()
    X = np.empty((N, 3, 3))
    for k in range(3):
        b = np.zeros(3 * F + 3)
        b[3 * F + k] = 1.0
        x = _solve(H, A.T @ b, order)
        X[:, k, :] = x[:3 * N].reshape(N, 3)
    return X


def closest_rotation(X):
    """U diag(1, 1, det(U V^T)) V^T of X = U S V^T"""
    U, _, Vt = np.linalg.svd(X)
    d = np.linalg.det(U @ Vt)
    return U @ np.diag([1.0, 1.0, d]) @ Vt


def initialize(chain_lengths, odom, li, lj, lZ, prior=None, order=None):
    """stage 1: (T [N, 4, 4] with the projected rotations and zero translations, X [N, 3, 3] before the projection)"""
    fi, fj, fZ = factors(chain_lengths, odom, li, lj, lZ)
    N = int(np.sum(chain_lengths))
    X = relaxed_rotations(N, fi, fj, fZ, prior, order)
    T = np.tile(np.eye(4), (N, 1, 1))
    for p in range(N):
        T[p, :3, :3] = closest_rotation(X[p])
    return T, X


def gn_delta(T, fi, fj, fZ, order=None):
    """one Gauss-Newton step with pose 0 held: delta [N, 6] of (sum J^T J) delta = -sum J^T e"""
    N = T.shape[0]
    delta = np.zeros((N, 6))
    if N == 1:
        return delta
    e, Hi, Hj = _linearize(T, fi, fj, fZ)
    F = fi.size
    # J: rows 12 f .. 12 f + 11, columns 6 p .. 6 p + 5; pose 0's columns are dropped afterwards
    r = (12 * np.arange(F)[:, None, None] + np.arange(12)[None, :, None] + np.zeros((1, 1, 6), np.int64))
    ci = 6 * fi[:, None, None] + np.arange(6)[None, None, :] + np.zeros((1, 12, 1), np.int64)
    cj = 6 * fj[:, None, None] + np.arange(6)[None, None, :] + np.zeros((1, 12, 1), np.int64)
    J = sp.coo_matrix((np.concatenate([Hi.reshape(-1), Hj.reshape(-1)]),
                       (np.concatenate([r.reshape(-1), r.reshape(-1)]), np.concatenate([ci.reshape(-1), cj.reshape(-1)]))),
                      shape=(12 * F, 6 * N)).tocsc()[:, 6:]
    H = (J.T @ J).tocsc()
    g = -(J.T @ e.reshape(-1))
    delta[1:] = _solve(H, g, order).reshape(N - 1, 6)
    return delta


def optimize(chain_lengths, odom, li, lj, lZ, prior=None, eps=EPS_DEFAULT, max_iterations=MAX_ITERATIONS_DEFAULT, order=None, iterations=None):
    """both stages -> Result.  The loop stops when max|delta| < eps or after max_iterations; `iterations` forces an exact count (for the
    solve-order comparison, which must not depend on the stop rule)."""
    fi, fj, fZ = factors(chain_lengths, odom, li, lj, lZ)
    if not connected(chain_lengths, li, lj):
        raise ValueError("a chain is not connected to chain 0")
    T, _ = initialize(chain_lengths, odom, li, lj, lZ, prior, order)
    e0 = total_error(T, fi, fj, fZ)
    its, conv, md, deltas = 0, False, 0.0, []
    limit = max_iterations if iterations is None else iterations
    while its < limit:
        d = gn_delta(T, fi, fj, fZ, order)
        T = retract(T, d)
        md = float(np.abs(d).max())
        deltas.append(md)
        its += 1
        if iterations is None and md < eps:
            conv = True
            break
    return Result(T, its, conv, md, e0, total_error(T, fi, fj, fZ), deltas)
