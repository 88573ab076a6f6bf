"""NumPy restatement of the reference's Pairwise Consistency Maximisation for one robot pair
(Mapping/src/global_manager/src/pairwise_consistency_maximization/): the consistency distance of every pair of inter-robot loops
(pairwise_consistency.cpp:40-137, with gtsam's Pose3::Logmap restated from upstream GTSAM 4.0) and the clique heuristic FMC::maxCliqueHeu
(third_parties/fast_max-clique_finder/src/findCliqueHeu.cpp:120-243) in its sequential form.  DESIGN.md 4.18 holds the contract.

Poses are [..., 4, 4] float64 arrays.  ref_pcm_clique.npz (written by tools/make_pcm_golden.py) holds graphs and what the reference's own
clique finder returned for them."""
import os

import numpy as np

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref_pcm_clique.npz")
THRESHOLDS = {0.01: 0.872, 0.05: 1.635, 0.10: 2.204, 0.25: 3.455, 0.50: 5.348, 0.75: 7.840}    # pairwise_consistency.cpp:7-38, dof 6


def inverse(T):
    """gtsam Pose3::inverse: (R^T, -R^T t)"""
    T = np.asarray(T, np.float64)
    out = np.zeros_like(T)
    Rt = np.swapaxes(T[..., :3, :3], -1, -2)
    out[..., :3, :3] = Rt
    out[..., :3, 3] = -(Rt @ T[..., :3, 3:4])[..., 0]
    out[..., 3, 3] = 1.0
    return out


def rot_logmap(R):
    """Rot3::Logmap of [n, 3, 3] -> [n, 3]"""
    R = np.asarray(R, np.float64).reshape(-1, 3, 3)
    tr = R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2]
    with np.errstate(invalid="ignore", divide="ignore"):
        tr_3 = tr - 3.0
        theta = np.arccos((tr - 1.0) / 2.0)
        m = np.where(tr_3 < -1e-7, theta / (2.0 * np.sin(theta)), 0.5 - tr_3 * tr_3 / 12.0)
        w = m[:, None] * np.stack([R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]], 1)
        for n in np.nonzero(np.abs(tr + 1.0) < 1e-10)[0]:
            r = R[n]
            if abs(r[2, 2] + 1.0) > 1e-10:
                w[n] = (np.pi / np.sqrt(2.0 + 2.0 * r[2, 2])) * np.array([r[0, 2], r[1, 2], 1.0 + r[2, 2]])
            elif abs(r[1, 1] + 1.0) > 1e-10:
                w[n] = (np.pi / np.sqrt(2.0 + 2.0 * r[1, 1])) * np.array([r[0, 1], 1.0 + r[1, 1], r[2, 1]])
            else:
                w[n] = (np.pi / np.sqrt(2.0 + 2.0 * r[0, 0])) * np.array([1.0 + r[0, 0], r[1, 0], r[2, 0]])
    return w


def logmap(T):
    """Pose3::Logmap of [n, 4, 4] (or one [4, 4]) -> [n, 6] = [omega, u]"""
    T = np.asarray(T, np.float64)
    one = T.ndim == 2
    T = T.reshape(-1, 4, 4)
    w = rot_logmap(T[:, :3, :3])
    t = T[:, :3, 3]
    th = np.sqrt(np.sum(w * w, 1))
    big = th >= 1e-10                       # a NaN angle goes to the small-angle branch and stays NaN
    with np.errstate(invalid="ignore", divide="ignore"):
        ths = np.where(big, th, 1.0)
        a = w / ths[:, None]
        Wt = np.cross(a, t)
        WWt = np.cross(a, Wt)
        u = t - (0.5 * ths)[:, None] * Wt + (1.0 - ths / (2.0 * np.tan(0.5 * ths)))[:, None] * WWt
    u = np.where(big[:, None], u, t)
    out = np.concatenate([w, u], 1)
    return out[0] if one else out


def consistency_distances(XA, XB, ia, kb, Z):
    """[L, L] float64: d(u, v) = |Logmap(Z_u^-1 (XA_i^-1 XA_j) Z_v (XB_l^-1 XB_k))| for u < v, mirrored, zero diagonal"""
    XA, XB, Z = (np.asarray(a, np.float64) for a in (XA, XB, Z))
    ia, kb = np.asarray(ia, np.int64), np.asarray(kb, np.int64)
    L = ia.size
    D = np.zeros((L, L))
    u, v = np.triu_indices(L, 1)
    if u.size:
        with np.errstate(invalid="ignore"):
            aXij = inverse(XA[ia[u]]) @ XA[ia[v]]
            bXlk = inverse(XB[kb[v]]) @ XB[kb[u]]
            E = inverse(Z[u]) @ ((aXij @ Z[v]) @ bXlk)
            xi = logmap(E)
            d = np.sqrt(np.sum(xi * xi, 1))
        D[u, v] = d
        D[v, u] = d
    return D


def consistency_matrix(D, threshold):
    """bool [L, L]: d < threshold off the diagonal; a distance that is not finite is not consistent"""
    with np.errstate(invalid="ignore"):
        A = D < threshold
    np.fill_diagonal(A, False)
    return A


def max_clique_heu(A):
    """FMC::maxCliqueHeu on a symmetric boolean adjacency with a zero diagonal -> (size, member list); (-1, []) for no vertex"""
    A = np.asarray(A, bool)
    n = A.shape[0]
    deg = A.sum(1)
    max_clq, best = -1, []
    for c in range(n):
        if max_clq > deg[c]:
            continue
        # the reference's list S = [c] + its eligible neighbours in ascending order, kept as (c is in it, the others)
        elig = deg >= max_clq
        has_c, others = True, np.flatnonzero(A[c] & elig)
        icc, members = 0, [c]
        while has_c or others.size:
            icc += 1
            m = int(others[-1]) if others.size else c               # the last element of S
            has_c = bool(has_c and A[m, c] and elig[c])
            others = others[A[m, others] & elig[others]]
            if has_c or others.size:
                members.append(m)
        if max_clq < icc:
            max_clq, best = icc, members
    return max_clq, best


def load():
    """[(n, edges int32 [m, 2] with u < v in row-major order, size, members)] of the fixture"""
    z = np.load(FIXTURE)
    return [(int(z["n"][g]), z["edges_%d" % g], int(z["size"][g]), z["members_%d" % g]) for g in range(z["n"].size)]


def adjacency(n, edges):
    A = np.zeros((n, n), bool)
    if len(edges):
        A[edges[:, 0], edges[:, 1]] = True
        A[edges[:, 1], edges[:, 0]] = True
    return A
