"""NumPy / scipy restatement of the pose-graph optimiser's marginal covariances: the information matrix of stage 2 at a
given result, its inverse by two exact routes, the change of frame and the covariance of a relative pose.  Test infrastructure only, built
on posegraph_robust_restate.py; everything is float64.

The inputs are public results of the handle under test (its poses T, its stage-1 poses T0 for the rotations the factors' information is
formed with, its loop weights w), so a comparison against this text isolates the inversion."""
import os
import sys

import numpy as np
import scipy.linalg

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import posegraph_restate as R  # noqa: E402
import posegraph_robust_restate as RR  # noqa: E402

CHORDAL, POSE3 = 0, 1


def information_matrix(T, T0, chain_lengths, odom, li, lj, lZ, oC=None, lC=None, w=None):
    """H dense [6 (N - 1)]^2 = sum_f w_f J_f^T Lam_f J_f at T with pose 0 held: Lam_f from the factor's covariance and the stage-1 rotation
    of its first pose (the unit model without one), w_f = 1 for odometry factors and w[u] for loop u"""
    fi, fj, fZ = R.factors(chain_lengths, odom, li, lj, lZ)
    n_loops = np.asarray(li).size
    n_odometry = fi.size - n_loops
    Lam = RR.information(T0, fi, RR.covariances(n_odometry, n_loops, oC, lC))
    scale = np.ones(fi.size)
    if w is not None and n_loops:
        scale[n_odometry:] = w
    H, _ = RR.system(T, fi, fj, fZ, Lam * scale[:, None, None])
    return H.toarray()


def inverse_direct(H):
    return np.linalg.inv(H)


def inverse_cholesky_reversed(H):
    """the inverse through a Cholesky factorisation of the system with its poses in reverse order"""
    n = H.shape[0] // 6
    perm = (6 * np.arange(n)[::-1, None] + np.arange(6)[None, :]).reshape(-1)
    c = scipy.linalg.cho_factor(H[np.ix_(perm, perm)], lower=True)
    X = scipy.linalg.cho_solve(c, np.eye(H.shape[0]))
    out = np.empty_like(X)
    out[np.ix_(perm, perm)] = X
    return out


def with_held_pose(S):
    """[6 N]^2 from the free poses' [6 (N - 1)]^2: the held pose 0 has zero rows and columns"""
    out = np.zeros((S.shape[0] + 6, S.shape[0] + 6))
    out[6:, 6:] = S
    return out


def spread(a, b):
    """max |a - b| / max |b|: the measure of every comparison of covariances"""
    m = np.abs(b).max() if np.size(b) else 0.0
    return float(np.abs(a - b).max() / m) if m > 0 else float(np.abs(a - b).max() if np.size(a) else 0.0)


def frame_matrix(T):
    """blockdiag over the poses of blockdiag(I, R^T): the optimiser's tangent (R <- R Exp(d[:3]), t <- t + d[3:]) to Pose3 local
    coordinates (rotation, then translation in the body frame) to first order"""
    N = T.shape[0]
    M = np.zeros((6 * N, 6 * N))
    for p in range(N):
        M[6 * p:6 * p + 3, 6 * p:6 * p + 3] = np.eye(3)
        M[6 * p + 3:6 * p + 6, 6 * p + 3:6 * p + 6] = T[p, :3, :3].T
    return M


def in_frame(S, T, frame):
    """S [6 N]^2 of the optimiser's tangent in `frame`"""
    if frame == CHORDAL:
        return S
    M = frame_matrix(T)
    return M @ S @ M.T


def marginals(S):
    """[N, 6, 6]: the diagonal blocks"""
    N = S.shape[0] // 6
    return np.array([S[6 * p:6 * p + 6, 6 * p:6 * p + 6] for p in range(N)]).reshape(N, 6, 6)


def joint(S, i, j):
    """[12, 12] of poses i and j"""
    idx = np.concatenate([6 * i + np.arange(6), 6 * j + np.arange(6)])
    return S[np.ix_(idx, idx)]


def adjoint(T):
    """Ad(T) = [[R, 0], [skew(t) R, R]] in the order (rotation, translation)"""
    Rm, t = T[:3, :3], T[:3, 3]
    A = np.zeros((6, 6))
    A[:3, :3] = Rm
    A[3:, 3:] = Rm
    A[3:, :3] = R.skew(t) @ Rm
    return A


def between_covariance(joint_pose3, Ti, Tj):
    """the 6 x 6 covariance of Z = Ti^-1 Tj in Pose3 local coordinates from the joint marginal [12, 12] of (i, j) in the Pose3 frame:
    J S J^T with J = [-Ad(Z^-1), I]"""
    Z = np.linalg.solve(Ti, Tj)
    J = np.hstack([-adjoint(np.linalg.inv(Z)), np.eye(6)])
    return J @ joint_pose3 @ J.T


def separators(chain_lengths, li, lj, segment_length, marks=()):
    """is_sep [N] of stage 2: the loops' poses, pose 0, the marked poses, and a cut after every run of segment_length other poses of a
    chain (0: no cuts)"""
    N = int(sum(chain_lengths))
    is_sep = np.zeros(N, bool)
    is_sep[np.asarray(li, int)] = True
    is_sep[np.asarray(lj, int)] = True
    is_sep[np.asarray(list(marks), int)] = True
    is_sep[0] = True
    start = 0
    for n in chain_lengths:
        run = 0
        for p in range(start, start + n):
            if is_sep[p]:
                run = 0
            elif segment_length > 0 and run == segment_length:
                is_sep[p] = True
                run = 0
            else:
                run += 1
        start += n
    return is_sep


def segments(chain_lengths, is_sep):
    """(first, length, left, right) per run of poses that are not separators: left / right are the bounding poses, or -1 at a chain's end
    and behind the held pose 0"""
    out, start = [], 0
    for n in chain_lengths:
        p, end = start, start + n
        while p < end:
            if is_sep[p]:
                p += 1
                continue
            q = p
            while q < end and not is_sep[q]:
                q += 1
            out.append((p, q - p, p - 1 if p - 1 > max(start - 1, 0) else -1, q if q < end else -1))
            p = q
        start += n
    return out
