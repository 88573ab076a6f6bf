"""NumPy restatement of pairwise consistency with covariances: the Mahalanobis distance of the cycle pose of two inter-robot
loops under the covariance accumulated around the cycle, evaluated as the direct chain of the reference's own lines:
graph_utils::poseCompose / poseBetween / poseInverse (graph_utils_functions.cpp:12-35), the covariance chain of buildTrajectory (:37-70),
computeConsistencyError (pairwise_consistency.cpp:99-128).  gtsam is not in the reference tree; its Jacobians are restated from upstream
GTSAM 4.0 (parity unpinned, like Pose3::Logmap in pcm_restate.py).

Tangent order is gtsam's Pose3 order: rotation xyz, then translation xyz.  Poses are [4, 4] float64, covariances [6, 6] float64 of which the
lower triangle is read.  Everything here is the contract; nothing here is fast."""
import numpy as np

import pcm_restate as R

NONE, SPAN, REFERENCE = 0, 1, 2
MODES = {"none": NONE, "span": SPAN, "reference": REFERENCE}
FIXED_COVARIANCE = np.diag([1e-4, 1e-4, 1e-4, 1e-2, 1e-2, 1e-2])      # graph_types.h:79-85
FIXED_COVARIANCE.setflags(write=False)
CHI2_UPPER = {0.90: 10.645, 0.95: 12.592, 0.99: 16.812, 0.999: 22.458}    # upper quantiles of chi-squared with 6 degrees of freedom


def skew(t):
    return np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])


def adjoint(T):
    """Ad(T) = [[R, 0], [[t]x R, R]]"""
    A = np.zeros((6, 6))
    Rm = T[:3, :3]
    A[:3, :3] = Rm
    A[3:, 3:] = Rm
    A[3:, :3] = skew(T[:3, 3]) @ Rm
    return A


def lower(C):
    """the symmetric matrix whose lower triangle is that of C"""
    C = np.asarray(C, np.float64)
    Lo = np.tril(C)
    return Lo + np.tril(C, -1).T


def conj(A, S):
    return A @ S @ A.T


# ---- Jacobians (gtsam 4.0: Pose3::compose, between, inverse)
def compose_jacobians(a, b):
    return adjoint(R.inverse(b)), np.eye(6)


def between_jacobians(a, b):
    return -adjoint(R.inverse(R.inverse(a) @ b)), np.eye(6)


def inverse_jacobian(a):
    return -adjoint(a)


# ---- graph_utils: a pose with its covariance
def pose_compose(a, Sa, b, Sb):
    Ha, _ = compose_jacobians(a, b)
    return a @ b, conj(Ha, Sa) + Sb


def pose_between(a, Sa, b, Sb):
    Ha, _ = between_jacobians(a, b)
    return R.inverse(a) @ b, conj(Ha, Sa) + Sb


def pose_inverse(a, Sa):
    return R.inverse(a), conj(inverse_jacobian(a), Sa)


def step_covariances(Q, n):
    """[n - 1, 6, 6] from the caller's Q (None: FIXED_COVARIANCE per step)"""
    if Q is None:
        return np.broadcast_to(FIXED_COVARIANCE, (max(n - 1, 0), 6, 6))
    return np.stack([lower(q) for q in np.asarray(Q, np.float64).reshape(-1, 6, 6)]) if n > 1 else np.zeros((0, 6, 6))


def span_sweep(X, Q, i):
    """S_{i,m} for m = i .. n - 1 as a dict-free array [n, 6, 6] (entries below i are NaN): S_{i,i} = 0,
    S_{i,m+1} = Ad(o_m^-1) S_{i,m} Ad(o_m^-1)^T + Q_m with o_m = X_m^-1 X_{m+1}"""
    n = X.shape[0]
    S = np.full((n, 6, 6), np.nan)
    S[i] = 0.0
    for m in range(i, n - 1):
        o = R.inverse(X[m]) @ X[m + 1]
        S[m + 1] = conj(adjoint(R.inverse(o)), S[m]) + Q[m]
    return S


def marginals(X, Q, first=None):
    """buildTrajectory's covariance chain: M_0 = first, M_{m+1} = Ad(o_m^-1) M_m Ad(o_m^-1)^T + Q_m"""
    n = X.shape[0]
    M = np.empty((n, 6, 6))
    M[0] = lower(FIXED_COVARIANCE if first is None else first)
    for m in range(n - 1):
        o = R.inverse(X[m]) @ X[m + 1]
        M[m + 1] = conj(adjoint(R.inverse(o)), M[m]) + Q[m]
    return M


def chain_odometry_covariance(odom, Q, first=None):
    """the marginals of buildTrajectory from odometry between-poses [n, 4, 4] and their covariances [n, 6, 6] -> [n + 1, 6, 6]"""
    odom = np.asarray(odom, np.float64).reshape(-1, 4, 4)
    Q = step_covariances(Q, odom.shape[0] + 1)
    M = np.empty((odom.shape[0] + 1, 6, 6))
    M[0] = lower(FIXED_COVARIANCE if first is None else first)
    for m in range(odom.shape[0]):
        M[m + 1] = conj(adjoint(R.inverse(odom[m])), M[m]) + Q[m]
    return M


class Trajectory:
    """the covariance of X_i^-1 X_j in one mode; SPAN sweeps once per distinct start pose"""

    def __init__(self, mode, X, Q, first=None):
        self.mode, self.X = mode, np.asarray(X, np.float64)
        self.Q = step_covariances(Q, self.X.shape[0])
        self.sweeps = {}
        self.M = marginals(self.X, self.Q, first) if mode == REFERENCE else None

    def span(self, i, j):
        """S_{i,j}, i <= j"""
        if i not in self.sweeps:
            self.sweeps[i] = span_sweep(self.X, self.Q, i)
        return self.sweeps[i][j]

    def between(self, i, j):
        """(X_i^-1 X_j, its covariance)"""
        r = R.inverse(self.X[i]) @ self.X[j]
        if self.mode == REFERENCE:                                 # composeOnTrajectory -> poseBetween of two marginals
            return pose_between(self.X[i], self.M[i], self.X[j], self.M[j])
        if i <= j:
            return r, self.span(i, j)
        return r, conj(adjoint(R.inverse(self.X[j]) @ self.X[i]), self.span(j, i))     # the covariance of the inverse


def pair(TA, TB, i, k, Zu, Cu, j, l, Zv, Cv):
    """computeConsistencyError for loops u = (i, k, Zu, Cu) and v = (j, l, Zv, Cv), u < v -> (xi [6], Sigma_E [6, 6], d2)"""
    aXij, Sa = TA.between(i, j)
    bXlk, Sb = TB.between(l, k)
    out1, S1 = pose_compose(aXij, Sa, Zv, lower(Cv))
    out2, S2 = pose_compose(out1, S1, bXlk, Sb)
    E, SE = pose_between(Zu, lower(Cu), out2, S2)
    SE = 0.5 * (SE + SE.T)
    xi = R.logmap(E)
    return xi, SE, mahalanobis2(xi, SE)


def mahalanobis2(xi, S):
    """xi^T S^-1 xi through a Cholesky factor; NaN where it is not finite or S is not positive definite"""
    if not (np.isfinite(xi).all() and np.isfinite(S).all()):
        return np.nan
    try:
        Lc = np.linalg.cholesky(S)
    except np.linalg.LinAlgError:
        return np.nan
    z = np.linalg.solve(Lc, xi)
    d2 = float(z @ z)
    return d2 if np.isfinite(d2) else np.nan


def loop_covariances(C, L):
    if C is None:
        return np.broadcast_to(FIXED_COVARIANCE, (L, 6, 6))
    return np.asarray(C, np.float64).reshape(L, 6, 6)


def evaluate(mode, XA, XB, ia, kb, Z, C=None, QA=None, QB=None, first=None, pairs=None):
    """every pair u < v (or the given ones) -> D [L, L] of d2 (mirrored, zero diagonal), XI [L, L, 6] and SE [L, L, 6, 6] (upper triangle
    only: the entry of (u, v), u < v)"""
    mode = MODES.get(mode, mode)
    TA, TB = Trajectory(mode, XA, QA, first), Trajectory(mode, XB, QB, first)
    L = len(ia)
    C = loop_covariances(C, L)
    D, XI, SE = np.zeros((L, L)), np.zeros((L, L, 6)), np.zeros((L, L, 6, 6))
    with np.errstate(invalid="ignore", divide="ignore"):
        for u, v in (pairs if pairs is not None else zip(*np.triu_indices(L, 1))):
            xi, S, d2 = pair(TA, TB, int(ia[u]), int(kb[u]), Z[u], C[u], int(ia[v]), int(kb[v]), Z[v], C[v])
            D[u, v] = D[v, u] = d2
            XI[u, v], SE[u, v] = xi, S
    return D, XI, SE


def consistency_matrix(D, threshold):
    """bool [L, L]: d2 < threshold off the diagonal; NaN is not consistent"""
    return R.consistency_matrix(D, threshold)
