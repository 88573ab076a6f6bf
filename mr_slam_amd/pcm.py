"""Pairwise Consistency Maximisation for the inter-robot loops of one robot pair (Mapping/src/global_manager/src/
pairwise_consistency_maximization/): which of the verified loops are mutually consistent and may enter the pose graph.

Thin host logic over the C ABI (mrs_pcm_*); there is no CPU fallback.  The consistency matrix and the clique heuristic run on the GPU;
`chi2_threshold`, `chain_odometry` and `reference_order` restate the three small host steps the reference takes before them.  The contract,
its two reproduced quirks and its three fixes are in DESIGN.md 4.18.  `set_covariances` turns the test into the Mahalanobis distance of the
cycle pose under the odometry and loop covariances; the threshold is then an upper chi-squared quantile, `chi2_upper`.
"""
import ctypes as C

import numpy as np

from . import _lib

MAX_LOOPS = _lib.header_int("MRS_PCM_MAX_LOOPS")
EXACT_DEFAULT_NODES, EXACT_OVERSHOOT = _lib.header_int("MRS_PCM_EXACT_DEFAULT_NODES"), _lib.header_int("MRS_PCM_EXACT_OVERSHOOT")
# getChiSquaredThreshold for 6 degrees of freedom (pairwise_consistency.cpp:7-38), keyed by round(100 p)
_CHI2 = {1: 0.872, 5: 1.635, 10: 2.204, 25: 3.455, 50: 5.348, 75: 7.840}
# upper quantiles of chi-squared with 6 degrees of freedom, keyed by round(1000 q): the thresholds of the covariance modes
_CHI2_UPPER = {900: 10.645, 950: 12.592, 990: 16.812, 999: 22.458}
COV_MODES = {"none": _lib.header_int("MRS_PCM_COV_NONE"), "span": _lib.header_int("MRS_PCM_COV_SPAN"),
             "reference": _lib.header_int("MRS_PCM_COV_REFERENCE")}
# graph_types.h:79-85: rotation std 0.01 rad, translation std 0.1 m, in gtsam's Pose3 tangent order (rotation, then translation)
FIXED_COVARIANCE = np.diag([1e-4, 1e-4, 1e-4, 1e-2, 1e-2, 1e-2])
FIXED_COVARIANCE.setflags(write=False)


def chi2_threshold(p):
    """the reference's threshold for confidence probability p (its launch default pcm_thresh is 0.01); it aborts on any other p, this raises"""
    key = round(float(p) * 100)
    if key not in _CHI2 or abs(float(p) * 100 - key) > 1e-9:
        raise ValueError("confidence probability %r is not supported: one of 0.01, 0.05, 0.10, 0.25, 0.50, 0.75" % (p,))
    return _CHI2[key]


def chi2_upper(q):
    """the squared Mahalanobis distance below which a share q of correct pairs falls (6 degrees of freedom): the threshold of a handle with
    covariances.  The reference's table (chi2_threshold) is keyed by lower-tail probabilities: with a real covariance its p = 0.01 would
    reject 99 % of the correct pairs."""
    key = round(float(q) * 1000)
    if key not in _CHI2_UPPER or abs(float(q) * 1000 - key) > 1e-9:
        raise ValueError("quantile %r is not supported: one of 0.90, 0.95, 0.99, 0.999" % (q,))
    return _CHI2_UPPER[key]


def _adjoint(T):
    """Ad(T) = [[R, 0], [[t]x R, R]] in gtsam's Pose3 tangent order"""
    t = T[:3, 3]
    A = np.zeros((6, 6))
    A[:3, :3] = A[3:, 3:] = T[:3, :3]
    A[3:, :3] = np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]]) @ T[:3, :3]
    return A


def chain_odometry_covariance(odom, Q, first=None):
    """buildTrajectory's covariance chain (graph_utils_functions.cpp:37-70): odometry between-poses [n, 4, 4] and their covariances
    [n, 6, 6] (None: FIXED_COVARIANCE each) -> the marginal of every trajectory pose [n + 1, 6, 6]: M_0 = first (None: FIXED_COVARIANCE),
    M_m+1 = Ad(odom_m^-1) M_m Ad(odom_m^-1)^T + Q_m, poseCompose's covariance with gtsam's Jacobian of compose"""
    odom = np.asarray(odom, np.float64).reshape(-1, 4, 4)
    n = odom.shape[0]
    Q = np.broadcast_to(FIXED_COVARIANCE, (n, 6, 6)) if Q is None else _covs(Q, "Q", n)
    M = np.empty((n + 1, 6, 6))
    M[0] = FIXED_COVARIANCE if first is None else _covs(first, "first", 1)[0]
    for m in range(n):
        inv = np.eye(4)
        inv[:3, :3] = odom[m, :3, :3].T
        inv[:3, 3] = -odom[m, :3, :3].T @ odom[m, :3, 3]
        A = _adjoint(inv)
        M[m + 1] = A @ M[m] @ A.T + Q[m]
    return M


def chain_odometry(odom):
    """buildTrajectory (graph_utils_functions.cpp:37-70): odometry between-poses [n, 4, 4] -> trajectory [n + 1, 4, 4]; the first pose is the
    identity and pose m + 1 = pose m @ odom[m]"""
    odom = np.asarray(odom, np.float64).reshape(-1, 4, 4)
    X = np.empty((odom.shape[0] + 1, 4, 4))
    X[0] = np.eye(4)
    for m in range(odom.shape[0]):
        X[m + 1] = X[m] @ odom[m]
    return X


def reference_order(ia, kb):
    """indices that put loops (ia, kb) into the reference's vertex order: the std::map order of (key1, key2) (interrobot_measurements.cpp:8-14),
    where a key pair met again is dropped (std::map::insert keeps the first)"""
    ia, kb = np.asarray(ia, np.int64).reshape(-1), np.asarray(kb, np.int64).reshape(-1)
    order = np.lexsort((kb, ia))                                 # stable: the first of equal pairs stays first
    if order.size:
        same = np.zeros(order.size, bool)
        same[1:] = (ia[order][1:] == ia[order][:-1]) & (kb[order][1:] == kb[order][:-1])
        order = order[~same]
    return order


def _poses(a, what):
    a = np.ascontiguousarray(a, np.float64)
    if a.ndim == 2:
        a = a[None]
    if a.ndim != 3 or a.shape[1:] != (4, 4):
        raise ValueError("%s: expected [n, 4, 4] poses, got %s" % (what, a.shape))
    return a


def _covs(a, what, n):
    """[n, 6, 6] float64, symmetric from the lower triangle"""
    a = np.asarray(a, np.float64)
    if a.ndim == 2:
        a = a[None]
    if a.ndim != 3 or a.shape != (n, 6, 6):
        raise ValueError("%s: expected [%d, 6, 6] covariances, got %s" % (what, n, a.shape))
    lo = np.tril(a)
    return np.ascontiguousarray(lo + np.swapaxes(np.tril(a, -1), -1, -2))


class PcmGraph(_lib.Handle):
    """The loops of one robot pair on the device: `set_trajectories(XA, XB)`, `add_loops(ia, kb, Z)` (vertex numbers follow the order of
    addition; pass them in `reference_order` to number them as the reference does), `solve()` -> (member list in the reference's order,
    number of rejected loops).  `matrix()` / `distances()` read the consistency matrix and the distances behind it; `set_matrix(A)` puts a
    given adjacency in place of the loops, for the clique stage alone.  `rounds` is the number of rounds the last solve took.
    `solve_exact()` -> (a MAXIMUM clique in ascending order, number of rejected loops) with `proof` and `nodes`.
    `set_covariances(mode, QA, QB, first)` after the trajectories makes the test a squared Mahalanobis distance (create the handle with
    threshold=chi2_upper(q) then); `add_loops(..., cov=C)` gives every loop its covariance and `pair(u, v)` explains one pair."""
    _destroy = "mrs_pcm_destroy"

    def __init__(self, capacity=MAX_LOOPS, p=0.01, threshold=None, device=0):
        self.device = int(device)
        self.capacity = int(capacity)
        self.threshold = chi2_threshold(p) if threshold is None else float(threshold)
        self.rounds = 0
        self.proof, self.nodes, self.launches = 0, 0, 0
        self._create("mrs_pcm_create", _lib.ctx(self.device), self.capacity, self.threshold)

    def __len__(self):
        n = C.c_int32(0)
        _lib.load().mrs_pcm_count(self._h, C.byref(n))
        return n.value

    def set_trajectories(self, XA, XB):
        """trajectory poses [na, 4, 4] and [nb, 4, 4] (see chain_odometry); clears the loops"""
        XA, XB = _poses(XA, "XA"), _poses(XB, "XB")
        _lib.load().mrs_pcm_set_trajectories(self._h, XA, XA.shape[0], XB, XB.shape[0])
        self._n = (XA.shape[0], XB.shape[0])

    def set_covariances(self, mode="span", QA=None, QB=None, first=None):
        """after set_trajectories; clears the loops.  mode "span" (the odometry between the two poses of a trajectory counts: the PCM
        paper's test, recommended), "reference" (the reference's lines: marginals from the chain start) or "none".
        QA [na - 1, 6, 6] / QB [nb - 1, 6, 6]: the covariance of every odometry step; first [6, 6]: that of the first pose ("reference"
        only).  None: FIXED_COVARIANCE.  Tangent order is gtsam's: rotation, then translation."""
        if mode not in COV_MODES:
            raise ValueError("mode %r: one of %s" % (mode, ", ".join(sorted(COV_MODES))))
        na, nb = getattr(self, "_n", (0, 0))
        QA = None if QA is None else _covs(QA, "QA", na - 1)
        QB = None if QB is None else _covs(QB, "QB", nb - 1)
        first = None if first is None else _covs(first, "first", 1)
        _lib.load().mrs_pcm_set_covariances(self._h, COV_MODES[mode], QA, QB, first)

    def add_loops(self, ia, kb, Z, cov=None):
        """appends loops: Z[u] [4, 4] is the measured pose of B_kb[u] in the frame of A_ia[u]; cov[u] [6, 6] its covariance (a handle with
        covariances only; None there: FIXED_COVARIANCE)"""
        ia, kb = np.ascontiguousarray(ia, np.int32).reshape(-1), np.ascontiguousarray(kb, np.int32).reshape(-1)
        Z = _poses(Z, "Z")
        if not ia.size == kb.size == Z.shape[0]:
            raise ValueError("ia, kb and Z must have one entry per loop")
        if cov is not None:
            cov = _covs(cov, "cov", ia.size)
            if ia.size:
                _lib.load().mrs_pcm_add_loops_cov(self._h, ia, kb, Z, cov, ia.size)
        elif ia.size:
            _lib.load().mrs_pcm_add_loops(self._h, ia, kb, Z, ia.size)

    def pair(self, u, v):
        """one pair recomputed on the host -> (xi [6] = Logmap of its cycle pose, cov [6, 6] = the covariance propagated around the cycle
        (the identity without covariances), d = the quantity compared with the threshold)"""
        xi, cov, d = np.zeros(6), np.zeros((6, 6)), C.c_double(0.0)
        _lib.load().mrs_pcm_get_pair(self._h, int(u), int(v), xi, cov, C.byref(d))
        return xi, cov, d.value

    def clear(self):
        _lib.load().mrs_pcm_clear_loops(self._h)

    def solve(self):
        """-> (clique int32 [size], n_rejected): FMC::maxCliqueHeu's member list and the loops it leaves out; empty without loops"""
        L = len(self)
        clique = np.zeros(max(L, 1), np.int32)
        n, rounds = C.c_int32(0), C.c_int32(0)
        _lib.load().mrs_pcm_solve(self._h, clique, C.byref(n), C.byref(rounds))
        self.rounds = rounds.value
        return clique[:n.value].copy(), L - n.value

    def solve_exact(self, max_nodes=None):
        """-> (clique int32 [size] ASCENDING, n_rejected): a maximum clique, FMC::maxClique's member list, searched with a budget
        of `max_nodes` nodes (None: EXACT_DEFAULT_NODES).  Sets `proof` (2: size proven and list canonical; 1: size proven; 0: the budget ran
        out, the list is the best clique found) and `nodes`.  `solve()` and `rounds` are not affected."""
        L = len(self)
        clique = np.zeros(max(L, 1), np.int32)
        n, proof, nodes = C.c_int32(0), C.c_int32(0), C.c_int64(0)
        _lib.load().mrs_pcm_solve_exact(self._h, EXACT_DEFAULT_NODES if max_nodes is None else int(max_nodes), clique, C.byref(n),
                                        C.byref(proof), C.byref(nodes))
        self.proof, self.nodes = proof.value, nodes.value
        launches = C.c_int64(0)
        _lib.load().mrs_pcm_exact_launches(self._h, C.byref(launches))
        self.launches = launches.value
        return clique[:n.value].copy(), L - n.value

    def matrix(self):
        """the consistency matrix, bool [L, L]"""
        L = len(self)
        A = np.zeros((L, L), np.uint8)
        if L:
            _lib.load().mrs_pcm_get_matrix(self._h, A)
        return A.astype(bool)

    def set_matrix(self, A):
        """replaces the loops by the vertices of a symmetric adjacency with a zero diagonal"""
        A = np.asarray(A)
        if A.ndim != 2 or A.shape[0] != A.shape[1]:
            raise ValueError("expected a square matrix, got %s" % (A.shape,))
        A = np.ascontiguousarray(A != 0, np.uint8)
        _lib.load().mrs_pcm_set_matrix(self._h, A.shape[0], A if A.size else None)

    def distances(self):
        """the compared quantity, float64 [L, L], recomputed on demand: |Logmap| without covariances, the squared Mahalanobis distance with"""
        L = len(self)
        D = np.zeros((L, L), np.float64)
        if L:
            _lib.load().mrs_pcm_get_distances(self._h, D)
        return D
