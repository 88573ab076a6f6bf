"""Pose-graph optimisation for the Mapping back end (Mapping/src/global_manager/src/distributed_mapper/evaluation_utils.cpp:273-329,
centralizedGNEstimation): rotations by chordal relaxation, then Gauss-Newton on chordal between factors, for a few odometry chains joined
by loop factors.

Thin host logic over the C ABI (mrs_pgo_*); there is no CPU fallback.  Both stages run on the GPU in fp64; `between`,
`odometry_from_trajectory` and `correction` are the small host steps around them.  The contract and its named deviations are in
DESIGN.md 4.23."""
import collections

import numpy as np

from . import _lib
from .pcm import _poses

MAX_CHAINS, MAX_POSES = _lib.header_int("MRS_PGO_MAX_CHAINS"), _lib.header_int("MRS_PGO_MAX_POSES")
MAX_LOOPS, MAX_SEPARATORS = _lib.header_int("MRS_PGO_MAX_LOOPS"), _lib.header_int("MRS_PGO_MAX_SEPARATORS")
DEFAULT_SEGMENT_LENGTH = _lib.header_int("MRS_PGO_DEFAULT_SEGMENT_LENGTH")
DEFAULT_EPS, DEFAULT_MAX_ITERATIONS = 1e-9, _lib.header_int("MRS_PGO_DEFAULT_MAX_ITERATIONS")
_INFO, _INFO_LM = _lib.header_int("MRS_PGO_INFO_DOUBLES"), _lib.header_int("MRS_PGO_LM_INFO_DOUBLES")
KERNELS = {None: _lib.header_int("MRS_PGO_KERNEL_NONE"), "none": _lib.header_int("MRS_PGO_KERNEL_NONE"),
           "huber": _lib.header_int("MRS_PGO_KERNEL_HUBER"), "cauchy": _lib.header_int("MRS_PGO_KERNEL_CAUCHY"),
           "geman_mcclure": _lib.header_int("MRS_PGO_KERNEL_GEMAN_MCCLURE")}
SOLVERS = {"dense": _lib.header_int("MRS_PGO_SOLVER_DENSE"), "sparse": _lib.header_int("MRS_PGO_SOLVER_SPARSE")}
MAX_SPARSE_BLOCKS, SPARSE_DEGREE_SLACK = _lib.header_int("MRS_PGO_MAX_SPARSE_BLOCKS"), _lib.header_int("MRS_PGO_SPARSE_DEGREE_SLACK")
_STATS = _lib.header_int("MRS_PGO_SOLVER_STATS")
FRAMES = {"chordal": _lib.header_int("MRS_PGO_FRAME_CHORDAL"), "pose3": _lib.header_int("MRS_PGO_FRAME_POSE3")}
_MARGINAL_INFO = _lib.header_int("MRS_PGO_MARGINAL_INFO")
# the reference's own factor noise (global_manager.cpp:103-109: loopNoise and odometryNoise), as Pose3 covariances: rotation xyz, then
# translation xyz
REFERENCE_LOOP_COVARIANCE = np.diag([1e-1, 1e-1, 1e-1, 1e-2, 1e-2, 1e-2])
REFERENCE_ODOMETRY_COVARIANCE = np.eye(6)

Result = collections.namedtuple("Result", "T iterations converged max_delta error_initial error_final separators")
Result.__doc__ = """T float64 [N, 4, 4]; iterations done; converged (max|delta| < eps was met); the last max|delta|; 0.5 sum |e|^2 at the
stage-1 values and at T (the reference's "Initial Error" and "GN Error"); the separators of the Gauss-Newton system."""
ResultLM = collections.namedtuple("ResultLM", "T solves accepted converged max_delta cost_initial cost_final separators lam")
ResultLM.__doc__ = """T float64 [N, 4, 4]; solves done and steps accepted; converged (an accepted step had max|delta| < eps); the last accepted
max|delta|; the cost (sum 0.5 r^2 over the odometry factors + sum rho(r) over the loops) at the stage-1 values and at T; the separators; the
final lambda."""
SolverStats = collections.namedtuple("SolverStats", "separators eliminated core levels blocks updates max_degree solver")
SolverStats.__doc__ = """the sparse tier of a stage: its separators, how many of them are eliminated before the dense Cholesky and how many are
left to it (the core), the levels (launches per direction), the blocks sum (d + 1) and block products sum d (d + 1) / 2 of the eliminated
columns, the largest d, and the solver in force ("dense": nothing is eliminated)."""


MarginalInfo = collections.namedtuple("MarginalInfo", "separators order bytes")
MarginalInfo.__doc__ = """what the handle holds for the marginals of the last result: the separators of stage 2, the order of the reduced
system whose inverse is kept dense (6 per separator), and the bytes of device memory (that inverse and two 6 x 6 per pose)."""


def _frame(frame):
    if frame not in FRAMES:
        raise ValueError("frame must be one of %s" % sorted(FRAMES))
    return FRAMES[frame]


def _adjoint(T):
    """Ad(T) = [[R, 0], [skew(t) R, R]] in Pose3's order (rotation, translation)"""
    R, t = T[:3, :3], T[:3, 3]
    A = np.zeros((6, 6))
    A[:3, :3] = A[3:, 3:] = R
    A[3:, :3] = np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]]) @ R
    return A


def between_covariance(joint_pose3, Ti, Tj):
    """the 6 x 6 covariance of Z = Ti^-1 Tj in Pose3 local coordinates (rotation, translation: the order PcmGraph.set_covariances and
    add_loops take) from the joint marginal [12, 12] of (i, j) in the "pose3" frame and the two poses [4, 4]: J S J^T with
    J = [-Ad(Z^-1), I].  What a consistency test of a loop between i and j, or a gate on a candidate's initial pose, needs."""
    S = np.asarray(joint_pose3, np.float64)
    if S.shape != (12, 12):
        raise ValueError("joint_pose3 must be [12, 12]")
    Zi = between(Tj, Ti)                                          # Z^-1 = Tj^-1 Ti
    J = np.hstack([-_adjoint(Zi), np.eye(6)])
    return J @ S @ J.T


def _covariances(C, n, name):
    C = np.ascontiguousarray(C, np.float64)
    if C.shape == (6, 6):
        C = np.ascontiguousarray(np.broadcast_to(C, (n, 6, 6)))
    if C.shape != (n, 6, 6):
        raise ValueError("%s must be [6, 6] or [%d, 6, 6]" % (name, n))
    return C


def _inverse(X):
    Xi = np.tile(np.eye(4), (X.shape[0], 1, 1))
    Rt = X[:, :3, :3].transpose(0, 2, 1)
    Xi[:, :3, :3] = Rt
    Xi[:, :3, 3] = -np.einsum("nab,nb->na", Rt, X[:, :3, 3])
    return Xi


def between(Xa, Xb):
    """Xa^-1 Xb: the pose of b in the frame of a, for one pair [4, 4] or n pairs [n, 4, 4]"""
    single = np.asarray(Xa).ndim == 2
    Z = _inverse(_poses(Xa, "Xa")) @ _poses(Xb, "Xb")
    return Z[0] if single else Z


def odometry_from_trajectory(X):
    """trajectory [n, 4, 4] -> odometry between-poses [n - 1, 4, 4]: the inverse of pcm.chain_odometry up to the first pose"""
    X = _poses(X, "X")
    return between(X[:-1], X[1:]) if X.shape[0] > 1 else np.zeros((0, 4, 4))


def correction(T_opt, T_origin):
    """optMapTF * originMapTF per pose (composeGlobalMap), float32 [n, 4, 4]: the optimised poses T_opt applied to the transforms T_origin
    the keyframes were stored with, as GlobalMap.rebuild's segment poses and ElevationSubmaps.update_global take them.  Both are rounded to
    float32 first, and every product and sum is rounded once in float32 in the order globalmap.pose_product documents."""
    from .globalmap import pose_product
    T_opt, T_origin = _poses(T_opt, "T_opt"), _poses(T_origin, "T_origin")
    if T_opt.shape != T_origin.shape:
        raise ValueError("T_opt and T_origin must have one pose each per entry")
    out = np.empty(T_opt.shape, np.float32)
    for k in range(T_opt.shape[0]):
        out[k] = pose_product(T_opt[k].astype(np.float32), T_origin[k].astype(np.float32))
    return out


class PoseGraph:
    """`nr` odometry chains on the device, poses numbered chain after chain: `set_odometry(Z)` (one factor per consecutive pair, chain
    after chain), `add_loops(i, j, Z)` (Z[u] is the measured pose of j[u] in the frame of i[u]; any two different poses),
    `set_prior(T)`, `set_segment_length(n)`, `initialize()` -> stage-1 poses, `optimize()` -> Result.  A refused call leaves the graph as
    it was.

    The C handle is owned by a plain `_lib.Handle` object (`_owner`, destroyed with this object by Handle's own `__del__`), not by a
    subclass: the set of Handle subclasses of the package is pinned by tests/test_python_layer_cpu.py."""

    def __init__(self, chain_lengths, device=0):
        self.device = int(device)
        self.chain_lengths = np.ascontiguousarray(chain_lengths, np.int32).reshape(-1)
        self.n_poses = int(self.chain_lengths.sum())
        self._owner = _lib.Handle()
        self._owner._destroy = "mrs_pgo_destroy"
        self._owner._create("mrs_pgo_create", _lib.ctx(self.device), self.chain_lengths.size, self.chain_lengths)

    @property
    def _h(self):
        return self._owner._h

    def __len__(self):
        import ctypes as C
        n = C.c_int32(0)
        _lib.load().mrs_pgo_count(self._h, C.byref(n))
        return n.value

    def set_odometry(self, Z):
        Z = _poses(Z, "Z") if np.size(Z) else np.zeros((0, 4, 4))
        _lib.load().mrs_pgo_set_odometry(self._h, Z if Z.size else None, Z.shape[0])

    def set_odometry_noise(self, C):
        """one Pose3 covariance [6, 6] per odometry factor (or one for all); None clears them"""
        if C is None:
            _lib.load().mrs_pgo_set_odometry_noise(self._h, None, 0)
            return
        n = self.n_poses - self.chain_lengths.size
        C = _covariances(C, n, "C")
        _lib.load().mrs_pgo_set_odometry_noise(self._h, C if n else None, n)

    def add_loops(self, i, j, Z, C=None):
        """C: a Pose3 covariance [6, 6] per loop (or one for all); None leaves these loops at the unit model"""
        i, j = np.ascontiguousarray(i, np.int32).reshape(-1), np.ascontiguousarray(j, np.int32).reshape(-1)
        if not i.size:
            return
        Z = _poses(Z, "Z")
        if not i.size == j.size == Z.shape[0]:
            raise ValueError("i, j and Z must have one entry per loop")
        if C is None:
            _lib.load().mrs_pgo_add_loops(self._h, i, j, Z, i.size)
        else:
            _lib.load().mrs_pgo_add_loops_noise(self._h, i, j, Z, _covariances(C, i.size, "C"), i.size)

    def set_loop_kernel(self, kernel, k=1.0):
        """a robust kernel on the loop factors for optimize(method="lm"): None, "huber", "cauchy" or "geman_mcclure" with parameter k"""
        if kernel not in KERNELS:
            raise ValueError("kernel must be one of %s" % sorted(n for n in KERNELS if n))
        _lib.load().mrs_pgo_set_loop_kernel(self._h, KERNELS[kernel], float(k))

    def loop_state(self):
        """(w, r2) float64 [loops]: the kernel's weight and e^T L e of every loop at the last result"""
        n = len(self)
        w, r2 = np.zeros(max(n, 1)), np.zeros(max(n, 1))
        _lib.load().mrs_pgo_get_loop_state(self._h, w, r2, w.size)
        return w[:n], r2[:n]

    def clear(self):
        _lib.load().mrs_pgo_clear_loops(self._h)

    def set_prior(self, T):
        _lib.load().mrs_pgo_set_prior(self._h, _poses(T, "T")[0].copy())

    def set_segment_length(self, length):
        _lib.load().mrs_pgo_set_segment_length(self._h, int(length))

    def set_solver(self, solver, dense_limit=None, max_blocks=None):
        """ "dense" (the default: every separator in one dense Cholesky, MAX_SEPARATORS of them at most) or "sparse": separators of low degree
        are eliminated first, level after level, until dense_limit (None: MAX_SEPARATORS) are left; the size limit is then max_blocks (None:
        MAX_SPARSE_BLOCKS) blocks of the eliminated columns"""
        if solver not in SOLVERS:
            raise ValueError("solver must be one of %s" % sorted(SOLVERS))
        _lib.load().mrs_pgo_set_solver(self._h, SOLVERS[solver], -1 if dense_limit is None else int(dense_limit),
                                       0 if max_blocks is None else int(max_blocks))

    def solver_stats(self, stage=2):
        """SolverStats of stage 1 (rotations) or 2 (Gauss-Newton) for the graph as it stands; host work only"""
        st = np.zeros(_STATS, np.int64)
        _lib.load().mrs_pgo_get_solver_stats(self._h, int(stage), st)
        return SolverStats(*[int(x) for x in st[:7]], {v: k for k, v in SOLVERS.items()}[int(st[7])])

    def initialize(self):
        """stage 1 alone -> float64 [N, 4, 4]: the relaxed rotations projected to SO(3), zero translations"""
        T = np.zeros((self.n_poses, 4, 4))
        _lib.load().mrs_pgo_initialize(self._h, T)
        return T

    def optimize(self, eps=DEFAULT_EPS, max_iterations=DEFAULT_MAX_ITERATIONS, method="gn"):
        """both stages -> Result; eps = 0 runs exactly max_iterations steps.  method="lm": Levenberg-Marquardt step control, max_iterations
        counts the solves (rejected ones too) -> ResultLM"""
        if method not in ("gn", "lm"):
            raise ValueError('method must be "gn" or "lm"')
        if method == "lm":
            T, info = np.zeros((self.n_poses, 4, 4)), np.zeros(_INFO_LM)
            _lib.load().mrs_pgo_optimize_lm(self._h, float(eps), int(max_iterations), T, info)
            return ResultLM(T, int(info[0]), int(info[1]), bool(info[2]), float(info[3]), float(info[4]), float(info[5]), int(info[6]),
                            float(info[7]))
        T, info = np.zeros((self.n_poses, 4, 4)), np.zeros(_INFO)
        _lib.load().mrs_pgo_optimize(self._h, float(eps), int(max_iterations), T, info)
        return Result(T, int(info[0]), bool(info[1]), float(info[2]), float(info[3]), float(info[4]), int(info[5]))

    # ---- marginal covariances of the last result

    def mark_poses(self, poses):
        """replaces the set of poses that stage 2 keeps as separators whether or not a loop touches them, so that joint marginals
        between them are answered; None or an empty list clears it.  A change of topology: the last result is gone."""
        poses = np.ascontiguousarray([] if poses is None else poses, np.int32).reshape(-1)
        _lib.load().mrs_pgo_mark_poses(self._h, poses if poses.size else None, poses.size)

    def marginal_info(self):
        """MarginalInfo of the marginals of the last result, computing them unless they are held already"""
        info = np.zeros(_MARGINAL_INFO, np.int64)
        _lib.load().mrs_pgo_compute_marginals(self._h, info)
        return MarginalInfo(*[int(x) for x in info[:3]])

    def marginals(self, poses=None, frame="chordal"):
        """float64 [n, 6, 6]: the marginal covariance of every pose named (None: of all poses) at the last result, in the optimiser's
        tangent ("chordal": rotation, then translation in the world frame) or in Pose3 local coordinates ("pose3").  The Gauss-Newton
        information matrix at the result is factored and inverted on first use after a result; pose 0 is held, its marginal is zero."""
        f = _frame(frame)
        self.marginal_info()
        if poses is None:
            out = np.zeros((self.n_poses, 6, 6))
            _lib.load().mrs_pgo_get_marginals(self._h, None, self.n_poses, f, out)
            return out
        poses = np.ascontiguousarray(poses, np.int32).reshape(-1)
        out = np.zeros((poses.size, 6, 6))
        if poses.size:
            _lib.load().mrs_pgo_get_marginals(self._h, poses, poses.size, f, out)
        return out

    def joint_marginals(self, i, j, frame="chordal"):
        """float64 [n, 12, 12]: [[S_ii, S_ij], [S_ji, S_jj]] per pair (i[u], j[u]).  Answered between separators of stage 2 (poses a loop
        touches, cut poses, marked poses) and pose 0, and between consecutive poses of a chain; any other pair is refused with the pose
        to mark named."""
        f = _frame(frame)
        i, j = np.ascontiguousarray(i, np.int32).reshape(-1), np.ascontiguousarray(j, np.int32).reshape(-1)
        if i.size != j.size:
            raise ValueError("i and j must have one entry per pair")
        self.marginal_info()
        out = np.zeros((i.size, 12, 12))
        if i.size:
            _lib.load().mrs_pgo_get_joint_marginals(self._h, i, j, i.size, f, out)
        return out

    def marginal_ms(self):
        """milliseconds of the last computation of the marginals (the factorisation at the result, the triangular inverse, the symmetric
        product, the segment walk); zeros unless the development timing switch was on"""
        ms = np.zeros(4, np.float32)
        _lib.load().mrs_pgo_last_marginal_ms(self._h, ms)
        return ms

    def stage_ms(self):
        """milliseconds of the last optimize's stages (stage 1, linearise, segment walks, assembly, dense solve, retraction); zeros unless
        the development timing switch was on"""
        ms = np.zeros(6, np.float32)
        _lib.load().mrs_pgo_last_stage_ms(self._h, ms)
        return ms

    def tier_ms(self):
        """milliseconds of the sparse tier within the last optimize's dense-solve stage (its way down with the core's update, its way
        back); zeros unless the development timing switch was on"""
        ms = np.zeros(2, np.float32)
        _lib.load().mrs_pgo_last_tier_ms(self._h, ms)
        return ms
