"""Inputs shared by the pairwise-consistency tests (test_pcm_cpu.py, test_pcm_gpu.py, test_pcm_adapter.py): random poses, the two-robot
scene, the large clique graph, and the restatement's results, computed once per process and never written to."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import pcm_restate as R  # noqa: E402

N_POSES = 40
EXTENT = 500.0                       # metres: trajectory translations lie in [-EXTENT, EXTENT]^3
INLIER_SHARE = 0.6
SIZES = (1, 2, 63, 64, 65, 129)      # loops: one word, its two edges, and three words with a ragged last one
MARGIN = 1e-9                        # no distance of a test scene lies this close to its threshold (test_pcm_cpu.py checks that)


def rotation(rotvec):
    """Rodrigues' formula, float64 [3] -> [3, 3]"""
    rotvec = np.asarray(rotvec, np.float64)
    th = np.linalg.norm(rotvec)
    if th == 0.0:
        return np.eye(3)
    a = rotvec / th
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * (K @ K)


def pose(rotvec, t):
    T = np.eye(4)
    T[:3, :3] = rotation(rotvec)
    T[:3, 3] = t
    return T


def random_pose(rng, extent, max_angle=np.pi):
    a = rng.normal(size=3)
    return pose(a / np.linalg.norm(a) * rng.uniform(0.0, max_angle), rng.uniform(-extent, extent, 3))


@functools.lru_cache(maxsize=None)
def scene(L, seed=0, n_poses=N_POSES, extent=EXTENT, inlier_share=INLIER_SHARE):
    """(XA, XB, ia, kb, Z): two trajectories of random poses, and L loops in the reference's vertex order with distinct key pairs.  An inlier
    measures XA_i^-1 G XB_k (G: the frame of robot B in that of robot A) with 2 cm / 0.3 degree noise, the others are random poses.

    The rotation angles are bounded (trajectory poses 0.3 rad, G 0.25, outliers 0.85, about random axes) so that the rotation of every
    consistency pose Z_u^-1 (XA_i^-1 XA_j) Z_v (XB_l^-1 XB_k) stays below 2 (0.3 + 0.25 + 0.3 + noise) + 4 x 0.3 < 3 rad.  The distance
    tolerance of the suite needs that: Logmap takes the angle from the trace and the axis from the skew part, and near a half turn a rounding
    of R of about 1e-15 (six products) becomes 1e-15 / sin^2 theta in omega and |t| times that in u.  With |t| up to 2e3 m that is 1e-10 at
    theta = 3 (sin^2 = 0.02) but 2e-8 at theta = pi - 0.007, in the restatement as much as in the kernels (an 80-bit evaluation of the same
    pose differs from the float64 one by as much); angles up to pi are covered by half_turn_scene(), with short translations."""
    rng = np.random.default_rng(1000 * L + seed)
    XA = np.stack([random_pose(rng, extent, 0.3) for _ in range(n_poses)])
    XB = np.stack([random_pose(rng, extent, 0.3) for _ in range(n_poses)])
    G = random_pose(rng, 50.0, 0.25)
    keys = np.sort(rng.choice(n_poses * n_poses, L, replace=False))
    ia, kb = (keys // n_poses).astype(np.int32), (keys % n_poses).astype(np.int32)
    Z = np.empty((L, 4, 4))
    for u in range(L):
        if rng.random() < inlier_share:
            noise = pose(rng.normal(0, np.deg2rad(0.3), 3), rng.normal(0, 0.02, 3))
            Z[u] = R.inverse(XA[ia[u]]) @ G @ XB[kb[u]] @ noise
        else:
            Z[u] = random_pose(rng, 30.0, 0.85)
    for a in (XA, XB, ia, kb, Z):
        a.setflags(write=False)
    return XA, XB, ia, kb, Z


@functools.lru_cache(maxsize=None)
def branch_scenes():
    """one two-loop scene (XA, XB, ia, kb, Z) per pose of branch_poses(): both trajectories stand still at the identity, loop 0 measures the
    identity and loop 1 the pose, which is then the consistency pose of the pair: every branch of Logmap, half turns included, with
    translations of a few metres (one pair per scene: the pose between a half turn and a turn by 2e-5 would be as ill-conditioned as
    scene() explains)"""
    X = np.stack([np.eye(4)] * 2)
    idx = np.arange(2, dtype=np.int32)
    return tuple((X, X, idx, idx, np.stack([np.eye(4), b])) for b in branch_poses())


@functools.lru_cache(maxsize=None)
def expected(L, seed=0):
    """the restatement's distances [L, L] of scene(L, seed) (read-only)"""
    D = R.consistency_distances(*scene(L, seed))
    D.setflags(write=False)
    return D


@functools.lru_cache(maxsize=None)
def expected_clique(L, p, seed=0):
    size, members = R.max_clique_heu(R.consistency_matrix(expected(L, seed), R.THRESHOLDS[p]))
    return size, tuple(members)


@functools.lru_cache(maxsize=None)
def big_graph():
    """(adjacency bool [4096, 4096], size, members): background density 0.02 and a planted near-clique of 600 that includes the last vertex"""
    n, planted = 4096, 600
    rng = np.random.default_rng(4096)
    A = np.triu(rng.random((n, n)) < 0.02, 1)
    members = np.concatenate([rng.choice(n - 1, planted - 1, replace=False), [n - 1]])
    P = np.zeros((n, n), bool)
    P[np.ix_(members, members)] = rng.random((planted, planted)) < 0.97
    A |= np.triu(P | P.T, 1)
    A = A | A.T
    A.setflags(write=False)
    size, got = R.max_clique_heu(A)
    return A, size, tuple(got)


def logmap_poses(n=1000, seed=5):
    """n random poses with rotation angle in (1e-3, 3) and translations of up to 2 m per axis, with their angles and unit axes.  The
    translations are short because of the 1e-12 the callers ask for: the Logmap formula takes omega = theta / (2 sin theta) (R32 - R23, ...),
    which turns a rounding of R by one unit in the last place into about 1e-16 / sin^2 theta of omega, 7e-14 at theta = 3 (sin^2 = 0.02, a few
    roundings), and u = V^-1 t carries that times |t|: 2.5e-13 at |t| = 3.5 m, but 1e-11 at 150 m."""
    rng = np.random.default_rng(seed)
    axis = rng.normal(size=(n, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    theta = rng.uniform(1e-3, 3.0, n)
    T = np.stack([pose(axis[i] * theta[i], rng.uniform(-2, 2, 3)) for i in range(n)])
    return T, theta, axis


def branch_poses():
    """the poses that take the other branches of Logmap: angle 0 and 1e-12 (small angle), half turns about each axis and about a skew axis
    (the three near-pi cases), and an angle just below the series threshold"""
    out = [pose([0, 0, 0], [1.0, -2.0, 3.0]), pose([1e-12, 0, 0], [4.0, 5.0, -6.0]), pose([0, 2e-5, 0], [0.5, 0.25, -1.0])]
    for d in (np.diag([1.0, -1.0, -1.0]), np.diag([-1.0, 1.0, -1.0]), np.diag([-1.0, -1.0, 1.0])):
        T = np.eye(4)
        T[:3, :3] = d
        T[:3, 3] = [0.7, -0.8, 0.9]                                # short: the distance, about 3.7, passes 7.840 and fails 0.872
        out.append(T)
    a = np.array([1.0, 2.0, 2.0]) / 3.0
    T = np.eye(4)
    T[:3, :3] = 2.0 * np.outer(a, a) - np.eye(3)               # a half turn about a: exact in floating point up to one rounding
    T[:3, 3] = [-1.0, 0.5, 2.0]
    out.append(T)
    return np.stack(out)
