"""CPU suite for pairwise consistency: the NumPy restatement (tests/golden/pcm_restate.py) returns what the reference's own clique finder
returned for the fixture graphs (tests/golden/ref_pcm_clique.npz), its Logmap agrees with an independent closed form and takes every branch,
the pose arithmetic of the kernels (pcm_pose.hpp, compiled by g++ into a stand-alone program) agrees with the restatement, the test scenes
keep the margin the GPU suite relies on, the C-ABI symbols are exported and bound, and the three host helpers do what the reference does."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pcm_cases as PC

R = PC.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def graphs():
    return R.load()


def test_fixture_graphs_present(graphs):
    ns = [g[0] for g in graphs]
    assert len(graphs) >= 24
    assert ns[:4] == [1, 3, 3, 4] and [len(g[1]) for g in graphs[:4]] == [0, 0, 3, 1]
    for n in (63, 64, 65, 128, 129):
        assert n in ns[6:], n
    assert (70, 0, 1) in [(g[0], len(g[1]), g[2]) for g in graphs]            # an empty graph
    assert (65, 65 * 64 // 2, 65) in [(g[0], len(g[1]), g[2]) for g in graphs]     # a complete one
    assert all(g[3].size == g[2] for g in graphs)
    assert os.path.getsize(R.FIXTURE) < 512 * 1024


def test_restatement_returns_the_reference_cliques(graphs):
    """the recorded size AND member list of every graph; the tiny ones are known by hand"""
    for k, (n, edges, size, members) in enumerate(graphs):
        got_size, got = R.max_clique_heu(R.adjacency(n, edges))
        assert got_size == size and got == members.tolist(), (k, n)
    assert [(g[2], g[3].tolist()) for g in graphs[:4]] == [(1, [0]), (1, [0]), (3, [0, 2, 1]), (2, [2, 3])]
    assert R.max_clique_heu(np.zeros((0, 0), bool)) == (-1, [])


def _closed_form_log(T):
    """independent Logmap: scipy's rotation vector, and u = V^-1 t with V^-1 = I - W/2 + (1 - (th/2) cot(th/2)) / th^2 W^2, W = skew(omega)"""
    from scipy.spatial.transform import Rotation
    w = Rotation.from_matrix(T[:, :3, :3]).as_rotvec()
    out = np.empty((T.shape[0], 6))
    for i in range(T.shape[0]):
        th = np.linalg.norm(w[i])
        W = np.array([[0, -w[i, 2], w[i, 1]], [w[i, 2], 0, -w[i, 0]], [-w[i, 1], w[i, 0], 0]])
        Vinv = np.eye(3) - 0.5 * W + (1.0 - 0.5 * th / np.tan(0.5 * th)) / (th * th) * (W @ W)
        out[i, :3], out[i, 3:] = w[i], Vinv @ T[i, :3, 3]
    return out


def test_logmap_agrees_with_closed_form():
    T, theta, axis = PC.logmap_poses()
    got = R.logmap(T)
    assert np.abs(got - _closed_form_log(T)).max() < 1e-12
    assert np.abs(got[:, :3] - axis * theta[:, None]).max() < 1e-12


def test_logmap_branches():
    B = PC.branch_poses()
    xi = R.logmap(B)
    assert np.array_equal(xi[0], [0, 0, 0, 1.0, -2.0, 3.0])                   # small angle: [omega, t]
    assert np.array_equal(xi[1, 3:], [4.0, 5.0, -6.0]) and abs(xi[1, 0] - 1e-12) < 1e-24 and not xi[1, 1:3].any()
    assert xi[2, 1] == B[2, 0, 2] and not np.array_equal(xi[2, 3:], B[2, :3, 3])     # series magnitude 0.5 (R13 - R31), full translation formula
    pi = np.pi
    assert np.array_equal(xi[3, :3], [pi, 0, 0]) and np.array_equal(xi[4, :3], [0, pi, 0]) and np.array_equal(xi[5, :3], [0, 0, pi])
    assert np.abs(xi[6, :3] - pi * np.array([1.0, 2.0, 2.0]) / 3.0).max() < 1e-14
    # a half turn: V^-1 t = t - (pi / 2) a x t + a x (a x t), tan(pi / 2) being huge
    a, t = np.array([1.0, 0, 0]), B[3, :3, 3]
    assert np.abs(xi[3, 3:] - (t - pi / 2 * np.cross(a, t) + np.cross(a, np.cross(a, t)))).max() < 1e-13
    assert R.logmap(B[0]).shape == (6,)


@pytest.fixture(scope="module")
def pose_program(tmp_path_factory):
    d = tmp_path_factory.mktemp("pcm")
    exe = d / "pcm_pose_host"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-I" + os.path.join(ROOT, "mr_slam_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "pcm_pose_host.cpp"), "-o", str(exe)], check=True)
    return exe, d


def _run(pose_program, mode, parts, shape):
    exe, d = pose_program
    with open(d / "in.bin", "wb") as f:
        for p in parts:
            np.ascontiguousarray(p).tofile(f)
    subprocess.run([str(exe), mode, str(d / "in.bin"), str(d / "out.bin")], check=True, timeout=120)
    return np.fromfile(d / "out.bin", np.float64).reshape(shape)


def test_pose_header_logmap_matches_restatement(pose_program):
    T = np.concatenate([PC.logmap_poses()[0], PC.branch_poses()])
    got = _run(pose_program, "logmap", [np.array([T.shape[0]], np.int32), T], (T.shape[0], 6))
    assert np.abs(got - R.logmap(T)).max() < 1e-12


@pytest.mark.parametrize("L", [n for n in PC.SIZES if n > 1])
def test_pose_header_distances_and_scene_margin(pose_program, L):
    """the kernels' order of products (records, one product, one conjugation) against the reference's order within the GPU suite's 1e-9, and
    the condition that suite puts on its inputs: no distance within 1e-9 of a threshold it uses"""
    XA, XB, ia, kb, Z = PC.scene(L)
    want = PC.expected(L)
    got = _run(pose_program, "dist", [np.array([XA.shape[0], XB.shape[0], L], np.int32), XA, XB, ia, kb, Z], (L, L))
    assert np.isfinite(want).all()
    assert np.abs(got - want).max() < 1e-9
    assert np.array_equal(got, got.T) and not got.diagonal().any()
    for p in (0.01, 0.75):
        off = ~np.eye(L, dtype=bool)
        assert np.abs(want[off] - R.THRESHOLDS[p]).min() > PC.MARGIN, p


def test_scenes_have_both_kinds_of_pairs():
    """the matrix tests mean something: consistent and inconsistent pairs under both thresholds, and rotations near pi among the pairs"""
    D = PC.expected(129)
    off = ~np.eye(129, dtype=bool)
    for p in (0.01, 0.75):
        A = R.consistency_matrix(D, R.THRESHOLDS[p])
        assert 10 < A.sum() < off.sum() - 10 and np.array_equal(A, A.T) and not A.diagonal().any()
    assert R.consistency_matrix(D, 7.840).sum() > R.consistency_matrix(D, 0.872).sum()
    assert PC.expected_clique(129, 0.75)[0] >= PC.expected_clique(129, 0.01)[0] >= 2


def test_restatement_nan_is_not_consistent():
    XA, XB, ia, kb, Z = PC.scene(65)
    Z = Z.copy()
    Z[7, 1, 3] = np.nan
    D = R.consistency_distances(XA, XB, ia, kb, Z)
    A = R.consistency_matrix(D, 7.840)
    assert np.isnan(D[7, 8]) and not A[7].any() and not A[:, 7].any()


def test_pcm_symbols_exported_and_bound():
    from mr_slam_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = C.CDLL(_lib.LIB_PATH)
    names = ("mrs_pcm_create", "mrs_pcm_destroy", "mrs_pcm_set_trajectories", "mrs_pcm_add_loops", "mrs_pcm_clear_loops", "mrs_pcm_count",
             "mrs_pcm_solve", "mrs_pcm_get_matrix", "mrs_pcm_set_matrix", "mrs_pcm_get_distances")
    for n in names:
        assert hasattr(lib, n), n
    assert lib.mrs_abi_version() == 1
    api = _lib.load()
    for n in names:
        assert callable(getattr(api, n)), n
    assert "#define MRS_PCM_MAX_LOOPS 4096" in open(_lib.HEADER).read()
    from mr_slam_amd import pcm
    assert pcm.MAX_LOOPS == 4096
    h = C.c_void_p()
    for call in (lambda: api.mrs_pcm_create(None, 16, 0.872, C.byref(h)), lambda: api.mrs_pcm_set_trajectories(None, None, 1, None, 1),
                 lambda: api.mrs_pcm_add_loops(None, None, None, None, 1), lambda: api.mrs_pcm_clear_loops(None),
                 lambda: api.mrs_pcm_count(None, None), lambda: api.mrs_pcm_solve(None, None, None, None),
                 lambda: api.mrs_pcm_get_matrix(None, None), lambda: api.mrs_pcm_set_matrix(None, 0, None),
                 lambda: api.mrs_pcm_get_distances(None, None)):
        with pytest.raises(_lib.MrsError) as e:                  # the C side's null checks, no GPU involved
            call()
        assert e.value.status == 1 and "null pointer" in str(e.value)
    assert api.mrs_pcm_destroy(None) == 0
    with pytest.raises(TypeError, match="h_Z.*float32"):          # the binding takes the element type from the header
        api.mrs_pcm_add_loops(None, None, None, np.zeros((1, 4, 4), np.float32), 1)


def test_chi2_threshold():
    from mr_slam_amd import pcm
    assert [pcm.chi2_threshold(p) for p in (0.01, 0.05, 0.10, 0.25, 0.50, 0.75)] == [0.872, 1.635, 2.204, 3.455, 5.348, 7.840]
    assert {p: pcm.chi2_threshold(p) for p in R.THRESHOLDS} == R.THRESHOLDS
    for p in (0.0, 0.02, 0.012, 0.9, 1.0, -0.01):
        with pytest.raises(ValueError):
            pcm.chi2_threshold(p)


def test_chain_odometry():
    from mr_slam_amd import pcm
    rng = np.random.default_rng(2)
    odom = np.stack([PC.random_pose(rng, 2.0, 0.5) for _ in range(5)])
    X = pcm.chain_odometry(odom)
    assert X.shape == (6, 4, 4) and np.array_equal(X[0], np.eye(4)) and np.array_equal(X[1], np.eye(4) @ odom[0])
    acc = np.eye(4)
    for m in range(5):
        acc = acc @ odom[m]                                        # poseCompose(temp_pose, transform): the running pose on the left
        assert np.array_equal(X[m + 1], acc)
    assert np.array_equal(pcm.chain_odometry(np.zeros((0, 4, 4))), np.eye(4)[None])
    step = PC.pose([0, 0, np.pi / 2], [1.0, 0, 0])                 # four quarter turns with a unit step: back at the start
    assert np.abs(pcm.chain_odometry(np.stack([step] * 4))[4] - np.eye(4)).max() < 1e-15


def test_reference_order():
    from mr_slam_amd import pcm
    ia = [5, 2, 5, 2, 9, 2, 5]
    kb = [1, 7, 0, 3, 4, 7, 1]
    order = pcm.reference_order(ia, kb)
    assert order.tolist() == [3, 1, 2, 0, 4]                       # (2,3) (2,7) (5,0) (5,1) (9,4); the second (2,7) and (5,1) are dropped
    assert pcm.reference_order([], []).size == 0
    assert pcm.reference_order([3], [3]).tolist() == [0]
    XA, XB, ia, kb, Z = PC.scene(129)
    assert pcm.reference_order(ia, kb).tolist() == list(range(129))           # the scenes come in the reference's order
