"""CPU suite for the RANSAC pose from correspondences (row S5): the public surface, the draw, the NumPy restatement
(tests/golden/ransac_restate.py) on the fixtures of tests/ransac_cases.py -- recovery, the margin condition the exact GPU comparisons
rest on, a refit that changes the count, a tie -- and mr_slam_amd/csrc/ransac_model.hpp, the text the device kernels compile, built for
the HOST with g++ against the restatement and under the address / undefined-behaviour sanitizers (a stand-alone program).  No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ransac_cases as K

R = K.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "cpp", "build")
SRC = os.path.join(ROOT, "tests", "cpp", "ransac_model_host.cpp")
HDRS = [os.path.join(ROOT, "mr_slam_amd", "csrc", f) for f in ("ransac_model.hpp", "icp_update.hpp", "eig3.hpp")]
EXACT = [n for n in K.CASES]                                    # every case is compared exactly on the GPU
HOST_CASES = ["M3", "M65", "H256", "M%d" % (K.TILE + 1), "repeated", "dead", "mirror", "no_edge_test", "refit_changes", "tie", "all_rejected"]


def test_public_surface():
    hdr = open(os.path.join(ROOT, "include", "mrslam_hip.h")).read()
    m = re.search(r"typedef struct mrs_ransac_params \{(.*?)\} mrs_ransac_params;", hdr, flags=re.S)
    assert m
    fields = re.findall(r"\b(int32_t|double)\s+(\w+);", re.sub(r"/\*.*?\*/", "", m[1], flags=re.S))
    assert fields == [("int32_t", "hypotheses"), ("int32_t", "refine_iters"), ("double", "max_distance"), ("double", "edge_similarity"),
                      ("double", "min_sin2")]
    assert "#define MRS_ABI_VERSION 1\n" in hdr and "#define MRS_RANSAC_MAX_HYPOTHESES 65536\n" in hdr
    from mr_slam_amd import _lib, fpfh
    protos = _lib.parse_header(_lib.HEADER)
    assert [p[2] for p in protos["mrs_ransac_pose_batch"][1]] == ["ctx", "d_src", "d_dst", "stride_floats", "d_offsets", "h_offsets", "n_pairs",
                                                                   "h_seeds", "params", "d_T", "d_info", "d_mask", "stream"]
    assert [f[0] for f in fpfh.RansacParams._fields_] == [f[1] for f in fields] and C.sizeof(fpfh.RansacParams) == 32
    assert callable(fpfh.ransac_pose) and callable(fpfh.correspondences) and fpfh.RANSAC_MAX_HYPOTHESES == 65536


def test_draw_is_distinct_in_range_and_a_function_of_seed_h_and_size():
    for seed in (0, 1, 2**63 + 5, 2**64 - 1):
        for M in (3, 4, 5, 64, 1000, 2**31 - 2):
            d = R.draws(seed, 200, M)
            assert ((d >= 0) & (d < M)).all()
            assert (d[:, 0] != d[:, 1]).all() and (d[:, 0] != d[:, 2]).all() and (d[:, 1] != d[:, 2]).all()
            assert np.array_equal(d, R.draws(seed, 200, M)) and np.array_equal(d[:50], R.draws(seed, 50, M))
    d3 = R.draws(9, 500, 3)
    assert (np.sort(d3, axis=1) == [0, 1, 2]).all() and len({tuple(r) for r in d3.tolist()}) == 6      # every permutation turns up
    # every index is drawn, about equally often
    c = np.bincount(R.draws(3, 6000, 10).reshape(-1), minlength=10)
    assert c.min() > 1500 and c.max() < 2100
    # the finaliser over the golden-ratio sequence is splitmix64 itself: its first two published outputs for seed 0
    assert R.mix(0) == 0 and R.mix(R.GOLDEN) == 0xE220A8397B1DCDAF and R.mix(2 * R.GOLDEN) == 0x6E789E6AA1B965F4


def test_pre_rejection_on_hand_made_triples():
    p = np.array([[0, 0, 0], [4, 0, 0], [0, 3, 0]], np.float64)
    idx = np.array([[0, 1, 2]])
    ok = lambda q, s=0.9, m=1e-6: bool(R.triples_ok(p, np.asarray(q, np.float64), idx, s, m)[0])
    assert ok(p + 5)
    assert ok(p * 1.05) and not ok(p * 1.2)                      # edges 5 % longer: 1 / 1.05^2 >= 0.81; 20 % longer: not
    assert ok(p * 1.2, s=0.0) and ok(p * 1000, s=0.0)
    assert not ok([[0, 0, 0], [0, 0, 0], [0, 3, 0]], s=0.0)      # a zero edge on the target side
    assert not ok([[0, 0, 0], [4, 0, 0], [np.nan, 3, 0]], s=0.0) and not ok([[0, 0, 0], [4, 0, 0], [np.inf, 3, 0]], s=0.0)
    line = np.array([[0, 0, 0], [1, 0, 0], [2, 1e-4, 0]], np.float64)        # sin^2 = 2.5e-9
    assert not R.triples_ok(line, line, idx, 0.9, 1e-6)[0] and R.triples_ok(line, line, idx, 0.9, 1e-9)[0]
    assert not R.triples_ok(line * [1, 0, 0], line * [1, 0, 0], idx, 0.9, 0.0)[0]         # exactly collinear: 0 <= 0 rejects even at min_sin2 = 0


@pytest.mark.parametrize("name", EXACT)
def test_margin_condition_of_every_fixture(name):
    """A condition on the INPUTS of tests/test_ransac_gpu.py, not a measurement: under no valid hypothesis and no refit step does the
    restatement find a residual within 1e-9 d^2 of d^2, so rounding differences between the device's Jacobi fit and LAPACK's cannot move an
    inlier verdict.  A fixture that fails this gets another seed (tests/ransac_cases.py), never another bound."""
    for hyp in (None, K.BATCH_H) if name in K.BATCH else (None,):
        r = K.expected(name, hyp)
        assert r["margin"] > K.MARGIN, r["margin"]


def _pose_error(T, Tt):
    return float(np.abs(T[:3, :3] - Tt[:3, :3]).max()), float(np.abs(T[:3, 3] - Tt[:3, 3]).max())


def test_restatement_recovers_the_planted_pose():
    Tt = np.eye(4); Tt[:3, :3] = K.TRUE_R; Tt[:3, 3] = K.TRUE_T
    for name in ("M63", "M64", "M65", "M%d" % (K.TILE + 1), "M%d" % (3 * K.TILE + 5), "H63", "H1000", "repeated", "dead", "stride5", "refit_changes",
                 "refit_rises"):
        r = K.expected(name)
        src, dst = K.inputs(name)
        planted = np.sqrt(R.residual2(Tt, R.widen(src), R.widen(dst))) <= K.D
        er, et = _pose_error(r["T"], Tt)
        assert er < 5e-3 and et < 0.1, (name, er, et)
        assert r["info"][0] >= 0.95 * planted.sum() and r["info"][0] == r["mask"].sum() == r["hist"][r["hist"].index(max(r["hist"]))], name
        assert abs(np.linalg.det(r["T"][:3, :3]) - 1) < 1e-12
    p, q, Tx = K.exact(14, 300)
    r = K.expected("exact")
    assert r["info"][0] == 300 and np.abs(r["T"] - Tx).max() < 1e-9


def test_fixtures_cover_a_refit_that_changes_the_count_a_drop_and_a_tie():
    assert K.expected("refit_changes")["hist"] == [70, 86, 87, 86]             # up, then down: iterate 2 is the result
    assert K.expected("refit_changes")["info"].tolist()[0::3] == [87, 3]
    assert K.expected("refit_rises")["hist"] == [81, 88, 88]                   # stops after the step that repeats the set
    assert K.expected("mirror")["hist"] == [13, 12, 12] and K.expected("mirror")["info"][0] == 13      # the refit only loses: iterate 0 stays
    assert K.expected("no_refit")["hist"] == [92] and K.expected("no_refit")["info"][3] == 0
    c = K.expected("tie")["counts"]
    assert (c == c.max()).sum() >= 2 and K.expected("tie")["info"][1] == int(np.argmax(c))             # the lowest h of the best
    assert K.expected("all_rejected")["info"].tolist() == [0, -1, 0, 0] and np.array_equal(K.expected("all_rejected")["T"], np.eye(4))
    assert K.expected("H1")["info"].tolist() == [0, -1, 0, 0]
    src, dst = K.inputs("dead")
    assert not K.expected("dead")["mask"][~R.live(R.widen(src), R.widen(dst))].any()


def test_end_to_end_scene_gives_enough_correct_matches_on_the_cpu():
    """the scene of the GPU suite's end-to-end test through the FPFH restatement: ISS keypoints, FPFH, nearest descriptor (over the
    float32-rounded descriptors, as fpfh.match) -> at least half of the matches are the true ones, and the restated RANSAC finds the pose"""
    F = K.F
    pts, nrm, pts2, nrm2, where, Rm = K.e2e_scene()
    kp, desc = [], []
    for P, N in ((pts, nrm), (pts2, nrm2)):
        k, _, margin = F.iss(P, F.ISS_SALIENT, F.ISS_NONMAX)
        assert margin > 1e-9                                     # no ISS decision hangs on rounding
        rows = F.radius_rows(P, F.RADIUS)
        kp.append(k)
        desc.append(F.fpfh(P, rows, F.spfh(P, N, rows, 5)[1], k).astype(np.float32).astype(np.float64))
    j = ((desc[0][:, None] - desc[1][None]) ** 2).sum(-1).argmin(1)
    share = (kp[1][j] == where[kp[0]]).mean()
    assert len(kp[0]) >= 50 and share >= 0.5, (len(kp[0]), share)
    r = R.ransac(pts[kp[0]], pts2[kp[1][j]], 0, K.E2E_D, hypotheses=256)
    assert r["info"][0] >= 0.5 * len(kp[0]) and np.abs(r["T"][:3, 3] - K.E2E_T).max() < K.E2E_D and np.abs(r["T"][:3, :3] - Rm).max() < 1e-3


# ---- the host build of csrc/ransac_model.hpp ---------------------------------------------------------------------------------------------
def _stale(out):
    return not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(p) for p in [SRC] + HDRS)


def _host_lib():
    so = os.path.join(BUILD, "libransac_model_host.so")
    os.makedirs(BUILD, exist_ok=True)
    if _stale(so):
        r = subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-shared", "-fPIC", SRC, "-o", so], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    lib = C.CDLL(so)
    lib.ransac_host_hypotheses.restype = None
    lib.ransac_host_hypotheses.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_long, C.c_ulonglong, C.c_int, C.c_double, C.c_double, C.c_void_p,
                                           C.c_void_p, C.c_void_p]
    lib.ransac_host_score.restype = C.c_int
    lib.ransac_host_score.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_long, C.c_void_p, C.c_double, C.c_void_p]
    return lib


def _host_hypotheses(name):
    src, dst = (np.ascontiguousarray(a) for a in K.inputs(name))
    p = K.params(name)
    H, M = p["hypotheses"], src.shape[0]
    idx = np.zeros((H, 3), np.int64); ok = np.zeros(H, np.uint8); D = np.zeros((H, 16))
    _host_lib().ransac_host_hypotheses(src.ctypes.data, dst.ctypes.data, src.shape[1], M, K.CASES[name][1], H, p["edge_similarity"], p["min_sin2"],
                                       idx.ctypes.data, ok.ctypes.data, D.ctypes.data)
    return src, dst, idx, ok.astype(bool), D.reshape(H, 4, 4)


@pytest.mark.parametrize("name", HOST_CASES)
def test_host_header_equals_the_restatement(name):
    """the same draws and the same verdicts EXACTLY; every valid model within 1e-9 (the bound tests/test_icp_cpu.py holds icp_rigid_fit to
    against NumPy's fit; coordinates within +-64 m); the same inlier mask and count under each of them"""
    src, dst, idx, ok, D = _host_hypotheses(name)
    r = K.expected(name)
    assert np.abs(src[:, :3][np.isfinite(src[:, :3])]).max() <= 64 and np.abs(dst[:, :3][np.isfinite(dst[:, :3])]).max() <= 64
    assert np.array_equal(idx, r["idx"]) and np.array_equal(ok, r["ok"])
    lib = _host_lib()
    mask = np.zeros(src.shape[0], np.uint8)
    for h in np.nonzero(ok)[0]:
        want = r["models"][int(h)]
        assert np.abs(D[h] - want).max() < 1e-9, (h, np.abs(D[h] - want).max())
        assert abs(np.linalg.det(D[h][:3, :3]) - 1) < 1e-12
        Dh = np.ascontiguousarray(D[h])
        n = lib.ransac_host_score(src.ctypes.data, dst.ctypes.data, src.shape[1], src.shape[0], Dh.ctypes.data, K.D, mask.ctypes.data)
        assert n == r["counts"][h] == mask.sum()
    assert (r["counts"][~ok] == -1).all()


def test_draw_of_the_host_header_for_large_seeds_and_sizes():
    """the draw alone, where 64-bit wrap-around matters: seeds near 2^64, h up to 65535, M = 3 and M near 2^31 (no coordinates are read: the
    entry point needs rows, so a small M with the same arithmetic stands in for the large one through R.draw's Python integers)"""
    rng = np.random.default_rng(5)
    pts = rng.normal(size=(7, 3)).astype(np.float32)
    lib = _host_lib()
    for seed in (2**64 - 1, 2**63, 0x9E3779B97F4A7C15):
        H = 65536
        idx = np.zeros((H, 3), np.int64); ok = np.zeros(H, np.uint8); D = np.zeros((H, 16))
        lib.ransac_host_hypotheses(pts.ctypes.data, pts.ctypes.data, 3, 7, seed, H, 0.9, 1e-6, idx.ctypes.data, ok.ctypes.data, D.ctypes.data)
        pick = np.r_[0:300, H - 300:H]
        assert np.array_equal(idx[pick], np.array([R.draw(seed, int(h), 7) for h in pick]))


def test_host_program_is_clean_under_asan_and_ubsan(tmp_path):
    """The same source as a stand-alone program, compiled with -fsanitize=address,undefined (runtimes linked statically: the program runs in
    the environment it inherits), over fixtures with dead, repeated and mirrored rows: no report, and the numbers of the plain build."""
    exe = os.path.join(BUILD, "ransac_model_host_san")
    os.makedirs(BUILD, exist_ok=True)
    if _stale(exe):
        r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-static-libasan", "-static-libubsan", SRC, "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    for name in ("dead", "repeated", "mirror", "M65"):
        src, dst, idx, ok, D = _host_hypotheses(name)
        H = K.params(name)["hypotheses"]
        fin, fout = tmp_path / (name + ".bin"), tmp_path / (name + ".out")
        np.concatenate([src[:, :3], dst[:, :3]], axis=1).astype(np.float32).tofile(fin)
        r = subprocess.run([exe, str(fin), str(fout), str(K.CASES[name][1]), str(H), repr(K.D)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "%d of %d hypotheses valid" % (ok.sum(), H) in r.stdout, r.stdout + r.stderr
        assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr
        got = np.fromfile(fout).reshape(H, 21)
        assert np.array_equal(got[:, :3], idx) and np.array_equal(got[:, 3] != 0, ok)
        assert np.abs(got[ok, 4:20].reshape(-1, 4, 4) - D[ok]).max() < 1e-13
        assert np.array_equal(got[:, 20], K.expected(name)["counts"])
