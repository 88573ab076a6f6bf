"""The noise, kernel and Levenberg-Marquardt methods of the C++ `mrslam::PoseGraph` adapter (include/mrslam/posegraph.hpp) compiled by plain
g++ against the C ABI, and on the GPU their results for one scene compared bit for bit with the Python path."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "cpp", "build", "posegraph_robust_adapter_test")


def _compile():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    lib_dir = os.path.join(ROOT, "mr_slam_amd")
    if not os.path.exists(os.path.join(lib_dir, "libmrslam_hip.so")):
        import __graft_entry__
        __graft_entry__.build()
    cmd = ["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "posegraph_robust_adapter_main.cpp"), "-o", OUT, "-L" + lib_dir, "-lmrslam_hip", "-Wl,-rpath," + lib_dir]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_posegraph_robust_adapter_compiles_and_links():
    _compile()
    assert os.path.exists(OUT)


@pytest.mark.gpu
def test_posegraph_robust_adapter_equals_the_python_path(tmp_path):
    import posegraph_robust_cases as RC
    from mr_slam_amd import posegraph
    _compile()
    c = RC.case("outliers_geman_mcclure")
    s = c.scene
    lC = np.array(c.lC)
    fin, fout = tmp_path / "scene.bin", tmp_path / "result.bin"
    with open(fin, "wb") as f:
        np.array([len(s.chain_lengths), s.li.size, c.kernel], np.int32).tofile(f)
        np.array([c.k], np.float64).tofile(f)
        for a in (np.array(s.chain_lengths, np.int32), s.odom, c.oC, s.li, s.lj, s.lZ, lC):
            np.ascontiguousarray(a).tofile(f)
    r = subprocess.run([OUT, str(fin), str(fout)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "FAILED" not in r.stdout, r.stdout + r.stderr
    got = np.fromfile(fout, np.float64)
    g = posegraph.PoseGraph(s.chain_lengths)
    g.set_odometry(s.odom)
    g.set_odometry_noise(c.oC)
    g.add_loops(s.li, s.lj, s.lZ, lC)
    g.set_loop_kernel(RC.KERNEL_NAMES[c.kernel], c.k)
    res = g.optimize(method="lm")
    w, r2 = g.loop_state()
    g.set_loop_kernel(None)
    gn = g.optimize(max_iterations=3)
    n, L = g.n_poses, s.li.size
    assert got.size == 8 + 16 * n + 2 * L + 2 + 16 * n
    assert got[:8].tolist() == [res.solves, res.accepted, float(res.converged), res.max_delta, res.cost_initial, res.cost_final, res.separators, res.lam]
    assert np.array_equal(got[8:8 + 16 * n].reshape(n, 4, 4), res.T)
    o = 8 + 16 * n
    assert np.array_equal(got[o:o + L], w) and np.array_equal(got[o + L:o + 2 * L], r2)
    assert got[o + 2 * L:o + 2 * L + 2].tolist() == [gn.iterations, float(gn.converged)]
    assert np.array_equal(got[o + 2 * L + 2:].reshape(n, 4, 4), gn.T)
    want = RC.expected_lm("outliers_geman_mcclure")
    assert np.abs(res.T - want.T).max() < 1e-9 and (res.solves, res.accepted) == (want.solves, want.accepted)
    assert "poses=%d loops=%d solves=%d accepted=%d converged=1" % (n, L, res.solves, res.accepted) in r.stdout
    assert "refused: mrs_pgo_optimize" in r.stdout and "refused: mrs_pgo_add_loops_noise" in r.stdout and "rotation variance" in r.stdout
