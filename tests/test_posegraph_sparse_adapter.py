"""`mrslam::PoseGraph::setSolver` / `solverStats` (include/mrslam/posegraph.hpp) compiled by plain g++ against the C ABI, and on the GPU their
numbers and poses for one scene compared bit for bit with the Python path."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "cpp", "build", "posegraph_sparse_adapter_test")
DENSE_LIMIT = 4


def _compile():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    lib_dir = os.path.join(ROOT, "mr_slam_amd")
    if not os.path.exists(os.path.join(lib_dir, "libmrslam_hip.so")):
        import __graft_entry__
        __graft_entry__.build()
    cmd = ["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "posegraph_sparse_adapter_main.cpp"), "-o", OUT, "-L" + lib_dir, "-lmrslam_hip", "-Wl,-rpath," + lib_dir]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_posegraph_sparse_adapter_compiles_and_links():
    _compile()
    assert os.path.exists(OUT)


@pytest.mark.gpu
def test_posegraph_sparse_adapter_equals_the_python_path(tmp_path):
    import posegraph_cases as PC
    from mr_slam_amd import posegraph
    _compile()
    s = PC.scene("r3x130")
    fin, fout = tmp_path / "scene.bin", tmp_path / "out.bin"
    with open(fin, "wb") as f:
        np.array([len(s.chain_lengths), s.li.size, DENSE_LIMIT], np.int32).tofile(f)
        for a in (np.array(s.chain_lengths, np.int32), s.odom, s.li, s.lj, s.lZ):
            np.ascontiguousarray(a).tofile(f)
    r = subprocess.run([OUT, str(fin), str(fout)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "FAILED" not in r.stdout, r.stdout + r.stderr
    got = np.fromfile(fout, np.float64)
    g = posegraph.PoseGraph(s.chain_lengths)
    g.set_odometry(s.odom)
    g.add_loops(s.li, s.lj, s.lZ)
    dense = g.optimize()
    g.set_solver("sparse", dense_limit=DENSE_LIMIT)
    res, st1, st2 = g.optimize(), g.solver_stats(1), g.solver_stats()
    n = g.n_poses
    assert got.size == 6 + 24 + 32 * n
    assert got[:6].tolist() == [res.iterations, float(res.converged), res.max_delta, res.error_initial, res.error_final, res.separators]
    assert got[6:14].tolist() == list(st1[:7]) + [posegraph.SOLVERS["sparse"]] and got[14:22].tolist() == list(st2[:7]) + [posegraph.SOLVERS["sparse"]]
    assert st2.core == DENSE_LIMIT and st2.eliminated == res.separators - DENSE_LIMIT > 0
    assert got[22:30].tolist() == [res.separators, 0, res.separators, 0, 0, 0, 0, posegraph.SOLVERS["dense"]]
    assert np.array_equal(got[30:30 + 16 * n].reshape(n, 4, 4), res.T) and np.array_equal(got[30 + 16 * n:].reshape(n, 4, 4), dense.T)
    assert np.abs(res.T - PC.expected("r3x130").T).max() < 1e-9
    assert "eliminated=%d core=%d" % (st2.eliminated, DENSE_LIMIT) in r.stdout
    assert "refused: mrs_pgo_set_solver" in r.stdout and "dense_limit" in r.stdout
