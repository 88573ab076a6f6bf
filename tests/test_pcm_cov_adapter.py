"""The covariance side of the C++ `mrslam::PairwiseConsistency` adapter (include/mrslam/pcm.hpp) compiled by plain g++ against the C ABI, and
on the GPU its member list for one 65-loop scene compared with the Python path."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "cpp", "build", "pcm_cov_adapter_test")


def _compile():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    lib_dir = os.path.join(ROOT, "mr_slam_amd")
    if not os.path.exists(os.path.join(lib_dir, "libmrslam_hip.so")):
        import __graft_entry__
        __graft_entry__.build()
    cmd = ["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "pcm_cov_adapter_main.cpp"),
           "-o", OUT, "-L" + lib_dir, "-lmrslam_hip", "-Wl,-rpath," + lib_dir]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_pcm_cov_adapter_compiles_and_links():
    _compile()
    assert os.path.exists(OUT)


@pytest.mark.gpu
def test_pcm_cov_adapter_equals_the_python_path(tmp_path):
    import pcm_cov_cases as CC
    from mr_slam_amd import pcm
    _compile()
    L = 65
    XA, XB, QA, QB, ia, kb, Z, Cv, _ = CC.scene(L)
    fin, fout = tmp_path / "scene.bin", tmp_path / "clique.bin"
    with open(fin, "wb") as f:
        np.array([XA.shape[0], XB.shape[0], L], np.int32).tofile(f)
        for a in (XA, XB, QA, QB, ia, kb, Z, Cv):
            np.ascontiguousarray(a).tofile(f)
    r = subprocess.run([OUT, str(fin), str(fout)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "FAILED" not in r.stdout, r.stdout + r.stderr
    got = np.fromfile(fout, np.int32)
    g = pcm.PcmGraph(capacity=L, threshold=pcm.chi2_upper(0.99))
    g.set_trajectories(XA, XB)
    g.set_covariances("span", QA, QB)
    g.add_loops(ia, kb, Z, Cv)
    clique, _ = g.solve()
    assert got[0] == clique.size and got[1] == g.rounds and got[2:].tolist() == clique.tolist()
    want = CC.R.max_clique_heu(CC.RC.consistency_matrix(CC.expected(L, "span")[0], 16.812))
    assert clique.tolist() == list(want[1])
