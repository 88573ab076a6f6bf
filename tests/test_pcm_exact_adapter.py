"""`mrslam::PairwiseConsistency::solveExact` (include/mrslam/pcm.hpp) compiled by plain g++ against the C ABI, and on the GPU its member
list for the 129-loop scene on which the heuristic falls short compared with the Python path."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "cpp", "build", "pcm_exact_adapter_test")


def _compile():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    lib_dir = os.path.join(ROOT, "mr_slam_amd")
    if not os.path.exists(os.path.join(lib_dir, "libmrslam_hip.so")):
        import __graft_entry__
        __graft_entry__.build()
    cmd = ["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "pcm_exact_adapter_main.cpp"),
           "-o", OUT, "-L" + lib_dir, "-lmrslam_hip", "-Wl,-rpath," + lib_dir]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_pcm_exact_adapter_compiles_and_links():
    _compile()
    assert os.path.exists(OUT)


@pytest.mark.gpu
def test_pcm_exact_adapter_equals_the_python_path(tmp_path):
    import pcm_cases as PC
    from mr_slam_amd import pcm
    _compile()
    L, seed = 129, 3
    XA, XB, ia, kb, Z = PC.scene(L, seed)
    fin, fout = tmp_path / "scene.bin", tmp_path / "clique.bin"
    with open(fin, "wb") as f:
        np.array([XA.shape[0], XB.shape[0], L, 25], np.int32).tofile(f)
        for a in (XA, XB, ia, kb, Z):
            np.ascontiguousarray(a).tofile(f)
    r = subprocess.run([OUT, str(fin), str(fout)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "FAILED" not in r.stdout, r.stdout + r.stderr
    got = np.fromfile(fout, np.int32)
    g = pcm.PcmGraph(capacity=L, p=0.25)
    g.set_trajectories(XA, XB)
    g.add_loops(ia, kb, Z)
    heuristic, _ = g.solve()
    clique, _ = g.solve_exact()
    assert g.proof == 2 and got[:4].tolist() == [clique.size, 2, heuristic.size, g.rounds] and got[4:].tolist() == clique.tolist()
    assert clique.size > heuristic.size
