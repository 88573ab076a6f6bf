"""`mrslam::PoseGraph::markPoses` / `marginals` / `jointMarginals` (include/mrslam/posegraph.hpp) compiled by plain g++ against the C ABI, and
on the GPU their blocks for one scene compared bit for bit with the Python path."""
import itertools
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "cpp", "build", "posegraph_marginals_adapter_test")
MARKS = [7, 100, 171]


def _compile():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    lib_dir = os.path.join(ROOT, "mr_slam_amd")
    if not os.path.exists(os.path.join(lib_dir, "libmrslam_hip.so")):
        import __graft_entry__
        __graft_entry__.build()
    cmd = ["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "posegraph_marginals_adapter_main.cpp"), "-o", OUT, "-L" + lib_dir, "-lmrslam_hip", "-Wl,-rpath," + lib_dir]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_posegraph_marginals_adapter_compiles_and_links():
    _compile()
    assert os.path.exists(OUT)


@pytest.mark.gpu
def test_posegraph_marginals_adapter_equals_the_python_path(tmp_path):
    import posegraph_cases as PC
    import posegraph_marginals_restate as MR
    from mr_slam_amd import posegraph
    _compile()
    s = PC.scene("r3x64")
    assert not MR.separators(s.chain_lengths, s.li, s.lj, 64)[MARKS].any()       # interior poses, were they not marked
    fin, fout = tmp_path / "scene.bin", tmp_path / "out.bin"
    with open(fin, "wb") as f:
        np.array([len(s.chain_lengths), s.li.size, len(MARKS)], np.int32).tofile(f)
        for a in (np.array(s.chain_lengths, np.int32), s.odom, s.li, s.lj, s.lZ, np.array(MARKS, np.int32)):
            np.ascontiguousarray(a).tofile(f)
    r = subprocess.run([OUT, str(fin), str(fout)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "FAILED" not in r.stdout, r.stdout + r.stderr
    got = np.fromfile(fout, np.float64)
    g = posegraph.PoseGraph(s.chain_lengths)
    g.set_odometry(s.odom)
    g.add_loops(s.li, s.lj, s.lZ)
    g.mark_poses(MARKS)
    res = g.optimize()
    info = g.marginal_info()
    n, L = g.n_poses, s.li.size
    pairs = list(itertools.combinations(MARKS, 2))
    want = np.concatenate([np.array(info, np.float64), g.marginals().reshape(-1), g.marginals(MARKS, frame="pose3").reshape(-1),
                           g.joint_marginals(s.li, s.lj).reshape(-1),
                           g.joint_marginals([p[0] for p in pairs], [p[1] for p in pairs], frame="pose3").reshape(-1)])
    assert got.size == want.size == 3 + 36 * n + 36 * len(MARKS) + 144 * L + 144 * len(pairs)
    assert np.array_equal(got, want)
    assert info.separators == res.separators == int(MR.separators(s.chain_lengths, s.li, s.lj, 64, MARKS).sum()) - 1
    assert "separators=%d order=%d" % (info.separators, 6 * info.separators) in r.stdout
    assert r.stdout.count("refused: ") == 2 and "no optimisation of the graph as it stands" in r.stdout and "two different poses" in r.stdout
