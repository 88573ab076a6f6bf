"""The C++ `mrslam::GlobalElevationMap` adapter (include/mrslam/gem.hpp) compiled by plain g++ against the C ABI, and on the GPU its
composed map and costmap for one scene of three mutually overlapping submaps compared with the bytes of the Python path."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "cpp", "build", "gem_adapter_test")


def _compile():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    lib_dir = os.path.join(ROOT, "mr_slam_amd")
    if not os.path.exists(os.path.join(lib_dir, "libmrslam_hip.so")):
        import __graft_entry__
        __graft_entry__.build()
    cmd = ["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "gem_adapter_main.cpp"),
           "-o", OUT, "-L" + lib_dir, "-lmrslam_hip", "-Wl,-rpath," + lib_dir]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_gem_adapter_compiles_and_links():
    _compile()
    assert os.path.exists(OUT)


@pytest.mark.gpu
def test_gem_adapter_equals_the_python_path(tmp_path):
    import gem_cases as GC
    from mr_slam_amd import gem
    _compile()
    sc = GC.scenes()["k3_weighted"]
    clouds = [a[0] for op, *a in sc["script"] if op == "append_cells"]
    closes = [a for op, *a in sc["script"] if op == "close_submap"]
    opt = sc["calls"][0]
    fin, fout = tmp_path / "scene.bin", tmp_path / "map.bin"
    with open(fin, "wb") as f:
        np.array([len(clouds), opt.shape[0]], np.int32).tofile(f)
        for c, (pose, centre) in zip(clouds, closes):
            np.array([c.size], np.int32).tofile(f)
            c.tofile(f)
            np.ascontiguousarray(pose, np.float32).tofile(f)
            np.array(centre, np.float32).tofile(f)
        np.ascontiguousarray(opt, np.float32).tofile(f)
    r = subprocess.run([OUT, str(fin), str(fout)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "FAILED" not in r.stdout, r.stdout + r.stderr
    st = GC.run(gem.ElevationSubmaps(), sc["script"])
    matched = st.update_global(opt)
    want = st.compose()
    grid = gem.costmap(want, (-2.0, -2.0), (25, 23), 0.2, travers_thresh=0.5)
    with open(fout, "rb") as f:
        head = np.fromfile(f, np.int64, 3)
        sizes = np.fromfile(f, np.int64, len(clouds))
        cells = np.fromfile(f, gem.CELL, int(head[2]))
        got_grid = np.fromfile(f, np.uint8, 25 * 23).reshape(23, 25)
    assert head.tolist() == [matched, st.dropped, want.size] and matched > 100
    assert sizes.tolist() == [st.submap(i)[0].size for i in range(len(st))]
    assert cells.tobytes() == want.tobytes()
    assert np.array_equal(got_grid, grid) and {0, 254, 255} <= set(grid.reshape(-1).tolist())
    assert "submaps=3 matched=%d dropped=%d cells=%d" % (matched, st.dropped, want.size) in r.stdout
