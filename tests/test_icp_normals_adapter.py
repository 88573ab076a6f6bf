"""The C++ `mrslam::addNormal` helper and `mrslam::IterativeClosestPointWithNormals` adapter (include/mrslam/icp_normals.hpp) compiled
against the mock of the pcl::Registration surface and of pcl::PointXYZINormal (tests/cpp/mock_pcl_normals.hpp; PCL is not in the image),
and on the GPU the call sequence that global_manager.cpp:2679-2693 prepares, compared with the Python path."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "cpp", "build", "icp_normals_adapter_test")


def _compile():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    lib_dir = os.path.join(ROOT, "mr_slam_amd")
    if not os.path.exists(os.path.join(lib_dir, "libmrslam_hip.so")):
        import __graft_entry__
        __graft_entry__.build()
    # plain g++: the adapter header needs the C ABI only
    cmd = ["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "cpp"),
           os.path.join(ROOT, "tests", "cpp", "icp_normals_adapter_main.cpp"), "-o", OUT, "-L" + lib_dir, "-lmrslam_hip", "-Wl,-rpath," + lib_dir]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_icp_normals_adapter_compiles_and_links():
    _compile()
    assert os.path.exists(OUT)


@pytest.mark.gpu
def test_icp_normals_adapter_equals_the_python_path(tmp_path):
    """addNormal's normals and both alignments (normals carried by the target type, normals computed by the adapter) on the 1500-point pair
    of tests/icp_plane_cases.py: the bits of GicpBatch.compute_normals / align_icp_plane."""
    import icp_plane_cases as PK
    from mr_slam_amd import gicp
    _compile()
    src, tgt, _ = PK.pair(6)
    fin, fout = tmp_path / "pair.bin", tmp_path / "result.bin"
    with open(fin, "wb") as f:
        np.array([src.shape[0], tgt.shape[0]], np.int32).tofile(f)
        src.tofile(f); tgt.tofile(f)
    r = subprocess.run([OUT, str(fin), str(fout)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "addNormal points=1500 ok" in r.stdout and "given normals converged=1" in r.stdout and "computed normals converged=1" in r.stdout
    assert "FAILED" not in r.stdout, r.stdout
    got = np.fromfile(fout, np.float32)
    n = tgt.shape[0]
    b = gicp.GicpBatch(1)
    b.set_sources([src]); b.set_targets([tgt])
    b.compute_normals(1, 15)
    assert np.array_equal(got[:4 * n].reshape(n, 4), b.normals(1))
    T, conv, its, state = b.align_icp_plane(**PK.SETTINGS["MAPPING_890"])
    for run in range(2):
        rec = got[4 * n + 19 * run:4 * n + 19 * (run + 1)]
        assert np.array_equal(rec[:16].reshape(4, 4), T[0].astype(np.float32)), run
        assert (rec[16], rec[18]) == (float(conv[0]), float(state[0])), run
