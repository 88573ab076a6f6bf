"""The C++ `mrslam::GeneralizedIterativeClosestPoint` adapter (include/mrslam/gicp.hpp) compiled against the mock of the pcl::Registration
surface (tests/cpp/mock_pcl.hpp; PCL is not in the image), and on the GPU the call sequence of global_manager.cpp:2419-2426 followed by
ICPCheck's (:2018-2021, :2058-2071)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "cpp", "build", "pclgicp_adapter_test")


def _compile():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    lib_dir = os.path.join(ROOT, "mr_slam_amd")
    if not os.path.exists(os.path.join(lib_dir, "libmrslam_hip.so")):
        import __graft_entry__
        __graft_entry__.build()
    # plain g++: the adapter header needs the C ABI only
    cmd = ["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "cpp"),
           os.path.join(ROOT, "tests", "cpp", "pclgicp_adapter_main.cpp"), "-o", OUT, "-L" + lib_dir, "-lmrslam_hip", "-Wl,-rpath," + lib_dir]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_pclgicp_adapter_compiles_and_links():
    _compile()
    assert os.path.exists(OUT)


@pytest.mark.gpu
def test_pclgicp_adapter_runs_the_registration_call_sequence():
    """converged=1 through a pcl::Registration::Ptr and on the derived type, the transform of mrs_gicp_batch_align_pcl called directly (bit
    for bit), and a GPU fitness within 1e-5 of the mock's brute-force score: the program checks them and prints what it saw."""
    _compile()
    r = subprocess.run([OUT], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PCL_GICP converged=1" in r.stdout and "derived converged=1" in r.stdout and "FAILED" not in r.stdout, r.stdout
