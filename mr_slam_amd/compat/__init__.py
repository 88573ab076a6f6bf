"""Drop-in replacements for the reference's native extension modules.

`mr_slam_amd.compat.install()` registers them in sys.modules under the reference's names so
that `import voxelocc`, `import gputransform`, `import voxelfeat`, `import torch_radon`,
`import pygicp` in the unmodified LoopDetection nodes resolve to the HIP implementation.  `install(node=True)` adds a `util` module with the
names the nodes import from RING_ros/util.py.  `install(scancontext=True)` adds `pr_methods.ScanContext` (the Scan Context functions main_SC.py
imports, mr_slam_amd/compat/ScanContext.py), `install(m2dp=True)` adds `pr_methods.M2DP` (mr_slam_amd/compat/M2DP.py) and
`install(fasthistogram=True)` adds `pr_methods.FastHistogram` (mr_slam_amd/compat/FastHistogram.py); nothing registers `pr_methods` otherwise.
`install(fpfh=True)` adds the top-level modules `FPFH` (get_spfh, describe and the `point_cloud_normals` global of RING_ros/FPFH.py:
mr_slam_amd/compat/FPFH.py) and `ISS` (the `iss` that file imports and the reference does not ship: mr_slam_amd/compat/ISS.py).
"""
import importlib
import sys
import types

_NAMES = ("gputransform", "voxelocc", "voxelfeat", "torch_radon", "pygicp")


def install(names=_NAMES, node=False, scancontext=False, m2dp=False, fasthistogram=False, fpfh=False):
    """node=True also registers `util` (the names the nodes pull in with `from util import *`: mr_slam_amd/compat/util.py); the candidate loop
    itself is replaced by `mr_slam_amd.node.bind_detect_loop_icp` (INTEGRATION.md 1a')."""
    for n in tuple(names) + (("util",) if node else ()):
        try:
            sys.modules[n] = importlib.import_module("mr_slam_amd.compat." + n)
        except ModuleNotFoundError:
            pass
    for wanted, name in ((scancontext, "ScanContext"), (m2dp, "M2DP"), (fasthistogram, "FastHistogram")):
        if not wanted:
            continue
        mod = importlib.import_module("mr_slam_amd.compat." + name)
        pkg = sys.modules.get("pr_methods")
        if pkg is None:
            pkg = types.ModuleType("pr_methods")
            pkg.__path__ = []
            sys.modules["pr_methods"] = pkg
        setattr(pkg, name, mod)
        sys.modules["pr_methods." + name] = mod
    if fpfh:
        for name in ("FPFH", "ISS"):
            sys.modules[name] = importlib.import_module("mr_slam_amd.compat." + name)
