"""GPU: the per-step timing lines of the development switches MRS_SUBMAP_TIMING, MRS_INTAKE_TIMING, MRS_MAP_TIMING and MRS_GEM_TIMING
keep the format the measurement tools parse.  The switches are read once per process, so the calls run in two fresh child processes: one
with MRS_DEV=1 and the four switches, one without any of them.  Each call is made once, at the smallest input that reaches the print:
two clouds of 64 points for the keyframe store, two closed submaps of four cells for the elevation submaps."""
import math
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from mr_slam_amd import gem, globalmap, submap
rng = np.random.default_rng(7)
clouds = [np.concatenate([rng.uniform(-5, 5, (64, 2)), rng.uniform(0, 2, (64, 2))], 1).astype(np.float32) for _ in range(2)]
I = np.eye(4, dtype=np.float32)
store = submap.KeyframeStore()
ids, counts = store.ingest_batch(clouds, [I, I])                           # mrs_keyframes_ingest
assert ids == [0, 1] and counts.min() > 0
pts, offs = store.assemble([[(0, I), (1, I)]])                             # mrs_submap_assemble
assert offs[-1] > 0
assert globalmap.GlobalMap([store]).rebuild([(0, 0, I), (0, 1, I)]).shape[0] > 0      # mrs_map_compose
g = gem.ElevationSubmaps(resolution=0.2, radius=15.0, min_neighbours=2)
for x0 in (0.0, 1.0):
    c = np.zeros(4, gem.CELL)
    c["x"], c["y"], c["z"], c["var"] = x0 + 0.2 * np.arange(4) + 0.1, 0.1, 0.5, 0.5
    g.append_cells(c)
    g.close_submap(I, (x0, 0.0))
g.update_global(np.stack([I, I]))                                          # mrs_gem_update_global
print("child done")
"""

SWITCHES = ("MRS_SUBMAP_TIMING", "MRS_INTAKE_TIMING", "MRS_MAP_TIMING", "MRS_GEM_TIMING")
# switch -> (the expression its tool searches stderr with, the number of leading groups that are times)
LINES = {
    # tools/bench_submap.py
    "MRS_SUBMAP_TIMING": (r"submap steps ms: cells\+grid (\S+) keys (\S+) sort (\S+) heads\+scan (\S+) means\+offsets (\S+)", 5),
    # tools/bench_intake.py
    "MRS_INTAKE_TIMING": (r"intake steps ms: upload (\S+) bounds\+grid (\S+) keys (\S+) sort (\S+) means (\S+) scan\+scatter (\S+) points \d+ bits (\d+)", 6),
    # tools/bench_globalmap.py
    "MRS_MAP_TIMING": (r"map steps ms: bounds\+grid (\S+) keys (\S+) sort (\S+) heads\+scan (\S+) means\+stitch (\S+) points \d+ bits (\d+)", 5),
    # tools/bench_gem.py has no expression: it takes the line that holds "gem update steps ms:" and reads what follows "ms:" as
    # "name value" pairs, of which records, bits and launches are integers and the rest times.  The same reading as an expression:
    "MRS_GEM_TIMING": (r"gem update steps ms: move (\S+) range (\S+) keys (\S+) sort (\S+) heads\+gather (\S+) fuse (\S+) records (\d+) bits (\d+) launches (\d+)$", 6),
}


def _child(switches):
    env = {k: v for k, v in os.environ.items() if k != "MRS_DEV" and k not in SWITCHES}
    if switches:
        env.update({"MRS_DEV": "1", **{s: "1" for s in switches}})
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "child done" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stderr


@pytest.fixture(scope="module")
def stderr_of():
    return {"on": _child(SWITCHES), "off": _child(())}


@pytest.mark.parametrize("switch", SWITCHES)
def test_timing_line_keeps_the_format_its_tool_parses(stderr_of, switch):
    rx, n_times = LINES[switch]
    hits = [m for m in (re.search(rx, line) for line in stderr_of["on"].splitlines()) if m]
    assert len(hits) == 1, stderr_of["on"][-2000:]
    times = [float(v) for v in hits[0].groups()[:n_times]]
    print(switch, times)
    assert all(math.isfinite(t) and t >= 0 for t in times), times
    assert not any(re.search(rx, line) for line in stderr_of["off"].splitlines()), stderr_of["off"][-2000:]
