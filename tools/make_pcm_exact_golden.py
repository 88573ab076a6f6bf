"""Writes tests/golden/ref_pcm_maxclique.npz: graphs and what the REFERENCE's own exact clique finder (FMC::maxClique(gio, 0, .),
Mapping/src/global_manager/src/pairwise_consistency_maximization/third_parties/fast_max-clique_finder/src/findClique.cpp) returns for them.

Works like tools/make_pcm_golden.py, whose helpers it uses: a small driver of our own is written to a temporary directory and compiled there
against the reference's four FMC source files where they lie (the tree named by MRSLAM_REFERENCE), every graph goes to the binary as the
Matrix-Market file that graph_utils::printConsistencyGraph writes, and only the graphs and the returned size and member list are stored.
The 26 graphs of ref_pcm_clique.npz are loaded from that file and only their new results are stored.  A graph the reference does not finish
within LIMIT_S seconds is not recorded.  --keep-binary leaves the binary in the ignored build/ directory, where tools/bench_pcm_exact.py
looks for its host baseline.

Run on a development machine that has the reference tree:  python tools/make_pcm_exact_golden.py
Not called by the build, the tests, the smoke run or any benchmark."""
import argparse
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_pcm_golden as G  # noqa: E402
import pcm_exact_restate as X  # noqa: E402
import pcm_restate as R  # noqa: E402

KEPT_BINARY = os.path.join(ROOT, "build", "pcm_fmc_exact_ref")
MAX_BYTES = 512 * 1024
LIMIT_S = 60.0

DRIVER = r"""
#include <chrono>
#include <cstdio>
#include "findClique.h"
int main(int argc, char** argv)
{
    for (int a = 1; a < argc; ++a) {
        FMC::CGraphIO gio;
        if (!gio.readGraph(argv[a])) return 2;
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<int> members;
        const int size = FMC::maxClique(gio, 0, members);
        const auto t1 = std::chrono::steady_clock::now();
        std::printf("clique %d :", size);
        for (int m : members) std::printf(" %d", m);
        std::printf("\ntimes_ms %.6f\n", std::chrono::duration<double, std::milli>(t1 - t0).count());
    }
    return 0;
}
"""


def build_fmc(out):
    """compile the driver against the reference's FMC sources -> the binary `out`"""
    if not os.path.isdir(G.FMC_DIR):
        raise RuntimeError("reference tree not present: " + G.FMC_DIR)
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "driver.cpp"), "w") as f:
            f.write(DRIVER)
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        subprocess.run(["g++", "-O2", "-w", "-I" + G.FMC_DIR, os.path.join(d, "driver.cpp")] + [os.path.join(G.FMC_DIR, s) for s in G.FMC_SOURCES]
                       + ["-o", out], check=True)
    return out


def run_fmc(binary, n, edges, workdir, limit=LIMIT_S):
    """-> (size, members, clique ms) of one graph, or None where the reference did not finish within `limit` seconds"""
    path = os.path.join(workdir, "graph.mtx")
    G.write_mtx(path, n, edges)
    try:
        out = subprocess.run([binary, path], check=True, capture_output=True, text=True, timeout=limit).stdout.splitlines()
    except subprocess.TimeoutExpired:
        return None
    head, _, tail = [ln for ln in out if ln.startswith("clique ")][0].partition(":")
    t = [ln for ln in out if ln.startswith("times_ms ")][0].split()
    return int(head.split()[1]), np.array(tail.split(), np.int32), float(t[1])


def scene_matrix(L, seed, p):
    """the consistency matrix of tests/pcm_cases.scene(L, seed) at confidence p, by the restatement"""
    import pcm_cases as PC
    return R.consistency_matrix(R.consistency_distances(*PC.scene(L, seed)), R.THRESHOLDS[p])


def graphs():
    """[(name, index in ref_pcm_clique.npz or -1, adjacency)]"""
    out = [("clique_fixture_%d" % g, g, R.adjacency(n, e)) for g, (n, e, _, _) in enumerate(R.load())]
    out.append(("random_5_300_0.3_30", -1, G.random_graph(5, 300, 0.3, 30)))
    out.append(("random_5_200_0.5_20", -1, G.random_graph(5, 200, 0.5, 20)))
    for L in (65, 129):
        for seed in range(4):
            for p in (0.01, 0.25):
                out.append(("scene_%d_%d_%g" % (L, seed, p), -1, scene_matrix(L, seed, p)))
    pair = np.zeros((2, 2), bool)
    out.append(("pair_without_edge", -1, pair))
    out.append(("pair_with_edge", -1, ~np.eye(2, dtype=bool)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keep-binary", action="store_true", help="leave the reference binary in build/ for tools/bench_pcm_exact.py")
    args = ap.parse_args()
    rec = {"names": [], "n": [], "size": [], "source": []}
    with tempfile.TemporaryDirectory() as d:
        binary = build_fmc(os.path.join(d, "fmc_exact"))
        for name, source, A in graphs():
            n, e = A.shape[0], G.edges_of(A)
            got = run_fmc(binary, n, e, d)
            if got is None:
                print("%-24s n = %3d  edges = %5d  NOT FINISHED in %g s: not recorded" % (name, n, len(e), LIMIT_S))
                continue
            size, members, ms = got
            assert members.size == size, (name, size, members)
            g = len(rec["n"])
            rec["names"].append(name); rec["n"].append(n); rec["size"].append(size); rec["source"].append(source)
            if source < 0:
                rec["edges_%d" % g] = e.reshape(-1, 2)
            rec["members_%d" % g] = members
            hs = R.max_clique_heu(A)[0]
            print("%-24s n = %3d  edges = %5d  heuristic %3d  exact %3d  reference %9.3f ms" % (name, n, len(e), hs, size, ms))
        if args.keep_binary:
            os.makedirs(os.path.dirname(KEPT_BINARY), exist_ok=True)
            shutil.copy(binary, KEPT_BINARY)
    rec["names"] = np.array(rec["names"])
    for k in ("n", "size", "source"):
        rec[k] = np.array(rec[k], np.int32)
    np.savez_compressed(X.FIXTURE, **rec)
    size = os.path.getsize(X.FIXTURE)
    print("%s: %d graphs, %d bytes" % (X.FIXTURE, rec["n"].size, size))
    assert size < MAX_BYTES


if __name__ == "__main__":
    main()
