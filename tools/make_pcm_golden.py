"""Writes tests/golden/ref_pcm_clique.npz: graphs and what the REFERENCE's own clique finder (FMC::maxCliqueHeu, Mapping/src/global_manager/src/
pairwise_consistency_maximization/third_parties/fast_max-clique_finder/src/) returns for them.

A small driver is written to a temporary directory and compiled there against the reference's four FMC source files where they lie (the
tree named by MRSLAM_REFERENCE).  Every graph goes to the binary the way the reference hands it over: as the Matrix-Market file that
graph_utils::printConsistencyGraph writes (upper triangle, row by row).  Only the graphs and the returned size and member list are stored;
nothing that was compiled is.  --keep-binary leaves the binary in the ignored build/ directory, where tools/bench_pcm.py looks for its
host baseline.

Run on a development machine that has the reference tree:  python tools/make_pcm_golden.py
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
import pcm_restate as R  # noqa: E402
import ref_import  # noqa: E402

FMC_DIR = os.path.join(ref_import.REF, "Mapping", "src", "global_manager", "src", "pairwise_consistency_maximization", "third_parties",
                       "fast_max-clique_finder", "src")
FMC_SOURCES = ("findClique.cpp", "findCliqueHeu.cpp", "graphIO.cpp", "utils.cpp")
KEPT_BINARY = os.path.join(ROOT, "build", "pcm_fmc_ref")
MAX_BYTES = 512 * 1024

DRIVER = r"""
#include <chrono>
#include <cstdio>
#include "findClique.h"
int main(int argc, char** argv)
{
    for (int a = 1; a < argc; ++a) {
        const auto t0 = std::chrono::steady_clock::now();
        FMC::CGraphIO gio;
        if (!gio.readGraph(argv[a])) return 2;
        const auto t1 = std::chrono::steady_clock::now();
        std::vector<int> members;
        const int size = FMC::maxCliqueHeu(gio, members);
        const auto t2 = std::chrono::steady_clock::now();
        std::printf("clique %d :", size);
        for (int m : members) std::printf(" %d", m);
        std::printf("\ntimes_ms %.6f %.6f\n", std::chrono::duration<double, std::milli>(t1 - t0).count(),
                    std::chrono::duration<double, std::milli>(t2 - t1).count());
    }
    return 0;
}
"""


def build_fmc(out):
    """compile the driver against the reference's FMC sources -> the binary `out`"""
    if not os.path.isdir(FMC_DIR):
        raise RuntimeError("reference tree not present: " + FMC_DIR)
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "driver.cpp"), "w") as f:
            f.write(DRIVER)
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        subprocess.run(["g++", "-O2", "-w", "-I" + FMC_DIR, os.path.join(d, "driver.cpp")] + [os.path.join(FMC_DIR, s) for s in FMC_SOURCES]
                       + ["-o", out], check=True)
    return out


def write_mtx(path, n, edges):
    """what graph_utils::printConsistencyGraph writes (graph_utils_functions.cpp:72-94)"""
    with open(path, "w") as f:
        f.write("%%MatrixMarket matrix coordinate pattern symmetric\n%d %d %d\n" % (n, n, len(edges)))
        for u, v in edges:
            f.write("%d %d\n" % (u + 1, v + 1))


def run_fmc(binary, n, edges, workdir):
    """-> (size, members, read ms, clique ms) of one graph"""
    path = os.path.join(workdir, "graph.mtx")
    write_mtx(path, n, edges)
    out = subprocess.run([binary, path], check=True, capture_output=True, text=True).stdout.splitlines()
    head, _, tail = [ln for ln in out if ln.startswith("clique ")][0].partition(":")
    t = [ln for ln in out if ln.startswith("times_ms ")][0].split()
    return int(head.split()[1]), np.array(tail.split(), np.int32), float(t[1]), float(t[2])


def edges_of(A):
    u, v = np.nonzero(np.triu(A, 1))             # row-major: the order of printConsistencyGraph
    return np.stack([u, v], 1).astype(np.int32)


def random_graph(seed, n, density, planted, keep=0.95):
    """background edges of the given density plus a planted near-clique (each of its edges kept with probability `keep`)"""
    rng = np.random.default_rng(seed)
    A = np.triu(rng.random((n, n)) < density, 1)
    if planted > 1:
        members = rng.choice(n, planted, replace=False)
        P = np.zeros((n, n), bool)
        P[np.ix_(members, members)] = rng.random((planted, planted)) < keep
        A |= np.triu(P | P.T, 1)
    return A | A.T


def graphs():
    tiny = [np.zeros((1, 1), bool), np.zeros((3, 3), bool), ~np.eye(3, dtype=bool), np.zeros((4, 4), bool)]
    tiny[3][2, 3] = tiny[3][3, 2] = True
    out = tiny + [np.zeros((70, 70), bool), ~np.eye(65, dtype=bool)]
    for k, n in enumerate((63, 64, 65, 128, 129)):
        out.append(random_graph(100 + k, n, 0.1, max(2, n // 4)))
    rng = np.random.default_rng(7)
    for k in range(15):
        n = 200 if k == 0 else int(rng.integers(2, 201))
        out.append(random_graph(200 + k, n, float(rng.uniform(0.02, 0.3)), int(rng.integers(0, max(2, n // 3)))))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keep-binary", action="store_true", help="leave the reference binary in build/ for tools/bench_pcm.py")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as d:
        binary = build_fmc(os.path.join(d, "fmc"))
        rec = {"n": [], "size": []}
        for g, A in enumerate(graphs()):
            n, e = A.shape[0], edges_of(A)
            size, members, _, _ = run_fmc(binary, n, e, d)
            assert members.size == size
            rec["n"].append(n); rec["size"].append(size)
            rec["edges_%d" % g] = e.reshape(-1, 2)
            rec["members_%d" % g] = members
            rs, rm = R.max_clique_heu(A)
            print("graph %2d: n = %3d  edges = %5d  size = %3d  restatement %s" % (g, n, len(e), size,
                                                                                   "equal" if (rs, rm) == (size, members.tolist()) else "DIFFERS"))
        if args.keep_binary:
            os.makedirs(os.path.dirname(KEPT_BINARY), exist_ok=True)
            shutil.copy(binary, KEPT_BINARY)
    rec["n"], rec["size"] = np.array(rec["n"], np.int32), np.array(rec["size"], np.int32)
    np.savez_compressed(R.FIXTURE, **rec)
    size = os.path.getsize(R.FIXTURE)
    print("%s: %d bytes" % (R.FIXTURE, size))
    assert size < MAX_BYTES


if __name__ == "__main__":
    main()
