"""NumPy restatement of the range histogram ("Fast Histogram") descriptor, vectorised over the points, and the loader of
tests/golden/ref_fasthist.npz.

Written from the contract, not from the reference's text: there is no loop over points or buckets; the ranges come from one
array expression, the buckets from np.searchsorted over the rounded edges fl(i w), the counts from np.bincount.  tests/test_fasthist_cpu.py
checks that it reproduces, count for count and bit for bit, what the reference's own FastHistogram.py produced for every fixture cloud.  It
needs NumPy only, so the GPU suite runs it as the live checker for clouds that are not in the fixture.

The rule.  All arithmetic is IEEE float64 (a float32 cloud is widened first).  d = sqrt((x x + y y) + z z) per point; M = the largest
finite d (0 for an empty cloud); w = M / b; edge e_i = i w, i = 0..b.  A point with 0 < d < M falls into the largest i < b with e_i <= d
(a point exactly on an interior edge goes to the upper bucket); any other point (d == 0, d == M, d not finite) into bucket b - 1.  A point
with 0 < d < M and d > e_b -- possible only when fl(b w) < M -- is counted in bucket b - 1 and in `unbound`; the reference raises there.
"""
import collections
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "ref_fasthist.npz")
DEFAULT_BINS = 100

Result = collections.namedtuple("Result", "counts hist M unbound")


def ranges(cloud):
    """float64 [n] ranges of an [n, >= 3] cloud"""
    p = np.asarray(cloud)
    p = p.reshape(-1, p.shape[-1] if p.ndim == 2 else 3)[:, :3].astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.sqrt((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2])


def edges(M, b):
    """e_i = fl(i fl(M / b)), i = 0..b"""
    return np.arange(b + 1, dtype=np.float64) * (np.float64(M) / np.float64(b))


def buckets(d, M, b):
    """(bucket [n], unbound [n] bool) of ranges d for a cloud whose largest finite range is M"""
    d = np.asarray(d, np.float64)
    e = edges(M, b)
    with np.errstate(invalid="ignore"):
        inside = (d > 0.0) & (d < M)
    k = np.full(d.shape, b - 1, np.int64)
    k[inside] = np.searchsorted(e[:b], d[inside], side="right") - 1       # the number of edges e_0..e_{b-1} that are <= d, less one
    unbound = np.zeros(d.shape, bool)
    unbound[inside] = d[inside] > e[b]
    return k, unbound


def range_histogram(cloud, b=DEFAULT_BINS):
    """Result(counts int64 [b], hist float64 [b], M float64, unbound int) of one cloud"""
    d = ranges(cloud)
    n = d.shape[0]
    finite = d[np.isfinite(d)]
    M = np.float64(finite.max()) if finite.size else np.float64(0.0)
    k, u = buckets(d, M, b)
    counts = np.bincount(k, minlength=b).astype(np.int64)
    hist = counts.astype(np.float64) / np.float64(n) if n else np.zeros(b, np.float64)
    return Result(counts, hist, M, int(u.sum()))


def emd(G, H):
    """getEMD / calculateW: |G_i - H_i| added in index order in float64 (a sequential sum, not NumPy's pairwise one), divided by the length"""
    G, H = np.asarray(G, np.float64).reshape(-1), np.asarray(H, np.float64).reshape(-1)
    return np.add.accumulate(np.abs(G - H))[-1] / np.float64(G.size)


def emd_all(q, entries):
    """emd(q, entry) for every row of entries [n, b] -> float64 [n], the same sequential sums"""
    entries = np.asarray(entries, np.float64)
    return np.add.accumulate(np.abs(np.asarray(q, np.float64)[None, :] - entries), axis=1)[:, -1] / np.float64(entries.shape[1])


def load():
    """{name: {"cloud": float32 / float64 [n, 3], "hist": float64 [b], "counts": int64 [b]}} in the generator's order"""
    z = np.load(FIXTURE)
    nclt = np.load(os.path.join(HERE, "nclt_scan.npz"))["hits"]
    out = collections.OrderedDict()
    for name in [str(s) for s in z["names"]]:
        cloud = nclt if name == "nclt" else z["cloud_" + name]
        out[name] = {"cloud": cloud, "hist": z["hist_" + name], "counts": z["counts_" + name].astype(np.int64)}
    return out
