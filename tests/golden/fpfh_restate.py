"""NumPy restatement of the FPFH contract of DESIGN.md 4.20, written from that contract: brute-force radius rows in fp64, SPFH counts and
values, FPFH with its fixed summation orders, ISS keypoints with numpy.linalg.eigvalsh, the margins a fixture must keep, and the seeded
scenes the fixtures and the GPU tests are made of.  One cloud at a time; rows are lists of int64 arrays of cloud-local indices.

tools/make_fpfh_golden.py records what the reference's own get_spfh / describe give on these scenes into ref_fpfh.npz (data only)."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "ref_fpfh.npz")
# (scene, bins) of every recorded run: even bin counts only with perturbed normals (with analytic plane normals alpha and theta of two
# points of one plane are 0 up to rounding, which is an edge of an even histogram)
RUNS = (("analytic", 5), ("analytic", 11), ("perturbed", 5), ("perturbed", 11), ("perturbed", 4), ("edge", 5), ("scaled", 5))
RADIUS = 0.2
N_KEYPOINTS = 80
ISS_SALIENT, ISS_NONMAX = 0.15, 0.1


# ---- scenes -------------------------------------------------------------------------------------------------------------------------
def scene(seed, perturb=0.0, scaled=False, n_plane=220, n_sphere=160, noise=0.002):
    """two noisy planes that meet at an edge plus a sphere patch: float32 points [n, 3] and float32 normals [n, 3] (analytic, or
    perturbed by `perturb` and renormalised; scaled: every third normal is 1.5 long, so that some alpha leave [-1, 1])"""
    rng = np.random.default_rng(seed)
    a = np.stack([rng.random(n_plane), rng.random(n_plane), noise * rng.standard_normal(n_plane)], 1)
    na = np.tile([0.0, 0.0, 1.0], (n_plane, 1))
    b = np.stack([rng.random(n_plane), 1.0 + noise * rng.standard_normal(n_plane), rng.random(n_plane)], 1)
    nb = np.tile([0.0, 1.0, 0.0], (n_plane, 1))
    d = rng.standard_normal((n_sphere, 3))
    d[:, 2] = np.abs(d[:, 2]) + 0.3
    d /= np.linalg.norm(d, axis=1)[:, None]
    s = np.array([0.5, 0.5, 0.25]) + 0.3 * d
    pts = np.concatenate([a, b, s]).astype(np.float32)
    nrm = np.concatenate([na, nb, d])
    if perturb:
        nrm = nrm + perturb * rng.standard_normal(nrm.shape)
        nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    if scaled:
        nrm[::3] *= 1.5
    order = rng.permutation(len(pts))
    return pts[order], nrm[order].astype(np.float32)


def edge_scene():
    """point 0 and point 1 lie along each other's normals with opposite normals: phi == 1.0 and theta == +-pi exactly, both on a closed
    outer edge; six more points around them"""
    pts = np.array([[0, 0, 0], [0, 0, 0.5], [0.3, 0.1, 0.2], [-0.2, 0.25, 0.1], [0.1, -0.3, 0.4], [0.25, 0.3, -0.1], [-0.3, -0.2, 0.3],
                    [0.05, 0.15, 0.7]], np.float32)
    nrm = np.array([[0, 0, 1], [0, 0, -1], [0.6, 0, 0.8], [0, 0.8, 0.6], [0.8, 0.6, 0], [0, -0.6, 0.8], [-0.8, 0, 0.6], [0.36, 0.48, 0.8]],
                   np.float32)
    return pts, nrm


def make_scene(name, seed):
    if name == "edge":
        return edge_scene()
    return scene(seed, perturb=0.0 if name == "analytic" else 0.1, scaled=name == "scaled")


# ---- rows ---------------------------------------------------------------------------------------------------------------------------
def _d2(points):
    P = np.asarray(points, np.float32)[:, :3].astype(np.float64)
    d = P[None, :, :] - P[:, None, :]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def radius_rows(points, radius):
    """row i = ascending j != i with (dx dx + dy dy) + dz dz <= r r in fp64 on the widened float32 coordinates"""
    n = len(points)
    if n == 0:
        return []
    with np.errstate(invalid="ignore"):
        hit = _d2(points) <= float(radius) * float(radius)
    hit[np.arange(n), np.arange(n)] = False
    return [np.nonzero(hit[i])[0].astype(np.int64) for i in range(n)]


def radius_margin(points, radius):
    """the least |d2 - r2| / r2 over all pairs (inf for fewer than two points)"""
    n = len(points)
    if n < 2:
        return np.inf
    r2 = float(radius) * float(radius)
    d2 = _d2(points)[np.triu_indices(n, 1)]
    return float(np.min(np.abs(d2 - r2)) / r2)


def to_csr(rows):
    lens = np.array([len(r) for r in rows], np.int64)
    row_start = np.zeros(len(rows) + 1, np.int64)
    np.cumsum(lens, out=row_start[1:])
    index = np.concatenate([np.asarray(r, np.int64) for r in rows]).astype(np.int32) if row_start[-1] else np.zeros(0, np.int32)
    return row_start, index


def from_csr(row_start, index):
    return [np.asarray(index[row_start[i]:row_start[i + 1]], np.int64) for i in range(len(row_start) - 1)]


def batch_csr(clouds, radius):
    """CSR rows of a ragged batch (a list of clouds), cloud-local indices: what radius_neighbors returns for the packed batch"""
    rows = []
    for c in clouds:
        rows += radius_rows(c, radius)
    return to_csr(rows)


# ---- SPFH ---------------------------------------------------------------------------------------------------------------------------
def _pairs(points, rows):
    """the kept (i, j) entries of all rows in row order: not the point itself, not at distance 0 -> I, J, unit direction [m, 3], distance"""
    P = np.asarray(points, np.float32)[:, :3].astype(np.float64)
    lens = np.array([len(r) for r in rows], np.int64)
    I = np.repeat(np.arange(len(rows), dtype=np.int64), lens)
    J = np.concatenate([np.asarray(r, np.int64) for r in rows]) if lens.sum() else np.zeros(0, np.int64)
    d = P[J] - P[I]
    dist = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    keep = (I != J) & ~(dist == 0.0)
    return I[keep], J[keep], d[keep], dist[keep]


def pair_features(points, normals, rows):
    """-> I, J, alpha, phi, theta of every kept entry: u = n_i, d the unit direction, v = u x d, w = u x v (two products and a subtraction
    per component), dots as three products added left to right"""
    I, J, d, dist = _pairs(points, rows)
    N = np.asarray(normals, np.float32).astype(np.float64)
    d = d / dist[:, None]
    u, m = N[I], N[J]

    def cross(a, b):
        return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)

    def dot(a, b):
        return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]

    v = cross(u, d)
    w = cross(u, v)
    with np.errstate(invalid="ignore"):
        return I, J, dot(v, m), dot(u, d), np.arctan2(dot(w, m), dot(u, m))


def bin_edges(lo, hi, bins):
    e = np.arange(bins + 1, dtype=np.float64) * ((hi - lo) / bins) + lo
    e[-1] = hi
    return e


def bin_of(v, lo, hi, bins):
    """bin i with e[i] <= v < e[i + 1], the last one closed on the right; -1 for a value outside [lo, hi] or NaN"""
    e = bin_edges(lo, hi, bins)
    with np.errstate(invalid="ignore"):
        inside = (v >= lo) & (v <= hi)
    b = np.searchsorted(e, np.where(inside, v, lo), side="right") - 1
    b = np.minimum(b, bins - 1)
    return np.where(inside, b, -1)


def edge_margin(v, lo, hi, bins):
    """the least distance of a value inside [lo, hi] to an edge, values exactly on lo or hi not counted"""
    e = bin_edges(lo, hi, bins)
    v = v[np.isfinite(v) & (v != lo) & (v != hi)]
    return float(np.min(np.abs(v[:, None] - e[None, :]))) if v.size else np.inf


def spfh(points, normals, rows, bins):
    """-> counts int32 [n, 3 bins], spfh float64 [n, 3 bins]: each third divided by its own sum, zeros where that is 0"""
    n = len(rows)
    I, _, alpha, phi, theta = pair_features(points, normals, rows)
    counts = np.zeros((n, 3 * bins), np.int32)
    for part, (v, lo, hi) in enumerate(((alpha, -1.0, 1.0), (phi, -1.0, 1.0), (theta, -np.pi, np.pi))):
        b = bin_of(v, lo, hi, bins)
        ok = b >= 0
        np.add.at(counts, (I[ok], part * bins + b[ok]), 1)
    out = np.zeros((n, 3 * bins), np.float64)
    for part in range(3):
        c = counts[:, part * bins:(part + 1) * bins]
        s = c.sum(axis=1)
        nz = s > 0
        out[nz, part * bins:(part + 1) * bins] = c[nz].astype(np.float64) / s[nz, None].astype(np.float64)
    return counts, out


# ---- FPFH ---------------------------------------------------------------------------------------------------------------------------
def fpfh(points, rows, spfh_all, keypoints=None):
    """f = spfh_i + (1 / k) sum_j (1 / |p_j - p_i|) spfh_j over the kept entries of row i in row order, then f / |f| with the squares added
    in bin order; zeros for k = 0 and for |f| = 0"""
    n = len(rows)
    I, J, _, dist = _pairs(points, rows)
    W = 1.0 / dist
    k = np.bincount(I, minlength=n)
    first = np.zeros(n + 1, np.int64)
    np.cumsum(k, out=first[1:])
    rank = np.arange(len(I)) - first[I]
    acc = np.zeros_like(spfh_all)
    for t in range(int(k.max()) if len(I) else 0):
        sel = rank == t
        acc[I[sel]] = acc[I[sel]] + W[sel, None] * spfh_all[J[sel]]
    f = np.zeros_like(spfh_all)
    has = k > 0
    f[has] = spfh_all[has] + (1.0 / k[has].astype(np.float64))[:, None] * acc[has]
    norm = np.sqrt(np.add.accumulate(f * f, axis=1)[:, -1])
    out = np.zeros_like(f)
    nz = ~(norm == 0.0)
    out[nz] = f[nz] / norm[nz, None]
    return out if keypoints is None else out[np.asarray(keypoints, np.int64)]


# ---- ISS ----------------------------------------------------------------------------------------------------------------------------
def iss_eigenvalues(points, rows):
    """members = the point and its row; fp64 covariance about their mean divided by their number -> (member counts, eigenvalues [n, 3]
    descending)"""
    P = np.asarray(points, np.float32)[:, :3].astype(np.float64)
    n = len(rows)
    m, lam = np.zeros(n, np.int64), np.zeros((n, 3))
    for i in range(n):
        r = np.asarray(rows[i], np.int64)
        X = P[np.sort(np.concatenate([[i], r[r != i]]))]      # one order per member set: equal sets tie exactly
        m[i] = len(X)
        X = X - X.mean(axis=0)
        lam[i] = np.linalg.eigvalsh(X.T @ X / len(X))[::-1]
    return m, lam


def iss(points, salient_radius, non_max_radius, gamma21=0.975, gamma32=0.975, min_neighbors=5):
    """-> (ascending keypoint indices, saliency [n], least relative margin of every decision taken)"""
    n = len(points)
    m, lam = iss_eigenvalues(points, radius_rows(points, salient_radius))
    enough = m >= min_neighbors
    t21, t32 = gamma21 * lam[:, 0], gamma32 * lam[:, 1]
    passed = enough & (lam[:, 1] < t21) & (lam[:, 2] < t32)
    sal = np.where(passed, lam[:, 2], 0.0)
    margin = np.inf
    with np.errstate(divide="ignore", invalid="ignore"):
        for a, b in ((lam[:, 1], t21), (lam[:, 2], t32)):
            rel = np.abs(a - b)[enough] / np.abs(b)[enough]
            margin = min(margin, float(np.min(rel))) if rel.size else margin
        if passed.any():
            margin = min(margin, float(np.min(lam[passed, 2] / lam[passed, 0])))
    keep = sal > 0
    for i, row in enumerate(radius_rows(points, non_max_radius)):
        if not keep[i]:
            continue
        for j in row:
            if sal[j] > 0 and sal[i] != sal[j]:
                margin = min(margin, abs(sal[i] - sal[j]) / max(sal[i], sal[j]))
            if not (sal[i] > sal[j] or (sal[i] == sal[j] and i < j)):
                keep[i] = False
    return np.nonzero(keep)[0].astype(np.int64), sal, margin


# ---- the fixture --------------------------------------------------------------------------------------------------------------------
def load():
    """-> (scenes, runs): scenes[name] = dict(points, normals, lists (sklearn's, the point itself included), keypoints, radius); runs = a list
    of dict(scene, bins, has, counts, spfh, fpfh) with the reference's numbers"""
    z = np.load(FIXTURE)
    names = [str(r) for r in z["runs"]]
    scenes = {}
    for name in sorted({r.split(":")[0] for r in names}):
        scenes[name] = dict(points=z["pts_" + name], normals=z["nrm_" + name], lists=from_csr(z["rs_" + name], z["idx_" + name]),
                            keypoints=z["kp_" + name], radius=float(z["radius_" + name]))
    runs = [dict(scene=r.split(":")[0], bins=int(r.split(":")[1]), has=z["has_%d" % k], counts=z["counts_%d" % k].astype(np.int32),
                 spfh=z["spfh_%d" % k], fpfh=z["fpfh_%d" % k]) for k, r in enumerate(names)]
    return scenes, runs


def fpfh_tolerance(m, bins):
    """relative tolerance per entry against the reference's recorded FPFH of a keypoint with m neighbours: the forward error of a
    non-negative length-m dot product in unknown order plus a length-3B norm, times 4 for the reference's 1.0 / k product order"""
    return 4.0 * (m + 3 * bins + 8) * 2.0 ** -53
