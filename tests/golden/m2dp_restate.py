"""NumPy restatement of the M2DP descriptor, vectorised over the 64 planes, and the loader of tests/golden/ref_m2dp.npz.

Written from the method's definition (He, Wang, Zhang, IROS 2016) and the semantics the reference settles (which axes, which bin edges,
np.histogram2d's edge rule, sklearn's component sign), not from the reference's text: there is no loop over planes, the PCA is an
eigen-decomposition of the covariance, and bins come from np.searchsorted.  tests/test_m2dp_cpu.py checks that it reproduces the integer
counts the reference's own M2DP.py produced for every fixture cloud.  It needs NumPy only, so the GPU suite runs it as the live checker
for random clouds, and it reports how many (point, plane) pairs lie so close to a bin edge that either side is a correct answer.
"""
import collections
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "ref_m2dp.npz")
N_AZIMUTH, N_ELEVATION, N_THETA, N_RHO = 4, 16, 16, 8
N_PLANES, N_BINS = N_AZIMUTH * N_ELEVATION, N_THETA * N_RHO
EDGE_EPS = 1e-9          # uncertain: within EDGE_EPS * maxRho of a bin edge

Result = collections.namedtuple("Result", "A desc sigma1 sigma2 uncertain max_rho counts uncertain_rows")
# Three points are coplanar with their centroid, so their third PCA coordinate is zero in exact arithmetic, and the four planes of elevation 0
# (rows 0, 16, 32, 48) have PY = (0, 0, -sin azimuth): there y is EXACTLY zero and theta exactly 0 or pi, a bin edge.  What any floating-point
# implementation, the reference included, counts for those 4 x 3 pairs is the sign of rounding noise.
EDGE_ON_ROWS = (0, 16, 32, 48)


def plane_axes():
    """(PX, PY) [64, 3]: the in-plane axes of plane 16 * azimuth_index + elevation_index.  The plane's normal is the unit vector at that
    azimuth and elevation; PX is the x axis with its normal component removed, PY = normal x PX."""
    az = np.repeat(np.linspace(-np.pi / 2, np.pi / 2, N_AZIMUTH), N_ELEVATION)
    el = np.tile(np.linspace(0, np.pi / 2, N_ELEVATION), N_AZIMUTH)
    normal = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], axis=1)
    px = np.array([1.0, 0.0, 0.0])[None, :] - normal[:, :1] * normal
    return px, np.cross(normal, px)


def pca(cloud):
    """(mean [3], components [3, 3] as rows by descending eigenvalue with the largest-magnitude coefficient positive, eigenvalues [3],
    cloud_pca [n, 3]) of an [n, 3] cloud, n >= 3, in float64"""
    X = np.asarray(cloud, dtype=np.float64)
    mean = X.mean(axis=0)
    Xc = X - mean
    w, V = np.linalg.eigh(Xc.T @ Xc / (X.shape[0] - 1))
    comps = V[:, ::-1].T.copy()
    for r in comps:
        if r[np.argmax(np.abs(r))] < 0:
            r *= -1.0
    return mean, comps, w[::-1].copy(), Xc @ comps.T


def _bin(values, edges):
    """np.histogram's rule: bin i is [edges[i], edges[i + 1]), the last one closed on the right; -1 outside"""
    b = np.searchsorted(edges, values, side="right") - 1
    b[values == edges[-1]] = len(edges) - 2
    b[(b < 0) | (b > len(edges) - 2)] = -1
    return b


def edges(max_rho):
    theta = np.linspace(-np.pi, np.pi, N_THETA + 1)
    rho = np.linspace(0, np.sqrt(max_rho), N_RHO + 1) ** 2
    rho[-1] += 0.001
    return theta, rho


def canonical(desc):
    """the product's sign rule: the pair (u0, v0) with sum(u0) >= 0"""
    d = np.asarray(desc, dtype=np.float64)
    return -d if d[:N_PLANES].sum() < 0 else d


def m2dp(cloud, chunk=4096):
    """-> Result(A [64, 128], desc [192] with the sign rule applied, sigma1, sigma2, number of uncertain (point, plane) pairs, maxRho,
    integer counts [64, 128], the uncertain pairs per plane [64])"""
    X = np.asarray(cloud, dtype=np.float64).reshape(-1, 3)
    n = X.shape[0]
    if n < 3:
        return Result(np.zeros((N_PLANES, N_BINS)), np.zeros(N_PLANES + N_BINS), 0.0, 0.0, 0, 0.0, np.zeros((N_PLANES, N_BINS), np.int64),
                      np.zeros(N_PLANES, np.int64))
    P = pca(X)[3]
    max_rho = np.sqrt(np.square(P).sum(axis=1).max())
    t_edges, r_edges = edges(max_rho)
    px, py = plane_axes()
    eps = EDGE_EPS * max_rho
    counts = np.zeros(N_PLANES * N_BINS, np.int64)
    plane = np.arange(N_PLANES)[None, :]
    uncertain = np.zeros(N_PLANES, np.int64)
    for i in range(0, n, chunk):
        x, y = P[i:i + chunk] @ px.T, P[i:i + chunk] @ py.T          # [m, 64]
        rho, theta = np.sqrt(x * x + y * y), np.arctan2(y, x)
        rb, tb = _bin(rho, r_edges), _bin(theta, t_edges)
        ok = (rb >= 0) & (tb >= 0)
        counts += np.bincount((plane * N_BINS + rb * N_THETA + tb)[ok], minlength=N_PLANES * N_BINS)
        near_r = np.abs(rho[..., None] - r_edges).min(axis=-1) <= eps
        near_t = (rho * np.abs(theta[..., None] - t_edges).min(axis=-1)) <= eps      # arc length to the nearest theta edge
        uncertain += (near_r | near_t).sum(axis=0)
    A = counts.reshape(N_PLANES, N_BINS) / n
    u, s, vh = np.linalg.svd(A)
    desc = canonical(np.concatenate([u[:, 0], vh[0, :]]))
    return Result(A, desc, float(s[0]), float(s[1]), int(uncertain.sum()), float(max_rho), counts.reshape(N_PLANES, N_BINS), uncertain)


def differing_pairs(counts_a, counts_b):
    """per plane [64]: the number of points the two count matrices put in different bins of that plane"""
    return np.abs(np.asarray(counts_a, np.int64) - np.asarray(counts_b, np.int64)).sum(axis=1) // 2


def svd_bound(sigma1, sigma2):
    """per-component bound on a leading singular vector computed with a backward error of a few hundred ulps of ||A||"""
    return 1024 * np.finfo(np.float64).eps * sigma1 / (sigma1 - sigma2)


def load():
    """the fixture as {case name: dict(cloud float32 [n, 3], counts int32 [64, 128], desc [192], sigma1, sigma2)}; the NCLT case reads
    its cloud from tests/golden/nclt_scan.npz"""
    g = np.load(FIXTURE)
    out = {}
    for name in g["names"]:
        name = str(name)
        cloud = np.load(os.path.join(HERE, "nclt_scan.npz"))["hits"] if name == "nclt" else g["cloud_" + name]
        out[name] = dict(cloud=cloud, counts=g["counts_" + name], desc=g["desc_" + name], sigma1=float(g["sigma_" + name][0]),
                         sigma2=float(g["sigma_" + name][1]))
    return out
