"""Float64 reference, derived allowance and the cloud zoo shared by tests/test_pointfeat_cases_cpu.py (the reference against the restatement
oracle/pointfeat_oracle.py, a NumPy emulation of the kernel's arithmetic against the allowance) and tests/test_pointfeat_edges_gpu.py /
tests/test_pointfeat_gpu.py (the comparisons with k_knn_cov, k_feat_from_knn and k_features_from_neighbors of csrc/gicp_device.hpp).
No test functions and no GPU import here.  Every cloud is computed once per process and shared read-only (functools.lru_cache).

The five eigenvalues of a point (util.py:123-160): the covariance of its k neighbours about their mean, divided by k - 1; the eigenvalues of
the 3x3 and of its xy 2x2 block, both descending.  eig_ref does exactly that in float64 on the widened float32 points.

The allowance of eig_allow is DERIVED, not measured.  The kernel (neighbour_moments + k_feat_from_knn) works in fp64 and rounds each
eigenvalue ONCE to float32; with v = 2^-53 (fp64 unit roundoff), q the query point, d_j = p_j - q and T = sum_j |d_j|^2:

  one rounding to float32        2^-24 |e_i|                                                          (the first term)
  d_j = (double)p_j - (double)q  one rounding each: a factor (1 + v) on every |d_j|, (1 + 2 v) on every product d_a d_b
  sc = sum_j d_a d_b             a chain of k fused or unfused multiply-adds: (k + 1) v sum |d_a d_b| <= (k + 1) v T   (|d_a d_b| <= |d|^2)
  sd = sum_j d_a                 a chain of k additions: k v sum |d_a| each; the product sd_a sd_b / cnt (the reciprocal, two products:
                                 3 roundings) is at most T in size (Cauchy-Schwarz: (sum |d_a|)^2 <= k sum d_a^2): (2 k + 3) v T
  sc - sd sd / cnt               1 rounding of a difference no larger than T;  / (cnt - 1): 1 more
  per covariance element         (k + 1 + 2 + 2 k + 3 + 2) v T / (k - 1) = (3 k + 8) v S,  S = T / (k - 1)
  eigenvalues                    move by at most the 2-norm of the perturbation (Weyl) <= 3 x the largest element: 3 (3 k + 8) v S; the 2x2
                                 block: 2 x, plus the 4 roundings of hm +- sqrt(hd^2 + c01^2) on values <= S -- less than the 3x3's share
  sym3_eigvals                   tests/test_eig3.py pins |w - LAPACK| <= 1e-14 ||A|| < 46 * 2^-52 ||A||, and ||A|| <= trace <= S (the spread
                                 about the mean is no larger than about q): 92 v S.  LAPACK's own error in eig_ref, ~ v ||A||, sits inside
                                 the slack of that measured 1e-14.
  total                          (9 k + 24 + 92) v S = (4.5 + 58 / k) k 2^-52 S <= 34 k 2^-52 S for every k >= 2

so C_FP64 = 34, a constant of the operation count, and the second term is C_FP64 * 2^-52 * k * S.  It is about 1e-5 of the first on a lidar
neighbourhood (the emulation of tests/test_pointfeat_cases_cpu.py stays inside the first term alone there) and decides only where an
eigenvalue is exactly zero: a plane, a line, coincident points (S = 0: the eigenvalues must then BE zero).
"""
import functools

import numpy as np

U32 = 2.0 ** -24
C_FP64 = 34
K_LIST = (2, 5, 7, 16, 17, 21, 30, 31, 32)      # every rung of dispatch_kmax (16 / 20 / 30 / 32), both sides of each edge; partial and whole chunks of 5
K_NOMINAL = 30
SMALL_SIZES = (1, 2, 3, 5, 29, 30, 31)
RAGGED_SIZES = (63, 64, 65, 255, 257, 1023, 1025)    # the 64-point blocks of knn_at, a 256-thread workgroup, a 1024-point tile
SHIFT = (1000.0, -2000.0, 50.0)
K_CLOUDS = ("lidar_norm", "lattice", "duplicates")  # the clouds that go through the whole K_LIST
FEAT_RTOL, FEAT_ATOL = 5e-5, 1e-6                   # finite features against the restatement (the form tests/test_pointfeat_gpu.py has used)


def _ro(x):
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _scan(seed, n, metric):
    from mr_slam_amd import synth
    return _ro(np.ascontiguousarray(synth.lidar_scan(seed, n, metric=metric), np.float32))


@functools.lru_cache(maxsize=None)
def zoo():
    """{name: float32 [n,3]}, every cloud at most 4 000 points"""
    rng = np.random.default_rng(4100)
    z = {"lidar_norm": _scan(401, 3000, False), "lidar_metric": _scan(402, 3000, True)}
    z["lidar_shifted"] = _ro((z["lidar_metric"] + np.asarray(SHIFT, np.float32)).astype(np.float32))
    plane = np.empty((1500, 3), np.float32)
    plane[:, :2] = rng.uniform(-5, 5, (1500, 2))
    plane[:, 2] = 0.25
    z["plane"] = _ro(plane)
    line = np.zeros((600, 3), np.float32)
    line[:, 0] = rng.permutation(np.cumsum(rng.uniform(0.01, 0.3, 600)) - 40.0)
    z["line"] = _ro(line)
    lat = np.stack(np.meshgrid(np.arange(12), np.arange(12), np.arange(12), indexing="ij"), -1).reshape(-1, 3).astype(np.float32) * 0.25
    z["lattice"] = _ro(lat[rng.permutation(lat.shape[0])])
    seven = rng.uniform(-3, 3, (7, 3)).astype(np.float32)
    z["duplicates"] = _ro(np.repeat(seven, 40, 0)[rng.permutation(280)])
    pool = _scan(403, 2000, True)
    for n in SMALL_SIZES:
        z["n%d" % n] = _ro(np.ascontiguousarray(pool[rng.choice(pool.shape[0], n, replace=False)]))
    return z


@functools.lru_cache(maxsize=None)
def ragged():
    """the block-edge batch: one metric scan per size of RAGGED_SIZES"""
    return tuple(_scan(420 + i, n, True) for i, n in enumerate(RAGGED_SIZES))


def cases():
    """(cloud name, k) of the GPU comparisons: every cloud at the nominal k, K_CLOUDS at every k of K_LIST"""
    out = [(name, K_NOMINAL) for name in zoo()]
    out += [(name, k) for name in K_CLOUDS for k in K_LIST if k != K_NOMINAL]
    return out


def exact_knn(pc, k):
    """int32 [n, min(k, n)]: the restatement's kd-tree search (self included); for the CPU tests, which have no GPU neighbours"""
    from oracle import pointfeat_oracle as P
    kk = min(k, pc.shape[0])
    return P.knn_indices(pc, kk).reshape(pc.shape[0], kk)


def _neigh(pc, idx):
    idx = np.asarray(idx)
    assert (idx >= 0).all(), "pass the filled slots only: idx[:, :min(k, n)]"
    return np.asarray(pc, np.float32).astype(np.float64)[idx]          # [n, k, 3]


def _eig5(cov):
    e3 = np.linalg.eigvalsh(cov)[:, ::-1]
    e2 = np.linalg.eigvalsh(cov[:, :2, :2])[:, ::-1]
    return np.concatenate([e3, e2], 1)


def eig_ref(pc, idx):
    """float64 [n,5] from the neighbour indices idx [n,k] (k >= 2, no -1): covariance about the mean / (k - 1), eigvalsh, descending"""
    nb = _neigh(pc, idx)
    d = nb - nb.mean(1, keepdims=True)
    return _eig5(np.einsum("nki,nkj->nij", d, d) / (nb.shape[1] - 1))


def spread(pc, idx):
    """S = sum_j |p_j - q|^2 / (k - 1) about the query point q = pc[i], float64 [n]"""
    d = _neigh(pc, idx) - np.asarray(pc, np.float32).astype(np.float64)[:, None, :]
    return (d * d).sum((1, 2)) / (idx.shape[1] - 1)


def eig_allow(pc, idx, ref):
    """per-element allowance [n,5] of the kernel's eigenvalues against ref = eig_ref(pc, idx): see the module docstring"""
    return U32 * np.abs(ref) + (C_FP64 * 2.0 ** -52 * idx.shape[1]) * spread(pc, idx)[:, None]


def eig_emulated(pc, idx):
    """The kernel's arithmetic in NumPy: fp64 sums of d = p - q and d d^T about the query, cov = (sum d d^T - sum d sum d^T / cnt) / (cnt - 1),
    the eigenvalues in fp64, ONE rounding to float32.  float32 [n,5]."""
    d = _neigh(pc, idx) - np.asarray(pc, np.float32).astype(np.float64)[:, None, :]
    cnt = idx.shape[1]
    sd = np.zeros((d.shape[0], 3))
    sc = np.zeros((d.shape[0], 3, 3))
    for j in range(cnt):                                                # slot by slot, like the kernel
        sd += d[:, j]
        sc += d[:, j, :, None] * d[:, j, None, :]
    cov = (sc - sd[:, :, None] * sd[:, None, :] * (1.0 / cnt)) / (cnt - 1)
    return _eig5(cov).astype(np.float32)


def oracle_noise_bound(pc, idx):
    """What the float32 restatement (oracle/pointfeat_oracle.covariation_eigenvalue) may differ from eig_ref by, [n] (first order, u = 2^-24):
    its mean of k float32 coordinates carries (k - 1) u max|p|, the subtraction one more rounding of a value up to 2 max|p|: every centred
    coordinate is off by delta <= (k + 1) u max|p|; a covariance element then moves by (2 sum |d| delta + k delta^2) / (k - 1) and its own
    float32 chain of k products adds (k + 2) u S'; eigenvalues move by at most 3 x the largest element (Weyl), and the float32 eigvalsh
    adds a few u ||A|| (16 allowed).  S' = the spread about the mean (the trace of the covariance)."""
    nb = _neigh(pc, idx)
    k = nb.shape[1]
    d = nb - nb.mean(1, keepdims=True)
    delta = (k + 1) * U32 * np.abs(nb).max((1, 2))
    dabs = np.sqrt((d * d).sum(2)).sum(1)
    tr = (d * d).sum((1, 2)) / (k - 1)
    return 3 * ((2 * dabs * delta + k * delta * delta) / (k - 1) + (k + 2) * U32 * tr) + 16 * U32 * tr


def classes(x):
    """0 finite, 1 +inf, 2 -inf, 3 NaN"""
    x = np.asarray(x)
    return np.where(np.isnan(x), 3, np.where(np.isposinf(x), 1, np.where(np.isneginf(x), 2, 0))).astype(np.int8)


def assert_features_match(got, want, what="", rtol=FEAT_RTOL, atol=FEAT_ATOL):
    """the class (finite, +inf, -inf, NaN) of EVERY element identical; finite elements within rtol / atol"""
    got, want = np.asarray(got), np.asarray(want)
    cg, cw = classes(got), classes(want)
    bad = np.argwhere(cg != cw)
    assert bad.size == 0, "%s: %d elements differ in class, first (row, feature) %s: %r against %r" % (
        what, bad.shape[0], bad[0], got[tuple(bad[0])], want[tuple(bad[0])])
    fin = cg == 0
    np.testing.assert_allclose(got[fin], want[fin], rtol=rtol, atol=atol, err_msg=what)


def assert_eigens_within_allowance(pc, idx, eig, what=""):
    """every element of eig [n,5] within eig_allow of the float64 reference built from idx; returns the largest used share of the allowance"""
    ref = eig_ref(pc, idx)
    allow = eig_allow(pc, idx, ref)
    err = np.abs(np.asarray(eig, np.float64) - ref)
    assert np.isfinite(np.asarray(eig)).all(), what
    bad = np.argwhere(err > allow)
    assert bad.size == 0, "%s: %d eigenvalues outside the allowance, first (row, which) %s: got %r, reference %r, allowance %.3e" % (
        what, bad.shape[0], bad[0], np.asarray(eig)[tuple(bad[0])], ref[tuple(bad[0])], allow[tuple(bad[0])])
    with np.errstate(invalid="ignore", divide="ignore"):
        share = np.where(allow > 0, err / allow, 0.0)
    return float(share.max())
