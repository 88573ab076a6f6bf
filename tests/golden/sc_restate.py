"""Vectorised NumPy restatement of RING_ros/pr_methods/ScanContext.py (fp64), used by the Scan Context tests to check the fixture
tests/golden/ref_scancontext.npz and to compute expectations for databases too large to run the reference on.  TEST INFRASTRUCTURE ONLY."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def load():
    return dict(np.load(os.path.join(HERE, "ref_scancontext.npz")))


def keys(sc):
    """(ring keys [.., R], sector keys [.., S]) of [.., R, S] (any leading axes are squeezed to the last two)"""
    a = np.asarray(sc, np.float64).reshape(np.shape(sc)[-2:])
    return a.mean(1), a.mean(0)


def sector_norms(k1, k2):
    """||k1 - roll(k2, s)|| for s = 0 .. S-1"""
    S = len(k1)
    idx = (np.arange(S)[None, :] - np.arange(S)[:, None]) % S          # [s, j] -> (j - s) mod S
    return np.sqrt(((np.asarray(k1, np.float64)[None, :] - np.asarray(k2, np.float64)[idx]) ** 2).sum(1))


def _nonempty(sc, norm64):
    """the columns that count: the reference tests np.linalg.norm(column) > 0 in the descriptor's own type, and in float32 the squares
    of values below 2^-75 underflow to 0, so such a column is empty although its fp64 norm is not"""
    a = np.asarray(sc)
    if a.dtype != np.float32:
        return norm64 > 0
    a = a.reshape(a.shape[-2:])
    return (a * a).sum(0, dtype=np.float32) > 0


def _cos(sc1, sc2):
    """[j, c]: cosine of column j of sc1 and column c of sc2 (0 where a norm is 0), and the engaged mask"""
    a = np.asarray(sc1, np.float64).reshape(np.shape(sc1)[-2:])
    b = np.asarray(sc2, np.float64).reshape(np.shape(sc2)[-2:])
    na, nb = np.sqrt((a * a).sum(0)), np.sqrt((b * b).sum(0))
    eng = _nonempty(sc1, na)[:, None] & _nonempty(sc2, nb)[None, :]
    g = a.T @ b
    with np.errstate(invalid="ignore", divide="ignore"):
        c = np.where(eng, g / (na[:, None] * nb[None, :]), 0.0)
    return c, eng


def window_dists(sc1, sc2, shifts):
    """dist_direct_sc(sc1, roll(sc2, t, axis=-1)) for every t of `shifts`"""
    c, eng = _cos(sc1, sc2)
    S = c.shape[0]
    j = np.arange(S)
    out = []
    for t in shifts:
        cc = (j - t) % S
        n = eng[j, cc].sum()
        out.append(1.0 - c[j, cc].sum() / n if n > 0 else 1.0)
    return np.array(out)


def dist_align(sc1, sc2, ratio):
    """(dist, shift, window start, window dists, sector norms)"""
    k1, k2 = keys(sc1)[1], keys(sc2)[1]
    nrm = sector_norms(k1, k2)
    S = len(k1)
    s = int(np.argmin(nrm))
    r = round(0.5 * ratio * S)
    win = list(range(max(-S, s - r), min(S, s + r + 1)))
    wd = window_dists(sc1, sc2, win)
    i = int(np.argmin(wd))
    return wd[i], win[i], win[0], wd, nrm


def distance_sc(sc1, sc2):
    """(1 - max sim, argmax + 1) over the rolls t = 1 .. S of sc1"""
    c, eng = _cos(sc2, sc1)                # [j of sc2, c of sc1]
    S = c.shape[0]
    j = np.arange(S)
    sims = []
    for t in range(1, S + 1):
        cc = (j - t) % S
        n = eng[j, cc].sum()
        sims.append(c[j, cc].sum() / n if n > 0 else 0.0)
    sims = np.array(sims)
    i = int(np.argmax(sims))
    return 1.0 - sims[i], i + 1


def clear_winner(values, pick, rel=None, abs_=None):
    """True when values[pick] is the minimum and beats every other value by the margin (relative or absolute), or when the
    minimum is an exact tie resolved to its first occurrence"""
    v = np.asarray(values, np.float64)
    m = v.min()
    if np.count_nonzero(v == m) > 1:
        return int(np.flatnonzero(v == m)[0]) == pick and np.all((v == m) | (v - m > (abs_ if abs_ else rel * max(abs(m), 1e-300))))
    others = np.delete(v, pick)
    if v[pick] != m:
        return False
    margin = abs_ if abs_ is not None else rel * max(abs(m), 1e-300)
    return others.size == 0 or others.min() - m > margin
