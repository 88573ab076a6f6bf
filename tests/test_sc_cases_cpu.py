"""The Scan Context cases of tests/sc_cases.py checked on the CPU, on the fp64 restatement alone: the conditions under which
tests/test_sc_shapes_gpu.py may compare shifts exactly, the radius table, the planted ties, the window lengths the ratios were chosen
for, and the restatement itself against what the reference's ScanContext.py computed at five geometries other than 120 x 120."""
import os

import numpy as np
import pytest

import sc_cases as sc
from sc_cases import R

GEOM_FIXTURE = os.path.join(sc.HERE, "golden", "ref_scancontext_geom.npz")


def test_geometries_and_pairs_are_the_planned_ones():
    assert len(sc.GEOMETRIES) == len(set(sc.GEOMETRIES)) == 17 and set(sc.PINNED) <= set(sc.GEOMETRIES)
    for geom in sc.GEOMETRIES:
        P = sc.pairs(geom)
        assert list(P)[:6] == sc.PAIR_NAMES[:6] and ("period" in P) == (geom[1] % 2 == 0)
        for name, (a, b) in P.items():
            assert a.shape == b.shape == geom and a.dtype == b.dtype == np.float32 and a.min() >= 0 and b.min() >= 0
        if geom[0] * geom[1] >= 100:
            a = P["other0"][0]
            assert 0.35 < np.count_nonzero(a) / a.size < 0.65            # about half the cells zero
        # the 1e-25 columns: not empty in fp64, empty to the float32 norm the reference and the kernel take
        t1, t2 = P["tiny"]
        cols = sorted({0, geom[1] // 3, geom[1] - 1})
        assert np.all(t2[:, cols] == np.float32(sc.TINY)) and np.all(np.sqrt((t2.astype(np.float64) ** 2).sum(0))[cols] > 0)
        assert not R._nonempty(t2, None)[cols].any() and np.all(np.linalg.norm(t2[:, cols], axis=0) == 0)
        c, eng = R._cos(t1, t2)
        assert not eng[:, cols].any()


def test_at_most_five_percent_of_the_cases_take_the_weaker_branch():
    total = weak = 0
    for geom in sc.GEOMETRIES:
        E = sc.expected(geom)
        for name in sc.pair_names(geom):
            if sc.never_exact(geom, name):
                continue
            for lab, _ in sc.ratios(geom[1]):
                total += 1
                weak += not sc.exact_shift(E[name]["align"][lab])
    print("weaker branch: %d of %d cases" % (weak, total))
    assert total >= 1200 and weak <= sc.MAX_WEAK * total, (weak, total)


def test_radius_table():
    for ratio, S, want, narrowed in sc.RADIUS_TABLE:
        assert (0.5 * ratio * S) % 1.0 == 0.5                             # a tie in double: round() goes to even
        assert round(0.5 * ratio * S) == sc.radius(ratio, S) == want
        assert int(np.rint(0.5 * float(np.float32(ratio)) * S)) == narrowed != want     # what rounding the float32 ratio gives
    # the ties that the geometries of the sweep meet
    assert {(0.1, 50), (0.15, 60), (0.1, 90)} <= {(r, s) for r, s, _, _ in sc.RADIUS_TABLE}
    assert {(7, 50), (20, 60), (33, 90)} <= set(sc.GEOMETRIES)


def test_planted_ties_are_exact_in_the_restatement():
    for geom in sc.GEOMETRIES:
        S = geom[1]
        P, E = sc.pairs(geom), sc.expected(geom)
        # A vs zero, zero vs zero, A vs A with all-equal keys aside: every shift of a zero key scores the same, the first wins
        for name in ("ZZ", "AZ"):
            nrm = E[name]["align"]["0.1"].nrm
            assert np.all(nrm == nrm[0])
            for lab, ratio in sc.ratios(S):
                e = E[name]["align"][lab]
                assert np.all(e.wd == 1.0) and e.dist == 1.0 and e.shift == e.start == max(-S, -sc.radius(ratio, S))
        if "period" in P:
            nrm = E["period"]["align"]["0"].nrm
            assert nrm[0] == 0.0 and nrm[S // 2] == 0.0 and int(np.argmin(nrm)) == 0
            assert S == 2 or np.all(np.delete(nrm, [0, S // 2]) > 0)
            assert E["period"]["align"]["0"].shift == 0
        # exact rolls: the score at the planted shift is exactly 0
        for name in ("roll3", "roll-2"):
            assert E[name]["align"]["0"].nrm[sc.KNOWN_SSTAR[name](S)] == 0.0
        # a window wider than S holds every shift twice, with equal values: the first (negative) one wins
        for name in sc.pair_names(geom):
            e = E[name]["align"]["4"]
            assert len(e.wd) == 2 * S and e.start == -S and np.array_equal(e.wd[:S], e.wd[S:]) and e.shift < 0


def test_window_lengths_are_the_ones_the_ratios_were_chosen_for():
    hit = {1: 0, 17: 0, 33: 0}
    for geom in sc.GEOMETRIES:
        S = geom[1]
        E = sc.expected(geom)
        rat = dict(sc.ratios(S))
        assert sc.radius(rat["r8"], S) == 8 and sc.radius(rat["r16"], S) == 16 and sc.radius(rat["0"], S) == 0 and sc.radius(rat["4"], S) == 2 * S
        seen = set()
        for name in sc.pair_names(geom):
            for lab, ratio in rat.items():
                e = E[name]["align"][lab]
                s = int(np.argmin(e.nrm))
                assert len(e.wd) == len(sc.window(s, ratio, S)) and e.start == sc.window(s, ratio, S)[0]
                if name in sc.KNOWN_SSTAR and not sc.never_exact(geom, name):
                    assert s == sc.KNOWN_SSTAR[name](S), (geom, name)
                seen.add((lab, len(e.wd)))
            assert len(E[name]["align"]["0"].wd) == 1 and len(E[name]["align"]["4"].wd) == 2 * S
        # s* = 0 (the zero pairs) leaves the window [-r, r] unclipped from S = r + 1 on
        for lab, want in (("r8", 17), ("r16", 33)):
            if S >= (want + 1) // 2:
                assert len(E["ZZ"]["align"][lab].wd) == want and (lab, want) in seen
                hit[want] += 1
            else:
                assert len(E["ZZ"]["align"][lab].wd) == 2 * S                               # S <= r: clipped to all of [-S, S)
        hit[1] += 1
    assert hit[17] >= 12 and hit[33] >= 12


# ---------------------------------------------------------------------------------------------------------------- the reference pin
@pytest.mark.parametrize("geom", sc.PINNED, ids=lambda g: "%dx%d" % g)
def test_restatement_reproduces_the_reference_at_other_geometries(geom):
    g = dict(np.load(GEOM_FIXTURE))
    t = "%dx%d/" % geom
    S = geom[1]
    names, a, b = sc.batch(geom)
    assert list(g[t + "names"]) == names
    assert np.array_equal(g[t + "ratios"], [r for _, r in sc.ratios(S)])
    assert np.array_equal(g[t + "input_sums"], np.stack([a.astype(np.float64).sum((1, 2)), b.astype(np.float64).sum((1, 2))], 1))
    E = sc.expected(geom)
    for p, name in enumerate(names):
        for side, d in enumerate((a[p], b[p])):
            rk, sk = R.keys(d)
            assert np.abs(rk - g[t + "ringkey"][p, side]).max() < sc.TOL_KEY and np.abs(sk - g[t + "sectorkey"][p, side]).max() < sc.TOL_KEY
        nrm = R.sector_norms(g[t + "sectorkey"][p, 0], g[t + "sectorkey"][p, 1])
        assert np.allclose(nrm, g[t + "sector_norms"][p], rtol=sc.REL_NORM, atol=sc.ABS_NORM)
        if R.clear_winner(g[t + "sector_norms"][p], int(np.argmin(nrm)), rel=1e-6):
            assert int(np.argmin(nrm)) == g[t + "sector_shift"][p]
        assert abs(E[name]["direct"] - g[t + "dist_direct"][p]) < sc.TOL_DIST
        for q, (lab, ratio) in enumerate(sc.ratios(S)):
            e = E[name]["align"][lab]
            dist, shift = g[t + "dist_align"][q, p]
            assert abs(e.dist - dist) < sc.TOL_DIST, (name, lab, e.dist, dist)
            if not sc.never_exact(geom, name) and sc.exact_shift(e):
                assert e.shift == int(shift), (name, lab, e.shift, shift)
            else:
                assert abs(R.window_dists(a[p], b[p], [int(shift)])[0] - dist) < sc.TOL_DIST
        d, yaw = E[name]["distance"]
        assert abs(d - g[t + "distance_sc"][p, 0]) < sc.TOL_DIST
    # the bug's geometries: the reference's own window starts at the even radius
    if (0.1, S) in [(r, s) for r, s, _, _ in sc.RADIUS_TABLE]:
        want = [w for r, s, w, _ in sc.RADIUS_TABLE if (r, s) == (0.1, S)][0]
        assert g[t + "dist_align"][1, names.index("ZZ"), 1] == -want
    assert os.path.getsize(GEOM_FIXTURE) <= 256 << 10
