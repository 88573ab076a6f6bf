"""CPU suite for tests/preprocess_cases.py: the cases are what they claim, the two voxel-grid references agree, the integer emulation of the
batch form stays inside the derived allowance (and three mutations of it do not), and oracle.approx_voxel_grid can be trusted on the new
approximate-grid shapes.  No GPU: what tests/test_preprocess_edges_gpu.py relies on is settled here first."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import preprocess_cases as PC  # noqa: E402
from test_oracle_voxel import _closed_form  # noqa: E402

F32 = np.float32


def test_sizes_and_patterns():
    z = PC.voxel_cases()
    for v in PC.VOXELS:
        for n in PC.SIZES:
            for pat in PC.PATTERNS:
                p, vv = z["%s_n%d_v%g" % (pat, n, v)]
                assert p.shape == (n, 3) and vv == v
                idx = PC.voxel_indices(p, v)
                np.testing.assert_array_equal(idx, PC.pattern_voxels(pat, n))                     # in double ...
                np.testing.assert_array_equal(PC.voxel_indices(p.astype(F32), v), idx)           # ... and after a float32 cast
            assert len(np.unique(PC.voxel_indices(z["one_voxel_n%d_v%g" % (n, v)][0], v), axis=0)) == 1
            assert len(np.unique(PC.voxel_indices(z["distinct_n%d_v%g" % (n, v)][0], v), axis=0)) == n
            a = PC.voxel_indices(z["alternating_n%d_v%g" % (n, v)][0], v)
            assert (a[0::2] == a[0]).all() and (a[1::2] == [3, 1, 2]).all()
    for name, (p, v) in z.items():
        assert p.shape[0] <= 4100 or name.startswith("headroom"), name
        assert PC.rejected_count(p, v) == 0, name
    for name in ("shifted", "shifted_f32"):                                       # 2.2 km out, and inside one binade whatever the seed
        p = z[name][0]
        assert p.shape[0] >= 300 and 2100 < np.linalg.norm(p, axis=1).min() and np.abs(p).max() < 2048
        assert np.abs(p[:, 1] + 2000).max() <= PC.SHIFTED_HALF_WIDTH + 1e-3
    assert z["headroom_2p17"][0].shape[0] == 131072 and z["headroom_2p17_plus1"][0].shape[0] == 131073
    assert PC.batch_bits(131072) == 46 and PC.batch_bits(131073) == 44                            # the last count at the 46-bit scale, and the next
    for n in (131072, 131073):
        p = PC.headroom(n)
        assert len(np.unique(PC.voxel_indices(p, 0.25), axis=0)) == 1
        assert (p[1:] == np.nextafter(p[0] + 0.125, -np.inf)).all() and (p[0] == p.min(0)).all()
    assert max(s.shape[0] for b, _ in PC.voxel_batches().values() for s in b) <= 4100
    assert max(p.shape[0] for p, _ in PC.avg_cases().values()) <= 4100
    assert max(s.shape[0] for b in PC.crop_batches().values() for s in b) <= 4100


def test_runs_land_on_the_lanes_stated():
    lens = PC.run_lengths(1025)
    assert lens[:8] == [1, 2, 3, 4, 5, 6, 1, 2] and sum(lens) == 1025
    start = np.r_[0, np.cumsum(lens)[:-1]]
    end = start + np.asarray(lens) - 1
    single = np.asarray(lens) == 1
    assert 63 in start[single] and 64 in start[single] and 127 in start[single]  # single-point runs on lanes 63, 0, 63
    assert 128 in start[~single]                                                  # a longer run from lane 0
    assert ((end % PC.WAVE == 63) & ~single).any()                                # a longer run that ends on lane 63
    assert ((start // PC.WAVE != end // PC.WAVE)).sum() >= 8                       # runs that straddle a wave edge ...
    assert ((start // 256 != end // 256)).any()                                   # ... and a workgroup edge
    assert 191 in start and 192 in end
    for n in (255, 256, 257):
        lens = PC.run_lengths(n)
        start = np.r_[0, np.cumsum(lens)[:-1]]
        end = start + np.asarray(lens) - 1
        assert sum(lens) == n and 64 in start and 128 in start and (start // PC.WAVE != end // PC.WAVE).any()
    ids = PC.run_ids(1025) % 7                                                    # neighbouring runs are different voxels; every voxel comes back
    v = PC.pattern_voxels("runs", 1025)
    change = (v[1:] != v[:-1]).any(1)
    np.testing.assert_array_equal(change, PC.run_ids(1025)[1:] != PC.run_ids(1025)[:-1])
    assert len(np.unique(ids)) == 7 and len(np.unique(v, axis=0)) == 7


def test_faces_and_extents_sit_where_stated():
    for v in PC.VOXELS:
        p = PC.faces(v)
        idx = PC.voxel_indices(p, v)
        assert (p.min(0) == PC.ANCHOR).all() and (idx[0] == 0).all()
        for a in range(3):
            t = idx[1 + 39 * a: 40 + 39 * a, a].reshape(13, 3)                    # (below, on, above) per face
            # below the face as computed is voxel k or, where rounding put the computed face a hair low or high, k + 1: but never further,
            # and the three neighbours never decrease
            assert (np.diff(t, axis=1) >= 0).all() and (t[:, 2] - t[:, 0] <= 1).all()
            assert (np.abs(t - (np.arange(13)[:, None] + 1)) <= 1).all()
            assert (t[:, 0] != t[:, 2]).sum() >= 3                                # faces that separate two NEIGHBOURING doubles
    z = PC.voxel_cases()
    for a, ax in enumerate("xyz"):
        idx = PC.voxel_indices(z["extent_ok_" + ax][0], 0.2)
        assert idx[:, a].max() == PC.EXTENT - 1 and idx.max() == PC.EXTENT - 1
        p, v, cnt = PC.refused_cases()["extent_bad_" + ax]
        f = np.floor((p - (p.min(0) - v * 0.5)) / v)
        assert f[:, a].max() == PC.EXTENT and cnt == 1
    for name, (p, v, cnt) in PC.refused_cases().items():
        assert PC.rejected_count(p, v) == cnt, name
        assert np.isfinite(p).sum() >= p.size - 1


def test_substep_plant():
    p = PC.substep()
    assert (PC.voxel_indices(p, 0.25) == [[0, 0, 0], [1, 1, 1]]).all()
    steps = (p[1] - 0.125) / PC.batch_step(0.25, 2)
    assert (steps % 1 == 115 / 128).all()


def test_sequential_reference_agrees_with_exact():
    worst = 0.0
    for name, (p, v) in PC.voxel_cases().items():
        em, ei = PC.voxel_exact(p, v)
        sm, si = PC.voxel_sequential(p, v)
        o = np.lexsort((ei[:, 2], ei[:, 1], ei[:, 0]))
        np.testing.assert_array_equal(ei[o], si, err_msg=name)
        assert len(np.unique(ei, axis=0)) == len(ei)
        err = float(np.abs(em[o] - sm).max())
        if PC.at_lidar_range(p):
            worst = max(worst, err)
            assert err <= PC.ACCURACY, (name, err)
        # first-occurrence order: the first point of every voxel, in input order
        idx = PC.voxel_indices(p, v)
        _, first = np.unique(idx, axis=0, return_index=True)
        np.testing.assert_array_equal(idx[np.sort(first)], ei)
    print("sequential vs exact, largest error at lidar range: %.3g m" % worst)


def test_batch_emulation_within_bound_and_63_bits():
    for name, (p, v) in PC.voxel_cases().items():
        bound = PC.batch_bound(p, v)
        em, _ = PC.voxel_exact(p, v)
        got, width = PC.batch_emulate(p, v)
        err = float(np.abs(got - em).max())
        print("batch_bound %-28s %.3g m (emulation off by %.3g), largest sum %d bits" % (name, bound, err, width))
        assert width <= 63, (name, width)                                         # |sum| < 2^63
        assert err <= bound, (name, err, bound)
        if PC.at_lidar_range(p):
            assert bound < PC.ACCURACY, (name, bound)
    for name in ("shifted", "shifted_f32"):                                       # 2.2 km out: the ulp term dominates
        p, v = PC.voxel_cases()[name]
        print("batch_bound %s: %.3g m, of which quantisation %.3g m" % (name, PC.batch_bound(p, v), 0.5 * PC.batch_step(v, p.shape[0])))
        assert PC.batch_bound(p, v) < PC.ACCURACY
    for name, (scans, v) in PC.voxel_batches().items():
        longest = max(s.shape[0] for s in scans)
        for s in scans:
            if s.shape[0]:
                got, width = PC.batch_emulate(s, v, longest)
                assert width <= 63 and np.abs(got - PC.voxel_exact(s, v)[0]).max() <= PC.batch_bound(s, v, longest) < PC.ACCURACY, name
    for name in ("headroom_2p17", "headroom_2p17_plus1"):
        p, v = PC.voxel_cases()[name]
        print("%s: largest sum %d bits at %d fixed-point bits" % (name, PC.batch_emulate(p, v)[1], PC.batch_bits(p.shape[0])))
    assert PC.batch_emulate(*PC.voxel_cases()["headroom_2p17"])[1] == 63           # the headroom is used up: no spare bit


@pytest.mark.parametrize("mutation", ["bits_plus_1", "float32_offset", "truncate"])
def test_cases_catch_mutations_of_the_batch_arithmetic(mutation):
    caught = []
    for name, (p, v) in PC.voxel_cases().items():
        if mutation == "bits_plus_1":
            got, _ = PC.batch_emulate(p, v, bits=PC.batch_bits(p.shape[0]) + 1)
        else:
            got, _ = PC.batch_emulate(p, v, mutate=mutation)
        if np.abs(got - PC.voxel_exact(p, v)[0]).max() > PC.batch_bound(p, v):
            caught.append(name)
    print(mutation, "caught by", caught)
    assert caught
    if mutation == "bits_plus_1":
        assert caught == ["headroom_2p17"]                                        # the one case with no spare bit
    if mutation == "truncate":
        assert "substep" in caught


def test_approximate_grid_cases_are_what_they_claim():
    for leaf in PC.LEAVES:
        for n in PC.AVG_SIZES:
            vox = PC.avg_voxels(PC.avg_cloud("own_bucket", n, leaf), leaf)
            assert len(np.unique(PC.avg_hash(vox))) == min(n, 512) == len(np.unique(vox, axis=0))
            vox = PC.avg_voxels(PC.avg_cloud("evicting", n, leaf), leaf)
            assert (PC.avg_hash(vox) == 0).all() and (vox[0::2] == [0, 0, 0]).all() and (vox[1::2] == [512, 0, 0]).all()
            assert len(np.unique(PC.avg_voxels(PC.avg_cloud("one_voxel", n, leaf), leaf), axis=0)) == 1
            p = PC.avg_cloud("negative", n, leaf)
            vox = PC.avg_voxels(p, leaf)
            assert (vox < 0).all()
            if n >= 511:
                assert (np.trunc(p.astype(F32) * (F32(1) / F32(leaf))) != vox).any()        # floor is not truncation here
            p = PC.avg_cloud("on_leaf", n, leaf)
            k = np.rint(p / leaf)
            np.testing.assert_array_equal(p, (k * leaf).astype(F32).astype(np.float64))
            p = PC.avg_cloud("f64_values", n, leaf)
            assert (p.astype(F32).astype(np.float64) != p).all()
    for p, leaf in PC.avg_cases().values():
        assert np.isfinite(p).all() and np.abs(p / leaf).max() < 2 ** 20


def test_oracle_approximate_grid_on_the_new_cases(oracle):
    for name, (p, leaf) in PC.avg_cases().items():
        want = _closed_form(p, leaf)
        got = oracle.approx_voxel_grid(p, leaf)
        assert got.shape == want.shape, name
        np.testing.assert_array_equal(got, want, err_msg=name)
        if name.startswith("evicting") and p.shape[0] > 1:
            assert got.shape[0] == p.shape[0]                                     # every point flushes the run before it
        if name.startswith(("own_bucket", "one_voxel")):
            assert got.shape[0] == len(np.unique(PC.avg_voxels(p, leaf), axis=0))


def test_crop_plants():
    plants = PC.crop_plants()
    block = PC.crop_planted_block()
    f = block.astype(F32)
    keep = (np.abs(f[:, 0]) < 70.) & (np.abs(f[:, 1]) < 70.) & (f[:, 2] < 30.) & (f[:, 2] > 0.)
    for (name, _, kept), k in zip(plants, keep):
        assert bool(k) == kept, name
    assert PC.crop_restate(block).shape[0] == sum(k for _, _, k in plants)
    by = {n: (p, k) for n, p, k in plants}
    # every threshold has a kept and a dropped plant
    for stem in ("x+70", "x-70", "y+70", "y-70", "z30"):
        assert by[stem + "_inside"][1] and not by[stem + "_exact"][1] and not by[stem + "_outside"][1]
        assert not by[stem + "_rounds_on"][1] and by[stem + "_rounds_in"][1]
    assert by["z0_subnormal"][1] and not by["z0_exact"][1] and not by["z0_negzero"][1] and not by["z0_double_1e-50"][1]
    # the rounding plants are doubles strictly inside the threshold that the float32 cast moves
    assert by["x+70_rounds_on"][0][0] < 70.0 and F32(by["x+70_rounds_on"][0][0]) == F32(70)
    assert F32(by["x+70_rounds_in"][0][0]) == np.nextafter(F32(70), F32(0))
    assert by["z30_rounds_on"][0][2] < 30.0 and F32(by["z30_rounds_on"][0][2]) == F32(30)
    assert F32(by["z30_rounds_in"][0][2]) == np.nextafter(F32(30), F32(0))
    assert by["z0_double_1e-50"][0][2] > 0 and F32(by["z0_double_1e-50"][0][2]) == 0
    assert by["z0_subnormal"][0][2] == 2.0 ** -149 and np.signbit(by["z0_negzero"][0][2])
    b = PC.crop_batches()
    for r in range(3):
        kinds = [("kept" if PC.crop_restate(s).shape[0] == s.shape[0] else "dropped" if PC.crop_restate(s).shape[0] == 0 else "mixed")
                 if s.shape[0] else "empty" for s in b["ends_%d" % r]]
        assert {"kept", "dropped", "empty"} <= set(kinds[1:-1])
        assert kinds[0] == ("kept", "dropped", "empty")[r] and kinds[-1] == ("dropped", "empty", "kept")[r]
    assert PC.crop_restate(b["b1_all_dropped"][0]).shape[0] == 0 and len(b["b1_all_dropped"]) == 1
    for B in (255, 256, 257):
        s = b["b%d_tiny" % B]
        assert len(s) == B and {x.shape[0] for x in s} == {0, 1, 2, 3}
        assert 0 < sum(PC.crop_restate(x).shape[0] for x in s if x.shape[0]) < sum(x.shape[0] for x in s)
