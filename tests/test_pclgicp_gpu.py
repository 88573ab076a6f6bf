"""GPU suite for the batched PCL-style GICP (row G11): HIP through the C ABI against the NumPy restatement
(tests/golden/pclgicp_restate.py) on the same clouds.  Pose tolerance from BASELINE.json north_star: 1e-4 m / 1e-4 rad.  The natural-stopping
fixtures are those whose margins tests/test_pclgicp_cpu.py checks; a step comparison checks the margin of its own inner decisions first."""
import os

import numpy as np
import pytest
from scipy.spatial.transform import Rotation as Rot

import pclgicp_cases as K

G = K.G
pytestmark = pytest.mark.gpu

TOL_T = 1e-4   # metres
TOL_R = 1e-4   # radians
DBL_MAX = G.I.DBL_MAX
BLOCKS = ((0, 1), (1, 7), (7, 10), (10, 11), (11, 29), (29, 38), (38, 74))     # n, sum M, sum Mq, sum q'Mq, sum p M, sum p Mq, sum p p M


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    from mr_slam_amd import _lib
    _lib.load()
    return "cuda:0"


def _batch(srcs, tgts, search=None):
    from mr_slam_amd import gicp
    b = gicp.GicpBatch(len(srcs))
    if search is not None:
        b.set_search(search)
    b.set_sources(srcs); b.set_targets(tgts)
    return b


def _handle_covs(b, srcs, tgts):
    """the handle's covariances per pair (computed here if the handle has none yet)"""
    b.compute_covariances(0); b.compute_covariances(1)
    ca, cb = b.covariances(0), b.covariances(1)
    so = np.cumsum([0] + [s.shape[0] for s in srcs]); to = np.cumsum([0] + [t.shape[0] for t in tgts])
    return [(ca[so[i]:so[i + 1]], cb[to[i]:to[i + 1]]) for i in range(len(srcs))]


def _close_blocks(got, want, tol):
    for lo, hi in BLOCKS:
        assert np.abs(got[lo:hi] - want[lo:hi]).max() <= tol * np.abs(want[lo:hi]).max(), (lo, got[lo:hi], want[lo:hi])


def _check_step(oracle, src, tgt, covs, T, max_corr, sums, nxt, inner, corr):
    w = G.step(src, tgt, T, covs=covs, max_correspondence_distance=max_corr)
    wcorr = w["corr"]
    # exact search: different indices only where the two candidates are at exactly the same float distance
    assert np.array_equal(oracle.pair_d2(src, T, tgt, corr), oracle.pair_d2(src, T, tgt, wcorr))
    assert np.array_equal(corr >= 0, wcorr >= 0)
    assert (corr == wcorr).mean() > 0.999
    assert (wcorr >= 0).sum() > 100
    # the restatement fed with the kernel's own (equally nearest) neighbours must agree to rounding
    k = G.step(src, tgt, T, covs=covs, corr=corr.astype(np.int64), max_correspondence_distance=max_corr)
    assert G.inner_margin(k["decisions"]) >= K.INNER_MARGIN          # a condition on the input
    for ref in ([w, k] if (corr == wcorr).all() else [k]):
        _close_blocks(sums, ref["sums"], 1e-9)
        print("step", max_corr, int(sums[0]), np.abs(nxt - ref["next"]).max(), tuple(inner), (ref["inner"], ref["end"]))
        assert np.abs(nxt - ref["next"]).max() <= 1e-9
        assert tuple(inner) == (ref["inner"], ref["end"])
    return k


def test_pcl_step_matches_restatement(dev, oracle):
    """9000 points: more than one block of 1024; 1031: one block and 7 points, a ragged last wave.  Thresholds 5.0, 0.5 and one that rejects."""
    big, small = K.pair(3), K.build(12, 1031)
    srcs, tgts = [big[0], small[0]], [big[1], small[1]]
    poses = []
    for _, _, Ttrue in (big, small):
        T = Ttrue.copy(); T[:3, 3] += [0.25, -0.1, 0.05]
        poses.append(T)
    b = _batch(srcs, tgts)
    covs = _handle_covs(b, srcs, tgts)
    n0 = big[0].shape[0]
    for max_corr in (5.0, 0.5, 0.27):
        sums, nxt, inner, corr = b.pcl_step(np.stack(poses), want_corr=True, max_correspondence_distance=max_corr)
        for i in range(2):
            lo = 0 if i == 0 else n0
            _check_step(oracle, srcs[i], tgts[i], covs[i], poses[i], max_corr, sums[i], nxt[i], inner[i], corr[lo:lo + srcs[i].shape[0]])
        if max_corr == 0.27:      # it does reject
            assert 100 < sums[0, 0] < n0 and (corr[:n0] < 0).any()
        else:
            assert sums[0, 0] == n0


def test_pcl_step_far_from_the_origin(dev, oracle):
    """Both clouds shifted by (+55, -48, 3) m: the sums are taken about the pivot, so the next pose keeps its digits."""
    src, tgt, Ttrue = K.pair(3)
    src = (src.astype(np.float64) + K.SHIFT).astype(np.float32)
    tgt = (tgt.astype(np.float64) + K.SHIFT).astype(np.float32)
    T = Ttrue.copy()
    T[:3, 3] += K.SHIFT - Ttrue[:3, :3] @ K.SHIFT + [0.25, -0.1, 0.05]
    b = _batch([src], [tgt])
    covs = _handle_covs(b, [src], [tgt])[0]
    sums, nxt, inner, corr = b.pcl_step(T[None], want_corr=True, max_correspondence_distance=5.0)
    k = _check_step(oracle, src, tgt, covs, T, 5.0, sums[0], nxt[0], inner[0], corr)
    assert np.abs(G.pivot(tgt) - (K.SHIFT + G.pivot(K.pair(3)[1]))).max() < 1e-4
    assert np.abs(nxt[0, :3, 3] - T[:3, 3]).max() > 0.01         # a real step
    assert np.abs(k["next"] - T).max() > 0.01


def test_pcl_step_below_four_correspondences_and_profile(dev):
    """A 3-point source and a target beyond the threshold in one batch with an ordinary pair: their sums are zeros, their pose stays and
    the inner loop did not run, as the restatement's step says.  The measurement hook on the same handle: three positive times, and the
    correspondence count of the step."""
    src, tgt, Ttrue = K.build(12, 1031)
    far = (tgt.astype(np.float64) + 500.0).astype(np.float32)
    srcs, tgts = [src[:3], src, src], [tgt, far, tgt]
    poses = np.stack([Ttrue] * 3)
    b = _batch(srcs, tgts)
    sums, nxt, inner, corr = b.pcl_step(poses, want_corr=True, max_correspondence_distance=2.0)
    w = G.step(srcs[0], tgts[0], Ttrue, max_correspondence_distance=2.0)
    assert not w["sums"].any() and w["inner"] == 0 and np.array_equal(w["next"], Ttrue)
    for i in (0, 1):
        assert not sums[i].any() and np.array_equal(nxt[i], Ttrue) and tuple(inner[i]) == (0, 0), i
    assert (corr[:3] >= 0).all() and (corr[3:3 + 1031] < 0).all()
    assert sums[2, 0] > 900 and inner[2, 0] >= 1 and np.abs(nxt[2] - Ttrue).max() > 0
    ms, cnt = b.pcl_profile(poses, reps=2, max_correspondence_distance=2.0)
    assert set(ms) == {"search", "pclgicp_sums", "pclgicp_update"} and all(0 < v < 1e3 for v in ms.values()), ms
    assert cnt == {"source_points": 3 + 2 * 1031, "correspondences": int((corr >= 0).sum())}
    assert cnt["correspondences"] == 3 + int(sums[2, 0])


def test_forced_iterations_on_the_ragged_batch(dev):
    """force_iterations = 6 on the three pairs of test_align_batch_within_north_star_tolerance: fixed-length parity with the restatement."""
    pairs = [K.pair(s) for s in (3, 4, 5)]
    b = _batch([p[0] for p in pairs], [p[1] for p in pairs])
    guess = np.stack([np.eye(4)] * 3)
    guess[1, :3, 3] = [-0.5, 0.2, 0.0]
    T, conv, its, state = b.align_pcl(guess, force_iterations=6, max_correspondence_distance=5.0)
    assert (its == 6).all() and not conv.any() and (state == G.NOT_CONVERGED).all()
    assert b.nn_passes == 6
    for i, seed in enumerate((3, 4, 5)):
        w = G.gicp(pairs[i][0], pairs[i][1], guess[i], covs=K.covs(seed), force_iterations=6, max_correspondence_distance=5.0)
        dt, dr = K.pose_err(T[i], w["T"])
        print("forced", i, dt, dr)
        assert dt < TOL_T and dr < TOL_R, (i, dt, dr)


def test_natural_stopping_matches_restatement(dev):
    """global_manager.cpp:2422-2425's settings: the same state, converged flag and outer iteration count as the restatement, poses within
    the tolerance, getFitnessScore within 1e-5."""
    pairs = [K.pair(s) for s in K.NATURAL]
    b = _batch([p[0] for p in pairs], [p[1] for p in pairs])
    T, conv, its, state = b.align_pcl(**K.MAPPING_2422)
    fit = b.fitness(T, DBL_MAX)
    for i, seed in enumerate(K.NATURAL):
        w = K.natural(seed)
        dt, dr = K.pose_err(T[i], w["T"])
        wfit = G.fitness(pairs[i][0], pairs[i][1], w["T"], DBL_MAX)
        print(seed, G.STATES[state[i]], its[i], dt, dr, fit[i], wfit)
        assert (state[i], bool(conv[i]), its[i]) == (w["state"], w["converged"], w["iterations"]), (seed, state[i], its[i], w["state"], w["iterations"])
        assert dt < TOL_T and dr < TOL_R, (seed, dt, dr)
        assert abs(fit[i] - wfit) < 1e-5
    assert b.nn_passes == its.max()


def _mixed():
    rng = np.random.default_rng(7)
    p3, p4, p5 = K.pair(3), K.pair(4), K.pair(5)
    blob = rng.normal(size=(800, 3)).astype(np.float32) * np.float32(4)
    srcs = [p3[0], blob, p5[0][:3], p4[0], p5[0]]
    tgts = [p3[1], blob + np.float32(500), p5[1], p4[1], p5[1]]
    guess = np.stack([np.eye(4)] * 5)
    guess[1, :3, 3] = [0.3, -0.2, 0.1]
    guess[1, :3, :3] = Rot.from_rotvec([0, 0, 0.2]).as_matrix()
    guess[3] = K.natural(4)["X"]         # two pairs that start where the restatement stopped: their first step is below the threshold
    guess[4] = K.natural(5)["X"]
    return srcs, tgts, guess


def test_mixed_endings_in_one_batch_equal_the_pairs_run_alone(dev):
    """Five pairs in one batch under a 2 m threshold and a limit of 2: a lidar pair still moving at the limit -> ITERATIONS, a target 500 m
    away and a 3-point source -> NO_CORRESPONDENCES (pose = guess narrowed), and two lidar pairs that start at their solution -> TRANSFORM
    after one iteration.  Every pair's result equals the pair run alone, bit for bit."""
    srcs, tgts, guess = _mixed()
    prm = dict(K.MAPPING_2422, max_correspondence_distance=2.0, max_iterations=2)
    b = _batch(srcs, tgts)
    T, conv, its, state = b.align_pcl(guess, **prm)
    assert list(state) == [G.ITERATIONS, G.NO_CORRESPONDENCES, G.NO_CORRESPONDENCES, G.TRANSFORM, G.TRANSFORM], state
    assert list(its) == [2, 0, 0, 1, 1] and list(conv) == [True, False, False, True, True]
    for i in (1, 2):
        assert np.array_equal(T[i], guess[i].astype(np.float32).astype(np.float64))
    assert np.isfinite(T).all()
    for i in range(5):
        one = _batch(srcs[i:i + 1], tgts[i:i + 1])
        T1, c1, i1, s1 = one.align_pcl(guess[i:i + 1], **prm)
        assert np.array_equal(T1[0], T[i]) and (c1[0], i1[0], s1[0]) == (conv[i], its[i], state[i]), i


def test_degenerate_geometry(dev):
    """A planar cloud against its copy rotated by 3 degrees about z: finite pose, a proper rotation, at least one iteration."""
    src, tgt = K.planar()
    b = _batch([src], [tgt])
    T, conv, its, state = b.align_pcl(max_iterations=30)
    assert np.isfinite(T).all() and its[0] >= 1
    assert abs(np.linalg.det(T[0, :3, :3]) - 1) < 1e-5 and np.abs(T[0, :3, :3] @ T[0, :3, :3].T - np.eye(3)).max() < 1e-5
    assert np.array_equal(T[0, 3], [0, 0, 0, 1])


def _with_env(env, fn):
    old = {k: os.environ.get(k) for k in ("MRS_DEV", "MRS_GICP_WINDOW")}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_same_bits_from_call_to_call_and_across_schedules(dev):
    """The same arguments give the same bits: a repeated call, the windowed and the per-tick schedule (MRS_GICP_WINDOW=0; a batch of 9 is beyond
    the windowed schedule's 8 pairs), search settings 0, 1 and 3, fresh handles."""
    nine = [K.build(50 + i, 2500 + 301 * i, (0.01 * (i % 3), -0.02, 0.03 + 0.01 * i), (0.3 + 0.05 * i, -0.2, 0.05)) for i in range(9)]
    per_tick = {"MRS_DEV": "1", "MRS_GICP_WINDOW": "0"}
    for pairs in (nine[:1], nine):
        srcs, tgts = [p[0] for p in pairs], [p[1] for p in pairs]
        for prm in (K.MAPPING_2422, dict(force_iterations=5, max_correspondence_distance=5.0)):
            b = _batch(srcs, tgts)
            want = b.align_pcl(**prm)
            assert _same(b.align_pcl(**prm), want)                                               # warm seeds and covariances, same handle
            assert _same(_batch(srcs, tgts).align_pcl(**prm), want)
            assert _same(_with_env(per_tick, lambda: _batch(srcs, tgts).align_pcl(**prm)), want)
            assert _same(_with_env({"MRS_DEV": "1", "MRS_GICP_WINDOW": "3"}, lambda: _batch(srcs, tgts).align_pcl(**prm)), want)
            assert _same(_batch(srcs, tgts, search=3).align_pcl(**prm), want)
            assert _same(_batch(srcs, tgts, search=0).align_pcl(**prm), want)
        assert want[2].min() == 5


def test_error_return_inside_align_pcl_leaves_handle_and_side_slot_usable(dev):
    """The twin of tests/test_gicp_gpu.py's test: search setting 3 chosen after the clouds were set under the default one (the sources have no
    hierarchy), so align_pcl raises after it has handed the target covariances to the borrowed side stream.  The same handle, set back to
    the default search, and a second fresh handle that borrows the returned slot in the same thread both equal a fresh default handle bit for
    bit."""
    from mr_slam_amd import _lib
    src, tgt, _ = K.build(50, 2500, (0.0, -0.02, 0.03), (0.3, -0.2, 0.05))
    want = _batch([src], [tgt]).align_pcl(**K.MAPPING_2422)
    b = _batch([src], [tgt])
    b.set_search(3)
    with pytest.raises(_lib.MrsError):
        b.align_pcl(**K.MAPPING_2422)
    b.set_search(1)
    assert _same(b.align_pcl(**K.MAPPING_2422), want)
    assert _same(_batch([src], [tgt]).align_pcl(**K.MAPPING_2422), want)


def test_three_methods_share_a_handle(dev):
    """align -> align_pcl -> align_icp -> align_pcl -> align on one handle equals fresh handles bit for bit; align_pcl leaves the covariances of
    compute_covariances behind and the handle's own correspondence distance alone."""
    pairs = [K.build(61, 4000), K.build(62, 3001)]
    srcs, tgts = [p[0] for p in pairs], [p[1] for p in pairs]
    icp = dict(G.I.MAPPING_890)

    def gicp_of(b):
        b.set_params(max_correspondence_distance=5.0)
        T, conv, its = b.align()
        return T, conv, its, b.hessian.copy()
    want_g = gicp_of(_batch(srcs, tgts))
    want_i = _batch(srcs, tgts).align_icp(**icp)
    fresh = _batch(srcs, tgts)
    want_p = fresh.align_pcl(**K.MAPPING_2422)
    ref = _batch(srcs, tgts)
    ref.compute_covariances(0); ref.compute_covariances(1)
    for which in (0, 1):
        assert np.array_equal(fresh.covariances(which), ref.covariances(which))
    b = _batch(srcs, tgts)
    assert _same(gicp_of(b), want_g)
    assert _same(b.align_pcl(**K.MAPPING_2422), want_p)
    assert _same(b.align_icp(**icp), want_i)
    assert _same(b.align_pcl(**K.MAPPING_2422), want_p)
    assert _same(gicp_of(b), want_g)
    assert b.params.max_correspondence_distance == 5.0   # the call's own threshold (100) did not replace the handle's
    e1 = b.linearize(np.stack([p[2] for p in pairs]))[0]
    e2 = _batch(srcs, tgts)
    e2.set_params(max_correspondence_distance=5.0)
    assert np.array_equal(e1, e2.linearize(np.stack([p[2] for p in pairs]))[0])
    assert want_p[1].all() and (want_p[3] == G.TRANSFORM).all()


def test_clouds_from_a_store_and_bad_arguments(dev):
    """set_clouds_from works like set_clouds (the pivot comes with the copied bounding box); parameter checks arrive as MrsError."""
    from mr_slam_amd import _lib, gicp
    pairs = [K.build(71, 3000), K.build(72, 2000)]
    store = gicp.GicpBatch(2)
    store.set_targets([p[1] for p in pairs])
    b = gicp.GicpBatch(2)
    b.set_sources([p[0] for p in pairs])
    b.set_targets_from(store, [1, 0])
    want = _batch([p[0] for p in pairs], [pairs[1][1], pairs[0][1]]).align_pcl(**K.MAPPING_2422)
    assert _same(b.align_pcl(**K.MAPPING_2422), want)
    for bad in (dict(max_iterations=0), dict(max_inner_iterations=0), dict(force_iterations=-1), dict(max_correspondence_distance=-1.0),
                dict(rotation_epsilon=0.0), dict(transformation_epsilon=0.0), dict(gradient_tolerance=0.0)):
        with pytest.raises(_lib.MrsError):
            b.align_pcl(**bad)
    with pytest.raises(_lib.MrsError):
        gicp.GicpBatch(1).align_pcl()               # no clouds set
    with pytest.raises(_lib.MrsError):
        gicp.GicpBatch(1).pcl_step(np.eye(4)[None])
    with pytest.raises(AttributeError):
        b.align_pcl(euclidean_fitness_epsilon=1e-3)
    with pytest.raises(AttributeError):
        b.pcl_step(np.stack([np.eye(4)] * 2), k_correspondences=15)
