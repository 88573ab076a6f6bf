"""GPU suite for the batched point-to-point ICP (row G9): HIP through the C ABI against the NumPy restatement
(tests/golden/icp_restate.py) on the same clouds.  Pose tolerance from BASELINE.json north_star: 1e-4 m / 1e-4 rad.  The natural-stopping
fixtures are those whose margins tests/test_icp_cpu.py checks."""
import os

import numpy as np
import pytest
from scipy.spatial.transform import Rotation as Rot

import icp_cases as K

R = K.R
pytestmark = pytest.mark.gpu

TOL_T = 1e-4   # metres
TOL_R = 1e-4   # radians
DBL_MAX = R.DBL_MAX


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    from mr_slam_amd import _lib
    _lib.load()
    return "cuda:0"


_pair = K.build


def _batch(srcs, tgts, search=None):
    from mr_slam_amd import gicp
    b = gicp.GicpBatch(len(srcs))
    if search is not None:
        b.set_search(search)
    b.set_sources(srcs); b.set_targets(tgts)
    return b


def _close_blocks(got, want, tol):
    """the 17 sums block by block (count, sum a, sum b, sum a b^T, sum |b - a|^2): absolute error below tol x the block's largest entry"""
    for lo, hi in ((0, 1), (1, 4), (4, 7), (7, 16), (16, 17)):
        assert np.abs(got[lo:hi] - want[lo:hi]).max() <= tol * np.abs(want[lo:hi]).max(), (lo, got[lo:hi], want[lo:hi])


def _check_step(oracle, src, tgt, T, max_corr, sums, delta, corr, always_tight=True):
    wcorr, _, wsums, wdelta = R.step(src, tgt, T, max_corr)
    # exact search: different indices only where the two candidates are at exactly the same float distance
    assert np.array_equal(oracle.pair_d2(src, T, tgt, corr), oracle.pair_d2(src, T, tgt, wcorr))
    assert np.array_equal(corr >= 0, wcorr >= 0)
    assert (corr == wcorr).mean() > 0.999
    assert (wcorr >= 0).sum() > 100
    tol = 1e-9 if (corr == wcorr).all() else 2e-3
    _close_blocks(sums, wsums, tol)
    assert np.abs(delta - wdelta).max() <= tol
    if always_tight:
        # an exact tie may resolve either way: the restatement fed with the kernel's (equally nearest) neighbours must agree to rounding
        s2, a, b = R.sums17(src, tgt, np.asarray(T, np.float64), corr.astype(np.int64))
        _close_blocks(sums, s2, 1e-9)
        assert np.abs(delta - R.rigid_fit(a, b)).max() <= 1e-9
    return wsums


def test_icp_step_matches_restatement(dev, oracle):
    """9000 points: more than one block of 1024; 1031: one block and 7 points, a ragged last wave.  Both thresholds."""
    big, small = _pair(2, 9000), _pair(12, 1031)
    poses = []
    for _, _, Ttrue in (big, small):
        T = Ttrue.copy(); T[:3, 3] += [0.25, -0.1, 0.05]
        poses.append(T)
    b = _batch([big[0], small[0]], [big[1], small[1]])
    for max_corr in (5.0, 0.5):
        sums, delta, corr = b.icp_step(np.stack(poses), want_corr=True, max_correspondence_distance=max_corr)
        for i, (src, tgt, _) in enumerate((big, small)):
            lo = 0 if i == 0 else big[0].shape[0]
            _check_step(oracle, src, tgt, poses[i], max_corr, sums[i], delta[i], corr[lo:lo + src.shape[0]])
    # a threshold that does reject: the kept masks and the sums of the rest still agree
    sums, delta, corr = b.icp_step(np.stack(poses), want_corr=True, max_correspondence_distance=0.27)
    assert 100 < sums[0, 0] < big[0].shape[0] and (corr[:big[0].shape[0]] < 0).any()
    _check_step(oracle, big[0], big[1], poses[0], 0.27, sums[0], delta[0], corr[:big[0].shape[0]])


def test_icp_step_far_from_the_origin(dev, oracle):
    """Cancellation: both clouds shifted by (+55, -48, 3) m -- sum a b^T - n abar bbar^T loses digits, the increment must not."""
    src, tgt, Ttrue = _pair(2, 9000)
    shift = np.array([55.0, -48.0, 3.0])
    src = (src.astype(np.float64) + shift).astype(np.float32)
    tgt = (tgt.astype(np.float64) + shift).astype(np.float32)
    T = Ttrue.copy()
    T[:3, 3] += shift - Ttrue[:3, :3] @ shift + [0.25, -0.1, 0.05]
    b = _batch([src], [tgt])
    sums, delta, corr = b.icp_step(T[None], want_corr=True, max_correspondence_distance=5.0)
    wcorr, _, _, wdelta = R.step(src, tgt, T, 5.0)
    assert np.array_equal(oracle.pair_d2(src, T, tgt, corr), oracle.pair_d2(src, T, tgt, wcorr))
    assert np.array_equal(corr >= 0, wcorr >= 0) and (corr == wcorr).mean() > 0.999       # only exact ties may differ
    s2, a, bb = R.sums17(src, tgt, T, corr.astype(np.int64))
    assert np.abs(delta[0] - R.rigid_fit(a, bb)).max() <= 1e-9
    if (corr == wcorr).all():
        assert np.abs(delta[0] - wdelta).max() <= 1e-9
    assert np.abs(delta[0, :3, 3]).max() > 0.01         # a real step


def test_forced_iterations_on_the_ragged_batch(dev):
    """force_iterations = 8 on the three pairs of test_align_batch_within_north_star_tolerance: fixed-length parity with the restatement."""
    pairs = [K.pair(s) for s in (3, 4, 5)]
    b = _batch([p[0] for p in pairs], [p[1] for p in pairs])
    guess = np.stack([np.eye(4)] * 3)
    guess[1, :3, 3] = [-0.5, 0.2, 0.0]
    T, conv, its, state = b.align_icp(guess, force_iterations=8, max_correspondence_distance=5.0)
    assert (its == 8).all() and not conv.any() and (state == R.NOT_CONVERGED).all()
    assert b.nn_passes == 8
    for i, (src, tgt, _) in enumerate(pairs):
        w = R.icp(src, tgt, guess[i], force_iterations=8, max_correspondence_distance=5.0)
        dt, dr = K.pose_err(T[i], w["T"])
        print("forced", i, dt, dr)
        assert dt < TOL_T and dr < TOL_R, (i, dt, dr)


@pytest.mark.parametrize("name", sorted(K.SETTINGS))
def test_natural_stopping_matches_restatement(dev, name):
    """global_manager.cpp:890-906's settings, and settings under which the relative change of the error decides: the same state, converged
    flag and iteration count as the restatement, poses within the tolerance, getFitnessScore within 1e-5."""
    seeds = [s for n, s in K.NATURAL if n == name]
    pairs = [K.pair(s) for s in seeds]
    b = _batch([p[0] for p in pairs], [p[1] for p in pairs])
    T, conv, its, state = b.align_icp(**K.SETTINGS[name])
    fit = b.fitness(T, DBL_MAX)
    for i, seed in enumerate(seeds):
        w = K.natural(name, seed)
        dt, dr = K.pose_err(T[i], w["T"])
        wfit = R.fitness(pairs[i][0], pairs[i][1], w["T"], DBL_MAX)
        print(name, seed, R.STATES[state[i]], its[i], dt, dr, fit[i], wfit)
        assert (state[i], bool(conv[i]), its[i]) == (w["state"], w["converged"], w["iterations"]), (seed, state[i], its[i], w["state"], w["iterations"])
        assert dt < TOL_T and dr < TOL_R, (seed, dt, dr)
        assert abs(fit[i] - wfit) < 1e-5
    assert b.nn_passes == its.max()


def _mixed():
    rng = np.random.default_rng(7)
    p3, p4, p5 = K.pair(3), K.pair(4), K.pair(5)
    blob = rng.normal(size=(800, 3)).astype(np.float32) * np.float32(4)
    srcs = [p3[0], blob, p5[0][:2], p4[0], p5[0]]
    tgts = [p3[1], blob + np.float32(500), p5[1], p4[1], p5[1]]
    guess = np.stack([np.eye(4)] * 5)
    guess[1, :3, 3] = [0.3, -0.2, 0.1]
    guess[1, :3, :3] = Rot.from_rotvec([0, 0, 0.2]).as_matrix()
    return srcs, tgts, guess


def test_mixed_endings_in_one_batch_equal_the_pairs_run_alone(dev):
    """Five pairs with mixed endings in one batch: a lidar pair still moving at the iteration limit (8) -> ITERATIONS, a target 500 m away with
    a 2 m threshold and a 2-point source -> NO_CORRESPONDENCES, and two ordinary lidar pairs that end by TRANSFORM after 7 and 3 iterations.
    The parameters hold for a whole call, so the pair that ends by ITERATIONS does so at the call's limit; the batch is run again with a limit
    of 1, where every pair that has correspondences ends at once.  Every pair's result equals the pair run alone, bit for bit."""
    srcs, tgts, guess = _mixed()
    prm = dict(K.MAPPING_890, max_iterations=8)
    b = _batch(srcs, tgts)
    T, conv, its, state = b.align_icp(guess, **prm)
    assert list(state) == [R.ITERATIONS, R.NO_CORRESPONDENCES, R.NO_CORRESPONDENCES, R.TRANSFORM, R.TRANSFORM], state
    assert list(its) == [8, 0, 0, 7, 3] and list(conv) == [True, False, False, True, True]
    for i in (1, 2):                                     # the pose stays the guess (narrowed to float32 like every result)
        assert np.array_equal(T[i], guess[i].astype(np.float32).astype(np.float64))
    assert np.isfinite(T).all()
    for i in range(5):
        one = _batch(srcs[i:i + 1], tgts[i:i + 1])
        T1, c1, i1, s1 = one.align_icp(guess[i:i + 1], **prm)
        assert np.array_equal(T1[0], T[i]) and (c1[0], i1[0], s1[0]) == (conv[i], its[i], state[i]), i
    T, conv, its, state = b.align_icp(guess, **dict(prm, max_iterations=1))
    assert list(state) == [R.ITERATIONS, R.NO_CORRESPONDENCES, R.NO_CORRESPONDENCES, R.ITERATIONS, R.ITERATIONS] and list(its) == [1, 0, 0, 1, 1]
    assert list(conv) == [True, False, False, True, True]


def test_degenerate_geometry(dev):
    """A planar and a collinear source against a point-for-point copy rotated by 3 degrees about z: rank-2 and rank-1 H.  Finite results, a
    proper rotation, and the residual error of the restatement (for a line every rotation about it attains the minimum)."""
    rng = np.random.default_rng(0)
    Rz = Rot.from_rotvec([0, 0, np.deg2rad(3)]).as_matrix()
    plane = np.c_[rng.uniform(-5, 5, (2000, 2)), np.zeros(2000)].astype(np.float32)
    line = (np.linspace(-1, 1, 500)[:, None] * np.array([3.0, 2.0, 1.0]) + [0.5, -0.2, 0.1]).astype(np.float32)
    for name, src in (("plane", plane), ("line", line)):
        tgt = (src.astype(np.float64) @ Rz.T).astype(np.float32)
        b = _batch([src], [tgt])
        sums, delta, corr = b.icp_step(np.eye(4)[None], want_corr=True)
        wcorr, _, wsums, wdelta = R.step(src, tgt, np.eye(4), R.DEFAULTS["max_correspondence_distance"])
        D = delta[0]
        assert np.isfinite(D).all() and abs(np.linalg.det(D[:3, :3]) - 1) < 1e-12, name
        assert np.abs(D[:3, :3] @ D[:3, :3].T - np.eye(3)).max() < 1e-12
        a = src.astype(np.float64); bb = tgt[wcorr].astype(np.float64)
        res = lambda M: (((a @ M[:3, :3].T + M[:3, 3]) - bb) ** 2).sum(1).mean()     # noqa: E731
        print(name, res(D), res(wdelta), (corr == wcorr).mean())
        if (corr == wcorr).all():
            assert abs(res(D) - res(wdelta)) <= 1e-9 * res(wdelta), name
        else:       # ties on a regular pattern: the same comparison on the kernel's own (equally nearest) neighbours
            s2, a2, b2 = R.sums17(src, tgt, np.eye(4), corr.astype(np.int64))
            res2 = lambda M: (((a2 @ M[:3, :3].T + M[:3, 3]) - b2) ** 2).sum(1).mean()     # noqa: E731
            assert abs(res2(D) - res2(R.rigid_fit(a2, b2))) <= 1e-9 * res2(R.rigid_fit(a2, b2)), name
        T, conv, its, state = b.align_icp(max_iterations=30)
        assert np.isfinite(T).all() and abs(np.linalg.det(T[0, :3, :3]) - 1) < 1e-5 and its[0] >= 1, name


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
    the windowed schedule's 8 pairs), search settings 1 and 3, fresh handles."""
    nine = [_pair(50 + i, 2500 + 301 * i, (0.01 * (i % 3), -0.02, 0.03 + 0.01 * i), (0.3 + 0.05 * i, -0.2, 0.05)) for i in range(9)]
    per_tick = {"MRS_DEV": "1", "MRS_GICP_WINDOW": "0"}
    for pairs in (nine[:1], nine):
        srcs, tgts = [p[0] for p in pairs], [p[1] for p in pairs]
        for prm in (K.MAPPING_890, dict(force_iterations=6, max_correspondence_distance=5.0)):
            b = _batch(srcs, tgts)
            want = b.align_icp(**prm)
            assert _same(b.align_icp(**prm), want)                                               # warm seeds, same handle
            assert _same(_with_env(per_tick, lambda: _batch(srcs, tgts).align_icp(**prm)), want)
            assert _same(_with_env({"MRS_DEV": "1", "MRS_GICP_WINDOW": "3"}, lambda: _batch(srcs, tgts).align_icp(**prm)), want)
            assert _same(_batch(srcs, tgts, search=3).align_icp(**prm), want)
            assert _same(_batch(srcs, tgts, search=0).align_icp(**prm), want)
        assert want[2].min() == 6


def test_gicp_and_icp_share_a_handle(dev):
    """GICP -> ICP -> GICP and ICP -> GICP -> ICP on one handle equal fresh handles bit for bit, and ICP computes no covariances."""
    from mr_slam_amd import _lib
    pairs = [_pair(61, 4000), _pair(62, 3001)]
    srcs, tgts = [p[0] for p in pairs], [p[1] for p in pairs]
    prm = K.MAPPING_890

    def gicp_of(b):
        b.set_params(max_correspondence_distance=5.0)
        T, conv, its = b.align()
        return T, conv, its, b.hessian.copy()
    want_g = gicp_of(_batch(srcs, tgts))
    fresh = _batch(srcs, tgts)
    want_i = fresh.align_icp(**prm)
    for which in (0, 1):                                 # side[*].cov_valid stays false: the accessor refuses
        with pytest.raises(_lib.MrsError, match="covariances not computed"):
            fresh.covariances(which)
    b = _batch(srcs, tgts)
    assert _same(gicp_of(b), want_g)
    assert _same(b.align_icp(**prm), want_i)
    assert _same(gicp_of(b), want_g)
    b = _batch(srcs, tgts)
    assert _same(b.align_icp(**prm), want_i)
    assert _same(gicp_of(b), want_g)
    assert _same(b.align_icp(**prm), want_i)
    assert b.params.max_correspondence_distance == 5.0   # ICP's own threshold did not replace GICP's
    e1 = b.linearize(np.stack([p[2] for p in pairs]))[0]
    e2 = _batch(srcs, tgts)
    e2.set_params(max_correspondence_distance=5.0)
    assert np.array_equal(e1, e2.linearize(np.stack([p[2] for p in pairs]))[0])


def test_clouds_from_a_store_and_bad_arguments(dev):
    """set_clouds_from works for ICP like set_clouds; parameter checks arrive as MrsError."""
    from mr_slam_amd import _lib, gicp
    pairs = [_pair(71, 3000), _pair(72, 2000)]
    store = gicp.GicpBatch(2)
    store.set_targets([p[1] for p in pairs])
    b = gicp.GicpBatch(2)
    b.set_sources([p[0] for p in pairs])
    b.set_targets_from(store, [0, 1])
    want = _batch([p[0] for p in pairs], [p[1] for p in pairs]).align_icp(**K.MAPPING_890)
    assert _same(b.align_icp(**K.MAPPING_890), want)
    with pytest.raises(_lib.MrsError):
        b.align_icp(max_iterations=0)
    with pytest.raises(_lib.MrsError):
        b.align_icp(max_correspondence_distance=-1.0)
    with pytest.raises(_lib.MrsError):
        gicp.GicpBatch(1).align_icp()               # no clouds set
    with pytest.raises(AttributeError):
        b.align_icp(k_correspondences=15)
