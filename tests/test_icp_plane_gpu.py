"""GPU suite for the batched point-to-plane ICP and its surface normals (row G12): HIP through the C ABI against the NumPy
restatement (tests/golden/icp_plane_restate.py) on the same clouds.  Pose tolerance from BASELINE.json north_star: 1e-4 m / 1e-4 rad.
The fixtures are those whose conditions tests/test_icp_plane_cpu.py checks."""
import os

import numpy as np
import pytest

import icp_plane_cases as PK

K = PK.K
R, PR = PK.R, PK.PR
pytestmark = pytest.mark.gpu

TOL_T = 1e-4   # metres
TOL_R = 1e-4   # radians
DBL_MAX = R.DBL_MAX
EPS64 = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    from mr_slam_amd import _lib
    _lib.load()
    return "cuda:0"


def _batch(srcs, tgts, search=None):
    from mr_slam_amd import gicp
    b = gicp.GicpBatch(len(tgts))
    if search is not None:
        b.set_search(search)
    if srcs is not None:
        b.set_sources(srcs)
    b.set_targets(tgts)
    return b


def _same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


# ---- 5: normals ----------------------------------------------------------------------------------------------------------------------------
CLOUDS = ("scan", "ten", "two", "plane")
PLANE_NORMAL = np.array([0.5, -0.25, -1.0]) / np.linalg.norm([0.5, -0.25, -1.0])


def _check_normals(name, got, w, vp):
    """one cloud's normals against the restatement's (both in input order)"""
    want = w["normals"].astype(np.float64)
    if name == "two":
        assert np.isnan(got).all()
        return
    assert np.isfinite(got).all()
    assert np.abs(np.linalg.norm(got[:, :3].astype(np.float64), axis=1) - 1).max() < 2e-7
    lam = w["lam"]
    with np.errstate(divide="ignore"):
        tol = np.maximum(2e-7, 256 * EPS64 * lam[:, 2] / (lam[:, 1] - lam[:, 0]))
    loose = PK.unreliable(w)                  # direction or orientation within rounding: up to sign, or not at all
    sure = ~loose & ~w["tie"]                 # a tie at the k-th place: the kernel may hold another (equally near) neighbour
    d = np.abs(got[:, :3] - want[:, :3])
    print(name, "compared", sure.sum(), "of", len(sure), "largest direction error", d[sure].max(), "curvature", np.abs(got[:, 3] - want[:, 3])[sure].max())
    assert sure.mean() > (0.6 if name == "plane" else 0.98)
    assert (d[sure].max(1) <= tol[sure]).all(), (d[sure].max(1) / tol[sure]).max()
    gap_ok = ~w["tie"] & (tol < 1e-3)
    flipped = np.minimum(d, np.abs(got[:, :3] + want[:, :3]))
    assert (flipped[gap_ok].max(1) <= tol[gap_ok]).all()
    curv_tol = 4 * PK.EIG3_CURVATURE_DEV + 0.5 * np.spacing(np.abs(want[:, 3]).astype(np.float32)).astype(np.float64)
    assert (np.abs(got[:, 3] - want[:, 3])[~w["tie"]] <= curv_tol[~w["tie"]]).all(), (np.abs(got[:, 3] - want[:, 3]) / curv_tol)[~w["tie"]].max()
    P = PK.normal_clouds()[name].astype(np.float64)
    toward = (got[:, :3] * (np.asarray(vp) - P)).sum(1)
    assert (toward[~loose] > 0).all()         # step 4 of contract A, whichever neighbours a tie chose
    if name == "plane":                       # whichever neighbours a tie chose, they lie in the plane: its normal, unless they are collinear
        off = np.abs(np.abs(got[:, :3] @ PLANE_NORMAL) - 1)
        assert off[sure].max() < 2e-7 and (off < 2e-7).mean() > 0.99 and np.abs(got[:, 3]).max() <= 4 * PK.EIG3_CURVATURE_DEV


@pytest.mark.parametrize("k", PK.NORMAL_K)
def test_normals_match_restatement(dev, k):
    """A ragged batch of four clouds (a scan, 10 points: fewer than k, 2 points: no normal, an exact plane), both viewpoints; the same bits
    from call to call, for the scan alone and for the other side of the handle; get_normals is in input order (so is the restatement)."""
    clouds = PK.normal_clouds()
    b = _batch(None, [clouds[n] for n in CLOUDS])
    offs = np.cumsum([0] + [clouds[n].shape[0] for n in CLOUDS])
    first = None
    for vp in PK.VIEWPOINTS:
        b.compute_normals(1, k, vp)
        got = b.normals(1)
        assert got.shape == (offs[-1], 4) and got.dtype == np.float32
        for i, name in enumerate(CLOUDS):
            _check_normals(name, got[offs[i]:offs[i + 1]], PK.cloud_normals(name, k, vp), vp)
        b.compute_normals(1, k, vp)                                     # cached: nothing runs, nothing changes
        assert np.array_equal(b.normals(1), got, equal_nan=True)
        first = got if first is None else first
    a, c = first[:offs[1]], got[:offs[1]]                              # the scan: (5, -3, 2) turns some of its normals, and only turns them
    flipped = (a[:, :3] != c[:, :3]).any(1)
    assert 0 < flipped.mean() < 1 and np.array_equal(a[flipped, :3], -c[flipped, :3]) and np.array_equal(a[:, 3], c[:, 3])
    b.compute_normals(1, 15 if k != 15 else 7, PK.VIEWPOINTS[1])        # another k in between, then the first request again
    b.compute_normals(1, k, PK.VIEWPOINTS[0])
    assert np.array_equal(b.normals(1), first, equal_nan=True)
    from mr_slam_amd import gicp
    one = gicp.GicpBatch(1)
    one.set_sources([clouds["scan"]])
    one.compute_normals(0, k)
    assert np.array_equal(one.normals(0), first[:offs[1]])


def test_a_cloud_without_points_is_refused(dev):
    """set_clouds has always refused an empty cloud (every cloud needs a point): a status, no fault, and no normals to ask for"""
    from mr_slam_amd import _lib, gicp
    b = gicp.GicpBatch(2)
    with pytest.raises(_lib.MrsError):
        b.set_targets([PK.normal_clouds()["ten"], np.zeros((0, 3), np.float32)])
    with pytest.raises(_lib.MrsError, match="set_clouds first"):
        b.compute_normals(1)


def test_neighbour_lists_hold_the_query_point(dev):
    """contract A step 1: the selection's list contains the point itself (checked on the lists the covariance front end hands out)"""
    clouds = PK.normal_clouds()
    b = _batch(None, [clouds["scan"], clouds["plane"]])
    b.set_params(k_correspondences=15)
    knn = b.compute_covariances(1, want_knn=True).cpu().numpy()
    n0 = clouds["scan"].shape[0]
    own = np.concatenate([np.arange(n0), np.arange(clouds["plane"].shape[0])])
    assert (knn == own[:, None]).any(1).all()


# ---- 6: one iteration -----------------------------------------------------------------------------------------------------------------------
BLOCKS = ((0, 1), (1, 22), (22, 28), (28, 29))


def _close_blocks(got, want, tol):
    """the 29 sums block by block (count, sum a a^T, sum a r, sum |d - s|^2): absolute error below tol x the block's largest entry"""
    for lo, hi in BLOCKS:
        assert np.abs(got[lo:hi] - want[lo:hi]).max() <= tol * np.abs(want[lo:hi]).max(), (lo, got[lo:hi], want[lo:hi])


def _check_step(oracle, src, tgt, N, T, max_corr, sums, delta, state, corr):
    wcorr, _, wsums, wdelta, wstate = PR.step(src, tgt, N, T, max_corr)
    # exact search: different indices only where the two candidates are at exactly the same float distance
    assert np.array_equal(oracle.pair_d2(src, T, tgt, corr), oracle.pair_d2(src, T, tgt, wcorr))
    assert np.array_equal(corr >= 0, wcorr >= 0)
    assert (corr == wcorr).mean() > 0.999
    assert (wcorr >= 0).sum() > 100 and wstate == R.NOT_CONVERGED and state in (R.ITERATIONS, R.TRANSFORM)
    tol = 1e-9 if (corr == wcorr).all() else 2e-3
    _close_blocks(sums, wsums, tol)
    print("step: equal correspondences", (corr == wcorr).all(), "largest delta error", np.abs(delta - wdelta).max())
    assert np.abs(delta - wdelta).max() <= tol
    # an exact tie may resolve either way: the restatement fed with the kernel's (equally nearest) neighbours must agree to rounding
    s2 = PR.sums29(src, tgt, N, np.asarray(T, np.float64), corr.astype(np.int64))
    _close_blocks(sums, s2, 1e-9)
    assert np.abs(delta - PR.fit(s2)[0]).max() <= 1e-9


def _step_batch():
    big, small = K.build(2, 9000), K.build(12, 1031)        # more than one block of 1024; one block and 7 points, a ragged last wave
    return big, small


def test_icp_plane_step_matches_restatement(dev, oracle):
    """The ragged batch at the identity and at poses near the truth, both thresholds and one that rejects.  The restatement takes the
    normals the handle holds (test_normals_match_restatement compares those): float32 values, the same on both sides."""
    big, small = _step_batch()
    b = _batch([big[0], small[0]], [big[1], small[1]])
    near = []
    for _, _, Ttrue in (big, small):
        T = Ttrue.copy(); T[:3, 3] += [0.25, -0.1, 0.05]
        near.append(T)
    n0 = big[0].shape[0]
    N = None
    for poses, max_corr in (([np.eye(4)] * 2, 5.0), (near, 5.0), (near, 0.5), (near, 0.27)):
        sums, delta, state, corr = b.icp_plane_step(np.stack(poses), want_corr=True, max_correspondence_distance=max_corr)
        if N is None:
            N = b.normals(1)                                # computed by the first call (k = 15, viewpoint at the origin)
        for i, (src, tgt, _) in enumerate((big, small)):
            if max_corr == 0.27 and i == 1:
                continue
            lo = 0 if i == 0 else n0
            Ni = N[:n0] if i == 0 else N[n0:]
            _check_step(oracle, src, tgt, Ni, poses[i], max_corr, sums[i], delta[i], state[i], corr[lo:lo + src.shape[0]])
    assert 100 < sums[0, 0] < n0 and (corr[:n0] < 0).any()           # 0.27 m does reject


def test_icp_plane_step_far_from_the_origin(dev, oracle):
    """Both clouds shifted by 500 m along x and y: the rotational and translational columns of the system are nearly dependent there, the
    scaled Cholesky must not lose the increment."""
    src, tgt, Ttrue = K.build(2, 9000)
    shift = np.array([500.0, -500.0, 3.0])
    src = (src.astype(np.float64) + shift).astype(np.float32)
    tgt = (tgt.astype(np.float64) + shift).astype(np.float32)
    T = Ttrue.copy()
    T[:3, 3] += shift - Ttrue[:3, :3] @ shift + [0.25, -0.1, 0.05]
    b = _batch([src], [tgt])
    sums, delta, state, corr = b.icp_plane_step(T[None], want_corr=True, max_correspondence_distance=5.0)
    _check_step(oracle, src, tgt, b.normals(1), T, 5.0, sums[0], delta[0], state[0], corr)
    assert np.abs(delta[0, :3, 3]).max() > 0.01          # a real step


# ---- 7, 8: whole alignments -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(PK.SETTINGS))
def test_natural_stopping_matches_restatement(dev, name):
    """The same state, converged flag and iteration count as the restatement, poses within the tolerance, getFitnessScore within 1e-5."""
    seeds = [s for n, s in PK.NATURAL if n == name]
    pairs = [PK.pair(s) for s in seeds]
    b = _batch([p[0] for p in pairs], [p[1] for p in pairs])
    T, conv, its, state = b.align_icp_plane(**PK.SETTINGS[name])
    fit = b.fitness(T, DBL_MAX)
    for i, seed in enumerate(seeds):
        w = PK.natural(name, seed)
        dt, dr = PK.pose_err(T[i], w["T"])
        wfit = R.fitness(pairs[i][0], pairs[i][1], w["T"], DBL_MAX)
        print(name, seed, PR.STATES[state[i]], its[i], dt, dr, fit[i], wfit)
        assert (state[i], bool(conv[i]), its[i]) == (w["state"], w["converged"], w["iterations"]), (seed, state[i], its[i], w["state"], w["iterations"])
        assert dt < TOL_T and dr < TOL_R, (seed, dt, dr)
        assert abs(fit[i] - wfit) < 1e-5
    assert b.nn_passes == its.max()


def test_forced_iterations_on_the_ragged_batch(dev):
    """force_iterations = 8 on the three pairs of tests/test_icp_gpu.py's forced run: fixed-length parity with the restatement."""
    pairs = [PK.pair(s) for s in (3, 4, 5)]
    b = _batch([p[0] for p in pairs], [p[1] for p in pairs])
    guess = np.stack([np.eye(4)] * 3)
    guess[1, :3, 3] = [-0.5, 0.2, 0.0]
    T, conv, its, state = b.align_icp_plane(guess, force_iterations=8, max_correspondence_distance=5.0)
    assert (its == 8).all() and not conv.any() and (state == R.NOT_CONVERGED).all()
    assert b.nn_passes == 8
    for i, seed in enumerate((3, 4, 5)):
        src, tgt, _ = pairs[i]
        w = PR.icp(src, tgt, PK.target_normals(seed)["normals"], guess[i], force_iterations=8, max_correspondence_distance=5.0)
        dt, dr = PK.pose_err(T[i], w["T"])
        print("forced", i, dt, dr)
        assert dt < TOL_T and dr < TOL_R, (i, dt, dr)


# ---- 9: mixed endings -------------------------------------------------------------------------------------------------------------------------
def _mixed():
    rng = np.random.default_rng(7)
    p3, p5 = PK.pair(3), PK.pair(5)
    flat = np.c_[rng.uniform(-5, 5, (2000, 2)), np.zeros(2000)].astype(np.float32)
    srcs = [p5[0], p3[0], p5[0][:2], flat + np.float32(0.01)]
    tgts = [p5[1], p3[1], p5[1], flat]
    return srcs, tgts


def test_mixed_endings_in_one_batch_equal_the_pairs_run_alone(dev):
    """Four pairs under global_manager.cpp:890's settings with a limit of 3 iterations: a pair that ends by TRANSFORM after 2, one that is
    still moving at the limit (ITERATIONS), a 2-point source (NO_CORRESPONDENCES) and a flat target whose given normals are all (0, 0, 1)
    (DEGENERATE: rotation about z and translation in the plane are free).  The normals are handed over with set_normals -- the computed
    ones read back, the flat target's replaced -- so that the pairs run alone see the same values."""
    srcs, tgts = _mixed()
    prm = dict(PK.SETTINGS["MAPPING_890"], max_iterations=3)
    b = _batch(srcs, tgts)
    b.compute_normals(1)
    N = b.normals(1)
    offs = np.cumsum([0] + [t.shape[0] for t in tgts])
    N[offs[3]:] = [0.0, 0.0, 1.0, 0.0]
    b.set_normals(1, N)
    assert np.array_equal(b.normals(1), N)
    guess = np.stack([np.eye(4)] * 4)
    guess[3, :3, 3] = [0.1, -0.2, 0.05]
    T, conv, its, state = b.align_icp_plane(guess, **prm)
    assert list(state) == [R.TRANSFORM, R.ITERATIONS, R.NO_CORRESPONDENCES, PR.DEGENERATE], state
    assert list(its) == [2, 3, 0, 0] and list(conv) == [True, True, False, False]
    for i in (2, 3):                                     # the pose stays the guess (narrowed to float32 like every result)
        assert np.array_equal(T[i], guess[i].astype(np.float32).astype(np.float64))
    assert np.isfinite(T).all()
    sums, delta, st, _ = b.icp_plane_step(guess)
    assert np.isfinite(sums).all() and np.isfinite(delta).all() and list(st[2:]) == [R.NO_CORRESPONDENCES, PR.DEGENERATE]
    assert np.array_equal(delta[2], np.eye(4)) and np.array_equal(delta[3], np.eye(4)) and sums[3, 0] == 2000 and sums[2, 0] == 2
    for i in range(4):
        one = _batch(srcs[i:i + 1], tgts[i:i + 1])
        one.set_normals(1, N[offs[i]:offs[i + 1]])
        T1, c1, i1, s1 = one.align_icp_plane(guess[i:i + 1], **prm)
        assert np.array_equal(T1[0], T[i]) and (c1[0], i1[0], s1[0]) == (conv[i], its[i], state[i]), i


# ---- 10, 11, 12 ---------------------------------------------------------------------------------------------------------------------------------
def test_given_normals_equal_computed_normals(dev):
    """set_normals with the read-back normals (host array, device tensor, PointXYZINormal's stride) gives the bits of the lazy path; another
    k does not; setting a side's clouds again drops its normals."""
    import torch
    from mr_slam_amd import _lib
    pairs = [PK.pair(6), PK.pair(103)]
    srcs, tgts = [p[0] for p in pairs], [p[1] for p in pairs]
    prm = PK.SETTINGS["MAPPING_890"]
    lazy = _batch(srcs, tgts)
    with pytest.raises(_lib.MrsError, match="normals neither computed nor given"):
        lazy.normals(1)
    want = lazy.align_icp_plane(**prm)
    N = lazy.normals(1)
    assert np.isfinite(N).all()
    with pytest.raises(_lib.MrsError, match="normals neither computed nor given"):
        lazy.normals(0)                                  # source normals are never used, so never computed
    wide = np.zeros((N.shape[0], 12), np.float32)        # normal_x .. of a PointXYZINormal: 12 floats per point
    wide[:, :3] = N[:, :3]
    for given in (N, N[:, :3].copy(), torch.from_numpy(N).to(dev), wide):
        b = _batch(srcs, tgts)
        b.set_normals(1, given)
        assert np.array_equal(b.normals(1)[:, :3], N[:, :3])
        assert _same(b.align_icp_plane(**prm), want)
        assert _same(b.align_icp_plane(**dict(prm, normal_k=5)), want)      # the normals at hand are used, whatever normal_k says
    assert _same(lazy.align_icp_plane(**prm), want)
    other = _batch(srcs, tgts)
    other.compute_normals(1, 5)
    assert not np.array_equal(other.normals(1), N)
    lazy.set_targets(tgts)                               # the same clouds again: the normals went with the old ones
    with pytest.raises(_lib.MrsError, match="normals neither computed nor given"):
        lazy.normals(1)
    assert _same(lazy.align_icp_plane(**prm), want)


def _nine():
    """nine pairs of unequal size (2 500 to 4 908 points): one more than the windowed schedule takes"""
    return [K.build(50 + i, 2500 + 301 * i, (0.01 * (i % 3), -0.02, 0.03 + 0.01 * i), (0.3 + 0.05 * i, -0.2, 0.05)) for i in range(9)]


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


def test_same_bits_from_call_to_call_and_across_schedules(dev):
    """The twin of tests/test_icp_gpu.py's schedule test: one pair (windowed by default) and nine (tick by tick), natural stopping and a forced
    run; the default schedule, the per-tick one (MRS_GICP_WINDOW=0), windows of 3 and a second call on the warm handle give the same pose,
    flag, iteration count, state and number of searches."""
    def run(b, prm):
        return b.align_icp_plane(**prm) + (b.nn_passes,)
    nine = _nine()
    for pairs in (nine[:1], nine):
        srcs, tgts = [p[0] for p in pairs], [p[1] for p in pairs]
        for prm in (PK.SETTINGS["MAPPING_890"], dict(force_iterations=6, max_correspondence_distance=5.0)):
            b = _batch(srcs, tgts)
            want = run(b, prm)
            assert len(want) == 5 and want[4] == want[2].max() >= 1
            assert _same(run(b, prm), want)                                                    # warm seeds and normals, same handle
            for window in ("0", "3"):
                got = _with_env({"MRS_DEV": "1", "MRS_GICP_WINDOW": window}, lambda: run(_batch(srcs, tgts), prm))
                assert _same(got, want), (len(pairs), prm, window)
        assert want[2].min() == 6


def test_four_methods_share_a_handle(dev):
    """align, align_icp, align_pcl and align_icp_plane interleaved on one handle each equal a fresh handle bit for bit, and point-to-plane
    ICP computes no covariances.  Two pairs (the four share the windowed loop) and nine (the per-tick loop)."""
    for pairs in ([K.build(61, 4000), K.build(62, 3001)], _nine()):
        _four_methods_share_a_handle(pairs)


def _four_methods_share_a_handle(pairs):
    from mr_slam_amd import _lib
    srcs, tgts = [p[0] for p in pairs], [p[1] for p in pairs]
    prm = PK.SETTINGS["MAPPING_890"]

    def gicp_of(b):
        b.set_params(max_correspondence_distance=5.0)
        T, conv, its = b.align()
        return T, conv, its, b.hessian.copy()
    calls = {"gicp": gicp_of, "icp": lambda b: b.align_icp(**prm), "pcl": lambda b: b.align_pcl(max_iterations=5, max_correspondence_distance=5.0),
             "plane": lambda b: b.align_icp_plane(**prm)}
    want = {n: f(_batch(srcs, tgts)) for n, f in calls.items()}
    fresh = _batch(srcs, tgts)
    assert _same(calls["plane"](fresh), want["plane"])
    for which in (0, 1):                                 # side[*].cov_valid stays false: the accessor refuses
        with pytest.raises(_lib.MrsError, match="covariances not computed"):
            fresh.covariances(which)
    for order in (("plane", "gicp", "icp", "pcl", "plane", "icp", "gicp"), ("pcl", "plane", "pcl", "icp", "plane", "gicp", "plane")):
        b = _batch(srcs, tgts)
        for n in order:
            assert _same(calls[n](b), want[n]), (order, n)
    assert want["plane"][2].max() <= want["icp"][2].max()


def test_bad_arguments(dev):
    from mr_slam_amd import _lib, gicp
    p = PK.pair(6)
    b = _batch([p[0]], [p[1]])
    for k in (2, 33, 0, -1):
        with pytest.raises(_lib.MrsError, match="normal_k"):
            b.align_icp_plane(normal_k=k)
        with pytest.raises(_lib.MrsError, match="normal_k"):
            b.compute_normals(1, k)
        with pytest.raises(_lib.MrsError, match="normal_k"):
            b.icp_plane_step(np.eye(4)[None], normal_k=k)
    for which in (2, -1):
        with pytest.raises(_lib.MrsError, match="which"):
            b.compute_normals(which)
        with pytest.raises(_lib.MrsError, match="which"):
            _lib.load().mrs_gicp_batch_get_normals(b._h, which, np.empty((p[1].shape[0], 4), np.float32))
        with pytest.raises(_lib.MrsError, match="which"):
            _lib.load().mrs_gicp_batch_set_normals_host(b._h, which, np.zeros((p[1].shape[0], 4), np.float32), 4)
    with pytest.raises(_lib.MrsError, match="normals neither computed nor given"):
        b.normals(1)
    with pytest.raises(_lib.MrsError, match="stride_floats"):
        _lib.load().mrs_gicp_batch_set_normals_host(b._h, 1, np.zeros((p[1].shape[0], 2), np.float32), 2)
    with pytest.raises(_lib.MrsError):
        b.align_icp_plane(max_iterations=0)
    with pytest.raises(_lib.MrsError):
        b.align_icp_plane(max_correspondence_distance=-1.0)
    with pytest.raises(_lib.MrsError):
        gicp.GicpBatch(1).align_icp_plane()              # no clouds set
    with pytest.raises(_lib.MrsError):
        gicp.GicpBatch(1).compute_normals(1)
    with pytest.raises(AttributeError):
        b.align_icp_plane(k_correspondences=15)
    T, conv, its, state = b.align_icp_plane(**PK.SETTINGS["MAPPING_890"])      # and the handle still works
    assert conv[0] and state[0] == R.TRANSFORM
