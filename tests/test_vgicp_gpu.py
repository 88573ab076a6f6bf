"""GPU suite of the voxelised GICP (row G7: FastVGICP / FastVGICPCuda, the Mapping node's default registration: resolution 0.5, DIRECT1,
k = 15): the voxel map (k_vox_keys, k_vox_heads, k_vox_build, build_voxel_map), k_linearize_voxel and the VGICP branches of align / linearize,
on batches of several pairs, ragged clouds, voxel edges and handles that are fed again.

References: the voxel map against a float64 restatement written here (numpy); linearize / align against the CPU restatement
oracle.Gicp(...).set_voxel(res, nb).  Library and restatement are compiled without floating-point contraction and take the voxel of a point
from the same float operation chain, floor(x / res - 0.5), so the voxel choice is compared exactly: no point is excluded for lying near a
voxel boundary.

Not covered here: an LM trial that is REJECTED in VGICP mode.  Twelve CPU runs of the restatement (the three (res, nb) settings of
test_mixed_endings_in_one_batch x four starts, up to 5 m and 0.4 rad off) never rejected a trial (trials == iterations), so that branch stays
covered only through the tests of k_lm_update, which plain GICP shares (tests/test_gicp_gpu.py)."""
import numpy as np
import pytest
from scipy.spatial.transform import Rotation as Rot

pytestmark = pytest.mark.gpu

TOL_T = 1e-4   # metres   (BASELINE.json north_star, as in tests/test_gicp_gpu.py)
TOL_R = 1e-4   # radians
PRM = dict(k_correspondences=15, max_iterations=50, transformation_epsilon=1e-3)


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    from mr_slam_amd import _lib
    _lib.load()
    return "cuda:0"


_scans = {}


def _scan(seed, n):
    """synth.lidar_scan, cast once per (seed, n) (a ray cast costs most of a second)"""
    from mr_slam_amd import synth
    if (seed, n) not in _scans:
        _scans[(seed, n)] = synth.lidar_scan(seed, n, metric=True).astype(np.float64)
    return _scans[(seed, n)]


def _pair(seed, n, rotvec=(0.02, -0.03, 0.08), t=(0.6, -0.4, 0.1), noise=0.01, scan=None):
    rng = np.random.default_rng(seed)
    base = _scan(seed if scan is None else scan, n)
    R = Rot.from_rotvec(rotvec).as_matrix()
    src = (base + rng.normal(0, noise, base.shape)).astype(np.float32)
    tgt = (base @ R.T + np.asarray(t) + rng.normal(0, noise, base.shape)).astype(np.float32)
    T = np.eye(4); T[:3, :3] = R; T[:3, 3] = t
    return src, tgt, T


def _thin(cloud, n):
    """n of the cloud's points, order kept (synth.lidar_scan's own thinning)"""
    return cloud[np.floor(np.arange(n) * (cloud.shape[0] / n)).astype(np.int64)]


def _pose(rotvec, t):
    T = np.eye(4); T[:3, :3] = Rot.from_rotvec(rotvec).as_matrix(); T[:3, 3] = t
    return T


def _pose_err(A, B):
    dt = np.linalg.norm(A[:3, 3] - B[:3, 3])
    dr = np.linalg.norm(Rot.from_matrix(A[:3, :3] @ B[:3, :3].T).as_rotvec())
    return dt, dr


def _batch(n_pairs, res, nb, **kw):
    from mr_slam_amd import gicp
    b = gicp.GicpBatch(n_pairs)
    b.set_params(**{**PRM, "voxel_resolution": res, "voxel_neighbors": nb, **kw})
    return b


def _restatement(oracle, src, tgt):
    g = oracle.Gicp(k=15, max_corr=1e300, max_iter=50, trans_eps=1e-3)
    g.set_source(src); g.set_target(tgt)
    return g


def _same(got, want, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), (what, i)


# ---- a. the voxel map ----

def _lattice():
    """6 x 6 x 4 points with spacing 0.25 = res / 2 around the origin: x, y in -0.75 .. 0.5, z in -0.5 .. 0.25.  At res 0.5 the voxel boundaries
    are (c + 0.5) res = ... -0.75, -0.25, 0.25 ...: every second plane of the lattice lies exactly on one, on both sides of zero (voxel -1 is
    [-0.25, 0.25))."""
    ax = np.arange(-3, 3) * 0.25
    g = np.stack(np.meshgrid(ax, ax, ax[1:5], indexing="ij"), -1).reshape(-1, 3)
    return g.astype(np.float32)


def _lattice_below():
    """The lattice with every boundary coordinate replaced by the next float towards -inf.  In the float chain only 0.25- changes voxel (to -1):
    (-0.25-) / 0.5 - 0.5 and (-0.75-) / 0.5 - 0.5 lie halfway between two floats and round to even, back to -1.0 and -2.0."""
    p = _lattice()
    on = np.isin(p, np.float32([-0.75, -0.25, 0.25]))
    p[on] = np.nextafter(p[on], np.float32(-np.inf))
    return p


def _restate_map(targets, covs, res):
    """The voxel map in float64: per pair the occupied voxels in ascending (x, y, z), with the count, the mean of the points and the mean of
    their covariances; cov_bound = count 2^-52 max|term| per entry (two sequential float64 sums of `count` terms and a division, here and on
    the device: each within count 2^-53 max|term| of the exact mean)."""
    out = []
    o = 0
    for pair, t in enumerate(targets):
        t = np.asarray(t, np.float32)
        c = np.floor(t / np.float32(res) - np.float32(0.5))
        assert c.dtype == np.float32
        uniq, inv, cnt = np.unique(c.astype(np.int64), axis=0, return_inverse=True, return_counts=True)
        inv = inv.reshape(-1)
        V = uniq.shape[0]
        mean = np.zeros((V, 3)); cov = np.zeros((V, 3, 3)); top = np.zeros((V, 3, 3))
        np.add.at(mean, inv, t.astype(np.float64))
        cv = covs[o:o + t.shape[0]]
        np.add.at(cov, inv, cv)
        np.maximum.at(top, inv, np.abs(cv))
        out.append((np.full(V, pair), uniq, cnt, mean / cnt[:, None], cov / cnt[:, None, None], cnt[:, None, None] * 2.0 ** -52 * top))
        o += t.shape[0]
    return [np.concatenate([p[i] for p in out]) for i in range(6)]


def _check_map(b, targets, res):
    pair, coord, mean, count, cov = b.voxel_map()
    wpair, wcoord, wcount, wmean, wcov, cov_bound = _restate_map(targets, b.covariances(1), res)
    assert np.array_equal(pair, wpair) and np.array_equal(coord, wcoord) and np.array_equal(count, wcount)
    assert mean.dtype == np.float32
    ulp = np.spacing(np.abs(wmean).astype(np.float32)).astype(np.float64)
    assert (np.abs(mean.astype(np.float64) - wmean) <= ulp).all()
    assert (np.abs(cov - wcov) <= cov_bound).all()
    return pair, coord, mean, count, cov


_scan_cache = {}


def _scan_pair(seed=21, n=4097):
    """one (source, target, true pose) scan pair of 4097 points: one point more than four 1024-point blocks"""
    if (seed, n) not in _scan_cache:
        _scan_cache[(seed, n)] = _pair(seed, n)
    return _scan_cache[(seed, n)]


@pytest.mark.parametrize("cloud", ["lattice", "lattice_below"])
def test_voxel_map_on_voxel_boundaries(dev, cloud):
    pts = _lattice() if cloud == "lattice" else _lattice_below()
    b = _batch(1, 0.5, 1)
    b.set_sources([pts]); b.set_targets([pts])
    _, coord, _, count, _ = _check_map(b, [pts], 0.5)
    # what the float chain gives by hand: a point ON a boundary belongs to the voxel above it
    if cloud == "lattice":      # x, y: -0.75 -0.5 | -0.25 0 | 0.25 0.5 -> voxels -2 -1 0 two planes each; z: -0.5 | -0.25 0 | 0.25 -> -2 -1 -1 0
        assert coord.min(0).tolist() == [-2, -2, -2] and coord.max(0).tolist() == [0, 0, 0] and count.size == 27
        assert count.reshape(3, 3, 3)[:, :, 1].tolist() == [[8] * 3] * 3 and count.sum() == 144
    else:                       # x, y: -0.75- -0.5 | -0.25- 0 0.25- | 0.5 -> voxels -2 -2 -1 -1 -1 0; z: -0.5 | -0.25- 0 0.25- -> -2 -1 -1 -1
        assert coord.min(0).tolist() == [-2, -2, -2] and coord.max(0).tolist() == [0, 0, -1] and count.size == 18
        assert count.max() == 27 and count.sum() == 144


@pytest.mark.parametrize("res", [0.25, 0.5, 1.0, 1000.0])
def test_voxel_map_of_a_scan(dev, res):
    src, tgt, _ = _scan_pair()
    b = _batch(1, res, 1)
    b.set_sources([src]); b.set_targets([tgt])
    _, coord, _, count, _ = _check_map(b, [tgt], res)
    assert count.sum() == 4097
    if res == 1000.0:           # one voxel holds the whole cloud (the scan reaches 70 m: |x / res - 0.5| < 1)
        assert count.tolist() == [4097] and coord.tolist() == [[-1, -1, -1]]
    else:
        assert count.size > 100 and (coord < 0).any() and (coord > 0).any() and (count == 1).any() and (count > 1).any()


def test_voxel_map_keeps_the_pairs_apart(dev):
    """pairs 0 and 2 share their target: equal coordinates under different pair ids stay separate voxels with equal contents"""
    src, tgt, _ = _scan_pair()
    other = _thin(_pair(22, 9001, scan=30)[1], 3001)
    b = _batch(3, 0.5, 1)
    b.set_sources([src[:700], src, src[:2000]]); b.set_targets([tgt, other, tgt])
    pair, coord, mean, count, cov = _check_map(b, [tgt, other, tgt], 0.5)
    assert (np.diff(pair) >= 0).all() and sorted(set(pair.tolist())) == [0, 1, 2]
    p0, p2 = pair == 0, pair == 2
    assert p0.sum() == p2.sum() > 100
    for a in (coord, mean, count, cov):
        assert np.array_equal(a[p0], a[p2])


# ---- b. linearize ----

_RAGGED_SRC = (700, 4096, 4097, 9001)       # below one 1024-point block; four blocks; one point into a fifth; nine blocks
_RAGGED_TGT = (5000, 3001, 9001, 4500)


@pytest.fixture(scope="module")
def ragged(oracle):
    """four pairs of unequal clouds, each with its pose (near the pair's solution, different for every pair) and its restatement"""
    pairs = []
    for i, (ns, nt) in enumerate(zip(_RAGGED_SRC, _RAGGED_TGT)):
        rv, t = (0.02 - 0.01 * i, -0.03, 0.08 - 0.04 * i), (0.6 - 0.3 * i, -0.4 + 0.2 * i, 0.1)
        src, tgt, Ttrue = _pair(30 + i, 9001, rv, t, scan=30 + i % 2)
        src, tgt = _thin(src, ns), _thin(tgt, nt)
        pose = Ttrue.copy()
        pose[:3, 3] += [0.08 - 0.03 * i, -0.05, 0.02 * i]
        pose[:3, :3] = Rot.from_rotvec([0, 0, 0.01 * (i - 1)]).as_matrix() @ pose[:3, :3]
        pairs.append((src, tgt, pose, _restatement(oracle, src, tgt)))
    return pairs


def _assert_linearized(got, want, what):
    (e, H, b), (we, wH, wb) = got, want
    assert we > 0, what
    assert abs(e - we) < 1e-6 * abs(we), what
    np.testing.assert_allclose(H, wH, rtol=1e-6, atol=1e-6 * np.abs(wH).max(), err_msg=str(what))
    np.testing.assert_allclose(b, wb, rtol=1e-6, atol=1e-6 * np.abs(wb).max(), err_msg=str(what))


@pytest.mark.parametrize("res,nb", [(0.5, 1), (0.5, 7), (1.0, 27), (0.25, 27)])
def test_linearize_ragged_batch(dev, ragged, res, nb):
    batch = _batch(4, res, nb)
    batch.set_sources([p[0] for p in ragged]); batch.set_targets([p[1] for p in ragged])
    e, H, b, _ = batch.linearize(np.stack([p[2] for p in ragged]))
    for i, (src, tgt, pose, g) in enumerate(ragged):
        g.set_voxel(res, nb)
        _assert_linearized((e[i], H[i], b[i]), g.linearize(pose)[:3], (res, nb, i))
        alone = _batch(1, res, nb)
        alone.set_sources([src]); alone.set_targets([tgt])
        e1, H1, b1, _ = alone.linearize(pose[None])
        _same((e[i], H[i], b[i]), (e1[0], H1[0], b1[0]), ("pair %d alone" % i, res, nb))


def _boundary_sources(rng, n=300):
    """points of [-1, 1]^3 with one coordinate each (x, y, z in turn) exactly on a voxel boundary of res 0.5; the other two are random, so no two
    neighbour distances tie and both sides compute the same covariances"""
    p = rng.uniform(-1, 1, (n, 3))
    p[np.arange(n), np.arange(n) % 3] = rng.choice([-0.75, -0.25, 0.25, 0.75], n)
    return p.astype(np.float32)


@pytest.mark.parametrize("target", ["cloud", "single_voxel"])
def test_linearize_hand_cases(dev, oracle, target):
    """Source points exactly on voxel boundaries, at the identity and moved by 0.25 = res / 2 along every axis (exact in float: boundary points
    land on the lattice between boundaries, the others on boundaries or between them); the target is a cloud of many voxels or one that
    occupies the single voxel -1 = [-0.25, 0.25)^3, which DIRECT27 finds from 26 different neighbour offsets and misses from everywhere else."""
    rng = np.random.default_rng(5)
    src = _boundary_sources(rng)
    tgt = (rng.uniform(-1.2, 1.2, (600, 3)) if target == "cloud" else rng.uniform(-0.24, 0.24, (200, 3))).astype(np.float32)
    g = _restatement(oracle, src, tgt)
    for nb in (1, 7, 27):
        b = _batch(1, 0.5, nb)
        b.set_sources([src]); b.set_targets([tgt])
        if target == "single_voxel":
            _, coord, _, count, _ = b.voxel_map()
            assert coord.tolist() == [[-1, -1, -1]] and count.tolist() == [200]
        g.set_voxel(0.5, nb)
        for shift in (0.0, 0.25):
            pose = _pose((0, 0, 0), (shift,) * 3)
            e, H, bb, _ = b.linearize(pose[None])
            _assert_linearized((e[0], H[0], bb[0]), g.linearize(pose)[:3], (target, nb, shift))


# ---- c. one batch, four endings ----

def _starts(Ttrue):
    """at the true pose; 8 cm off; 0.5 / -0.4 / 0.1 m and 0.03 rad off; the source 1000 m away (no voxel of the target is met)"""
    out = [Ttrue.copy() for _ in range(4)]
    out[1][:3, 3] += [0.08, -0.05, 0.02]
    out[1][:3, :3] = Rot.from_rotvec([0, 0, 0.01]).as_matrix() @ out[1][:3, :3]
    out[2][:3, 3] += [0.5, -0.4, 0.1]
    out[2][:3, :3] = Rot.from_rotvec([0, 0, 0.03]).as_matrix() @ out[2][:3, :3]
    out[3][:3, 3] += [1000.0, 0.0, 0.0]
    return np.stack(out)


@pytest.mark.parametrize("res,nb", [(0.5, 1), (0.5, 7), (1.0, 27)])
def test_mixed_endings_in_one_batch(dev, oracle, res, nb):
    """One scan pair four times in a batch, from four starts: the pairs end at different iterations, one of them at once for want of any
    correspondence.  The restatement takes 2, 5, 7 and 0 iterations at (0.5, 1), 3, 5, 5, 0 at (0.5, 7) and 3, 3, 5, 0 at (1.0, 27)."""
    src, tgt, Ttrue = _scan_pair()
    guess = _starts(Ttrue)
    g = _restatement(oracle, src, tgt)
    g.set_voxel(res, nb)
    want = [g.align(guess[i]) for i in range(4)]
    assert len({w[2] for w in want}) >= 3, [w[2] for w in want]       # the test's point: several endings in one batch
    assert not want[3][1] and want[3][2] == 0 and np.array_equal(want[3][0], guess[3].astype(np.float32).astype(np.float64))
    b = _batch(4, res, nb)
    b.set_sources([src] * 4); b.set_targets([tgt] * 4)
    T, conv, its = b.align(guess)
    print("iterations: restatement", [w[2] for w in want], "library", its.tolist())
    for i, (wT, wconv, wits, _) in enumerate(want):
        dt, dr = _pose_err(T[i], wT)
        assert dt < TOL_T and dr < TOL_R, (i, dt, dr)
        assert conv[i] == wconv and abs(int(its[i]) - wits) <= 1, (i, conv[i], wconv, its[i], wits)
    assert not conv[3] and its[3] == 0 and np.isfinite(T[3]).all()
    assert np.array_equal(T[3], guess[3].astype(np.float32).astype(np.float64))
    for i in range(4):
        alone = _batch(1, res, nb)
        alone.set_sources([src]); alone.set_targets([tgt])
        _same(alone.align(guess[i][None]), (T[i:i + 1], conv[i:i + 1], its[i:i + 1]), ("pair %d alone" % i, res, nb))


# ---- d. a handle that is fed again ----

_REFED_SIZES = (3000, 9000, 3100)
_refed_cache = {}


def _refed_clouds(r):
    """three (source, target) pairs of about _REFED_SIZES[r] points, every cloud of another size, thinned from two scans"""
    if r not in _refed_cache:
        rng = np.random.default_rng(60 + r)
        srcs, tgts = [], []
        for i in range(3):
            base = _thin(_scan(30 + (i + r) % 2, 9001), _REFED_SIZES[r] + 137 * i)
            R = Rot.from_rotvec((0.01, -0.01, 0.01 + 0.005 * i)).as_matrix()
            srcs.append((base + rng.normal(0, 0.01, base.shape)).astype(np.float32))
            tgts.append((base @ R.T + np.array([0.15 - 0.05 * i, -0.1, 0.05]) + rng.normal(0, 0.01, base.shape)).astype(np.float32))
        _refed_cache[r] = (srcs, tgts)
    return _refed_cache[r]


def _run(b, linearize=False):
    """everything a registration shows of the handle's state: transforms, converged, iterations, the voxel map (VGICP), the fitness, and on
    request the sums of a linearisation at the final transforms"""
    T, conv, its = b.align()
    out = [T, conv, its, b.fitness(T, 1.0)]
    if b.params.voxel_resolution > 0:
        out += list(b.voxel_map())
    if linearize:
        out += list(b.linearize(T)[:3])
    return out


def _fresh_run(n_pairs, srcs, tgts, linearize=False, **prm):
    f = _batch(n_pairs, prm.pop("voxel_resolution", 0.5), prm.pop("voxel_neighbors", 1), **prm)
    f.set_sources(srcs); f.set_targets(tgts)
    return _run(f, linearize)


_ROUNDS = ("set_clouds", "targets_from_store", "targets_from_store_again", "resolution", "neighbors", "plain_gicp_and_back", "k_correspondences")


@pytest.mark.parametrize("n_pairs", [1, 3])
@pytest.mark.parametrize("round_", _ROUNDS)
def test_refed_handle_equals_fresh_handles_bit_for_bit(dev, n_pairs, round_):
    """A handle that has registered in VGICP mode and is then given other clouds or other parameters gives what a fresh handle gives for the same
    inputs, bit for bit: transforms, converged, iterations, fitness and the voxel map.  The map is cached on the handle (GicpVoxelMap::res_built):
    every way of replacing the targets, the covariances behind the map or its resolution must build it again."""
    P = n_pairs
    (s0, t0), (s1, t1), (s2, t2) = [[c[:P] for c in _refed_clouds(r)] for r in range(3)]
    h = _batch(P, 0.5, 1)
    h.set_sources(s0); h.set_targets(t0)
    first = _run(h)
    _same(first, _fresh_run(P, s0, t0), "first use")
    if round_ == "set_clouds":                      # small, large (every buffer is re-allocated), small again (in the spare capacity)
        h.set_sources(s1); h.set_targets(t1)
        _same(_run(h), _fresh_run(P, s1, t1), "large")
        h.set_sources(s2); h.set_targets(t2)
        _same(_run(h), _fresh_run(P, s2, t2), "small again")
    elif round_.startswith("targets_from_store"):   # the Mapping flow: one scan against stored submaps, the targets swapped on the device
        store = _batch(3, 0.5, 1)
        store.set_targets(_refed_clouds(2)[1])
        store.compute_covariances(1)
        ids = [2, 0, 1][:P]
        h.set_targets_from(store, ids)
        _same(_run(h), _fresh_run(P, s0, [_refed_clouds(2)[1][i] for i in ids]), "targets from the store")
        if round_ == "targets_from_store_again":    # other ids, and linearize as the first call that meets the new targets
            ids = [1, 2, 0][:P]
            h.set_targets_from(store, ids)
            tg = [_refed_clouds(2)[1][i] for i in ids]
            poses = np.stack([np.eye(4)] * P)
            f = _batch(P, 0.5, 1)
            f.set_sources(s0); f.set_targets(tg)
            _same(h.linearize(poses)[:3], f.linearize(poses)[:3], "linearize after other ids")
            _same(_run(h, True), _run(f, True), "align after other ids")
    elif round_ == "resolution":                    # another resolution rebuilds the map (the cache is keyed by it)
        h.set_params(voxel_resolution=1.0)
        coarse = _run(h)
        _same(coarse, _fresh_run(P, s0, t0, voxel_resolution=1.0), "0.5 -> 1.0")
        assert coarse[4].size < first[4].size       # fewer, larger voxels
        h.set_params(voxel_resolution=0.5)
        _same(_run(h), first, "1.0 -> 0.5")
    elif round_ == "neighbors":                     # same map, other lookups
        h.set_params(voxel_neighbors=27)
        wide = _run(h)
        _same(wide, _fresh_run(P, s0, t0, voxel_neighbors=27), "DIRECT1 -> DIRECT27")
        _same(wide[4:], first[4:], "the map does not depend on the neighbourhood")
    elif round_ == "plain_gicp_and_back":           # plain GICP leaves warm-start seeds and certificates behind; the map must survive or be rebuilt
        h.set_params(voxel_resolution=0.0)
        _same(_run(h), _fresh_run(P, s0, t0, voxel_resolution=0.0), "0.5 -> plain GICP")
        h.set_params(voxel_resolution=0.5)
        _same(_run(h), first, "plain GICP -> 0.5")
    elif round_ == "k_correspondences":             # another k: other covariances, hence another map of the same voxels
        h.set_params(k_correspondences=20)
        k20 = _run(h)
        _same(k20, _fresh_run(P, s0, t0, k_correspondences=20), "k 15 -> 20")
        _same(k20[4:8], first[4:8], "same voxels, means and counts")
        assert not np.array_equal(k20[8], first[8])


@pytest.mark.parametrize("n_pairs", [2, 1])
def test_voxel_gicp_stays_out_of_the_windows(dev, n_pairs):
    """The voxelised variant always runs tick by tick (k_linearize_voxel does not gate itself on a pair's state, so its ticks cannot be
    enqueued ahead): the development switch that sets the window length changes nothing, for a batch of two and for a single pair."""
    import os
    src, tgt, Ttrue = _scan_pair()
    srcs = [src, _thin(src, 3001)][:n_pairs]
    tgts = [tgt, _thin(tgt, 2999)][:n_pairs]
    guess = Ttrue.copy()
    guess[:3, 3] += [0.05, -0.03, 0.02]                 # 5 cm from the truth: more than one outer iteration, so more than one window's worth of ticks

    def run():
        b = _batch(n_pairs, 0.5, 1)
        b.set_sources(srcs); b.set_targets(tgts)
        T, conv, its = b.align(np.stack([guess] * n_pairs))
        return T, conv, its, b.hessian.copy()
    old = {k: os.environ.pop(k, None) for k in ("MRS_DEV", "MRS_GICP_WINDOW")}
    try:
        want = run()
        assert want[2].min() >= 2
        os.environ["MRS_DEV"] = "1"
        for window in ("0", "3", "16"):
            os.environ["MRS_GICP_WINDOW"] = window
            _same(run(), want, "MRS_GICP_WINDOW=" + window)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
