"""GPU suite for the RANSAC pose from correspondences (row S5): mrs_ransac_pose_batch through fpfh.ransac_pose against the
NumPy restatement on the fixtures of tests/ransac_cases.py.  Everything integer -- info, the mask -- is compared EXACTLY (the fixtures meet
the margin condition, tests/test_ransac_cpu.py), T within 1e-9."""
import ctypes as C

import numpy as np
import pytest
import torch

import ransac_cases as K

pytestmark = pytest.mark.gpu
R = K.R
DEV = "cuda:0"


def _run(src, dst, offsets, seeds, **kw):
    from mr_slam_amd import fpfh
    T, info, mask = fpfh.ransac_pose(torch.tensor(np.asarray(src)).to(DEV), torch.tensor(np.asarray(dst)).to(DEV),
                                     np.asarray(offsets, np.int64), K.D, seeds=seeds, return_mask=True, **kw)
    return T.cpu().numpy(), info.cpu().numpy(), mask.cpu().numpy()


def _run_case(name):
    src, dst = K.inputs(name)
    return _run(src, dst, [0, src.shape[0]], [K.CASES[name][1]], **K.params(name))


def _check(got, want, name):
    T, info, mask = got
    assert info.tolist() == want["info"].tolist(), (name, info, want["info"])
    assert np.array_equal(mask, want["mask"]), name
    assert np.abs(T - want["T"]).max() < 1e-9, (name, np.abs(T - want["T"]).max())
    assert T[3].tolist() == [0, 0, 0, 1]


SINGLE = [n for n in K.CASES]


@pytest.mark.parametrize("name", SINGLE)
def test_single_pair_equals_the_restatement(name):
    """sizes 0 .. 3, around the wave (64) and the LDS tile (T - 1, T, T + 1, 3 T + 5); hypothesis counts 1, 63, 64, 65, 256, 1000; every
    triple rejected; coincident and repeated rows; dead rows; a mirrored target; no refit; a refit whose count goes down; a tie"""
    T, info, mask = _run_case(name)
    _check((T[0], info[0], mask), K.expected(name), name)


def test_special_results():
    T, info, mask = _run_case("all_rejected")
    assert np.array_equal(T[0], np.eye(4)) and info[0].tolist() == [0, -1, 0, 0] and not mask.any()
    for name in ("M0", "M1", "M2"):
        T, info, mask = _run_case(name)
        assert np.array_equal(T[0], np.eye(4)) and info[0].tolist() == [0, -1, 0, 0] and not mask.any() and mask.size == int(name[1:])
    src, dst = K.inputs("dead")
    T, info, mask = _run_case("dead")
    assert not mask[~R.live(R.widen(src), R.widen(dst))].any() and info[0, 0] == mask.sum() > 50
    p, q, Tx = K.exact(14, 300)
    T, info, mask = _run_case("exact")
    assert info[0, 0] == 300 and mask.all() and np.abs(T[0] - Tx).max() < 1e-9        # all inliers, no noise: the planted pose itself
    T, info, mask = _run_case("mirror")
    assert abs(np.linalg.det(T[0, :3, :3]) - 1) < 1e-12                              # never a reflection
    assert _run_case("no_refit")[1][0, 3] == 0
    assert _run_case("refit_changes")[1][0].tolist() == [87, K.expected("refit_changes")["info"][1], 27, 3]
    c = K.expected("tie")["counts"]
    assert _run_case("tie")[1][0, 1] == int(np.argmax(c)) and (c == c.max()).sum() >= 2


def test_ragged_batch_alone_in_the_batch_and_call_to_call():
    """nine pairs, an empty one in the middle, one with dead rows: each pair equals the restatement, and -- bit for bit, T included -- the
    same pair run alone with the same seed, and the same batch run again"""
    src, dst, off, seeds = K.pack(K.BATCH)
    T, info, mask = _run(src, dst, off, seeds, hypotheses=K.BATCH_H)
    for i, name in enumerate(K.BATCH):
        sl = slice(off[i], off[i + 1])
        _check((T[i], info[i], mask[sl]), K.expected(name, K.BATCH_H), name)
        T1, info1, mask1 = _run(src[sl], dst[sl], [0, off[i + 1] - off[i]], seeds[i:i + 1], hypotheses=K.BATCH_H)
        assert T1[0].tobytes() == T[i].tobytes() and np.array_equal(info1[0], info[i]) and np.array_equal(mask1, mask[sl]), name
    T2, info2, mask2 = _run(src, dst, off, seeds, hypotheses=K.BATCH_H)
    assert T2.tobytes() == T.tobytes() and np.array_equal(info2, info) and np.array_equal(mask2, mask)
    # the neighbours of the pair with dead rows keep their bits when its dead rows are healed, and default seeds are 0 .. P - 1
    healed_s, healed_d = src.copy(), dst.copy()
    k = K.BATCH.index("dead")
    bad = ~R.live(R.widen(src), R.widen(dst))
    assert bad[off[k]:off[k + 1]].sum() == bad.sum() == 7
    healed_s[bad], healed_d[bad] = 1.0, 2.0
    T3, info3, mask3 = _run(healed_s, healed_d, off, seeds, hypotheses=K.BATCH_H)
    for i in range(len(K.BATCH)):
        if i != k:
            assert T3[i].tobytes() == T[i].tobytes() and np.array_equal(info3[i], info[i]) and np.array_equal(mask3[off[i]:off[i + 1]], mask[off[i]:off[i + 1]])
    Td, infod, _ = _run(src, dst, off, None, hypotheses=64)
    Te, infoe, _ = _run(src, dst, off, np.arange(len(K.BATCH)), hypotheses=64)
    assert Td.tobytes() == Te.tobytes() and np.array_equal(infod, infoe)


def test_mask_is_optional_and_more_pairs_than_one_round_holds():
    """without a mask the same T and info; 40 pairs at 65 536 hypotheses go through three rounds of the scratch (16 pairs each)"""
    from mr_slam_amd import fpfh
    src, dst = K.inputs("M65")
    s, d = torch.tensor(src).to(DEV), torch.tensor(dst).to(DEV)
    T, info = fpfh.ransac_pose(s, d, [0, 65], K.D, seeds=[K.CASES["M65"][1]], hypotheses=256)
    _check((T[0].cpu().numpy(), info[0].cpu().numpy(), K.expected("M65")["mask"]), K.expected("M65"), "M65")
    P = 40
    T, info, mask = fpfh.ransac_pose(s.repeat(P, 1), d.repeat(P, 1), np.arange(P + 1) * 65, K.D, seeds=np.full(P, 77), hypotheses=65536,
                                     return_mask=True)
    want = R.ransac(src, dst, 77, K.D, hypotheses=65536)
    assert want["margin"] > K.MARGIN
    T, info, mask = T.cpu().numpy(), info.cpu().numpy(), mask.cpu().numpy()
    for i in (0, 15, 16, 39):
        _check((T[i], info[i], mask[65 * i:65 * i + 65]), want, "pair %d" % i)
    assert all(T[i].tobytes() == T[0].tobytes() for i in range(P)) and (info == info[0]).all()


BAD = [("stride", dict(stride=2)), ("offsets start", dict(offsets=[1, 100])), ("offsets descend", dict(offsets=[0, 60, 50, 100])),
       ("hypotheses 0", dict(hypotheses=0)), ("hypotheses 65537", dict(hypotheses=65537)), ("refine -1", dict(refine_iters=-1)),
       ("refine 17", dict(refine_iters=17)), ("distance 0", dict(max_distance=0.0)), ("distance -1", dict(max_distance=-1.0)),
       ("distance nan", dict(max_distance=float("nan"))), ("distance inf", dict(max_distance=float("inf"))),
       ("similarity -0.1", dict(edge_similarity=-0.1)), ("similarity 1.1", dict(edge_similarity=1.1)), ("similarity nan", dict(edge_similarity=float("nan"))),
       ("sin2 -1e-9", dict(min_sin2=-1e-9)), ("sin2 1", dict(min_sin2=1.0)), ("sin2 nan", dict(min_sin2=float("nan"))),
       ("null src", dict(null="src")), ("null dst", dict(null="dst")), ("null d_offsets", dict(null="d_off")), ("null h_offsets", dict(null="h_off")),
       ("null seeds", dict(null="seeds")), ("null params", dict(null="params")), ("null T", dict(null="T")), ("null info", dict(null="info")),
       ("null ctx", dict(null="ctx")), ("pairs -1", dict(n_pairs=-1))]


@pytest.mark.parametrize("case", BAD, ids=[b[0] for b in BAD])
def test_bad_arguments_are_refused_and_write_nothing(case):
    from mr_slam_amd import _lib, fpfh
    kw = dict(case[1])
    src, dst = K.inputs("M64")
    a = dict(src=torch.tensor(src).to(DEV), dst=torch.tensor(dst).to(DEV))
    off = np.asarray(kw.get("offsets", [0, 64]), np.int64)
    P = kw.get("n_pairs", off.size - 1)
    a.update(h_off=off, d_off=torch.from_numpy(off).to(DEV), seeds=np.zeros(max(P, 1), np.uint64), ctx=_lib.ctx(0),
             T=torch.full((max(P, 1), 16), 7.0, dtype=torch.float64, device=DEV), info=torch.full((max(P, 1), 4), 7, dtype=torch.int32, device=DEV))
    mask = torch.full((100,), 7, dtype=torch.uint8, device=DEV)
    par = fpfh.RansacParams(kw.get("hypotheses", 64), kw.get("refine_iters", 3), kw.get("max_distance", K.D), kw.get("edge_similarity", 0.9),
                            kw.get("min_sin2", 1e-6))
    a["params"] = C.byref(par)
    if "null" in kw:
        a[kw["null"]] = None
    with pytest.raises(_lib.MrsError) as e:
        _lib.load().mrs_ransac_pose_batch(a["ctx"], a["src"], a["dst"], kw.get("stride", 3), a["d_off"], a["h_off"], P, a["seeds"], a["params"],
                                          a["T"], a["info"], mask, _lib.current_stream(0))
    assert e.value.status == 1
    torch.cuda.synchronize()
    for t in (a["T"], a["info"], mask):
        if t is not None:
            assert bool((t == 7).all())


def test_correspondences_against_a_torch_restatement():
    from mr_slam_amd import fpfh
    g = torch.Generator().manual_seed(3)
    fa = torch.rand((150, 15), generator=g).to(DEV)
    fb = torch.cat([fa[:90] + 0.01 * torch.rand((90, 15), generator=g).to(DEV), torch.rand((70, 15), generator=g).to(DEV)])[torch.randperm(160, generator=g).to(DEV)]
    d = torch.cdist(fa.double(), fb.double()) ** 2
    nn_ab, nn_ba = d.argmin(1), d.argmin(0)
    ia, ib = fpfh.correspondences(fa, fb)
    assert ia.dtype == ib.dtype == torch.int64 and ia.is_cuda and torch.equal(ia, torch.arange(150, device=DEV)) and torch.equal(ib, nn_ab)
    ma, mb = fpfh.correspondences(fa, fb, mutual=True)
    keep = nn_ba[nn_ab] == torch.arange(150, device=DEV)
    assert 80 <= int(keep.sum()) < 150 and torch.equal(ma, torch.arange(150, device=DEV)[keep]) and torch.equal(mb, nn_ab[keep])
    ka, kb = fpfh.correspondences(fa, fb, k=3)
    assert torch.equal(ka, torch.arange(150, device=DEV).repeat_interleave(3)) and torch.equal(kb.reshape(150, 3), d.topk(3, dim=1, largest=False).indices)
    ea, eb = fpfh.correspondences(fa, fb[:0], mutual=True)
    assert ea.numel() == eb.numel() == 0
    ea, eb = fpfh.correspondences(fa[:2], fb[:2], k=3)          # fewer rows than k: the empty slots are dropped
    assert ea.tolist() == [0, 0, 1, 1]


def test_end_to_end_keypoints_descriptors_matches_pose_gicp():
    """one synthetic cloud and its rigid copy (points and normals moved, order permuted, so the true matches are known) through
    iss_keypoints -> fpfh -> correspondences -> ransac_pose -> GicpBatch.align(guesses=...)"""
    from mr_slam_amd import fpfh, gicp
    F = K.F
    pts, nrm, pts2, nrm2, where, Rm = K.e2e_scene()
    kp, desc = [], []
    for P, N in ((pts, nrm), (pts2, nrm2)):
        p, n, off = torch.tensor(P).to(DEV), torch.tensor(N).to(DEV), [0, len(P)]
        k, _ = fpfh.iss_keypoints(p, off, F.ISS_SALIENT, F.ISS_NONMAX)
        kp.append(k[0])
        desc.append(fpfh.fpfh(p, n, off, F.RADIUS, keypoints=k))
    ia, ib = fpfh.correspondences(desc[0], desc[1])
    a, b = kp[0][ia].cpu().numpy(), kp[1][ib].cpu().numpy()
    share = (b == where[a]).mean()
    print("keypoints %d / %d, correct matches %.3f" % (len(kp[0]), len(kp[1]), share))
    assert len(a) >= 50 and share >= 0.5            # at this share 256 hypotheses all miss with probability (1 - 0.5^3)^256 < 1e-14
    src, dst = torch.tensor(pts[a]).to(DEV), torch.tensor(pts2[b]).to(DEV)
    T, info = fpfh.ransac_pose(src, dst, [0, len(a)], K.E2E_D, hypotheses=256)
    T, info = T.cpu().numpy(), info.cpu().numpy()
    print("info", info[0].tolist(), "translation error %.3e" % np.abs(T[0, :3, 3] - K.E2E_T).max())
    assert info[0, 0] >= 0.5 * len(a) and np.abs(T[0, :3, 3] - K.E2E_T).max() < K.E2E_D
    g = gicp.GicpBatch(1)
    g.set_params(max_correspondence_distance=0.2)
    g.set_sources([pts]); g.set_targets([pts2])
    Tg, conv, its = g.align(guesses=T)
    print("gicp converged", conv, "iterations", its, "translation error %.3e" % np.abs(Tg[0][:3, 3] - K.E2E_T).max())
    assert bool(np.asarray(conv).reshape(-1)[0])
    assert np.abs(np.asarray(Tg[0])[:3, 3] - K.E2E_T).max() < K.E2E_D and np.abs(np.asarray(Tg[0])[:3, :3] - Rm).max() < 0.02


def test_profiled_call_returns_the_same_result_and_three_stage_times():
    """mrs_ransac_pose_batch_profile on two pairs of eight correspondences, 64 hypotheses: T, info and the mask of the plain call with the
    same seeds, bit for bit, and the three stage times"""
    from mr_slam_amd import fpfh
    rng = np.random.default_rng(16)
    src = rng.uniform(-1, 1, (16, 3)).astype(np.float32)
    dst = (src + np.float32([0.5, -0.25, 0.125])).astype(np.float32)
    s, d = torch.tensor(src).to(DEV), torch.tensor(dst).to(DEV)
    kw = dict(seeds=[3, 4], hypotheses=64, return_mask=True)
    plain = fpfh.ransac_pose(s, d, [0, 8, 16], K.D, **kw)
    *profiled, ms = fpfh.ransac_pose(s, d, [0, 8, 16], K.D, profile=True, **kw)
    torch.cuda.synchronize()
    print("stage ms", ms.tolist())
    assert ms.shape == (3,) and np.isfinite(ms).all() and (ms >= 0).all()
    assert len(profiled) == 3
    for a, b in zip(plain, profiled):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    assert plain[1].cpu().numpy()[:, 0].min() >= 3          # a pose was found for both pairs
