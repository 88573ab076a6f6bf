"""CPU suite for the Fast Histogram descriptor: the NumPy restatement (tests/golden/fasthist_restate.py) reproduces what the reference's own
FastHistogram.py computed for the fixture clouds (tests/golden/ref_fasthist.npz), the bucket rule of the kernels (fasthist_bucket.hpp,
compiled by g++) agrees with the restatement on adversarial ranges, the new C-ABI symbols are exported and bound, and the drop-in is only
registered when asked for."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import fasthist_restate as R  # noqa: E402


@pytest.fixture(scope="module")
def g():
    return R.load()


def test_fixture_cases(g):
    assert list(g) == ["gauss1", "gauss2", "gauss7", "gauss100", "gauss1000", "gauss4097", "lidar", "nclt", "edges", "grid", "zeros"]
    sizes = [c["cloud"].shape[0] for c in g.values()]
    assert sizes[:6] == [1, 2, 7, 100, 1000, 4097] and 4097 < sizes[6] <= 20000 and sizes[8:] == [101, 300, 5]
    assert all(c["cloud"].dtype == np.float32 for n, c in g.items() if n != "nclt")
    assert all(c["hist"].dtype == np.float64 and c["hist"].shape == (100,) for c in g.values())
    assert os.path.getsize(R.FIXTURE) < 512 * 1024


def test_restatement_reproduces_reference(g):
    """counts exactly, the float64 vector bit for bit, and no point above the last edge in any stored case"""
    for name, c in g.items():
        r = R.range_histogram(c["cloud"], 100)
        n = c["cloud"].shape[0]
        assert c["counts"].sum() == n, name
        assert np.array_equal(r.counts, c["counts"]), name
        assert r.hist.tobytes() == c["hist"].tobytes(), name
        assert r.unbound == 0, name


def test_restatement_known_answers(g):
    """edges: point i at range i with M = 100, w = 1: ranges 1..99 sit on edges 1..99 and go to the upper bucket, 0 and 100 to bucket 99"""
    want = np.ones(100, np.int64)
    want[0] = 0
    want[99] = 3
    assert np.array_equal(g["edges"]["counts"], want)
    assert g["zeros"]["counts"][99] == 5 and g["zeros"]["counts"].sum() == 5
    assert g["gauss1"]["counts"][99] == 1


def test_restatement_small_clouds():
    for b in (1, 7, 100):
        r = R.range_histogram(np.zeros((0, 3)), b)
        assert r.counts.shape == (b,) and not r.counts.any() and not r.hist.any() and r.hist.dtype == np.float64 and r.M == 0.0 and r.unbound == 0
        r = R.range_histogram(np.array([[3.0, 4.0, 12.0]]), b)
        assert r.M == 13.0 and r.counts[b - 1] == 1 and r.counts.sum() == 1 and r.hist[b - 1] == 1.0 and r.unbound == 0
    # non-finite points go to the last bucket and do not take part in M
    r = R.range_histogram(np.array([[1.0, 0, 0], [np.nan, 0, 0], [0, np.inf, 0], [4.0, 0, 0], [0, 0, -np.inf]]), 4)
    assert r.M == 4.0 and r.counts.tolist() == [0, 1, 0, 4] and r.unbound == 0


def test_emd_is_a_sequential_sum():
    rng = np.random.default_rng(3)
    G, H = rng.random(100), rng.random(100)
    acc = 0.0
    for a, b in zip(G.tolist(), H.tolist()):
        acc += abs(a - b)
    assert R.emd(G, H) == acc / 100 and R.emd_all(G, np.stack([H, G]))[0] == acc / 100 and R.emd_all(G, np.stack([H, G]))[1] == 0.0


@pytest.fixture(scope="module")
def bucket_lib(tmp_path_factory):
    """fasthist_bucket.hpp, the text the bin kernel compiles, built for the host by g++"""
    d = tmp_path_factory.mktemp("fh")
    src = d / "bucket.cpp"
    src.write_text('#include "fasthist_bucket.hpp"\n'
                   'extern "C" void buckets(const double* d, int n, double M, int b, int* out, int* unbound) {\n'
                   '    const double w = mrs::fh_width(M, b), inv_w = 1.0 / w;\n'
                   '    for (int i = 0; i < n; ++i) out[i] = mrs::fh_bucket(d[i], M, w, inv_w, b, unbound + i);\n'
                   '}\n')
    so = d / "libbucket.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "mr_slam_amd", "csrc"),
                    str(src), "-o", str(so)], check=True)
    return C.CDLL(str(so))


def _buckets(lib, d, M, b):
    d = np.ascontiguousarray(d, np.float64)
    out, unb = np.full(d.size, -7, np.int32), np.full(d.size, -7, np.int32)
    lib.buckets(d.ctypes.data_as(C.c_void_p), C.c_int(d.size), C.c_double(M), C.c_int(b), out.ctypes.data_as(C.c_void_p),
                unb.ctypes.data_as(C.c_void_p))
    return out, unb


def test_bucket_header_matches_restatement(bucket_lib):
    """Adversarial ranges: every edge fl(i w) and its neighbours one and two ulps either side, plus 0, M, M less one ulp, NaN and inf, for
    200 random M (over 30 binary orders of magnitude; every eighth one a power of two, below which doubles lie twice as dense) and each b"""
    rng = np.random.default_rng(17)
    for trial in range(200):
        M = float((1.0 if trial % 8 == 0 else rng.uniform(0.5, 1.0)) * 2.0 ** int(rng.integers(-15, 16)))
        for b in (1, 7, 100, 256):
            e = R.edges(M, b)
            lo, hi = np.nextafter(e, -np.inf), np.nextafter(e, np.inf)
            d = np.concatenate([e, lo, hi, np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf), [0.0, M, np.nextafter(M, 0.0), np.nan, np.inf],
                                rng.uniform(0.0, M, 32)])
            want, want_u = R.buckets(d, M, b)
            got, got_u = _buckets(bucket_lib, d, M, b)
            assert np.array_equal(got, want), (trial, M, b, d[got != want][:4])
            assert np.array_equal(got_u.astype(bool), want_u), (trial, M, b)
            assert got.min() >= 0 and got.max() <= b - 1


def test_bucket_header_degenerate_ranges(bucket_lib):
    """M = 0 (all points at the origin), and subnormal M whose bucket width underflows to 0 or rounds far down: nothing indexes out of
    range, and the gap above the last edge fl(b w) < M, which normal ranges all but never show, is reported as unbound"""
    tiny = 5e-324
    gaps = 0
    for M, d in ((0.0, [0.0, np.nan, np.inf]), (2 * tiny, [tiny, 0.0, 2 * tiny]), (300 * tiny, [tiny, 2 * tiny, 150 * tiny, 299 * tiny])):
        for b in (1, 7, 100, 256):
            want, want_u = R.buckets(np.array(d), M, b)
            got, got_u = _buckets(bucket_lib, np.array(d), M, b)
            assert np.array_equal(got, want) and np.array_equal(got_u.astype(bool), want_u), (M, b, got, want)
            gaps += int(got_u.sum())
    assert gaps >= 2          # (2 tiny, d = tiny): w = 0; (300 tiny, b = 256, d = 299 tiny): w = tiny, fl(b w) = 256 tiny


def test_fh_symbols_exported_and_bound():
    from mr_slam_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = C.CDLL(_lib.LIB_PATH)
    names = ("mrs_fh_batch", "mrs_fh_host", "mrs_loopdb_append_fh", "mrs_loopdb_query_fh", "mrs_loopdb_distances_fh")
    for n in names:
        assert hasattr(lib, n), n
    assert lib.mrs_abi_version() == 1
    api = _lib.load()
    for n in names:
        assert callable(getattr(api, n)), n
    src = open(_lib.HEADER).read()
    assert "MRS_LOOPDB_FH = 5" in src and "#define MRS_FH_MAX_BINS 256" in src
    from mr_slam_amd import fasthist
    assert fasthist.TILE_POINTS >= 64 and fasthist.MAX_BINS == 256 and fasthist.KIND_FH == 5 and fasthist.DEFAULT_BINS == 100
    with pytest.raises(_lib.MrsError) as e:                       # the C side's null check, no GPU involved
        api.mrs_fh_batch(None, None, 0, 3, None, None, 1, 100, None, None, None, None, None)
    assert e.value.status == 1 and "null pointer" in str(e.value)
    with pytest.raises(_lib.MrsError) as e:
        api.mrs_fh_host(None, None, 0, 3, 0, 100, None, None, None, None)
    assert e.value.status == 1
    for call in (lambda: api.mrs_loopdb_append_fh(None, None, 0, None), lambda: api.mrs_loopdb_distances_fh(None, None, 0, None, None),
                 lambda: api.mrs_loopdb_query_fh(None, None, 0, 1, None, None, None, None)):
        with pytest.raises(_lib.MrsError) as e:
            call()
        assert e.value.status == 1 and "null pointer" in str(e.value)
    with pytest.raises(_lib.MrsError, match="d_points.*no CPU fallback"):
        api.mrs_fh_batch(None, np.zeros((4, 3), np.float32), 0, 3, None, None, 1, 100, None, None, None, None, None)
    with pytest.raises(ValueError):
        fasthist.FastHistogramDatabase(0, 16, bins=257)


def test_install_registers_fasthistogram_only_when_asked():
    from mr_slam_amd import compat
    saved = {k: sys.modules.pop(k) for k in list(sys.modules) if k.split(".")[0] in ("pr_methods",) + compat._NAMES + ("util",)}
    try:
        compat.install()
        assert "pr_methods" not in sys.modules
        compat.install(scancontext=True, m2dp=True)
        assert "pr_methods.FastHistogram" not in sys.modules
        compat.install(fasthistogram=True)
        from pr_methods.FastHistogram import calculateRange, calculateW, distanceJudge, getEMD, statisticsOnRange
        from mr_slam_amd.compat import FastHistogram as mod
        assert statisticsOnRange is mod.statisticsOnRange and sys.modules["pr_methods"].FastHistogram is mod
        assert callable(calculateRange) and calculateW is getEMD
        # the host-side functions: the two-vector distance is the sequential sum, the one-range bucket follows the contract
        rng = np.random.default_rng(5)
        G, H = rng.random(100), rng.random(100)
        assert getEMD(G, H) == R.emd(G, H) and calculateW(H, G) == R.emd(H, G) and isinstance(getEMD(G, H), float)
        M, b = 37.3, 100
        e = R.edges(M, b)
        d = np.concatenate([e, np.nextafter(e, -np.inf), np.nextafter(e, np.inf), [0.0, M, np.nan, np.inf]])
        assert [distanceJudge(x, 0.0, M, b) for x in d.tolist()] == R.buckets(d, M, b)[0].tolist()
    finally:
        for k in [k for k in sys.modules if k.split(".")[0] in ("pr_methods",) + compat._NAMES + ("util",)]:
            sys.modules.pop(k)
        sys.modules.update(saved)
