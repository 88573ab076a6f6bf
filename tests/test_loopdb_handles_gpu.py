"""The host side of the loop database handles (csrc/loopdb.hip) and the keyframe store (csrc/submap.hip): what owns the buffers, how an
argument reaches the handle's stream and what a refused call leaves behind.  Every comparison is bit for bit between two ways of making the
same calls; what the kernels compute is checked against references in the suites of the kinds.

Shapes: the first allocation of a handle is 256 entries, so 257 entries are the fewest that make it grow with live entries; a handle has
four pinned stage slots, so six host queries in a row are the fewest that reuse two of them."""
import ctypes as C

import numpy as np
import pytest
import torch

from mr_slam_amd import _lib, fasthist, m2dp, node, scancontext
from mr_slam_amd.submap import KeyframeStore

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FH_BINS = 5
RINGPP_C = 2


class _Kind:
    """One kind of database behind one face: make(capacity), descriptors(n, seed) as host values, append(db, d), query(db, d) -> a tuple of
    arrays (every form of query the kind has), dev(d) -> the same descriptor on the device."""

    def __init__(self, name, make, descriptors, query, append=None):
        self.name, self.make, self.descriptors, self.query = name, make, descriptors, query
        self.append = append or (lambda db, d: db.append(d))

    @staticmethod
    def dev(d):
        if isinstance(d, tuple):
            return tuple(_Kind.dev(x) for x in d)
        return torch.as_tensor(d).to(DEV)


def _np(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _ring_desc(n, seed):
    from mr_slam_amd import ring
    g = torch.Generator(device=DEV).manual_seed(seed)
    full = ring.fft_angle(ring.normalize(torch.randn((n, 1, 120, 120), device=DEV, generator=g))[:, 0].contiguous())
    return [full[i:i + 1].cpu() for i in range(n)]                     # complex64 [1, 120, 120], what generate_RING hands the node


def _ringpp_desc(n, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.rand((RINGPP_C, 120, 120), generator=g) * 3.0 for _ in range(n)]


def _disco_desc(n, seed):
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal(1024).astype(np.float32),
             (rng.standard_normal((40, 120)) + 1j * rng.standard_normal((40, 120))).astype(np.complex64)) for _ in range(n)]


def _sc_desc(n, seed):
    rng = np.random.default_rng(seed)
    return [(rng.random((120, 120)) * 5.0).astype(np.float32) for _ in range(n)]


def _ring_query(db, d):
    return db.query(d, 0.9, want_all=True)


def _sc_query(db, d):
    return db.query(d, 3, 0.1) + db.query_all(d, 0.1)


def _fh_query(db, d):
    return db.query(d, 3) + (db.distances(d),)


KINDS = {
    "ring": _Kind("ring", lambda cap: node.LoopDatabase("ring", capacity=cap), _ring_desc, _ring_query),
    "ringpp": _Kind("ringpp", lambda cap: node.LoopDatabase("ringpp", channels=RINGPP_C, capacity=cap), _ringpp_desc, _ring_query),
    "disco": _Kind("disco", lambda cap: node.DiscoDatabase(capacity=cap), _disco_desc, lambda db, d: db.query(*d),
                   append=lambda db, d: db.append(*d)),
    "sc": _Kind("sc", lambda cap: scancontext.ScanContextDatabase(capacity=cap), _sc_desc, _sc_query),
    "m2dp": _Kind("m2dp", lambda cap: m2dp.M2DPDatabase(capacity=cap),
                  lambda n, seed: list(np.random.default_rng(seed).standard_normal((n, 192))), lambda db, d: db.query(d, 3)),
    "fh": _Kind("fh", lambda cap: fasthist.FastHistogramDatabase(capacity=cap, bins=FH_BINS),
                lambda n, seed: list(np.random.default_rng(seed).random((n, FH_BINS))), _fh_query),
}


def _same_bits(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        x, y = _np(x), _np(y)
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()


def _entries(db):
    """(n, entry_floats) as mrs_loopdb_device_entries reports them"""
    p, n, ef = C.c_void_p(), C.c_int32(0), C.c_int64(0)
    _lib.load().mrs_loopdb_device_entries(db._h, C.byref(p), None, C.byref(n), C.byref(ef))
    assert p.value
    return n.value, ef.value


def _destroy(obj):
    """destroy the handle now (what __del__ would do), whatever is still queued on its stream"""
    fn = _lib.load().mrs_keyframes_destroy if isinstance(obj, KeyframeStore) else _lib.load().mrs_loopdb_destroy
    fn(obj._h)
    obj._h = None


@pytest.mark.parametrize("name", ["disco", "sc", "m2dp", "fh"])
def test_growth_carries_entries_and_signatures(name):
    K = KINDS[name]
    descs = K.descriptors(257, 11)
    grown, roomy = K.make(1), K.make(512)                              # 256 -> 512 with 256 live entries (and signatures / keys); never grows
    for d in descs:
        K.append(grown, d)
        K.append(roomy, d)
    assert len(grown) == len(roomy) == 257
    assert _entries(grown) == _entries(roomy) and _entries(grown)[0] == 257
    for i in (0, 255, 256):
        a, b = K.query(grown, descs[i]), K.query(roomy, descs[i])
        _same_bits(a, b)
        assert int(_np(a[0]).reshape(-1)[0]) == i                      # the entry itself is its own nearest: it arrived where it was put


@pytest.mark.parametrize("name", list(KINDS))
def test_host_and_device_arguments_agree_and_stage_slots_recycle(name):
    K = KINDS[name]
    descs = K.descriptors(9, 23)
    db = K.make(4)
    for d in descs[:3]:
        K.append(db, d)
    from_host = [K.query(db, d) for d in descs[3:]]                    # six host arguments through four pinned slots (DiSCO: two parts each)
    from_device = [K.query(db, K.dev(d)) for d in descs[3:]]
    for a, b in zip(from_host, from_device):
        _same_bits(a, b)
    assert any(_np(x).tobytes() != _np(y).tobytes() for x, y in zip(from_host[0], from_host[5]))      # six different answers, not one


HAND = np.array([[0.1, 0.1, 0.1, 1], [0.15, 0.12, 0.05, 3], [59.99, 0, 0, 5], [60.0, 0, 0, 7], [-0.05, -0.05, -0.05, 2]], np.float32)
EYE = np.eye(4, dtype=np.float32)


def _ring_round(descs):
    db = KINDS["ring"].make(4)
    for d in descs[:3]:
        db.append(d)
    out = db.query(descs[3], 0.9, want_all=True)
    _destroy(db)
    return out


def _keyframe_round():
    s = KeyframeStore(capacity_hint=1024)
    s.append(HAND, EYE)
    pts, offs = s.assemble([[(0, EYE)]])
    out = (pts.cpu().numpy(), offs)
    _destroy(s)
    return out


def test_handle_churn_leaves_later_handles_unharmed():
    ring_descs = KINDS["ring"].descriptors(5, 31)
    before = _ring_round(ring_descs), _keyframe_round()
    for name, K in KINDS.items():
        descs = K.descriptors(2, 37)
        for i in range(32):
            db = K.make(1 + i % 3)
            if i % 4 == 1:
                K.append(db, descs[0])                                 # host argument: its copy may still be queued
            elif i % 4 >= 2:
                K.append(db, K.dev(descs[0]))                          # device argument: the caller's stream waits on the handle's event
            if i % 4 == 3 and name == "ring":
                db.query_multi(torch.cat([ring_descs[0], ring_descs[1]]).to(DEV))     # scratch blocks last used on the stream about to go
            _destroy(db)                                               # no query, no synchronisation by the caller
    hand_dev = torch.as_tensor(HAND).to(DEV)
    for i in range(32):
        s = KeyframeStore(capacity_hint=1024)
        if i % 4 == 1:
            s.append(HAND, EYE)
        elif i % 4 >= 2:
            s.append(hand_dev, EYE)
        if i % 4 == 3:
            s.assemble([[(0, EYE)]])
        _destroy(s)
    after = _ring_round(ring_descs), _keyframe_round()
    _same_bits(before[0], after[0])
    _same_bits(before[1], after[1])


def test_refusals_leave_the_handle_usable():
    api = _lib.load()
    i32, f32, f64, cnt = np.zeros(64, np.int32), np.zeros(64, np.float32), np.zeros(64, np.float64), C.c_int32(0)
    m2dp_arg, sc_arg = np.zeros(192, np.float64), np.zeros((120, 120), np.float32)
    sig, spec = np.zeros(1024, np.float32), np.zeros((40, 120), np.complex64)

    def refusals(name, h, q):
        """(call, message) triples: a wrong-kind call, a count out of range, a null output pointer"""
        if name in ("ring", "ringpp"):
            return [(lambda: api.mrs_loopdb_append_disco(h, sig, spec, 0, None), "not a DiSCO database"),
                    (lambda: api.mrs_loopdb_query_multi(h, q, 0, 0, 64, f32, i32, C.byref(cnt), None), "count in 1..1024"),
                    (lambda: api.mrs_loopdb_query(h, q, 0, 0.5, 0, None, None, None, None, 0, None, None, None, None), "null pointer")]
        if name == "disco":
            return [(lambda: api.mrs_loopdb_append(h, spec, 0, 1, None), "not a RING / RING\\+\\+ database.*mrs_loopdb_append_disco"),
                    (lambda: api.mrs_loopdb_query_sc(h, sc_arg, 0, 65, 0.1, i32, f32, f32.copy(), i32.copy(), C.byref(cnt), None),
                     "not a Scan Context database"),
                    (lambda: api.mrs_loopdb_query_disco(h, q[0], q[1], 0, None, f32, C.byref(cnt), None), "null pointer")]
        if name == "sc":
            return [(lambda: api.mrs_loopdb_append_m2dp(h, m2dp_arg, 0, None), "not an M2DP database.*mrs_loopdb_append_fh"),
                    (lambda: api.mrs_loopdb_query_sc(h, q, 0, 65, 0.1, i32, f32, f32.copy(), i32.copy(), C.byref(cnt), None),
                     "num_candidates in 1..64"),
                    (lambda: api.mrs_loopdb_query_sc(h, q, 0, 1, 0.1, None, f32, f32.copy(), i32, C.byref(cnt), None), "null pointer")]
        if name == "m2dp":
            return [(lambda: api.mrs_loopdb_append_sc(h, sc_arg, 0, None), "not a Scan Context database.*mrs_loopdb_append_fh"),
                    (lambda: api.mrs_loopdb_query_m2dp(h, q, 0, 33, i32, f32, C.byref(cnt), None), "k in 1..32"),
                    (lambda: api.mrs_loopdb_query_m2dp(h, q, 0, 1, None, f32, C.byref(cnt), None), "null pointer")]
        return [(lambda: api.mrs_loopdb_append_m2dp(h, m2dp_arg, 0, None), "not an M2DP database.*mrs_loopdb_append_fh"),
                (lambda: api.mrs_loopdb_query_fh(h, q, 0, 33, i32, f64, C.byref(cnt), None), "k in 1..32"),
                (lambda: api.mrs_loopdb_query_fh(h, q, 0, 1, None, f64, C.byref(cnt), None), "null pointer")]

    for name, K in KINDS.items():
        descs = K.descriptors(4, 41)
        db = K.make(4)
        for d in descs[:3]:
            K.append(db, d)
        before = K.query(db, descs[3])
        q = descs[3]
        q = q if isinstance(q, tuple) else np.ascontiguousarray(_np(q))
        for call, message in refusals(name, db._h, q):
            with pytest.raises(_lib.MrsError, match=message) as e:
                call()
            assert e.value.status == 1, (name, message)
        assert len(db) == 3
        _same_bits(before, K.query(db, descs[3]))
