"""The shared pieces of the Python layer, without a GPU and without the built library: _lib.Handle (who destroys a C handle, and when),
_lib.header_int (constants of the C ABI header) and loopdb.query_grown (the query that is asked again when the list grew).  `_lib.load`
is replaced by a namespace that records every call."""
import gc
import re

import numpy as np
import pytest

from mr_slam_amd import _lib, loopdb

HANDLE_CLASSES = {"LoopDatabase", "DiscoDatabase", "ScanContextDatabase", "M2DPDatabase", "FastHistogramDatabase", "PcmGraph",
                  "KeyframeStore", "ElevationSubmaps", "ElevationMap", "GicpBatch", "RadonPlan", "Exchange", "PlannedFetch"}
BASES = {"LoopDb", "VectorLoopDb"}           # the loop databases' shared bases: no handle of their own kind


class _Recorder:
    """stands in for the bound C ABI: every attribute is a function that notes (name, args); a `*_create` fills the handle it is given
    unless its name is in `failing`, and a name in `failing` raises"""

    def __init__(self, failing=()):
        self.calls, self.failing = [], set(failing)

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            if name in self.failing:
                raise _lib.MrsError(name + " refused")
            if name.endswith("_create"):
                args[-1]._obj.value = 0x1000 + len(self.calls)
            return 0
        return call

    def names(self):
        return [n for n, _ in self.calls]


@pytest.fixture
def fake(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(_lib, "load", lambda: rec)
    return rec


class _Thing(_lib.Handle):
    _destroy = "mrs_thing_destroy"

    def __init__(self, size):
        self._create("mrs_thing_create", size)


def _walk(cls):
    for sub in cls.__subclasses__():
        yield sub
        yield from _walk(sub)


def test_every_handle_class_derives_and_names_a_declared_destroy():
    from mr_slam_amd import (elevation, fasthist, gem, gicp, m2dp, node, pcm, ring, scancontext, shard, submap)  # noqa: F401
    found = {c.__name__: c for c in _walk(_lib.Handle) if c.__module__.startswith("mr_slam_amd.")}
    assert set(found) == HANDLE_CLASSES | BASES
    protos = _lib.parse_header(_lib.HEADER)
    for name in HANDLE_CLASSES:
        cls = found[name]
        assert cls._destroy in protos, (name, cls._destroy)
        assert [depth for _, depth, _ in protos[cls._destroy][1]] == [1], name              # takes the handle and nothing else
        assert "__del__" not in vars(cls) and cls.__del__ is _lib.Handle.__del__, name
    assert {found[n]._destroy for n in HANDLE_CLASSES if issubclass(found[n], loopdb.LoopDb)} == {"mrs_loopdb_destroy"}
    assert found["PlannedFetch"]._destroy == "mrs_exchange_fetch_plan_destroy" and found["Exchange"]._destroy == "mrs_exchange_destroy"


def test_a_handle_is_destroyed_once_on_del(fake):
    t = _Thing(3)
    assert fake.names() == ["mrs_thing_create"] and fake.calls[0][1][0] == 3
    h = t._h
    assert h.value
    del t
    gc.collect()
    assert fake.names() == ["mrs_thing_create", "mrs_thing_destroy"]
    assert fake.calls[1][1] == (h,)


def test_a_second_del_destroys_nothing(fake):
    t = _Thing(1)
    t.__del__()
    t.__del__()
    del t
    gc.collect()
    assert fake.names().count("mrs_thing_destroy") == 1


def test_a_failed_create_destroys_nothing(fake):
    fake.failing.add("mrs_thing_create")
    with pytest.raises(_lib.MrsError, match="refused"):
        _Thing(1)
    gc.collect()
    assert fake.names() == ["mrs_thing_create"]


def test_a_handle_without_h_destroys_nothing(fake):
    t = _Thing.__new__(_Thing)                  # __init__ raised before _create
    del t
    gc.collect()
    assert fake.calls == []


def test_a_destroy_that_raises_stays_silent(fake, recwarn, capsys):
    fake.failing.add("mrs_thing_destroy")
    t = _Thing(1)
    del t
    gc.collect()
    assert fake.names() == ["mrs_thing_create", "mrs_thing_destroy"]
    assert len(recwarn) == 0 and capsys.readouterr().err == ""        # an exception that leaves __del__ is printed to stderr


def test_a_loop_database_creates_and_destroys_through_the_base(fake, monkeypatch):
    monkeypatch.setattr(_lib, "ctx", lambda device=0: "ctx%d" % device)
    from mr_slam_amd import fasthist, node
    db = fasthist.FastHistogramDatabase(device=0, capacity=9, bins=7)
    assert fake.calls[0][0] == "mrs_loopdb_create" and fake.calls[0][1][:4] == ("ctx0", fasthist.KIND_FH, 7, 9)
    assert len(db) == 0 and fake.names()[-1] == "mrs_loopdb_size"
    d = node.DiscoDatabase(capacity=2)
    assert fake.calls[-1][1][:4] == ("ctx0", node.KIND["disco"], 1, 2)
    del db, d
    gc.collect()
    assert fake.names().count("mrs_loopdb_destroy") == 2


def test_header_int_reads_the_abi_version():
    src = open(_lib.HEADER).read()
    declared = [int(line.split()[2]) for line in src.splitlines() if line.startswith("#define MRS_ABI_VERSION ")]
    assert len(declared) == 1 and _lib.header_int("MRS_ABI_VERSION") == declared[0]
    assert _lib.header_int("MRS_FH_MAX_BINS") == 256 and _lib.header_int("MRS_PCM_MAX_LOOPS") == 4096


def test_header_int_names_an_unknown_constant():
    with pytest.raises(_lib.MrsError, match=r"mrslam_hip\.h does not define MRS_NO_SUCH_CONSTANT") as e:
        _lib.header_int("MRS_NO_SUCH_CONSTANT")
    assert _lib.HEADER in str(e.value)
    with pytest.raises(_lib.MrsError, match="MRS_FH_MAX"):             # a prefix of a defined name is not that name
        _lib.header_int("MRS_FH_MAX")


def test_header_is_read_once(monkeypatch):
    _lib.header_int("MRS_ABI_VERSION")
    monkeypatch.setattr(_lib, "open", lambda *a, **k: pytest.fail("the header was opened again"), raising=False)
    assert _lib.header_int("MRS_M2DP_TILE_POINTS") > 0
    assert "mrs_abi_version" in _lib.parse_header(_lib.HEADER)


@pytest.mark.parametrize("name, hi", [("k", 32), ("bins", 256), ("num_candidates", 64)])
def test_in_range_texts(name, hi):
    assert _lib.in_range(name, 1, hi) == 1 and _lib.in_range(name, np.int64(hi), hi) == hi
    for bad in (0, hi + 1, -1):
        with pytest.raises(ValueError, match=re.escape("%s in 1..%d" % (name, hi)) + "$"):
            _lib.in_range(name, bad, hi)


def _growing(counts):
    """a query over a list whose length is counts[i] at the i-th call: -> (call, the capacities it was asked with)"""
    caps = []

    def call(cap):
        n = counts[len(caps)]
        caps.append(cap)
        return n, np.arange(max(cap, 1))[:n]
    return call, caps


def test_query_grown_asks_again_when_the_list_grew():
    call, caps = _growing([70, 70])
    out = loopdb.query_grown(call, 65, slack=64)
    assert caps == [65, 70 + 64] and np.array_equal(out, np.arange(70))
    call, caps = _growing([3, 5, 5])                                   # exact sizing: grew between each of the first two calls
    out = loopdb.query_grown(call, 2)
    assert caps == [2, 3, 5] and np.array_equal(out, np.arange(5))


def test_query_grown_asks_once_when_the_count_fits():
    for n, cap in ((0, 0), (4, 4), (4, 68)):
        call, caps = _growing([n])
        out = loopdb.query_grown(call, cap, slack=64)
        assert caps == [cap] and out.shape == (n,)


def test_ragged_refuses_host_points():
    import torch
    with pytest.raises(_lib.MrsError, match="no CPU fallback"):
        _lib.ragged(torch.zeros((4, 3)), [0, 4])
