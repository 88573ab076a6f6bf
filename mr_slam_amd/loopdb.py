"""What the wrappers of the device-resident descriptor lists (C ABI `mrs_loopdb_*`, csrc/loopdb.hip) share: the handle, its length and
entries, the one-vector argument of the vector kinds (Scan Context, M2DP, Fast Histogram) and the query that is asked again when the
list grew meanwhile.  The classes themselves are node.LoopDatabase / DiscoDatabase, scancontext.ScanContextDatabase, m2dp.M2DPDatabase
and fasthist.FastHistogramDatabase."""
import ctypes as C

import numpy as np
import torch

from . import _lib


def query_grown(call, cap, slack=0):
    """`call(cap)` sizes its arrays for `cap` entries, runs the query and returns (entries the C side needed room for, result).  Another
    thread may append between the sizing and the sweep: while the list outgrew the arrays the query is asked again with room for what
    was needed plus `slack`.  -> the result of the call that fitted"""
    while True:
        need, out = call(cap)
        if need <= cap:
            return out
        cap = need + slack


class LoopDb(_lib.Handle):
    """One robot's descriptor list on one device (mrs_loopdb of the given kind)."""
    _destroy = "mrs_loopdb_destroy"

    def __init__(self, kind, channels, device, capacity):
        self.device = int(device)
        self._create("mrs_loopdb_create", _lib.ctx(self.device), kind, channels, int(capacity))

    def __len__(self):
        n = C.c_int32(0)
        _lib.load().mrs_loopdb_size(self._h, C.byref(n))
        return n.value

    def device_entries(self):
        """(device pointer of the packed entries, device pointer of the signatures / keys, n, floats per entry); the pointers view the
        handle's memory and are valid until it grows"""
        pe, ps, n, ef = C.c_void_p(), C.c_void_p(), C.c_int32(0), C.c_int64(0)
        _lib.load().mrs_loopdb_device_entries(self._h, C.byref(pe), C.byref(ps), C.byref(n), C.byref(ef))
        return pe.value, ps.value, n.value, ef.value


class VectorLoopDb(LoopDb):
    """A kind whose entry is one vector: `_elem` = (torch dtype, numpy dtype, element count) of what append / query take."""
    _elem = None

    def _arg(self, x):
        """(descriptor, on_device, stream) of one descriptor (torch host / device tensor or numpy array)"""
        tdtype, ndtype, count = self._elem
        if isinstance(x, torch.Tensor):
            t = x.detach().to(tdtype).contiguous()
            assert t.numel() == count, tuple(t.shape)
            if t.is_cuda:
                return t, 1, _lib.current_stream(t.device.index or 0)
            return t, 0, None
        a = np.ascontiguousarray(x, dtype=ndtype)
        assert a.size == count, a.shape
        return a, 0, None
