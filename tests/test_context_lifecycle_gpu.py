"""GPU: a context owns what its calls left in it -- the sector tables of the polar BEV (one per num_sector), the twiddle tables of the
correlation kernels, the pool of side-stream slots a small GICP alignment borrows -- and mrs_ctx_destroy gives all of it back.  A second
context, created through the C ABI next to the process's own, is filled, destroyed, created again and filled again: the second pass returns
the bits of the first and no call raises."""
import ctypes as C

import numpy as np
import pytest

import corr_cases as cc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SPECTRA = cc.SPECTRA_CASES[0]          # (1, 30, 34): the smallest shape of tests/test_corr_shapes_gpu.py


def _fill(ctx):
    """every call that leaves something in the context, once; -> the results as host arrays"""
    import torch
    from mr_slam_amd import _lib, bev, gicp
    rng = np.random.default_rng(64)
    out = []
    xyz, offs = bev.pack_scans([rng.uniform(-1, 1, (64, 3)).astype(np.float32)], DEV)
    for num_sector in (20, 24):                                                # two sector tables
        out.append(bev.polar_bev(xyz, offs, 1, 1, 10, num_sector, 2).cpu().numpy())
    Cc, A, D = SPECTRA
    a, b = (torch.from_numpy(np.array(v)).to(DEV) for v in cc.spectra_case(SPECTRA))        # complex64 [4, C, A, D]
    dist = torch.empty(4, dtype=torch.float32, device=DEV)
    ang = torch.empty(4, dtype=torch.int32, device=DEV)
    corr = torch.empty((4, A), dtype=torch.float32, device=DEV)
    _lib.load().mrs_ring_corr_spectra(ctx, a, b, 4, Cc, A, D, dist, ang, corr, _lib.current_stream(0))      # twiddles of length A
    out += [dist.cpu().numpy(), ang.cpu().numpy(), corr.cpu().numpy()]
    src = rng.uniform(-1, 1, (64, 3))
    g = gicp.GicpBatch(1)                                                      # one pair: the alignment borrows a side slot
    g.set_sources([src]); g.set_targets([src + [0.02, -0.01, 0.015]])
    T, conv, its = g.align()
    out += [T, conv, its]
    del g                                                                      # the handle goes before its context
    torch.cuda.synchronize()
    return out


def test_destroy_and_create_again_reproduces(monkeypatch):
    import torch
    assert torch.cuda.is_available()
    from mr_slam_amd import _lib
    lib = _lib.load()
    _lib.ctx(0)                                                                # the process's own context stays as it is
    passes = []
    for _ in range(2):
        ctx = C.c_void_p()
        lib.mrs_ctx_create(0, C.byref(ctx))
        assert ctx.value
        monkeypatch.setattr(_lib, "ctx", lambda device=0, h=ctx: h)             # the Python layer's calls go to this context
        try:
            passes.append(_fill(ctx))
        finally:
            monkeypatch.undo()
            lib.mrs_ctx_destroy(ctx)
    assert len(passes[0]) == len(passes[1]) == 8
    assert passes[0][0].any() and passes[0][1].any() and np.isfinite(passes[0][5]).all()
    for k, (x, y) in enumerate(zip(*passes)):
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), k
