"""The library's scratch cache outlives the handles that used it: a block released on a loop database's own stream stays cached after the
database and its stream are destroyed.  mrs::scratch_forget_stream gives such blocks a fresh event and no stream before the stream goes,
and the cache drops the status of an event query it swallows.  What that repairs (a stale "stream is capturing" status met by the next
launch check, in some runs of the whole suite only) depends on the runtime's heap and cannot be forced from a test; this test guards the
other side: blocks handed on from a destroyed stream's database to the next one still carry no one else's data, through every query form."""
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_scratch_blocks_survive_the_stream_that_used_them():
    import torch
    from mr_slam_amd import node, ring
    N, Q = 130, 3
    g = torch.Generator(device="cuda:0").manual_seed(5)
    norm = ring.normalize(torch.randn((N + Q, 1, 120, 120), device="cuda:0", generator=g))[:, 0].contiguous()
    half = ring.half_spectrum(norm).contiguous()
    full = torch.cat([half, half[:, 1:60].flip(1).conj()], 1).contiguous()
    want = None
    for generation in range(4):
        db = node.LoopDatabase("ring", capacity=16)
        db.extend_spectra(half[:N])
        got = [db.query_multi(q) for q in (full[N:].cpu(), full[N:], half[N:])]        # host, device and spectrum forms: the same scores
        for D, A in got[1:]:
            assert np.array_equal(D, got[0][0]) and np.array_equal(A, got[0][1])
        if want is None:
            want = got[0]
        assert np.array_equal(got[0][0], want[0]) and np.array_equal(got[0][1], want[1]), generation
        del db                                                                          # destroys the database's stream
        gc.collect()
