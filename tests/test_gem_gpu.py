"""GPU suite for the global elevation map (mr_slam_amd/gem.py over mrs_gem_*): every case of tests/gem_cases.py against the vectorised
NumPy restatement (tests/golden/gem_restate.py; tests/test_gem_cpu.py shows it equal to the literal one).  Integers, keys and floats are
compared bit for bit: every operation of the contract is one IEEE add, multiply, divide, ceil or compare in a fixed order, in a library
built with -ffp-contract=off."""
import numpy as np
import pytest

import gem_cases as GC

R = GC.R
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gem():
    import torch
    assert torch.cuda.is_available()        # PyTorch's runtime has to see the device before the library's does
    from mr_slam_amd import gem
    return gem


def _same_store(got, want):
    assert len(got) == len(want.subs)
    for k, w in enumerate(want.subs):
        cells, pose, centre = got.submap(k)
        assert R.same(cells, w), "submap %d: %d records, %d expected" % (k, cells.size, w.size)
        assert np.array_equal(pose, want.poses[k]) and np.array_equal(centre, want.centres[k])
    assert R.same(got.compose(), want.compose())
    assert got.n_cells == want.compose().size


@pytest.mark.parametrize("name", sorted(GC.open_scripts()))
def test_open_submap(gem, name):
    script = GC.open_scripts()[name]
    got, want = GC.run(gem.ElevationSubmaps(), script), GC.run(R.Vectorised(), script)
    _same_store(got, want)
    assert got.n_open == 0


def test_cells_from_device_memory(gem):
    import torch
    script = GC.open_scripts()["dup_across_calls"]
    dev = [(op, torch.from_numpy(R.bits(a[0]).view(np.int32).copy()).cuda(), *a[1:]) if op == "append_cells" else (op, *a) for op, *a in script]
    got, want = GC.run(gem.ElevationSubmaps(), dev), GC.run(R.Vectorised(), script)
    _same_store(got, want)
    t, _, _ = got.submap(0, device=True)
    assert t.is_cuda and np.array_equal(t.cpu().numpy().view(np.uint32), R.bits(want.subs[0]))
    assert np.array_equal(got.compose(device=True).cpu().numpy().view(np.uint32), R.bits(want.compose()))
    leaving = GC.open_scripts()["leaving2"]
    (op, w, *window), close = leaving
    dev = [(op, torch.from_numpy(R.bits(w).view(np.float32).copy()).cuda(), *window), close]       # the same words as a float32 tensor
    _same_store(GC.run(gem.ElevationSubmaps(), dev), GC.run(R.Vectorised(), leaving))


def _play(name, make):
    st, calls = GC.build(name, make)
    stats = []
    for opt in calls:
        st.update_global(opt)
        stats.append((st.dropped, st.matched))
    return st, stats


@pytest.mark.parametrize("name", sorted(GC.scenes()))
def test_update_global(gem, name):
    got, sg = _play(name, gem.ElevationSubmaps)
    want, sw = _play(name, R.Vectorised)
    print(name, "dropped / matched per call:", sg, "expected", sw)
    assert sg == sw
    _same_store(got, want)


def test_update_global_repeats_its_bits(gem):
    a, sa = _play("k3_twice", gem.ElevationSubmaps)
    b, sb = _play("k3_twice", gem.ElevationSubmaps)
    assert sa == sb and R.same(a.compose(), b.compose())


@pytest.fixture(scope="module")
def robots(gem):
    scripts, poses, local_maps, refs = GC.robots()
    got, want = [GC.run(gem.ElevationSubmaps(), s) for s in scripts], [GC.run(R.Vectorised(), s) for s in scripts]
    for g, w, p in zip(got, want, poses):
        g.update_global(p)
        w.update_global(p)
    return got, want, poses, local_maps, refs


@pytest.mark.parametrize("merge, rule", [(False, R.WEIGHTED), (True, R.WEIGHTED), (True, R.AS_WRITTEN)])
def test_compose_robots(gem, robots, merge, rule):
    got, want, poses, local_maps, refs = robots
    w, dropped = R.compose_robots_vec(want, poses, local_maps, refs, merge, rule, GC.RES)
    g = gem.compose_robots(got, poses, local_maps, refs, merge_cells=merge, rule=rule)
    assert R.same(g, w), (g.size, w.size)
    d = gem.compose_robots(got, poses, local_maps, refs, merge_cells=merge, rule=rule, device=True)
    assert d.is_cuda and np.array_equal(d.cpu().numpy().view(np.uint32), R.bits(w))
    import torch
    dev_maps = [torch.from_numpy(np.ascontiguousarray(m).view(np.int32).reshape(-1, 10)).to("cuda:0") for m in local_maps]
    dd = gem.compose_robots(got, poses, dev_maps, refs, merge_cells=merge, rule=rule, device=True)     # local maps that never leave the device
    assert np.array_equal(dd.cpu().numpy().view(np.uint32), R.bits(w))
    with pytest.raises(ValueError):
        gem.compose_robots(got, poses, [dev_maps[0]] + list(local_maps[1:]), refs)
    if not merge:
        assert g.size == sum(len(s.compose()) for s in want) + sum(m.size for m in local_maps)
        n = gem.compose_robots(got, poses)                           # without local maps
        assert R.same(n, R.compose_robots_vec(want, poses)[0])


@pytest.mark.parametrize("name", sorted(GC.costmap_cases()))
def test_costmap(gem, name):
    import torch
    cloud, origin, size, res, kw = GC.costmap_cases()[name]
    want = R.costmap_vec(cloud, origin, size, res, **kw)
    got = gem.costmap(cloud, origin, size, res, **kw)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    if cloud.size:
        t = torch.from_numpy(R.bits(cloud).view(np.int32).copy()).cuda()
        dev = gem.costmap(t, origin, size, res, device=True, **kw)
        assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), want)


def test_costmap_of_a_store(gem):
    got, _ = _play("k3_weighted", gem.ElevationSubmaps)
    want, _ = _play("k3_weighted", R.Vectorised)
    g = got.costmap((-2.0, -2.0), (25, 23), 0.2, travers_thresh=0.5)
    assert np.array_equal(g, R.costmap_vec(want.compose(), (-2.0, -2.0), (25, 23), 0.2, travers_thresh=0.5))


def test_bad_arguments_are_refused(gem):
    from mr_slam_amd import MrsError
    s = gem.ElevationSubmaps()
    with pytest.raises(MrsError):
        s.submap(0)
    with pytest.raises(MrsError):
        gem.ElevationSubmaps(resolution=0.0)
    with pytest.raises(MrsError):
        s.close_submap(np.full((4, 4), np.nan, np.float32), (0, 0))
    assert len(s) == 0 and s.update_global(np.zeros((0, 4, 4), np.float32)) == 0
