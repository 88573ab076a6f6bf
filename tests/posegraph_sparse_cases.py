"""Scenes for the tests of the pose-graph optimiser's sparse elimination tier (test_posegraph_sparse_cpu.py, test_posegraph_sparse_gpu.py,
test_posegraph_sparse_adapter.py) beyond those of posegraph_cases.py, the restatement's result on the one that is optimised, and the
ordering restatement (tests/golden/posegraph_order_restate.py) on any scene.  Computed once per process and never written to.

Both new scenes have more separators than the dense solver holds (MRS_PGO_MAX_SEPARATORS = 1024) and almost no fill:
  three460 : three chains of 460 poses, every pose of the first joined to its partner in the second, every other pose of the second to
             its partner in the third: 1149 separators of Gauss-Newton at segment length 64.  The restatement converges in 44 iterations.
  laps1400 : one chain of 1400 poses, loops (k, k + 700): 1398 separators.  For the ordering tests only: Gauss-Newton does not reach 1e-9
             on it within 200 iterations, and after 3 iterations two exact solve orders already differ by 3.9e-10 m, too close to the
             suite's tolerance to compare against."""
import functools

import posegraph_cases as PC
import posegraph_order_restate as OR  # noqa: E402  (posegraph_cases puts tests/golden on the path)

R = PC.R
DENSE_LIMITS = (0, 4, 1024)


@functools.lru_cache(maxsize=None)
def scene(name):
    if name == "three460":
        return PC.make("three460", 4, (460, 460, 460), [(k, 460 + k) for k in range(460)] + [(460 + k, 920 + k) for k in range(0, 460, 2)])
    if name == "laps1400":
        return PC.make("laps1400", 3, (1400,), [(k, k + 700) for k in range(1, 700)])
    return PC.with_prior() if name == "quirks_prior" else PC.scene(name)


@functools.lru_cache(maxsize=None)
def expected(name, order=None, max_iterations=R.MAX_ITERATIONS_DEFAULT):
    s = scene(name)
    return R.optimize(s.chain_lengths, s.odom, s.li, s.lj, s.lZ, prior=s.prior, order=order, max_iterations=max_iterations)


@functools.lru_cache(maxsize=None)
def block_graph(name, segment_length, stage):
    """(sep_node, edges) of the scene's reduced system"""
    s = scene(name)
    return OR.block_graph(s.chain_lengths, s.li.tolist(), s.lj.tolist(), segment_length, stage)


@functools.lru_cache(maxsize=None)
def order(name, segment_length, stage, dense_limit, slack=OR.SLACK_DEFAULT):
    sep, edges = block_graph(name, segment_length, stage)
    return OR.order(len(sep), edges, dense_limit, slack)
