"""The symbolic phase of the pose-graph optimiser's sparse elimination tier (mr_slam_amd/csrc/posegraph_order.hpp) in
plain Python: the block graph of a stage's reduced system from the chains and the loops, and the rounds that pick what is eliminated before
the dense Cholesky.

Nodes are the separators 0 .. E - 1, an edge per off-diagonal block.  While more than `dense_limit` nodes are alive, a round takes, in
ascending index, every alive node whose degree (at the start of the round) is at most the smallest degree plus `slack`, none of whose
neighbours was taken in this round, as long as more than `dense_limit` nodes stay; the neighbours of a taken node become a clique.  A round
is a level; what stays is the core, ascending.  A node's position is its place in the elimination order, the core's nodes last."""
import collections

SLACK_DEFAULT = 1
Order = collections.namedtuple("Order", "E eliminated core levels blocks updates max_degree order level_ptr structs rows core_nodes")
Order.__doc__ = """order: position -> node; level_ptr: positions; structs[k]: the positions of column k's blocks below the diagonal, ascending;
rows[p]: the (k, slot) with p in structs[k], ascending k; core_nodes: the nodes left for the dense system."""


def separators(chain_lengths, li, lj, segment_length):
    """is_sep [N]: pose 0, the poses a loop touches, and the cuts that keep every run of other poses within segment_length (0: unbounded)"""
    N = int(sum(chain_lengths))
    is_sep = [False] * N
    for i, j in zip(li, lj):
        is_sep[int(i)] = is_sep[int(j)] = True
    is_sep[0] = True
    p = 0
    for n in chain_lengths:
        run = 0
        for q in range(p, p + n):
            if is_sep[q]:
                run = 0
            elif segment_length > 0 and run == segment_length:
                is_sep[q] = True
                run = 0
            else:
                run += 1
        p += n
    return is_sep


def block_graph(chain_lengths, li, lj, segment_length, stage):
    """(sep_node, edges): the separators of a stage as pose numbers (stage 1: the anchor, node N, is last; stage 2: pose 0 is held and drops
    out) and the off-diagonal blocks (a, b), a > b, of its reduced system in ascending (a, b): an odometry or loop factor between two
    separators, or a run of other poses between two separators of a chain"""
    N = int(sum(chain_lengths))
    is_sep = separators(chain_lengths, li, lj, segment_length)
    rot = stage == 1
    sep_of = {}
    for p in range(0 if rot else 1, N):
        if is_sep[p]:
            sep_of[p] = len(sep_of)
    if rot:
        sep_of[N] = len(sep_of)
    edges = set()

    def join(i, j):
        if i in sep_of and j in sep_of and i != j:
            a, b = sep_of[i], sep_of[j]
            edges.add((max(a, b), min(a, b)))

    start = 0
    for n in chain_lengths:
        last = None                                              # the separator a run began behind; None behind a chain's start
        for p in range(start, start + n):
            if is_sep[p]:
                if last is not None:                             # last == p - 1: their odometry factor; else the run between them
                    join(last, p)
                last = p
        start += n
    for i, j in zip(li, lj):
        join(int(i), int(j))
    if rot:
        join(N, 0)
    return sorted(sep_of, key=sep_of.get), sorted(edges)


def order(E, edges, dense_limit, slack=SLACK_DEFAULT):
    adj = [set() for _ in range(E)]
    for a, b in edges:
        adj[a].add(b)
        adj[b].add(a)
    alive = set(range(E))
    seq, level_ptr, structs = [], [0], []
    blocks = updates = max_degree = 0
    while len(alive) > dense_limit:
        deg = {a: len(adj[a]) for a in alive}
        dmin = min(deg.values())
        taken, blocked = [], set()
        for a in sorted(alive):
            if deg[a] <= dmin + slack and a not in blocked and len(alive) - len(taken) > dense_limit:
                taken.append(a)
                blocked |= adj[a]
        for a in taken:
            s = sorted(adj[a])
            d = len(s)
            blocks += d + 1
            updates += d * (d + 1) // 2
            max_degree = max(max_degree, d)
            for r in s:
                adj[r] |= set(s)
                adj[r] -= {r, a}
            alive.discard(a)
            seq.append(a)
            structs.append(s)
            adj[a] = set()
        level_ptr.append(len(seq))
    n_elim = len(seq)
    core_nodes = sorted(alive)
    seq = seq + core_nodes
    pos = {a: p for p, a in enumerate(seq)}
    structs = [sorted(pos[r] for r in s) for s in structs]
    rows = [[] for _ in range(E)]
    for k, s in enumerate(structs):
        for slot, p in enumerate(s):
            rows[p].append((k, slot))
    return Order(E, n_elim, len(core_nodes), len(level_ptr) - 1, blocks, updates, max_degree, seq, level_ptr, structs, rows, core_nodes)


def stats(o):
    """the seven numbers mrs_pgo_get_solver_stats reports before the solver in force"""
    return [o.E, o.eliminated, o.core, o.levels, o.blocks, o.updates, o.max_degree]
