// posegraph_order.hpp -- the symbolic phase of the pose-graph optimiser's sparse elimination tier (posegraph.hip): which
// separators of a stage's reduced system are eliminated before the dense Cholesky, in which order, and the block pattern that leaves.
// Plain C++17 for the host: posegraph.hip runs it whenever a topology is rebuilt, and g++ compiles it for the CPU tests
// (tests/cpp/posegraph_order_host.cpp), where tests/golden/posegraph_order_restate.py states the same rounds in Python.
//
// The block graph: nodes 0 .. E - 1 (the separators), an edge per off-diagonal block of the reduced system.  With `alive` the nodes not yet
// eliminated, rounds repeat while |alive| > dense_limit:
//   dmin is the smallest degree among the alive nodes (degrees count alive neighbours, as they stand when the round starts);
//   the alive nodes are scanned in ascending index, and node a is taken if deg(a) <= dmin + slack, no neighbour of a was taken in this
//   round, and |alive| - taken > dense_limit;
//   the taken nodes are eliminated: the alive neighbours of each (its struct, d of them) become a clique.
// A round is a level: its nodes are pairwise non-adjacent, so a level's columns depend on earlier levels only.  What stays alive is the
// core, in ascending index.  A node's position is its place in the elimination order, the core's nodes following in their order.
#pragma once
#include <algorithm>
#include <cstdint>
#include <iterator>
#include <map>
#include <utility>
#include <vector>

namespace mrs {
namespace pgo {

struct SparseOrder {
    int E = 0, eliminated = 0, core = 0, levels = 0, max_degree = 0;
    long long blocks = 0;                    // sum (d + 1): a column's diagonal block and its d blocks below
    long long updates = 0;                   // sum d (d + 1) / 2: the block products the columns send on
    std::vector<int> order;                  // [E] position -> node
    std::vector<int> level_ptr;              // [levels + 1] positions
    std::vector<int> col_ptr;                // [eliminated + 1] into col_struct and col_tgt; column k's blocks start at block col_ptr[k] + k
    std::vector<int> col_struct;             // per slot: the position of the block's row, ascending within a column
    std::vector<int> col_tgt;                // per slot: target << 1 | 1 if the target is the block's transpose; -1: fill only
    std::vector<int> row_ptr;                // [E + 1] by position, into row_k and row_slot
    std::vector<int> row_k, row_slot;        // rows(a): the (k, slot) with a in struct(k), ascending k
    std::vector<int> core_tgt;               // the targets inside the core: its diagonal blocks in its order, then the others as given
};

// Targets 0 .. E - 1 are the diagonal blocks in order; the others have tgt_a > tgt_b.  Returns false when the running block count passes
// max_blocks: *count is then the count that passed it, and *out is unspecified.
inline bool sparse_order(int E, int n_tgt, const int* tgt_a, const int* tgt_b, int dense_limit, int slack, long long max_blocks, SparseOrder* out,
                         long long* count)
{
    SparseOrder& o = *out;
    o = SparseOrder();
    o.E = E;
    std::vector<std::vector<int>> adj(E);
    std::map<std::pair<int, int>, int> target;
    for (int t = E; t < n_tgt; ++t) {
        adj[tgt_a[t]].push_back(tgt_b[t]);
        adj[tgt_b[t]].push_back(tgt_a[t]);
        target[{tgt_a[t], tgt_b[t]}] = t;
    }
    for (int a = 0; a < E; ++a) std::sort(adj[a].begin(), adj[a].end());
    std::vector<char> alive(E, 1), blocked(E);
    std::vector<int> pos(E, -1), taken, merged;
    std::vector<std::vector<int>> structs;                       // by elimination position, as nodes
    int n_alive = E;
    o.level_ptr.push_back(0);
    *count = 0;
    while (n_alive > dense_limit) {
        int dmin = E;
        for (int a = 0; a < E; ++a)
            if (alive[a]) dmin = std::min(dmin, (int)adj[a].size());
        std::fill(blocked.begin(), blocked.end(), 0);
        taken.clear();
        for (int a = 0; a < E; ++a) {
            if (!alive[a] || blocked[a] || (int)adj[a].size() > dmin + slack || n_alive - (int)taken.size() <= dense_limit) continue;
            taken.push_back(a);
            for (int r : adj[a]) blocked[r] = 1;
        }
        for (int a : taken) {
            const std::vector<int> s = adj[a];
            const long long d = (long long)s.size();
            o.blocks += d + 1;
            o.updates += d * (d + 1) / 2;
            o.max_degree = std::max(o.max_degree, (int)d);
            if (o.blocks > max_blocks) {
                *count = o.blocks;
                return false;
            }
            for (int r : s) {                                    // adj[r] <- (adj[r] + s) without r and a
                merged.clear();
                std::set_union(adj[r].begin(), adj[r].end(), s.begin(), s.end(), std::back_inserter(merged));
                adj[r].clear();
                for (int v : merged)
                    if (v != r && v != a) adj[r].push_back(v);
            }
            alive[a] = 0;
            pos[a] = (int)o.order.size();
            o.order.push_back(a);
            structs.push_back(s);
            adj[a].clear();
        }
        n_alive -= (int)taken.size();
        o.level_ptr.push_back((int)o.order.size());
    }
    o.eliminated = (int)o.order.size();
    o.levels = (int)o.level_ptr.size() - 1;
    o.core = n_alive;
    for (int a = 0; a < E; ++a)
        if (alive[a]) {
            pos[a] = (int)o.order.size();
            o.order.push_back(a);
        }
    std::vector<std::vector<std::pair<int, int>>> rows(E);
    o.col_ptr.push_back(0);
    for (int k = 0; k < o.eliminated; ++k) {
        std::vector<int>& s = structs[k];
        for (int& r : s) r = pos[r];
        std::sort(s.begin(), s.end());
        const int nk = o.order[k];
        for (int slot = 0; slot < (int)s.size(); ++slot) {
            const int nr = o.order[s[slot]];
            const auto it = target.find({std::max(nk, nr), std::min(nk, nr)});
            o.col_struct.push_back(s[slot]);
            o.col_tgt.push_back(it == target.end() ? -1 : (it->second << 1 | (nr < nk ? 1 : 0)));
            rows[s[slot]].push_back({k, slot});
        }
        o.col_ptr.push_back((int)o.col_struct.size());
    }
    o.row_ptr.push_back(0);
    for (int p = 0; p < E; ++p) {
        for (const auto& ks : rows[p]) {
            o.row_k.push_back(ks.first);
            o.row_slot.push_back(ks.second);
        }
        o.row_ptr.push_back((int)o.row_k.size());
    }
    for (int c = 0; c < o.core; ++c) o.core_tgt.push_back(o.order[o.eliminated + c]);
    for (int t = E; t < n_tgt; ++t)
        if (alive[tgt_a[t]] && alive[tgt_b[t]]) o.core_tgt.push_back(t);
    *count = o.blocks;
    return true;
}

}  // namespace pgo
}  // namespace mrs
