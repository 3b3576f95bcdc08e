// pu_treeform.h -- the host's checks and conversions of the tree forms that the parsimony calls
// and the tree-set calls share (pu_parsimony.hip, pu_treeset.hip): the op-list check of
// pu_fitch_lengths, and the edge list of DESIGN 4.22 with its adjacency, its check and its
// schedule.  Host code only.  Not part of the public ABI.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "pu_ctx.h"

#pragma GCC visibility push(hidden)
namespace pu {

// ops [n_ops][3] with root edge (ra, rb) is a post-order of a binary tree whose tips are exactly
// rows 0..n_taxa-1 and whose internal nodes are n_taxa..2 n_taxa-3
inline int check_ops(const char *fn, int64_t t, int n_taxa, const int32_t *ops, const int32_t *root,
                     std::vector<char> &state) {
    const int n_nodes = 2 * n_taxa - 2;
    // 0 not made yet, 1 made (tips are made), 2 has a parent
    state.assign(n_nodes, 0);
    std::fill(state.begin(), state.begin() + n_taxa, 1);
    for (int i = 0; i < n_taxa - 2; ++i) {
        const int par = ops[3 * i], l = ops[3 * i + 1], r = ops[3 * i + 2];
        if (par < n_taxa || par >= n_nodes || state[par] != 0)
            return set_err(nullptr, PU_E_ARG, "%s: tree %lld op %d: parent %d is no new internal "
                           "node of [%d, %d)", fn, (long long)t, i, par, n_taxa, n_nodes);
        for (int c : {l, r}) {
            if (c < 0 || c >= n_nodes || state[c] != 1)
                return set_err(nullptr, PU_E_ARG, "%s: tree %lld op %d: child %d is not made yet "
                               "or has a parent already (not a post-order of a binary tree)", fn,
                               (long long)t, i, c);
            state[c] = 2;
        }
        state[par] = 1;
    }
    const int ra = root[0], rb = root[1];
    if (ra < 0 || rb < 0 || ra >= n_nodes || rb >= n_nodes || ra == rb || state[ra] != 1 ||
        state[rb] != 1)
        return set_err(nullptr, PU_E_ARG, "%s: tree %lld: root edge (%d, %d) does not join the two "
                       "nodes left without a parent", fn, (long long)t, ra, rb);
    return PU_OK;
}

// An edge list [2n-3][2] with its adjacency.  Row 2 g + side of the directional sets is
// D(edges[g][side] -> edges[g][1 - side]).
struct EdgeTree {
    int n = 0;
    const int32_t *edges = nullptr;
    std::vector<int32_t> adj;  // [2n-2][3][2] = (neighbour, edge id); a tip uses the first only
    std::vector<int32_t> work;

    int row(int from, int g) const { return 2 * g + (edges[2 * g] == from ? 0 : 1); }

    // the edges are a binary tree over tips 0..n-1 and internal nodes n..2n-3, or PU_E_ARG
    int build(const char *fn, int64_t t, int n_taxa, const int32_t *e) {
        n = n_taxa;
        edges = e;
        const int n_nodes = 2 * n - 2, n_edges = 2 * n - 3;
        adj.assign((size_t)n_nodes * 6, -1);
        std::vector<int32_t> &deg = work;
        deg.assign(n_nodes, 0);
        for (int g = 0; g < n_edges; ++g) {
            const int a = e[2 * g], b = e[2 * g + 1];
            if (a < 0 || b < 0 || a >= n_nodes || b >= n_nodes || a == b)
                return set_err(nullptr, PU_E_ARG, "%s: tree %lld edge %d = (%d, %d) of %d nodes",
                               fn, (long long)t, g, a, b, n_nodes);
            for (int v : {a, b}) {
                if (deg[v] >= (v < n ? 1 : 3))
                    return set_err(nullptr, PU_E_ARG, "%s: tree %lld: node %d is on more than %d "
                                   "edge(s) (not a binary tree over the %d rows)", fn,
                                   (long long)t, v, v < n ? 1 : 3, n);
                adj[(size_t)v * 6 + 2 * deg[v]] = v == a ? b : a;
                adj[(size_t)v * 6 + 2 * deg[v] + 1] = g;
                ++deg[v];
            }
        }
        // 2n - 3 edges with these degrees put every node on its full count; connected?
        std::vector<int32_t> seen(n_nodes, 0), todo{0};
        seen[0] = 1;
        int n_seen = 0;
        while (!todo.empty()) {
            const int v = todo.back();
            todo.pop_back();
            ++n_seen;
            for (int j = 0; j < (v < n ? 1 : 3); ++j) {
                const int x = adj[(size_t)v * 6 + 2 * j];
                if (!seen[x]) {
                    seen[x] = 1;
                    todo.push_back(x);
                }
            }
        }
        if (n_seen != n_nodes)
            return set_err(nullptr, PU_E_ARG, "%s: tree %lld: the edges are not connected (not a "
                           "binary tree over the %d rows)", fn, (long long)t, n);
        return PU_OK;
    }

    // k_fitch's schedule, rooted on edge 0: ops [n-2][3], root [2] and per op-order edge the row
    // of its child -> parent set
    void schedule(int32_t *ops, int32_t *root, int32_t *slot) {
        std::vector<int32_t> &order = work;  // (node, came from) in pre-order
        order.clear();
        std::vector<int32_t> todo;
        for (int side = 0; side < 2; ++side) {
            todo.push_back(edges[side]);
            todo.push_back(edges[1 - side]);
            while (!todo.empty()) {
                const int came = todo.back();
                todo.pop_back();
                const int v = todo.back();
                todo.pop_back();
                if (v < n) continue;
                order.push_back(v);
                order.push_back(came);
                for (int j = 0; j < 3; ++j) {
                    const int x = adj[(size_t)v * 6 + 2 * j];
                    if (x != came) {
                        todo.push_back(x);
                        todo.push_back(v);
                    }
                }
            }
        }
        // a node comes before its descendants in `order`: backwards it is a post-order
        int i = 0;
        for (int64_t q = (int64_t)order.size() - 2; q >= 0; q -= 2, ++i) {
            const int v = order[q], came = order[q + 1];
            ops[3 * i] = v;
            int c = 0;
            for (int j = 0; j < 3; ++j) {
                const int x = adj[(size_t)v * 6 + 2 * j], g = adj[(size_t)v * 6 + 2 * j + 1];
                if (x == came) continue;
                ops[3 * i + 1 + c] = x;
                slot[2 * i + c] = row(x, g);
                ++c;
            }
        }
        root[0] = edges[0];
        root[1] = edges[1];
        slot[2 * i] = 0;  // D(edges[0][0] -> edges[0][1])
    }
};

}  // namespace pu
#pragma GCC visibility pop
