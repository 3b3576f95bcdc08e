// pu_plan.cpp -- the traversal planner (pu_plan.h): host code only.
#include "pu_plan.h"

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>

#include "../../include/phylo_hip.h"

namespace pu {
namespace {

int set_err(std::string *err, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (err) *err = buf;
    return code;
}

}  // namespace

PlanKnobs read_plan_knobs() {
    auto env_int = [](const char *name) {
        const char *env = getenv(name);
        return PlanKnobs::Int{env != nullptr, env ? atoi(env) : 0};
    };
    PlanKnobs k;
    k.lds_slots = env_int("PU_LDS_SLOTS");
    k.split = env_int("PU_SPLIT");
    k.lds_pad = env_int("PU_LDS_PAD");
    k.keep_occ = env_int("PU_KEEP_OCC").v;
    const PlanKnobs::Int uses = env_int("PU_CHUNK_USES");
    k.chunk_uses = uses.set ? std::max(2, uses.v) : 0;
    k.force_generic = env_int("PU_FORCE_GENERIC").set;
    k.debug_plan = env_int("PU_DEBUG_PLAN").set;
    return k;
}

int make_plan(const PlanInput &in, int L, bool reorder, bool keep_all, Plan &pl,
              std::string *err, int split) {
    const int N = in.n_nodes, n_ops = in.n_ops, root_a = in.root_a, root_b = in.root_b;
    const int32_t *ops = in.ops;
    const int *tip_slot = in.tip_slot;
    std::vector<int> prod(N, -1), cons_count(N, 0);
    for (int o = 0; o < n_ops; ++o) {
        const int p = ops[3 * o], a = ops[3 * o + 1], b = ops[3 * o + 2];
        if (p < 0 || p >= N || a < 0 || a >= N || b < 0 || b >= N || a == b || p == a ||
            p == b)
            return set_err(err, PU_E_SCHED, "op %d (%d,%d,%d): node index out of range "
                           "or repeated (n_nodes=%d)", o, p, a, b, N);
        if (prod[p] >= 0)
            return set_err(err, PU_E_SCHED, "node %d is the parent of ops %d and %d", p,
                           prod[p], o);
        prod[p] = o;
        cons_count[a]++;
        cons_count[b]++;
    }
    if (root_a < 0 || root_a >= N || root_b < 0 || root_b >= N || root_a == root_b)
        return set_err(err, PU_E_SCHED, "bad root edge (%d,%d)", root_a, root_b);
    cons_count[root_a]++;
    cons_count[root_b]++;
    for (int v = 0; v < N; ++v) {
        if (prod[v] >= 0 && cons_count[v] != 1)
            return set_err(err, PU_E_SCHED, "internal node %d is consumed %d times "
                           "(expected once)", v, cons_count[v]);
        if (prod[v] < 0 && cons_count[v] > 1)
            return set_err(err, PU_E_SCHED, "tip node %d is consumed %d times", v,
                           cons_count[v]);
    }
    // order
    pl.order.clear();
    if (!reorder) {
        for (int o = 0; o < n_ops; ++o) {
            for (int k = 1; k <= 2; ++k) {
                const int ch = ops[3 * o + k];
                if (prod[ch] >= o)
                    return set_err(err, PU_E_SCHED, "op %d reads node %d before it is "
                                   "computed (not a post-order)", o, ch);
            }
            pl.order.push_back(o);
        }
    } else {
        // need[] bottom-up without recursion (depth can reach N for caterpillars)
        std::vector<int> need(N, 0), state(N, 0);
        std::vector<int> stack;
        auto visit_need = [&](int root) -> int {
            stack.push_back(root);
            while (!stack.empty()) {
                const int v = stack.back();
                if (prod[v] < 0) {
                    need[v] = 0;
                    state[v] = 2;
                    stack.pop_back();
                    continue;
                }
                const int o = prod[v], a = ops[3 * o + 1], b = ops[3 * o + 2];
                if (state[v] == 0) {
                    state[v] = 1;
                    if (state[a] == 1 || state[b] == 1) return -1;  // cycle
                    if (state[a] == 0) stack.push_back(a);
                    if (state[b] == 0) stack.push_back(b);
                    continue;
                }
                stack.pop_back();
                if (state[v] == 2) continue;
                const int na = need[a], nb = need[b];
                need[v] = na == nb ? na + 1 : std::max(na, nb);
                state[v] = 2;
            }
            return 0;
        };
        if (visit_need(root_a) < 0 || visit_need(root_b) < 0)
            return set_err(err, PU_E_SCHED, "schedule contains a cycle");
        int reached = 0;
        // emit post-order, larger-need child first
        auto emit = [&](int root) {
            std::vector<std::pair<int, int>> st;  // (node, phase)
            st.push_back({root, 0});
            while (!st.empty()) {
                auto [v, ph] = st.back();
                st.pop_back();
                if (prod[v] < 0) continue;
                const int o = prod[v], a = ops[3 * o + 1], b = ops[3 * o + 2];
                if (ph == 0) {
                    st.push_back({v, 1});
                    const int first = need[a] >= need[b] ? a : b;
                    const int second = first == a ? b : a;
                    st.push_back({second, 0});
                    st.push_back({first, 0});
                } else {
                    pl.order.push_back(o);
                    ++reached;
                }
            }
        };
        const int fa = need[root_a] >= need[root_b] ? root_a : root_b;
        emit(fa);
        emit(fa == root_a ? root_b : root_a);
        if (reached != n_ops)
            return set_err(err, PU_E_SCHED, "%d of %d ops are not below the root edge",
                           n_ops - reached, n_ops);
    }
    // Split into tasks.  The post-order is one dependency chain per (tile, category) wave;
    // with few waves per SIMD its length sets the time of the SIMDs that carry one wave more
    // than the average.  Disjoint subtrees ("chains", about n_ops / split ops each) are
    // independent: a first launch runs every chain as a wave task of its own, a second the ops
    // above them (the "top": ancestors of the cut nodes, then the root combine), reading the
    // chain roots back from HBM.  Cuts: starting from the root's children, the largest subtree
    // is replaced by its children's while it exceeds the target (bounded top and task count).
    std::vector<int> region(n_ops + 1, 0);  // device op -> task (the top task is the last)
    pl.tasks.clear();
    pl.top_lo = 0;
    if (split > 1 && reorder && n_ops > 2) {
        std::vector<int> size(N, 0), parent(N, -1);
        for (int o : pl.order) {
            const int p = ops[3 * o], a = ops[3 * o + 1], b = ops[3 * o + 2];
            size[p] = 1 + size[a] + size[b];
            parent[a] = parent[b] = p;
        }
        std::vector<int> cuts;
        for (int r : {root_a, root_b})
            if (prod[r] >= 0) cuts.push_back(r);
        std::vector<char> is_top(N, 0);
        const int target = (n_ops + split - 1) / split;
        // at most n_ops / 16 top ops and 32 chains (r03 sweeps: no better value; cfg4 8 / 16 / 32
        // / 64 chains 3.70 / 3.44 / 3.37 / 3.38 ms)
        const int max_top = std::max(1, n_ops / 16);
        const size_t max_chains = 32;
        int n_top = 0;
        while (!cuts.empty()) {
            auto it = std::max_element(cuts.begin(), cuts.end(),
                                       [&](int x, int y) { return size[x] < size[y]; });
            if (size[*it] <= target || n_top >= max_top || cuts.size() >= max_chains) break;
            const int v = *it;
            cuts.erase(it);
            is_top[v] = 1;
            ++n_top;
            for (int k = 1; k <= 2; ++k) {
                const int ch = ops[3 * prod[v] + k];
                if (prod[ch] >= 0) cuts.push_back(ch);
            }
        }
        if (cuts.size() >= 2) {
            // longest chain first: the dispatcher hands out workgroups in block order
            std::stable_sort(cuts.begin(), cuts.end(),
                             [&](int x, int y) { return size[x] > size[y]; });
            std::vector<int> chain_of(N, -1), rank(N, -1);
            for (size_t k = 0; k < cuts.size(); ++k) rank[cuts[k]] = (int)k;
            for (int t = n_ops - 1; t >= 0; --t) {  // parents before children
                const int v = ops[3 * pl.order[t]];
                chain_of[v] = is_top[v] ? -1 : rank[v] >= 0 ? rank[v] : chain_of[parent[v]];
            }
            std::vector<int> order;
            order.reserve(n_ops);
            for (size_t k = 0; k < cuts.size(); ++k) {
                const int lo = (int)order.size();
                for (int o : pl.order)
                    if (chain_of[ops[3 * o]] == (int)k) order.push_back(o);
                pl.tasks.push_back({lo, (int)order.size()});
            }
            pl.top_lo = (int)order.size();
            for (int o : pl.order)
                if (chain_of[ops[3 * o]] < 0) order.push_back(o);
            pl.order = std::move(order);
            for (size_t k = 0; k < pl.tasks.size(); ++k)
                for (int t = pl.tasks[k].first; t < pl.tasks[k].second; ++t) region[t] = (int)k;
            for (int t = pl.top_lo; t <= n_ops; ++t) region[t] = (int)pl.tasks.size();
        }
    }
    const bool split_on = !pl.tasks.empty();
    const int top_region = (int)pl.tasks.size();
    // lifetimes in device order (root combine = time n_ops)
    std::vector<int> t_prod(N, -1), t_cons(N, -1);
    for (int t = 0; t < n_ops; ++t) {
        const int o = pl.order[t];
        t_prod[ops[3 * o]] = t;
        t_cons[ops[3 * o + 1]] = t;
        t_cons[ops[3 * o + 2]] = t;
    }
    t_cons[root_a] = n_ops;
    t_cons[root_b] = n_ops;
    // Child kinds: a tip, the previous op's parent (the kernel's "current" registers), a
    // waiting parent in an LDS stash slot, or one read back from HBM.  A parent waits when
    // its consumer is not the next op; at each production, if more parents wait than
    // there are L stash slots, the one whose consumer is latest stays in HBM (Belady,
    // optimal for intervals); stash slots are then assigned by interval colouring.
    std::vector<char> waits(N, 0), in_lds(N, 0);
    for (int t = 0; t < n_ops; ++t) {
        const int v = ops[3 * pl.order[t]];
        waits[v] = t_cons[v] != t + 1 || region[t_cons[v]] != region[t];
    }
    // the LDS stash serves values produced and consumed inside one chain task (the top task
    // reads every waiting parent back from HBM)
    auto stashable = [&](int v) {
        return !split_on || (region[t_prod[v]] != top_region &&
                             region[t_cons[v]] == region[t_prod[v]]);
    };
    // The stash serves DFS orders, where a waiting parent is always paired with the
    // current one (PAT_LC).  Other caller orders read every waiting parent back from HBM.
    auto dfs_pair = [&](int t, int a, int b) {
        for (int x : {a, b})
            if (prod[x] >= 0 && waits[x]) {
                const int y = x == a ? b : a;
                if (prod[y] < 0 || t_prod[y] != t - 1) return false;
            }
        return true;
    };
    for (int t = 0; t <= n_ops && L > 0; ++t) {
        if (split_on && region[t] == top_region) continue;
        const int a = t < n_ops ? ops[3 * pl.order[t] + 1] : root_a;
        const int b = t < n_ops ? ops[3 * pl.order[t] + 2] : root_b;
        if (!dfs_pair(t, a, b)) L = 0;
    }
    pl.max_live = 0;
    {
        std::vector<int> waiting, live;
        for (int t = 0; t < n_ops; ++t) {
            auto gone = [&](int x) { return t_cons[x] <= t; };
            waiting.erase(std::remove_if(waiting.begin(), waiting.end(), gone), waiting.end());
            live.erase(std::remove_if(live.begin(), live.end(), gone), live.end());
            const int v = ops[3 * pl.order[t]];
            if (!waits[v]) continue;
            waiting.push_back(v);
            pl.max_live = std::max(pl.max_live, (int)waiting.size());
            if (L == 0 || !stashable(v)) continue;
            live.push_back(v);
            in_lds[v] = 1;
            if ((int)live.size() > L) {
                auto it = std::max_element(live.begin(), live.end(), [&](int x, int y) {
                    return t_cons[x] < t_cons[y];
                });
                in_lds[*it] = 0;
                live.erase(it);
            }
        }
    }
    std::vector<int> lds_slot(N, -1);
    {
        std::vector<int> busy(std::max(L, 1), -1);
        for (int t = 0; t < n_ops; ++t) {
            const int v = ops[3 * pl.order[t]];
            if (!in_lds[v]) continue;
            for (int r = 0; r < L; ++r)
                if (busy[r] <= t) {  // the previous occupant was read at op busy[r]
                    busy[r] = t_cons[v];
                    lds_slot[v] = r;
                    break;
                }
            if (lds_slot[v] < 0)
                return set_err(err, PU_E_SCHED, "LDS stash planner overflow");
        }
    }
    // storage slots: KEEP -- every internal node; LNL_ONLY -- only parents read back from
    // HBM, slots reused by interval colouring
    pl.store_slot.assign(N, -1);
    if (keep_all) {
        int s = 0;
        for (int v = 0; v < N; ++v)
            if (prod[v] >= 0) pl.store_slot[v] = s++;
        pl.n_store = s;
    } else {
        // interval colouring; a split plan colours each task apart (disjoint slot ranges):
        // chain tasks run concurrently, so no slot may pass from one chain's value to another's
        int base = 0;
        const int n_regions = split_on ? top_region + 1 : 1;
        for (int r = 0; r < n_regions; ++r) {
            std::vector<int> busy_until;
            for (int t = 0; t < n_ops; ++t) {
                if (split_on && region[t] != r) continue;
                const int v = ops[3 * pl.order[t]];
                if (!waits[v] || in_lds[v]) continue;
                int slot = -1;
                for (size_t k = 0; k < busy_until.size(); ++k)
                    if (busy_until[k] <= t) {  // the op that reads it writes after its reads
                        slot = (int)k;
                        break;
                    }
                if (slot < 0) {
                    slot = (int)busy_until.size();
                    busy_until.push_back(0);
                }
                busy_until[slot] = t_cons[v];
                pl.store_slot[v] = base + slot;
            }
            base += (int)busy_until.size();
        }
        pl.n_store = base;
    }
    // descriptors: canonical child order -- waiting parent first, then the current parent,
    // then tips; swap[t] records that the caller's (child 1, child 2) became (b, a)
    enum { K_WAIT, K_CUR, K_TIP };
    auto kind_at = [&](int node, int t) {
        if (prod[node] < 0) return (int)K_TIP;
        return t_prod[node] == t - 1 && region[t - 1] == region[t] ? (int)K_CUR : (int)K_WAIT;
    };
    pl.n_mem = pl.n_tip = pl.n_cur = pl.n_lds = 0;
    pl.descs.assign(n_ops + 1, OpDesc{-1, 0, 0, 0, -1, 0, 0});
    pl.swap.assign(n_ops + 1, 0);
    auto describe = [&](int t, int a, int b, int par_slot, int dst) -> int {
        int ka = kind_at(a, t), kb = kind_at(b, t);
        const bool swp = kb < ka;
        if (swp) {
            std::swap(a, b);
            std::swap(ka, kb);
        }
        int pat, ia = 0, ib = 0;
        if (ka == K_WAIT && kb == K_CUR) {
            pat = in_lds[a] ? pu::PAT_LC : pu::PAT_MC;
            ia = in_lds[a] ? lds_slot[a] : pl.store_slot[a];
        } else if (ka == K_CUR && kb == K_TIP) {
            pat = pu::PAT_CT;
            ib = tip_slot[b];
        } else if (ka == K_TIP && kb == K_TIP) {
            pat = pu::PAT_TT;
            ia = tip_slot[a];
            ib = tip_slot[b];
        } else if (ka == K_WAIT && !in_lds[a] && kb == K_TIP) {
            pat = pu::PAT_MT;
            ia = pl.store_slot[a];
            ib = tip_slot[b];
        } else if (ka == K_WAIT && !in_lds[a] && kb == K_WAIT && !in_lds[b]) {
            pat = pu::PAT_MM;
            ia = pl.store_slot[a];
            ib = pl.store_slot[b];
        } else {
            // a stashed parent that is not paired with the current one (not a DFS order)
            return set_err(err, PU_E_SCHED, "op %d: child pair not supported", t);
        }
        for (int k : {ka, kb}) {
            if (k == K_TIP) pl.n_tip++;
            if (k == K_CUR) pl.n_cur++;
        }
        for (int n : {a, b})
            if (prod[n] >= 0 && kind_at(n, t) == K_WAIT) (in_lds[n] ? pl.n_lds : pl.n_mem)++;
        pl.descs[t] = OpDesc{par_slot, pat, ia, ib, dst, 0, 0};
        pl.swap[t] = swp;
        return PU_OK;
    };
    for (int t = 0; t < n_ops; ++t) {
        const int o = pl.order[t];
        const int p = ops[3 * o], a = ops[3 * o + 1], b = ops[3 * o + 2];
        int slot = pl.store_slot[p];
        // a stored value that a later op reads back from HBM is written through the
        // caches; everything else is streamed
        if (slot >= 0 && waits[p] && !in_lds[p]) slot |= pu::kReadBack;
        if (int rc = describe(t, a, b, slot, lds_slot[p])) return rc;
    }
    if (int rc = describe(n_ops, root_a, root_b, -1, -1)) return rc;
    return PU_OK;
}

int tip_uses(int pat) { return pat == PAT_TT ? 2 : (pat == PAT_CT || pat == PAT_MT) ? 1 : 0; }

// Tip uses in device op order (child a before child b), grouped into staging chunks of at
// most kChunkOps ops and about kChunkUses tip uses: the traversal stages one chunk's tip
// codes in LDS at a time, and the fewer bytes that takes, the more workgroups fit a CU.
// the chunking: tip uses in order (seq), first use and first op of every chunk; returns the
// largest number of uses in a chunk (>= 1)
// (a task of a split plan starts a chunk: `breaks`, ascending op indices)
// (cap: the uses target, 0 = kChunkUses; PU_CHUNK_USES overrides both)
static int chunk_schedule(const PlanKnobs &kn, const std::vector<OpDesc> &descs, std::vector<int> &seq,
                   std::vector<int> &tip0, std::vector<int> &op0,
                   const std::vector<int> &breaks = {}, int cap = 0) {
    const int n = (int)descs.size();
    int maxu = 0, start = 0;
    size_t nb = 0;
    const int cap_uses = kn.chunk_uses ? kn.chunk_uses : cap > 0 ? cap : pu::kChunkUses;
    for (int t = 0; t < n; ++t) {
        const OpDesc &d = descs[t];
        const int uses = tip_uses(d.pat);
        const bool brk = nb < breaks.size() && breaks[nb] == t;
        if (brk) ++nb;
        if (t == 0 || brk || t - start == pu::kChunkOps ||
            (int)seq.size() - tip0.back() + uses > cap_uses) {
            if (t > 0) maxu = std::max(maxu, (int)seq.size() - tip0.back());
            op0.push_back(t);
            tip0.push_back((int)seq.size());
            start = t;
        }
        if (d.pat == pu::PAT_TT) seq.push_back(d.ia);
        if (uses > 0) seq.push_back(d.ib);
    }
    maxu = std::max(maxu, (int)seq.size() - tip0.back());
    op0.push_back(n);
    tip0.push_back((int)seq.size());
    return std::max(maxu, 1);
}

// A CU's 160 KiB of LDS, less a byte, is shared in 512-byte allocation granules: the rounds of
// workgroups a grid takes at per_cu workgroups per CU, or as many as the LDS request allows
constexpr size_t kLdsCap = 160 * 1024 - 1, kLdsGran = 512;
static int rounds(int grid, size_t lds, int per_cu, int n_cu) {
    const int by_lds = lds ? (int)(kLdsCap / ((lds + kLdsGran - 1) / kLdsGran * kLdsGran)) : 8;
    const int slots = std::max(1, std::min(per_cu, by_lds)) * n_cu;
    return (grid + slots - 1) / slots;
}

// Occupancy-aware build choice for k_prune plans outside the KEEP occupancy rule (lnL-only,
// caller orders, explicit slots).  The default build needs ~106 SGPRs: with the 16 the hardware
// adds per wave that is 6 waves per SIMD (scripts/probes/occupancy_probe.hip); the 7-wave build
// trims SGPRs with a few spills to VGPR lanes, which costs latency per op.  It is chosen only
// when it saves a round of workgroups, and only for the tip-product lnL-only variant (the one
// other variant built for 7 waves is the KEEP occupancy plan's, pu_kernels.hip).
int pick_waves(int K, int n_cu, size_t lds, int grid) {
    if (K > 4) return 0;
    return rounds(grid, lds, 7, n_cu) < rounds(grid, lds, 6, n_cu) ? 7 : 0;
}

// ---------------------------------------------------------------- KEEP occupancy (r04)
// A DNA KEEP traversal is a store stream: every op writes each workgroup's 4 x 64 lanes x
// (K + 1) doubles once.  How fast HBM absorbs it depends on how many workgroups share a CU,
// which the LDS request sets (k per CU for a request of at most lds_cap_for(k) bytes; the
// default build's 106 SGPRs allow 6 waves per SIMD, the 7- and 8-wave builds spill SGPRs).
//
// Measured (r04 sweeps, profiles/r04_occ_*.txt; k_prune ms, min of 2-3 interleaved rounds):
// * the store stream runs fastest at 4 workgroups per CU with the spill-free default build:
//   cfg4 (1000 taxa x 125k sites, 1954 workgroups) 2.58 / 2.84-3.11 ms on two boxes, against
//   3.34-4.05 at 3, 5 or 6 per CU, 3.76 with the 8-wave build and 3.13-3.38 for the r03 split
//   plan; 200 / 500 taxa at 100k-125k sites likewise;
// * what remains is batch arithmetic.  Every CU receives n = ceil(grid / CUs) workgroups and
//   runs them in ceil(n / k) batches.  At 4 per CU, n = 5 or 6 leaves a last batch of 1-2
//   workgroups per CU that takes nearly a full batch's time (latency, not bandwidth): 50 taxa
//   at 74k-82k sites 0.104 ms at 4 per CU, 0.088-0.091 with the 7-wave build at 7 per CU (one
//   batch); 100 taxa at 75k / 90k 0.208 / 0.205 against 0.178-0.193 / 0.200.  At n = 7 the
//   last 4-per-CU batch is 3/4 full and the two are level (cfg2: 0.1173 vs 0.1220); for
//   n <= 4 or n >= 7 every k in 4..8 is within the 5-10 % that the same plan varies between
//   two allocations in one process (cfg4: 2.84 vs 3.10 ms), except the spilling 7- / 8-wave
//   builds below 4 per CU (50 taxa at 40k-65k: 0.078-0.100 vs 0.058-0.071 ms).
// So: 4 per CU and the most stash slots that fit 40 KB, unless n is 5 or 6 -- then the 7-wave
// build at 7 per CU runs every workgroup in one batch.

// largest LDS request (bytes, a multiple of the 512-byte allocation granule) that still lets
// k workgroups share a CU's 160 KiB
size_t lds_cap_for(int k) { return kLdsCap / k / kLdsGran * kLdsGran; }

// workgroups per CU of the chosen plan (see above); n: ceil(grid / CUs)
static int keep_per_cu(int n) { return (n == 5 || n == 6) ? 7 : 4; }

// the dynamic LDS of a plan with nl stash slots (staging chunks: see chunk_schedule)
static size_t lds_of(const PlanInput &in, const Plan &p, int nl,
                     const std::vector<int> &breaks = {}, int cap = 0) {
    std::vector<int> s1, t1, o1;
    return in.lds_bytes(in.K, in.C, in.n_codes,
                        chunk_schedule(in.knobs, p.descs, s1, t1, o1, breaks, cap),
                        in.coded_tips, nl);
}

// fills out.plan, L, r_slots, lds_pad, waves and occ_k (0: no slot fits)
static int keep_occupancy(const PlanInput &in, int grid, Schedule &out, std::string *err) {
    constexpr int kMaxSlots = 5;
    // LDS of 1..kMaxSlots stash slots (the tip-code chunking, and so the rest of the LDS, does
    // not depend on the slot count)
    Plan p1;
    if (int rc = make_plan(in, 1, true, true, p1, err)) return rc;
    size_t lds[kMaxSlots + 1] = {0};
    for (int L = 1; L <= kMaxSlots; ++L) lds[L] = lds_of(in, p1, L);
    const int forced = in.knobs.keep_occ;
    if (forced && (forced < 3 || forced > 7))
        return set_err(err, PU_E_ARG, "PU_KEEP_OCC must be in [3, 7]");
    const int n = (grid + in.n_cu - 1) / in.n_cu;
    int best_k = 0, best_L = 0;
    for (int k : {forced ? forced : keep_per_cu(n), 4}) {  // (4: if the first does not fit)
        const size_t cap = lds_cap_for(k);
        for (int l = kMaxSlots; l >= 1 && !best_L; --l)
            if (lds[l] <= cap) best_L = l;
        if (best_L) {
            best_k = k;
            break;
        }
    }
    if (!best_k) {  // not even one slot fits (huge code tables): the planner's default
        out.occ_k = out.L = out.r_slots = out.lds_pad = 0;
        out.waves = -1;
        return make_plan(in, 0, true, true, out.plan, err);
    }
    // stash overflow left: the default build also keeps two waiting parents in registers
    // (TV_RSLOTS); the spilling 7- / 8-wave builds do not
    Plan pL;
    if (int rc = make_plan(in, best_L, true, true, pL, err)) return rc;
    const int R = (best_k <= 6 && pL.n_mem > 0) ? 2 : 0;
    if (int rc = make_plan(in, best_L + R, true, true, out.plan, err)) return rc;
    out.occ_k = best_k;
    out.L = best_L;
    out.r_slots = R;
    // the pad from the final plan's own LDS (its chunking matches p1's, so this is lds[best_L];
    // computed again so that a planner change cannot leave the pad sized for another plan)
    const size_t lds_final = lds_of(in, out.plan, best_L);
    if (lds_final > lds_cap_for(best_k))
        return set_err(err, PU_E_STATE, "occupancy plan: %zu LDS bytes exceed %zu", lds_final,
                       lds_cap_for(best_k));
    out.lds_pad = (int)(lds_cap_for(best_k) - lds_final);
    out.waves = best_k <= 6 ? 1 : 7;
    return PU_OK;
}

int plan_schedule(const PlanInput &in, Schedule &out, std::string *err) {
    const PlanKnobs &kn = in.knobs;
    const int n_ops = in.n_ops;
    const bool keep = !(in.flags & PU_LNL_ONLY);
    const bool reorder = !(in.flags & PU_NO_REORDER);
    out = Schedule();
    Plan &pl = out.plan;
    int &L = out.L;
    L = kn.lds_slots.set ? kn.lds_slots.v : in.K == 20 ? 3 : 2;
    if (L < 0 || L > 8) return set_err(err, PU_E_ARG, "PU_LDS_SLOTS must be in [0, 8]");
    // protein KEEP traversals: chain tasks + a top task (make_plan).  cfg3 (2512 waves, 2.45
    // per SIMD): 0.380 -> 0.330 ms with a target of n_ops / 3 (r03 sweep of 2 / 3 / 4 / 8);
    // 12288 sites (exactly 3 waves per SIMD) unchanged.  PU_SPLIT=0 or 1: one task.
    // DNA plans: see the occupancy rule below
    int split = kn.split.set ? kn.split.v : in.K == 20 ? 3 : 0;
    // (the protein kernel's wait-for-zero check mode has no chain tasks)
    if (in.K == 20 && kn.force_generic) split = 0;
    int rc = make_plan(in, L, reorder, keep, pl, err, split);
    if (rc) return rc;
    out.n_tiles = (int)tile_count(in.S);
    out.grid = (int)((tile_count(in.S) * in.C + 3) / 4);
    // Occupancy.  When the default plan needs a second round of workgroups (cfg4's 125k-site
    // shard), a KEEP plan of >= 128 ops is split into chain tasks of about 100 ops (a split
    // plan's grid is dealt in many short rounds, so two stash slots and the default build no
    // longer cost a round): cfg4 4.16-4.30 -> 3.29-3.61 ms (r03 sweep: targets n/2..n/16, 0-3
    // slots, 1 / 7 / 8 waves); at 125k sites 200 / 400 taxa 0.849 -> 0.758 / 1.609 -> 1.493 ms,
    // 100 taxa even, 50 taxa (131k sites) 0.213 -> 0.282 ms, hence the 128-op floor.
    // Otherwise (short trees, lnL-only, caller order) a plan with one stash slot and the 8-wave
    // build may fit the grid in one round (r02: cfg4 4.58 -> 4.31 ms); cfg2 fits one round with
    // the default plan.
    // DNA KEEP plans (r04): an occupancy plan -- k workgroups per CU, the most LDS stash slots
    // that fit k, the build that allows k -- chosen by keep_occupancy (above).  PU_KEEP_OCC=k
    // forces k (sweeps); the env overrides of the slots, split, waves or pad bypass it.
    const bool occ_plan = keep && in.K <= 4 && reorder && !kn.lds_slots.set && !kn.split.set &&
                          !kn.lds_pad.set;
    if (occ_plan) {
        if ((rc = keep_occupancy(in, out.grid, out, err))) return rc;
        if (kn.debug_plan)
            fprintf(stderr, "[pu plan] KEEP S=%lld ops=%d grid=%d: %d per CU, %d stash slots "
                    "+ %d register slots (%d read-backs), build %d, pad %d B (%d workgroups per "
                    "CU in all)\n", (long long)in.S, n_ops, out.grid, out.occ_k, L, out.r_slots,
                    pl.n_mem, out.waves, out.lds_pad,
                    out.occ_k ? (out.grid + in.n_cu - 1) / in.n_cu : 0);
    } else if (!kn.lds_slots.set && in.K <= 4 && L > 1) {
        const size_t lds_def = lds_of(in, pl, L);
        if (std::min(rounds(out.grid, lds_def, 6, in.n_cu),
                     rounds(out.grid, lds_def, 7, in.n_cu)) > 1) {
            Plan p1;
            std::string unused;
            if (reorder && !kn.split.set && n_ops >= 128 &&
                make_plan(in, L, reorder, keep, p1, &unused, std::max(2, n_ops / 100)) == PU_OK &&
                !p1.tasks.empty()) {
                pl = std::move(p1);
                out.waves = 1;  // the default build
            }
        }
    }
    if (kn.lds_pad.set) out.lds_pad = kn.lds_pad.v;  // an experiment knob (scripts/sweep.py)
    std::vector<int> breaks;  // the task boundaries of a split plan, ascending
    for (const auto &r : pl.tasks) breaks.push_back(r.first);
    if (!pl.tasks.empty()) breaks.push_back(pl.top_lo);
    // Protein plans (r05 late): the kernel's 114-119 VGPRs allow 4 waves per SIMD, but 3 LDS
    // stash slots (36 KB) + the code table + a chunk of ~32 tip uses' codes take just over
    // 40 KB, so only 3 workgroups fit a CU.  Shorter staging chunks (more, cheaper barriers)
    // fit the fourth: cfg3 traversal 0.325-0.327 -> 0.316-0.318 ms at 8 uses per chunk on one
    // box (scripts/r05/exp39_cfg3_chunks.sh).  The largest chunk target >= 8 that fits 4 per CU.
    if (in.K == 20 && in.coded_tips && !kn.chunk_uses) {
        auto lds_at = [&](int cap) { return lds_of(in, pl, L, breaks, cap); };
        // 4 per CU, measured (scripts/r05/exp47_cfg3_occupancy.sh: resident waves per CU from
        // SQ_WAVE_CYCLES / SQ_BUSY_CU_CYCLES): 40.6 KB of dynamic LDS (8 uses) fits 4, 40.9 KB
        // (13 uses) does not -- so the kernel's static LDS and a 1 KB margin are counted
        auto fits4 = [](size_t lds) { return 4 * ((lds + 64 + 255) / 256 * 256) <= 163840 - 1024; };
        if (!fits4(lds_at(pu::kChunkUses)))
            for (int cap = pu::kChunkUses - 1; cap >= 8; --cap)
                if (fits4(lds_at(cap))) {
                    out.chunk_cap = cap;
                    break;
                }
    }
    // the staging chunks and every op's first tip use inside its chunk
    std::vector<int> &op0 = out.op0, &tip0 = out.tip0;
    out.max_chunk_uses = chunk_schedule(kn, pl.descs, out.seq, tip0, op0, breaks, out.chunk_cap);
    int used = 0;
    for (size_t k = 0; k + 1 < op0.size(); ++k)
        for (int t = op0[k]; t < op0[k + 1]; ++t) {
            pl.descs[t].use0 = used - tip0[k];
            used += tip_uses(pl.descs[t].pat);
        }
    if (!pl.tasks.empty()) {
        auto chunk_at = [&](int t) {
            return (int)(std::lower_bound(op0.begin(), op0.end(), t) - op0.begin());
        };
        std::vector<int> &tk = out.tasks;
        for (const auto &r : pl.tasks)
            tk.insert(tk.end(), {r.first, r.second, chunk_at(r.first), chunk_at(r.second)});
        tk.insert(tk.end(), {pl.top_lo, n_ops, chunk_at(pl.top_lo), (int)op0.size() - 1});
        for (size_t k = 0; k + 1 < tk.size() / 4; ++k)
            if (op0[tk[4 * k + 2]] != tk[4 * k] || op0[tk[4 * k + 3]] != tk[4 * k + 1])
                return set_err(err, PU_E_SCHED, "split plan: task %zu does not start a chunk", k);
    }
    // skip-zero scalers need one writer per slot and run (kept partials); HBM read-backs
    // need the general kernel variant
    int &variant = out.variant;
    variant = keep ? pu::TV_SKIP_ZERO_SCALE : 0;
    for (const OpDesc &d : pl.descs)  // (the K = 20 kernel reads back in every mode)
        if (in.K != 20 && (d.pat == pu::PAT_MC || d.pat == pu::PAT_MT || d.pat == pu::PAT_MM))
            variant |= pu::TV_GENERIC;
    if (kn.force_generic) variant |= pu::TV_GENERIC;
    // a split DNA plan: the top task reads the chain roots back (K = 20: a.tasks selects it)
    if (in.K != 20 && !pl.tasks.empty()) variant |= pu::TV_GENERIC | pu::TV_CHAIN;
    // the protein kernel's waits count on every op storing its parent (KEEP)
    for (int t = 0; t < n_ops; ++t) out.n_store_ops += pl.descs[t].par_slot >= 0;
    if (out.n_store_ops == n_ops) variant |= pu::TV_KEEP;
    if (out.r_slots) variant |= pu::TV_RSLOTS;
    return PU_OK;
}

}  // namespace pu
