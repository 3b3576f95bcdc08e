// plan_check.cpp -- a stand-alone host check of the whole traversal plan (csrc/pu_plan.h).
// Links pu_plan.o and nothing else of the library; tests/test_plan.py builds and runs it.
//
// The LDS function it hands the planner is a stub of its own (stub_lds), sized so that every
// rule has both outcomes among the cases; it is NOT the kernels' byte count.  What is checked
// is the structure of the plan: sources, chunks, tasks, slot lifetimes, pad, build and variant.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <random>
#include <string>
#include <vector>

#include "../include/phylo_hip.h"
#include "../phylo_utils_amd/csrc/pu_plan.h"

using namespace pu;

static int g_fail = 0, g_cases = 0;
static std::string g_case;
#define CHECK(cond, ...)                                       \
    do {                                                       \
        if (!(cond)) {                                         \
            if (++g_fail <= 20) {                              \
                fprintf(stderr, "FAIL [%s] %s: ", g_case.c_str(), #cond); \
                fprintf(stderr, __VA_ARGS__);                  \
                fprintf(stderr, "\n");                         \
            }                                                  \
        }                                                      \
    } while (0)

// per stash slot one CLV of the workgroup's 4 waves (DNA) or 12 KB (protein), the code table,
// the staged codes
static size_t stub_lds(int K, int C, int n_codes, int max_chunk_uses, bool coded, int n_lds) {
    (void)C;
    const size_t slot = K == 20 ? 12288 : (size_t)4 * 64 * (K + 1) * 8;
    return n_lds * slot + (coded ? (size_t)n_codes * K * 8 : 0) +
           (size_t)max_chunk_uses * (K == 20 ? 16 : 256);
}

struct Tree {
    int n_nodes = 0, n_ops = 0, root_a = 0, root_b = 0;
    std::vector<int32_t> ops;
    std::vector<int> tip_slot;
};

// tips 0..n-1 joined at random: the ops come in a valid post-order that is not a DFS order
static Tree random_tree(int n_tips, unsigned seed) {
    std::mt19937 rng(seed);
    Tree t;
    t.n_nodes = 2 * n_tips - 2;
    t.n_ops = n_tips - 2;
    std::vector<int> live(n_tips);
    for (int i = 0; i < n_tips; ++i) live[i] = i;
    std::shuffle(live.begin(), live.end(), rng);
    t.tip_slot.assign(t.n_nodes, -1);
    for (int i = 0; i < n_tips; ++i) t.tip_slot[live[i]] = i;
    for (int p = n_tips; live.size() > 2; ++p) {
        int ab[2];
        for (int &x : ab) {
            const size_t i = rng() % live.size();
            x = live[i];
            live.erase(live.begin() + i);
        }
        t.ops.insert(t.ops.end(), {p, ab[0], ab[1]});
        live.push_back(p);
    }
    t.root_a = live[0];
    t.root_b = live[1];
    return t;
}

static PlanInput input_of(const Tree &t, int K, int flags, int n_per_cu, const PlanKnobs &kn) {
    PlanInput in(t.n_nodes, t.tip_slot.data(), t.n_ops, t.ops.data(), t.root_a, t.root_b);
    in.K = K;
    in.C = 4;
    in.n_codes = K == 20 ? 22 : 16;
    in.flags = flags;
    in.n_cu = 256;
    in.S = (int64_t)(256 * n_per_cu - 100) * 64;  // C = 4: one workgroup per tile
    in.coded_tips = true;
    in.lds_bytes = stub_lds;
    in.knobs = kn;
    return in;
}

static void check_schedule(const PlanInput &in, const Schedule &sc) {
    const Plan &pl = sc.plan;
    const int n_ops = in.n_ops, N = in.n_nodes;
    const bool keep = !(in.flags & PU_LNL_ONLY);
    const int n_stash = sc.L + sc.r_slots;
    CHECK((int)pl.descs.size() == n_ops + 1 && (int)pl.order.size() == n_ops &&
              (int)pl.swap.size() == n_ops + 1, "sizes");
    CHECK(sc.n_tiles == (int)tile_count(in.S) && sc.grid == (sc.n_tiles * in.C + 3) / 4, "grid");
    // device order: a permutation; production and consumption times (root combine: n_ops)
    std::vector<int> seen(n_ops, 0), t_prod(N, -1), t_cons(N, -1);
    for (int t = 0; t < n_ops; ++t) {
        const int o = pl.order[t];
        CHECK(o >= 0 && o < n_ops && !seen[o]++, "order[%d] = %d", t, o);
        t_prod[in.ops[3 * o]] = t;
        t_cons[in.ops[3 * o + 1]] = t_cons[in.ops[3 * o + 2]] = t;
    }
    t_cons[in.root_a] = t_cons[in.root_b] = n_ops;
    // tasks: contiguous chains, then the top; every task starts a chunk
    std::vector<int> region(n_ops + 1, 0);
    const int n_chains = (int)pl.tasks.size();
    CHECK(sc.tasks.size() == (n_chains ? 4 * (size_t)(n_chains + 1) : 0), "task table size");
    if (n_chains && sc.tasks.size() == 4 * (size_t)(n_chains + 1)) {
        int at = 0;
        for (int k = 0; k <= n_chains; ++k) {
            const int *tk = &sc.tasks[4 * k];
            CHECK(tk[0] == at && tk[1] >= tk[0], "task %d ops [%d,%d) from %d", k, tk[0], tk[1], at);
            CHECK(tk[2] >= 0 && tk[2] < (int)sc.op0.size() && sc.op0[tk[2]] == tk[0],
                  "task %d does not start a chunk", k);
            if (k < n_chains)
                CHECK(tk[3] < (int)sc.op0.size() && sc.op0[tk[3]] == tk[1], "task %d chunk_hi", k);
            for (int t = tk[0]; t < (k < n_chains ? tk[1] : n_ops + 1); ++t) region[t] = k;
            at = tk[1];
        }
        CHECK(sc.tasks[4 * n_chains] == pl.top_lo && at == n_ops &&
                  sc.tasks[4 * n_chains + 3] == (int)sc.op0.size() - 1, "top task");
    }
    // chunks
    const int cap = in.knobs.chunk_uses ? in.knobs.chunk_uses
                                         : sc.chunk_cap ? sc.chunk_cap : kChunkUses;
    const int n_chunks = (int)sc.op0.size() - 1;
    CHECK(n_chunks >= 1 && sc.tip0.size() == sc.op0.size() && sc.op0[0] == 0 &&
              sc.op0.back() == n_ops + 1 && sc.tip0.back() == (int)sc.seq.size(), "chunk ends");
    int max_uses = 1;
    for (int k = 0; k < n_chunks; ++k) {
        const int nop = sc.op0[k + 1] - sc.op0[k], nuse = sc.tip0[k + 1] - sc.tip0[k];
        CHECK(nop >= 1 && nop <= kChunkOps, "chunk %d has %d ops", k, nop);
        CHECK(nuse <= cap || nop == 1, "chunk %d: %d uses in %d ops, cap %d", k, nuse, nop, cap);
        max_uses = std::max(max_uses, nuse);
    }
    CHECK(sc.max_chunk_uses == max_uses, "max_chunk_uses %d vs %d", sc.max_chunk_uses, max_uses);
    // every child's one source; tip0 / use0 / seq
    enum { TIP, CUR, LDS, MEM };
    std::vector<int> src(N, -1);
    int used = 0, n_mpat = 0, n_stores = 0;
    for (int k = 0; k < n_chunks; ++k)
        for (int t = sc.op0[k]; t < sc.op0[k + 1]; ++t) {
            const OpDesc &d = pl.descs[t];
            int a = t < n_ops ? in.ops[3 * pl.order[t] + 1] : in.root_a;
            int b = t < n_ops ? in.ops[3 * pl.order[t] + 2] : in.root_b;
            if (pl.swap[t]) std::swap(a, b);
            int ka, kb;
            switch (d.pat) {
            case PAT_LC: ka = LDS, kb = CUR; break;
            case PAT_MC: ka = MEM, kb = CUR; break;
            case PAT_CT: ka = CUR, kb = TIP; break;
            case PAT_TT: ka = TIP, kb = TIP; break;
            case PAT_MT: ka = MEM, kb = TIP; break;
            case PAT_MM: ka = MEM, kb = MEM; break;
            default: ka = kb = -1; CHECK(false, "op %d: pattern %d", t, d.pat);
            }
            n_mpat += d.pat == PAT_MC || d.pat == PAT_MT || d.pat == PAT_MM;
            CHECK(d.use0 == used - sc.tip0[k], "op %d: use0 %d, expected %d", t, d.use0,
                  used - sc.tip0[k]);
            const int nodes[2] = {a, b}, kinds[2] = {ka, kb}, idx[2] = {d.ia, d.ib};
            for (int j = 0; j < 2; ++j) {
                const int v = nodes[j], tp = t_prod[v];
                CHECK(src[v] < 0 && t_cons[v] == t, "node %d is read twice", v);
                src[v] = kinds[j];
                if (kinds[j] == TIP) {
                    CHECK(tp < 0 && in.tip_slot[v] >= 0 && idx[j] == in.tip_slot[v],
                          "op %d: tip child %d", t, v);
                    CHECK(used < (int)sc.seq.size() && sc.seq[used] == idx[j], "seq[%d]", used);
                    ++used;
                    continue;
                }
                CHECK(tp >= 0, "op %d: child %d is a tip read as a parent", t, v);
                if (tp < 0) continue;
                const OpDesc &p = pl.descs[tp];
                if (kinds[j] == CUR)
                    CHECK(tp == t - 1 && region[tp] == region[t], "op %d: current %d", t, v);
                if (kinds[j] == LDS)
                    CHECK(p.dst == idx[j] && idx[j] >= 0 && idx[j] < n_stash &&
                              region[tp] == region[t], "op %d: stash child %d slot %d", t, v, idx[j]);
                else
                    CHECK(p.dst < 0, "op %d: child %d waits in the stash unread", t, v);
                if (kinds[j] == MEM)
                    CHECK(p.par_slot == (idx[j] | kReadBack) && idx[j] == pl.store_slot[v] &&
                              idx[j] >= 0 && idx[j] < pl.n_store, "op %d: HBM child %d", t, v);
                else
                    CHECK(p.par_slot < 0 || !(p.par_slot & kReadBack),
                          "op %d: child %d is written for a read-back nobody makes", t, v);
            }
            if (t < n_ops) n_stores += d.par_slot >= 0;
        }
    CHECK(used == (int)sc.seq.size(), "%d tip uses, seq holds %zu", used, sc.seq.size());
    CHECK(pl.descs[n_ops].par_slot < 0 && pl.descs[n_ops].dst < 0, "root combine stores");
    // no two values whose lifetimes overlap share a stash slot or an HBM slot; values of
    // different tasks (they run concurrently) never share an HBM slot
    struct Val { int slot, region, from, to; };
    std::vector<Val> stash, mem;
    for (int t = 0; t < n_ops; ++t) {
        const OpDesc &d = pl.descs[t];
        const int v = in.ops[3 * pl.order[t]];
        if (d.dst >= 0) stash.push_back({d.dst, region[t], t, t_cons[v]});
        if (d.par_slot >= 0) mem.push_back({d.par_slot & ~kReadBack, region[t], t, t_cons[v]});
    }
    auto by_slot = [](const Val &x, const Val &y) {
        return x.slot != y.slot ? x.slot < y.slot : x.from < y.from;
    };
    std::sort(mem.begin(), mem.end(), by_slot);
    for (size_t i = 1; i < mem.size(); ++i)
        if (mem[i].slot == mem[i - 1].slot)
            CHECK(mem[i].region == mem[i - 1].region && mem[i].from >= mem[i - 1].to,
                  "HBM slot %d: [%d,%d] task %d and [%d,%d] task %d", mem[i].slot,
                  mem[i - 1].from, mem[i - 1].to, mem[i - 1].region, mem[i].from, mem[i].to,
                  mem[i].region);
    for (size_t i = 0; i < stash.size(); ++i)  // (few live at once: compare neighbours in time)
        for (size_t j = i + 1; j < stash.size() && stash[j].from < stash[i].to; ++j)
            CHECK(stash[j].slot != stash[i].slot || stash[j].region != stash[i].region,
                  "stash slot %d: [%d,%d] and [%d,%d]", stash[i].slot, stash[i].from,
                  stash[i].to, stash[j].from, stash[j].to);
    // occupancy plan, build, variant
    const bool occ = keep && in.K <= 4 && !(in.flags & PU_NO_REORDER) &&
                     !in.knobs.lds_slots.set && !in.knobs.split.set;
    CHECK((sc.occ_k > 0) == occ, "occupancy plan %d, expected %d", sc.occ_k, (int)occ);
    if (sc.occ_k > 0) {
        const int n = (sc.grid + in.n_cu - 1) / in.n_cu, k = sc.occ_k;
        const size_t lds = stub_lds(in.K, in.C, in.n_codes, sc.max_chunk_uses, true, sc.L);
        CHECK(k == (in.knobs.keep_occ ? in.knobs.keep_occ : n == 5 || n == 6 ? 7 : 4), "k %d", k);
        CHECK(lds <= lds_cap_for(k) && sc.lds_pad == (int)(lds_cap_for(k) - lds), "pad %d",
              sc.lds_pad);
        CHECK(sc.L == 5 || stub_lds(in.K, in.C, in.n_codes, sc.max_chunk_uses, true, sc.L + 1) >
                               lds_cap_for(k), "%d stash slots are not the most that fit", sc.L);
        CHECK(sc.r_slots == 0 || (k <= 6 && sc.r_slots == 2), "register slots %d", sc.r_slots);
        CHECK(sc.tasks.empty(), "an occupancy plan with chain tasks");
    } else {
        CHECK(sc.lds_pad == 0 && sc.r_slots == 0, "pad or register slots without the rule");
    }
    CHECK((sc.waves == 7) == (sc.occ_k == 7), "waves %d at k %d", sc.waves, sc.occ_k);
    CHECK(sc.waves == 7 || sc.waves == 1 || sc.waves == -1, "waves %d", sc.waves);
    const int v = sc.variant;
    CHECK(!(v & TV_GENERIC) == !(in.K != 20 && (n_mpat > 0 || n_chains > 0)), "TV_GENERIC");
    CHECK(!(v & TV_CHAIN) == !(in.K != 20 && n_chains > 0), "TV_CHAIN");
    CHECK(!(v & TV_KEEP) == !(n_stores == n_ops), "TV_KEEP with %d of %d stores", n_stores, n_ops);
    CHECK(!keep || n_stores == n_ops, "KEEP: %d of %d ops store", n_stores, n_ops);
    CHECK(sc.n_store_ops == n_stores, "n_store_ops");
    CHECK(!(v & TV_SKIP_ZERO_SCALE) == !keep, "TV_SKIP_ZERO_SCALE");
    CHECK(!(v & TV_RSLOTS) == !sc.r_slots, "TV_RSLOTS");
}

static void check_refused(const char *what, Tree t, const char *text = nullptr,
                          int code = PU_E_SCHED, const PlanKnobs &kn = PlanKnobs()) {
    for (int flags : {0, (int)PU_NO_REORDER}) {
        g_case = std::string("refused: ") + what + (flags ? " (caller order)" : "");
        ++g_cases;
        Schedule sc;
        std::string err;
        const int rc = plan_schedule(input_of(t, 4, flags, 4, kn), sc, &err);
        CHECK(rc == code && !err.empty(), "rc %d, message '%s'", rc, err.c_str());
        if (text) CHECK(err.find(text) != std::string::npos, "message '%s'", err.c_str());
    }
}

// the knobs as the library reads them: through the environment
static PlanKnobs knobs_from_env(const char *name, const char *value) {
    if (name) setenv(name, value, 1);
    const PlanKnobs kn = read_plan_knobs();
    if (name) unsetenv(name);
    return kn;
}

int main() {
    for (const char *name : {"PU_LDS_SLOTS", "PU_SPLIT", "PU_KEEP_OCC", "PU_LDS_PAD",
                             "PU_CHUNK_USES", "PU_FORCE_GENERIC", "PU_DEBUG_PLAN"})
        unsetenv(name);
    const char *knob_sets[][2] = {{nullptr, nullptr}, {"PU_LDS_SLOTS", "0"}, {"PU_SPLIT", "3"},
                                  {"PU_KEEP_OCC", "7"}, {"PU_CHUNK_USES", "3"}};
    int n_occ7 = 0, n_split = 0, n_chunk_cap = 0, n_rslots = 0;
    for (int n_tips : {3, 4, 17, 130, 1000}) {  // 130 tips: 128 ops, the chain-split floor
        const Tree tree = random_tree(n_tips, 1000u + n_tips);
        for (int K : {4, 20})
            for (int mode : {0, (int)PU_LNL_ONLY})
                for (int ord : {0, (int)PU_NO_REORDER})
                    for (int n_per_cu : {4, 5, 7})
                        for (const auto &ks : knob_sets) {
                            char name[160];
                            snprintf(name, sizeof name, "%d tips K=%d flags=%d n=%d %s=%s", n_tips,
                                     K, mode | ord, n_per_cu, ks[0] ? ks[0] : "-", ks[0] ? ks[1] : "");
                            g_case = name;
                            ++g_cases;
                            const PlanInput in = input_of(tree, K, mode | ord, n_per_cu,
                                                          knobs_from_env(ks[0], ks[1]));
                            Schedule sc;
                            std::string err;
                            const int rc = plan_schedule(in, sc, &err);
                            CHECK(rc == PU_OK, "rc %d: %s", rc, err.c_str());
                            if (rc != PU_OK) continue;
                            check_schedule(in, sc);
                            n_occ7 += sc.occ_k == 7;
                            n_split += !sc.tasks.empty();
                            n_chunk_cap += sc.chunk_cap > 0;
                            n_rslots += sc.r_slots > 0;
                        }
    }
    // the cases above reach both outcomes of every rule
    g_case = "coverage";
    CHECK(n_occ7 > 0 && n_split > 0 && n_chunk_cap > 0 && n_rslots > 0,
          "7 per CU %d, split %d, chunk cap %d, register slots %d", n_occ7, n_split, n_chunk_cap,
          n_rslots);
    // malformed schedules (17 tips: ops 0..14, internal nodes 17..31)
    const Tree good = random_tree(17, 7);
    Tree t = good;
    t.ops[3 * 14 + 1] = t.ops[3 * 13 + 1];  // op 14 reads a child op 13 also reads
    check_refused("repeated child", t, "consumed 2 times");
    t = good;
    t.ops[3 * 1] = t.ops[3 * 0];
    check_refused("two producers", t, "is the parent of ops");
    t = good;  // ops 0 and 1 produce each other's child
    t.ops[3 * 0 + 1] = t.ops[3 * 1];
    t.ops[3 * 1 + 1] = t.ops[3 * 0];
    check_refused("cycle", t);
    t = good;  // a second component: two more ops that feed each other, each read once
    const int p = t.n_nodes, q = p + 1, u = p + 2, w = p + 3;
    t.n_nodes += 4;
    t.n_ops += 2;
    t.tip_slot.resize(t.n_nodes, -1);
    t.tip_slot[u] = 17;
    t.tip_slot[w] = 18;
    t.ops.insert(t.ops.end(), {p, q, u, q, p, w});
    check_refused("ops not under the root edge", t);
    check_refused("PU_LDS_SLOTS=9", good, "PU_LDS_SLOTS must be in [0, 8]", PU_E_ARG,
                  knobs_from_env("PU_LDS_SLOTS", "9"));
    g_case = "PU_KEEP_OCC=8";
    {
        Schedule sc;
        std::string err;
        const int rc = plan_schedule(input_of(good, 4, 0, 4, knobs_from_env("PU_KEEP_OCC", "8")),
                                     sc, &err);
        CHECK(rc == PU_E_ARG && err == "PU_KEEP_OCC must be in [3, 7]", "rc %d '%s'", rc,
              err.c_str());
    }
    printf("plan_check: %d cases, %d failures (LDS sizes: this program's stub, not the "
           "kernels')\n", g_cases, g_fail);
    return g_fail ? 1 : 0;
}
