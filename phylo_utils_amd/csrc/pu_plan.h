// pu_plan.h -- the traversal planner: everything that decides what the traversal kernels are
// asked to do (op order, chain tasks, LDS stash and HBM slots, descriptors, staging chunks,
// occupancy plan, build and variant).  Host-only: no device context, no HIP call; the
// environment is read by read_plan_knobs alone.  Not part of the public ABI.
#pragma once
#include <string>
#include <utility>
#include <vector>

#include "pu_internal.h"

namespace pu {

// the planning knobs of the environment (sweeps and A/B runs), read once per schedule
struct PlanKnobs {
    struct Int { bool set = false; int v = 0; };
    Int lds_slots, split, lds_pad;  // PU_LDS_SLOTS, PU_SPLIT, PU_LDS_PAD
    int keep_occ = 0;               // PU_KEEP_OCC (0: unset)
    int chunk_uses = 0;             // PU_CHUNK_USES, at least 2 (0: unset)
    bool force_generic = false, debug_plan = false;  // PU_FORCE_GENERIC, PU_DEBUG_PLAN: set
};
PlanKnobs read_plan_knobs();

struct PlanInput {
    // the tree: tip_slot [n_nodes] node -> tip slot (-1: not a tip), ops [n_ops] (par, c1, c2)
    int n_nodes, n_ops, root_a, root_b;
    const int *tip_slot;
    const int32_t *ops;
    PlanInput(int n_nodes, const int *tip_slot, int n_ops, const int32_t *ops, int root_a,
              int root_b)
        : n_nodes(n_nodes), n_ops(n_ops), root_a(root_a), root_b(root_b), tip_slot(tip_slot),
          ops(ops) {}
    int K = 4, C = 1, n_codes = 0, flags = 0, n_cu = 256;
    int64_t S = 1;
    bool coded_tips = true;         // no dense tip
    // dynamic LDS of a traversal launch (the library: pu::traverse_lds_bytes)
    size_t (*lds_bytes)(int K, int C, int n_codes, int max_chunk_uses, bool coded,
                        int n_lds) = nullptr;
    PlanKnobs knobs;
};

// Evaluate the post-order so that the subtree with the larger register need
// goes first (Strahler / Sethi-Ullman), then keep as many parent CLVs in
// registers as R slots allow: among overlapping lifetimes the value whose
// consumer comes last is the one left in memory (optimal for intervals).
struct Plan {
    std::vector<int> order;          // device op -> caller op
    std::vector<OpDesc> descs;       // n_ops + root
    std::vector<int> store_slot;     // node -> storage slot
    int n_store = 0;
    std::vector<char> swap;          // device op: children exchanged w.r.t. the caller's op
    int n_mem = 0;                   // children read back from HBM
    int n_lds = 0;                   // children from the LDS stash
    int n_tip = 0, n_cur = 0;        // children that are tips / the previous op's parent
    int max_live = 0;                // peak number of waiting parents (stack depth)
    // split plan (K = 20 KEEP): device ops [tasks[i].first, tasks[i].second) are chain i, an
    // independent subtree; the ops from top_lo on and the root combine form the top task
    std::vector<std::pair<int, int>> tasks;
    int top_lo = 0;
};

// what pu_set_schedule latches into the context or uploads
struct Schedule {
    Plan plan;                       // descs with use0 filled (par_off: upload_schedule)
    // tip uses in device op order (seq), first use and first op of every staging chunk
    std::vector<int> seq, tip0, op0;
    int max_chunk_uses = 1;
    // tasks [chains..., top]: {op_lo, op_hi, chunk_lo, chunk_hi} (kernel: TraverseArgs::tasks)
    std::vector<int> tasks;
    int L = 0, r_slots = 0;          // LDS stash slots; stash slots in registers (TV_RSLOTS)
    int lds_pad = 0, waves = -1;     // waves -1: pick_waves at enqueue
    int chunk_cap = 0;               // tip uses per staging chunk (0: kChunkUses)
    int occ_k = 0;                   // DNA KEEP occupancy plan: workgroups per CU (0: none)
    int variant = 0, grid = 0, n_tiles = 0, n_store_ops = 0;
};

// errors: a PU_E_* code, the message in *err
int make_plan(const PlanInput &in, int L, bool reorder, bool keep_all, Plan &pl,
              std::string *err, int split = 0);
int plan_schedule(const PlanInput &in, Schedule &out, std::string *err);

int tip_uses(int pat);        // tip children of an op of this pattern
size_t lds_cap_for(int k);    // largest LDS request that lets k workgroups share a CU
int pick_waves(int K, int n_cu, size_t lds, int grid);

}  // namespace pu
