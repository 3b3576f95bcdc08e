// pu_treeset_stages.h -- what pu_treeset.hip shares with pu_treedist.hip: the argument rules of a
// tree-set call, the host's conversion of every tree form to the device form, and the device
// stages (splits, ids, RF) with the id arrays they leave behind.  Defined in pu_treeset.hip;
// DESIGN 4.27 has the rule.  Included after pu_ctx.h.  Not part of the public ABI.
#pragma once
#include <stdint.h>

#include <vector>

#include "pu_ctx.h"

#pragma GCC visibility push(hidden)
namespace pu {

// PU_E_ARG for what pu_treeset_compare refuses in its scalar arguments and input pointers
int treeset_check_args(const char *fn, int n, int n_trees, int form, const int32_t *trees,
                       const int32_t *roots, int n_rows);

// the device form of a tree set (pu_treeset.hip's header comment): cj [T][n-2][2], y [T] and, for
// an edge batch, emap [T][2n-3]: where the edge of op order k stands in the caller's edge order
struct TreesetForm {
    std::vector<int32_t> cj, y, emap;
};
// checks every tree (PU_E_ARG, the message names it) and fills f; PU_E_NOMEM where the host cannot
// hold the converted trees
int treeset_device_form(const char *fn, int n, int n_trees, int form, const int32_t *trees,
                        const int32_t *roots, TreesetForm &f);

// device outputs of the stages: edge_ids [T][2n-3] and n_unique [1] are written always, count
// (room for T (n - 3)), uniq_bits (room for T (n - 3) nw) and rf [n_rows][T] where not null
struct TreesetOut {
    int32_t *edge_ids, *count, *rf;
    int64_t *n_unique;
    uint64_t *uniq_bits;
};

// The id arrays of the last treeset_run on a device, in that device's tree-set state.  They stay
// valid while the caller holds the HostCall (the device's scratch mutex) it ran under and queues
// on the same stream; all null for n = 3.
//   split_id [T][n-3]   the id of cluster m of tree t
//   perm [T (n-3)]      the (tree, cluster) indices t (n - 3) + m sorted by split; the sort is
//                       stable from the identity, so within one id the trees ascend
//   first [U]           the first position in perm of every id
struct TreesetIds {
    const int32_t *split_id = nullptr;
    const uint32_t *perm = nullptr, *first = nullptr;
};

// everything on the device, queued on st; ids (nullable) receives the arrays above
int treeset_run(int device, hipStream_t st, int n, int64_t T, const int32_t *d_cj,
                const int32_t *d_y, const int32_t *d_emap, int n_rows, const TreesetOut &o,
                TreesetIds *ids);

}  // namespace pu
#pragma GCC visibility pop
