// pu_resident.h -- the host layer that the calls on the device-resident partials of a context
// share (pu_edge.cpp's optimising sweep, pu_nni.hip, pu_ancestral.hip, pu_counts.hip,
// pu_place.hip, pu_spr.hip): the limits their kernels are sized by and the category limit that
// follows from them, the dispatch on the alphabet, the one list of refusals, a context buffer
// that only grows, and the walk over the rows of the optimising traversal.  The
// non-template bodies are in pu_edge.cpp, next to the edge functions they wrap; LaunchTimer, a
// member of the context, is declared in pu_ctx.h.  A call's own temporaries are pu_service.h's
// HostCall.  Not part of the public ABI: nothing declared here is exported by the library.
#pragma once
#include <limits.h>

#include <type_traits>

#include "pu_ctx.h"

#pragma GCC visibility push(hidden)
namespace pu {

constexpr size_t kCuLdsBytes = 160 * 1024;  // the LDS of one CU, all of which one workgroup may use
constexpr int kCtxMaxCat = 64;              // pu_ctx_create takes no more categories

// the edge calls' readiness checks and buffers (prepare), a node's source, the key of edge
// (u, v) into up_len, the kernels' common arguments, and n in-place updates (par, c1, c2) at
// lengths brlens[n][2], queued on the context's stream
int edge_prepare(pu_ctx *c);
int edge_node_src(pu_ctx *c, int node, NodeSrc *out);
int edge_key(pu_ctx *c, int u, int v, int *key);
void edge_fill_args(const pu_ctx *c, EdgeArgs &a);
int edge_update_ops(pu_ctx *c, int n, const int32_t *ops, const double *brlens);

// what every call on the resident partials needs of the context, PU_E_STATE / PU_E_ARG as the
// header lists them: edge_prepare, kept partials, an eigen-decomposed model, no ascertainment
// correction, K in {2, 4, 20} and at most max_cat categories (the kernel's *_max_cat(K))
int resident_ready(pu_ctx *c, const char *what, int max_cat);

// the alphabets the resident kernels are built for, and one of them as a template argument:
// f(std::integral_constant<int, K>) for K in {2, 4, 20} (any other K, which resident_ready
// refuses, goes to 20)
inline bool known_k(int K) { return K == 2 || K == 4 || K == 20; }
template <class F>
auto dispatch_k(int K, F f) {
    switch (K) {
        case 2: return f(std::integral_constant<int, 2>{});
        case 4: return f(std::integral_constant<int, 4>{});
        default: return f(std::integral_constant<int, 20>{});
    }
}

// a kernel's category limit: the largest C <= cap whose lds_bytes(K, C) fit the LDS of a CU
template <class Bytes>
int max_cat(int K, Bytes lds_bytes, int cap = kCtxMaxCat) {
    int C = 0;
    while (C < cap && lds_bytes(K, C + 1) <= kCuLdsBytes) ++C;
    return C;
}

// the pu_*_max_cat entry points: PU_E_ARG for an alphabet without kernels
template <class F>
int max_cat_call(const char *fn, int K, F kernel_max_cat) {
    if (!known_k(K)) return set_err(nullptr, PU_E_ARG, "%s: K=%d is not supported", fn, K);
    return kernel_max_cat(K);
}

// a device buffer of the context that only grows: at least `need` elements in p
template <class T>
int ctx_grow(pu_ctx *c, T *&p, size_t &cap, size_t need) {
    if (cap >= need) return PU_OK;
    dfree(p);
    cap = 0;
    if (int rc = dalloc(&c->err, &p, need)) return rc;
    cap = need;
    return PU_OK;
}

// ---- the walk over the rows of the optimising traversal -----------------------------------------

// One row (x0, x1, x2, NOD, PAR): when x0 >= 0, the update of x0 from x1 and x2 at their current
// lengths -- a re-orientation (PAR, SIB, GPA) or a restore (NOD, CH1, CH2) -- then the key of
// edge (NOD, PAR) into up_len, -1 for a row that names no edge (NOD < 0).
int walk_row(pu_ctx *c, const int32_t *row, int *key);
// The end of a walk.  Every node is back in its post-order orientation by the restore rows'
// updates; one traversal rewrites them, the lnL (to *lnl_out, nullable) and the sitewise lnL
// with pu_run's own arithmetic.  After an error (rc != 0) nodes are still re-oriented towards
// the edge the walk stood on: the same traversal puts the context back, and the first error is
// the one returned, code and message (bad rows are refused before they touch anything; a failed
// launch may fail the traversal too).  moved_lengths: up_len is pushed to the device first, so
// that the traversal runs at the lengths reached so far.
int walk_close(pu_ctx *c, int rc, bool moved_lengths, double *lnl_out);

// visit(r, row, key) is called for every row r that names an edge, after the row's update, with
// the walk standing on that edge; collect() after the last row drains the stream and copies the
// call's results to the host.  The first non-zero return of either ends the walk.
template <class Visit, class Collect>
int resident_walk(pu_ctx *c, int n_rows, const int32_t *rows, Visit visit, Collect collect,
                  bool moved_lengths = false, double *lnl_out = nullptr) {
    int rc = PU_OK;
    for (int r = 0; r < n_rows && !rc; ++r) {
        const int32_t *row = rows + 5 * (size_t)r;
        int key;
        if (!(rc = walk_row(c, row, &key)) && key >= 0) rc = visit(r, row, key);
    }
    if (!rc) rc = collect();
    return walk_close(c, rc, moved_lengths, lnl_out);
}

}  // namespace pu
#pragma GCC visibility pop
