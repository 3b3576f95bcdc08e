// pu_ancestral.hip -- marginal ancestral states and site-rate posteriors on the device-resident
// CLVs of a context: the gfx950 kernel that turns the two partials at the ends of
// an edge into the posterior of one end's state, and its C ABI (include/phylo_hip.h):
//   pu_ancestral_max_cat   the kernel's category limit per alphabet (host only)
//   pu_ancestral_edge      the posterior of one node's state from the far end of one edge
//   pu_ancestral_sweep     one pass of the optimising traversal that reconstructs every
//                          internal node
//   pu_site_rates          posterior of the rate category and mean rate of every pattern
//
// While the optimising traversal stands on edge (n, o), partials[n] holds the subtree below n
// and partials[o], re-oriented, everything else.  For a reversible model, with A, B the two
// vectors of (site, category c), sA, sB their log scalers and t the edge length:
//   g_c(i)  = pi_i A_c(i) sum_j P_c(t)[i][j] B_c(j)      joint of state i at n and the data
//   F_c     = sum_i g_c(i),  sigma_c = sA_c + sB_c,  m = max_c sigma_c
//   Z       = sum_c w_c e^{sigma_c - m} F_c
//   q(i)    = sum_c w_c e^{sigma_c - m} g_c(i) / Z       posterior of state i at n
//   r(c)    = w_c e^{sigma_c - m} F_c / Z                posterior of category c
//   lnL_s   = m + log Z                                  the site's log-likelihood
// The kernel only reads the context: no pre-order pass, no second set of partials.
//
// Mapping (k_edge's): a workgroup is one 64-site tile, a lane a site, wave w owns
// rate categories w, w + nw, ...; the categories of a site meet in LDS, where wave 0 mixes them.
// Every sum runs in a fixed order (categories ascending, states ascending); every workgroup
// writes its weighted lnL sum and a one-workgroup second launch adds them (k_tile_sums).
#include <math.h>

#include <cmath>

#include "pu_ctx.h"
#include "pu_edge_dev.h"
#include "pu_resident.h"
#include "pu_service.h"

using namespace pu;

namespace {

struct AncArgs {
    NodeSrc n, o;        // the node reconstructed, the other end of the edge
    double t;            // the edge length
    uint8_t *map_state;  // [S] argmax_i q(i), lowest index on a tie (nullptr: not written)
    double *map_prob;    // [S] its posterior (nullptr: not written)
    double *post;        // [S][K] q (nullptr: not written)
    double *cat_post;    // [S][C] r (nullptr: not written)
    double *mean_rate;   // [S] sum_c r(c) rate_c (nullptr: not written)
    double *part;        // [grid] per-workgroup sums of pattern weight x lnL_s
};

constexpr int kAncMaxWaves = 8;
__host__ __device__ inline int anc_waves(int C) { return C < kAncMaxWaves ? C : kAncMaxWaves; }

// LDS of one workgroup (doubles): the model (ModelLds), then [exponentials C*K][P C*K*K][per
// (category, site): g(0..K-1), F, sigma -- later the mix weight: C*(K+2)*64]
struct AncLds : ModelLds {
    size_t ex, P, vals, total;
    __host__ __device__ AncLds(int K, int C) : ModelLds(K, C) {
        ex = body;
        P = ex + (size_t)C * K;
        vals = P + (size_t)C * K * K;
        total = vals + (size_t)C * (K + 2) * kLanes;
    }
};

template <int K>
__global__ void __launch_bounds__(64 * kAncMaxWaves) k_ancestral(EdgeArgs a, AncArgs q) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int C = a.C;
    const AncLds L(K, C);
    const int tile = blockIdx.x, l = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nw = blockDim.x >> 6;
    const int64_t site = (int64_t)tile * kLanes + l;
    const int64_t site_c = site < a.S ? site : a.S - 1;
    const double *ev = lds + L.evecs, *iv = lds + L.ivecs, *el = lds + L.evals,
                 *pi = lds + L.pi, *rt = lds + L.rates, *ex = lds + L.ex, *P = lds + L.P;
    double *vals = lds + L.vals;
    constexpr int kRow = (K + 2) * kLanes;  // doubles per category in vals

    load_model<K>(a, lds, L);
    __syncthreads();
    exp_tables<K>(lds + L.ex, el, rt, C, 1, &q.t);
    __syncthreads();
    p_tables<K, true>(lds + L.P, ev, iv, ex, rt, C);
    __syncthreads();

    // K = 20: the rows of P are read from LDS where they are used (unrolled, they are hoisted
    // and spill); y_i waits in the lane's own LDS slot, so the row loop indexes no registers
    constexpr int kRowUnroll = K > 4 ? 1 : K;
    for (int c = w; c < C; c += nw) {
        double A[K], B[K], sA, sB;
        node_vec<K>(a, q.n, c, tile, l, site_c, A, sA);
        node_vec<K>(a, q.o, c, tile, l, site_c, B, sB);
        const double *Pc = P + (size_t)c * K * K;
        double *g = vals + (size_t)c * kRow + l;
#pragma unroll kRowUnroll
        for (int i = 0; i < K; ++i) {
            double y = 0.0;
#pragma unroll
            for (int j = 0; j < K; ++j) y = fma(Pc[i * K + j], B[j], y);
            g[i * kLanes] = y;
        }
        double F = 0.0;
#pragma unroll
        for (int i = 0; i < K; ++i) {
            const double gi = (pi[i] * A[i]) * g[i * kLanes];
            g[i * kLanes] = gi;
            F += gi;
        }
        g[K * kLanes] = F;
        g[(K + 1) * kLanes] = sA + sB;
    }
    __syncthreads();
    if (w != 0) return;

    // wave 0 mixes the categories of its 64 sites; the mix weight replaces sigma_c
    double v0 = 0.0;
    if (site < a.S) {
        double *vs = vals + l;
        const double m = mix_max(vs + K * kLanes, vs + (K + 1) * kLanes, kRow, C);
        const double Z = mix_weights(vs + K * kLanes, vs + (K + 1) * kLanes, kRow, C, a.weights, m);
        int best = 0;
        double bestq = 0.0;
        dbl2 *post = q.post ? reinterpret_cast<dbl2 *>(q.post + (size_t)site * K) : nullptr;
        constexpr int kPairUnroll = K > 4 ? 1 : K / 2;
#pragma unroll kPairUnroll
        for (int ip = 0; ip < K / 2; ++ip) {
            double q0 = 0.0, q1 = 0.0;
            for (int c = 0; c < C; ++c) {
                const double we = vs[(size_t)c * kRow + (K + 1) * kLanes];
                q0 += we * vs[(size_t)c * kRow + (2 * ip) * kLanes];
                q1 += we * vs[(size_t)c * kRow + (2 * ip + 1) * kLanes];
            }
            q0 = q0 / Z;
            q1 = q1 / Z;
            if (ip == 0 || q0 > bestq) {
                best = 2 * ip;
                bestq = q0;
            }
            if (q1 > bestq) {
                best = 2 * ip + 1;
                bestq = q1;
            }
            if (post) post[ip] = dbl2{q0, q1};  // [site][state]: K = 4 two 16-byte stores
        }
        if (q.map_state) q.map_state[site] = (uint8_t)best;
        if (q.map_prob) q.map_prob[site] = bestq;
        if (q.cat_post || q.mean_rate) {
            double mr = 0.0;
            for (int c = 0; c < C; ++c) {
                const double r = vs[(size_t)c * kRow + (K + 1) * kLanes] *
                                 vs[(size_t)c * kRow + K * kLanes] / Z;
                if (q.cat_post) q.cat_post[(size_t)site * C + c] = r;
                mr += r * rt[c];
            }
            if (q.mean_rate) q.mean_rate[site] = mr;
        }
        v0 = mix_lnl(a.pattern_w[site], m, Z);
    }
    v0 = wave_sum(v0);
    if (l == 0) q.part[blockIdx.x] = v0;
}

size_t anc_lds_bytes(int K, int C) { return AncLds(K, C).total * sizeof(double); }

// the largest C whose P matrices and mix area fit the LDS of a CU, and a context can hold
// (K = 2: 64, 4: 50, 20: 10)
int anc_max_cat(int K) { return max_cat(K, anc_lds_bytes); }

bool is_tip(const pu_ctx *c, int node) { return c->tip_slot[node] >= 0; }

// what every call needs of the context, and its partial sums
int ancestral_ready(pu_ctx *c, const char *what) {
    const int rc = resident_ready(c, what, anc_max_cat(c->K));
    return rc ? rc : ctx_grow(c, c->d_a_part, c->a_part_cap, (size_t)c->n_tiles);
}

template <int K>
void launch_ancestral_k(hipStream_t st, const EdgeArgs &a, const AncArgs &q) {
    const dim3 grid((unsigned)a.n_tiles), block(64 * anc_waves(a.C));
    hipLaunchKernelGGL(k_ancestral<K>, grid, block, anc_lds_bytes(K, a.C), st, a, q);
}

// one k_ancestral launch and its sum, queued on the context's stream; the weighted lnL sum
// lands in *lnl_dev (device memory)
int ancestral_enqueue(pu_ctx *c, AncArgs q, double *lnl_dev) {
    EdgeArgs a;
    edge_fill_args(c, a);
    q.part = c->d_a_part;
    int rc;
    if ((rc = c->a_timer.begin(c))) return rc;
    dispatch_k(c->K, [&](auto k) { launch_ancestral_k<k()>(c->stream, a, q); });
    HIPCHK(&c->err, hipGetLastError());
    if ((rc = c->a_timer.end(c))) return rc;
    hipLaunchKernelGGL(k_tile_sums<1>, dim3(1), dim3(256), 0, c->stream, c->d_a_part, c->n_tiles,
                       lnl_dev, 0.0);
    HIPCHK(&c->err, hipGetLastError());
    return PU_OK;
}

}  // namespace

extern "C" {

int pu_ancestral_max_cat(int n_states) {
    return max_cat_call("pu_ancestral_max_cat", n_states, anc_max_cat);
}

int pu_ancestral_edge(pu_ctx *c, int node, int other, double length, uint8_t *map_state,
                      double *map_prob, double *post, double *lnl_out) {
    if (!c) return set_err(nullptr, PU_E_ARG, "null context");
    if (!map_state || !map_prob || !lnl_out)
        return set_err(&c->err, PU_E_ARG, "pu_ancestral_edge: null buffer");
    int rc = ancestral_ready(c, "ancestral reconstruction");
    if (rc) return rc;
    DeviceGuard g(c->device);
    int key;
    AncArgs q = {};
    if ((rc = edge_key(c, node, other, &key)) || (rc = edge_node_src(c, node, &q.n)) ||
        (rc = edge_node_src(c, other, &q.o)))
        return rc;
    if (is_tip(c, node))
        return set_err(&c->err, PU_E_ARG, "pu_ancestral_edge: node %d is a tip", node);
    if (!std::isfinite(length) || length == 0.0)
        return set_err(&c->err, PU_E_ARG, "pu_ancestral_edge: length %g", length);
    q.t = length < 0.0 ? c->up_len[key] : length;
    const size_t S = (size_t)c->S, K = (size_t)c->K;
    HostCall h(c->stream, &c->err);
    q.map_state = h.alloc<uint8_t>(S);
    q.map_prob = h.alloc<double>(S);
    q.post = h.alloc<double>(post ? S * K : 0);
    double *d_lnl = h.alloc<double>(1);
    if (!h.rc) h.rc = ancestral_enqueue(c, q, d_lnl);
    h.to_host(map_state, q.map_state, S);
    h.to_host(map_prob, q.map_prob, S);
    h.to_host(post, q.post, post ? S * K : 0);
    h.to_host(lnl_out, d_lnl, 1);
    rc = h.finish("pu_ancestral_edge");
    return rc ? rc : c->a_timer.stamp(c);
}

int pu_ancestral_sweep(pu_ctx *c, int n_rows, const int32_t *rows, int32_t *nodes_out,
                       uint8_t *map_state_out, double *map_prob_out, double *post_out,
                       double *node_lnl_out, int *n_nodes_out) {
    if (!c) return set_err(nullptr, PU_E_ARG, "null context");
    if (n_rows < 1 || !rows || !nodes_out || !map_state_out || !map_prob_out || !node_lnl_out ||
        !n_nodes_out)
        return set_err(&c->err, PU_E_ARG, "pu_ancestral_sweep: no rows or a null buffer");
    int rc = ancestral_ready(c, "ancestral reconstruction");
    if (rc) return rc;
    DeviceGuard g(c->device);
    const size_t cap = (size_t)c->n_tips - 2, S = (size_t)c->S, K = (size_t)c->K;
    // the results of all nodes stay on the device until the walk is over
    HostCall h(c->stream, &c->err);
    uint8_t *d_state = h.alloc<uint8_t>(cap * S);
    double *d_prob = h.alloc<double>(cap * S);
    double *d_post = h.alloc<double>(post_out ? cap * S * K : 0);
    double *d_lnl = h.alloc<double>(cap);
    if (h.rc) return h.rc;
    size_t count = 0;
    // reconstruct `node` from `other`, the far end of their edge, on the current partials
    auto visit = [&](int node, int other, int key) -> int {
        if (is_tip(c, node)) return PU_OK;
        if (count >= cap)
            return set_err(&c->err, PU_E_ARG, "pu_ancestral_sweep: more than n_tips - 2 = %d "
                           "internal nodes in the rows", (int)cap);
        AncArgs q = {};
        int r;
        if ((r = edge_node_src(c, node, &q.n)) || (r = edge_node_src(c, other, &q.o))) return r;
        q.t = c->up_len[key];
        q.map_state = d_state + count * S;
        q.map_prob = d_prob + count * S;
        q.post = post_out ? d_post + count * S * K : nullptr;
        if ((r = ancestral_enqueue(c, q, d_lnl + count))) return r;
        nodes_out[count++] = node;
        return PU_OK;
    };
    return resident_walk(
        c, n_rows, rows,
        // NOD from PAR, which holds everything but NOD's subtree; on the root edge (row 0) each
        // end is the other's complement
        [&](int r, const int32_t *row, int key) {
            const int e = visit(row[3], row[4], key);
            return e || r != 0 ? e : visit(row[4], row[3], key);
        },
        [&] {
            h.to_host(map_state_out, d_state, count * S);
            h.to_host(map_prob_out, d_prob, count * S);
            h.to_host(post_out, d_post, post_out ? count * S * K : 0);
            h.to_host(node_lnl_out, d_lnl, count);
            if (const int e = h.finish("pu_ancestral_sweep")) return e;
            *n_nodes_out = (int)count;
            return c->a_timer.stamp(c);
        });
}

int pu_site_rates(pu_ctx *c, double *cat_post_out, double *mean_rate_out) {
    if (!c) return set_err(nullptr, PU_E_ARG, "null context");
    if (!mean_rate_out) return set_err(&c->err, PU_E_ARG, "pu_site_rates: null buffer");
    int rc = ancestral_ready(c, "site rates");
    if (rc) return rc;
    DeviceGuard g(c->device);
    int key;
    AncArgs q = {};
    if ((rc = edge_key(c, c->root_a, c->root_b, &key)) ||
        (rc = edge_node_src(c, c->root_a, &q.n)) || (rc = edge_node_src(c, c->root_b, &q.o)))
        return rc;
    q.t = c->up_len[key];
    const size_t S = (size_t)c->S, C = (size_t)c->C;
    HostCall h(c->stream, &c->err);
    q.cat_post = h.alloc<double>(cat_post_out ? S * C : 0);
    q.mean_rate = h.alloc<double>(S);
    double *d_lnl = h.alloc<double>(1);
    if (!h.rc) h.rc = ancestral_enqueue(c, q, d_lnl);
    h.to_host(cat_post_out, q.cat_post, cat_post_out ? S * C : 0);
    h.to_host(mean_rate_out, q.mean_rate, S);
    rc = h.finish("pu_site_rates");
    return rc ? rc : c->a_timer.stamp(c);
}

int pu_ancestral_kernel_ms(pu_ctx *c, double *ms_out) {
    if (!c || !ms_out) return set_err(c ? &c->err : nullptr, PU_E_ARG, "null argument");
    *ms_out = (double)c->a_timer.ms;
    return PU_OK;
}

}  // extern "C"
