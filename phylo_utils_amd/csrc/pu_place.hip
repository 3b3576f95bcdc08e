// pu_place.hip -- phylogenetic placement of query sequences on the device-resident CLVs of a
// context (the reference has none): the gfx950 kernels that score and optimise a
// query joined at the midpoint of an edge, and their C ABI (include/phylo_hip.h):
//   pu_place_max_cat     the table kernel's category limit per alphabet (host only)
//   pu_place_edge        all queries at one edge on the current partials
//   pu_place_prescore    one pass of the optimising traversal: every query at every edge, at a
//                        fixed pendant length
//   pu_place_refine      the same pass: the pendant length of chosen (edge, query) pairs
//                        optimised in the kernel
//   pu_place_kernel_ms   the kernel times of the last launches under pu_ctx_profile
//
// While the optimising traversal stands on edge (n, o) of length t, partials[n] holds the
// subtree below n and partials[o], re-oriented, everything else (pu_ancestral.hip).  A query
// joined at the midpoint is a third vector meeting those two at a new node.  With A, B the two
// vectors of (pattern p, category c), sA, sB their log scalers, z the query's tip vector (a row
// of its code table) and l its pendant length:
//   a_pc(i)   = pi_i [P_c(t/2) A_pc](i) [P_c(t/2) B_pc](i)
//   sigma_pc  = sA_pc + sB_pc,  m_p = max_c sigma_pc  (over the categories with sum_i a_pc > 0)
//   f_pc(l,z) = sum_i a_pc(i) [P_c(l) z](i) = sum_k T_pc(k) e^{lambda_k r_c l} u_k(z)
//               T_pc = V^T a_pc,  u(z) = V^-1 z
//   F_p(l,z)  = sum_c w_c e^{sigma_pc - m_p} f_pc(l,z)
//   lnL(q,l)  = sum_s sw_s (m_p(s) + log F_p(s)(l, z_qs))
// p(s) the pattern of the query's column s, sw its weight.  The kernels only read the context.
//
// k_place_table (k_ancestral's mapping: a workgroup is one 64-pattern tile, a lane a pattern,
// wave w owns categories w, w + nw, ...) writes, per pattern, the pre-mixed eigen-basis table
// W_pc(k) = w_c e^{sigma_pc - m_p} T_pc(k) as [p][c][k], m_p and -- for a pendant length l0 --
// the log table G[p][code] = m_p + log sum_c sum_k W_pc(k) e^{lambda_k r_c l0} u_k(code).
// k_place_prescore adds sw_s G[p(s)][code_qs] over fixed chunks of kPlaceChunk sites, one
// workgroup per (query, chunk), and k_row_sums adds a query's chunks in ascending order.
// k_place_newton runs the Newton rule (pu_newton.h) for one query per workgroup on W.  Every sum runs
// in a fixed order and nothing written is read by another workgroup of the same launch: two
// runs are bitwise equal, and a query's numbers do not depend on the other queries.
#include <math.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "pu_ctx.h"
#include "pu_edge_dev.h"
#include "pu_newton.h"
#include "pu_resident.h"
#include "pu_service.h"

using namespace pu;

namespace {

// (rows of a query code table at most: pu_service.h's kMaxCodes)
constexpr int kPlaceMaxWaves = 8;  // k_place_table
constexpr int kPlaceChunk = 2048;  // sites per k_place_prescore workgroup: a constant, so that a
                                   // query's sum order depends on nothing else
constexpr int kPlaceThreads = 256;  // k_place_prescore
// k_place_newton: 16 waves on one candidate.  A walk over many edges launches few candidates per
// edge, each workgroup alone on its CU and bound by the latency of its strided reads of W: the
// refine pass of 5000 candidates over 97 edges (cfg2) took 770 ms with 4 waves
constexpr int kNewtonThreads = 1024;
constexpr int kPlaceMaxCK = 256;    // C * K of any context the table kernel takes (64 x 4)

__host__ __device__ inline int place_waves(int C) {
    return C < kPlaceMaxWaves ? C : kPlaceMaxWaves;
}

struct TableArgs {
    NodeSrc n, o;     // the two ends of the edge
    double half;      // t / 2
    double l0;        // the pendant length of G
    int n_codes;
    const double *u;  // [n_codes][K] u(code) = V^-1 table[code]
    double *W;        // [S][C][K]
    double *m;        // [S]
    double *G;        // [S][n_codes] (nullptr: not written)
};

// LDS of one workgroup (doubles): the model (ModelLds), then [u 32*K][e^{lambda r t/2} C*K]
// [e^{lambda r l0} C*K][P C*K*K][m 64][per (category, pattern): a / T / W (0..K-1), sum_i a,
// sigma -- later the mix weight: C*(K+2)*64]
struct PlaceLds : ModelLds {
    size_t u, ex, ex0, P, mx, vals, total;
    __host__ __device__ PlaceLds(int K, int C) : ModelLds(K, C) {
        u = body;
        ex = u + (size_t)kMaxCodes * K;
        ex0 = ex + (size_t)C * K;
        P = ex0 + (size_t)C * K;
        mx = P + (size_t)C * K * K;
        vals = mx + kLanes;
        total = vals + (size_t)C * (K + 2) * kLanes;
    }
};

template <int K>
__global__ void __launch_bounds__(64 * kPlaceMaxWaves) k_place_table(EdgeArgs a, TableArgs q) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int C = a.C;
    const PlaceLds L(K, C);
    const int tile = blockIdx.x, l = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nw = blockDim.x >> 6;
    const int64_t site = (int64_t)tile * kLanes + l;
    const int64_t site_c = site < a.S ? site : a.S - 1;
    const bool live = site < a.S;
    const double *ev = lds + L.evecs, *iv = lds + L.ivecs, *el = lds + L.evals,
                 *pi = lds + L.pi, *rt = lds + L.rates, *ex = lds + L.ex, *ex0 = lds + L.ex0,
                 *P = lds + L.P, *u = lds + L.u;
    double *vals = lds + L.vals, *mx = lds + L.mx;
    constexpr int kRow = (K + 2) * kLanes;  // doubles per category in vals

    load_model<K>(a, lds, L);
    for (int i = threadIdx.x; i < q.n_codes * K; i += blockDim.x) lds[L.u + i] = q.u[i];
    __syncthreads();
    const double t2[2] = {q.half, q.l0};  // ex, ex0: adjacent tables
    exp_tables<K>(lds + L.ex, el, rt, C, 2, t2);
    __syncthreads();
    p_tables<K, false>(lds + L.P, ev, iv, ex, rt, C);  // P_c(t/2)
    __syncthreads();

    // K = 20: the state loops stay rolled over the rows (k_ancestral's way: the rows of P and V
    // are read from LDS where they are used, a_i waits in the lane's own LDS column)
    constexpr int kRowUnroll = K > 4 ? 1 : K;
    for (int c = w; c < C; c += nw) {
        double A[K], B[K], sA, sB;
        node_vec<K>(a, q.n, c, tile, l, site_c, A, sA);
        node_vec<K>(a, q.o, c, tile, l, site_c, B, sB);
        const double *Pc = P + (size_t)c * K * K;
        double *g = vals + (size_t)c * kRow + l;
        double asum = 0.0;
#pragma unroll kRowUnroll
        for (int i = 0; i < K; ++i) {
            double ya = 0.0, yb = 0.0;
#pragma unroll
            for (int j = 0; j < K; ++j) {
                ya = fma(Pc[i * K + j], A[j], ya);
                yb = fma(Pc[i * K + j], B[j], yb);
            }
            const double ai = (pi[i] * ya) * yb;
            g[i * kLanes] = ai;
            asum += ai;
        }
        // T = V^T a: row i of V against a_i, the K sums in registers
        double T[K];
#pragma unroll
        for (int k = 0; k < K; ++k) T[k] = 0.0;
#pragma unroll kRowUnroll
        for (int i = 0; i < K; ++i) {
            const double ai = g[i * kLanes];
#pragma unroll
            for (int k = 0; k < K; ++k) T[k] = fma(ev[i * K + k], ai, T[k]);
        }
#pragma unroll
        for (int k = 0; k < K; ++k) g[k * kLanes] = T[k];
        g[K * kLanes] = asum;
        g[(K + 1) * kLanes] = sA + sB;
    }
    __syncthreads();
    if (w == 0) {
        // wave 0 mixes the categories of its 64 patterns on sum_i a; the mix weight w_c
        // e^{sigma_c - m} replaces sigma_c
        double *vs = vals + l;
        const double m = mix_max(vs + K * kLanes, vs + (K + 1) * kLanes, kRow, C);
        mix_weights(vs + K * kLanes, vs + (K + 1) * kLanes, kRow, C, a.weights, m);
        mx[l] = m;
        if (live) q.m[site] = m;
    }
    __syncthreads();
    // W = mix weight x T, kept in LDS for G and written [p][c][k]: a lane's C*K values are one
    // contiguous run
    constexpr int kPairUnroll = K > 4 ? 2 : K / 2;
    for (int c = w; c < C; c += nw) {
        double *g = vals + (size_t)c * kRow + l;
        const double we = g[(K + 1) * kLanes];
        dbl2 *dst = reinterpret_cast<dbl2 *>(q.W + ((size_t)site_c * C + c) * K);
#pragma unroll kPairUnroll
        for (int kp = 0; kp < K / 2; ++kp) {
            const double w0 = we * g[(2 * kp) * kLanes], w1 = we * g[(2 * kp + 1) * kLanes];
            g[(2 * kp) * kLanes] = w0;
            g[(2 * kp + 1) * kLanes] = w1;
            if (live) dst[kp] = dbl2{w0, w1};
        }
    }
    if (!q.G) return;
    __syncthreads();
    // H(k) = sum_c W_c(k) e^{lambda_k r_c l0}, by every wave for its own lanes; then the codes
    // are dealt to the waves: G[p][code] = m + log sum_k H(k) u_k(code)
    double H[K];
#pragma unroll
    for (int k = 0; k < K; ++k) H[k] = 0.0;
#pragma unroll 1
    for (int c = 0; c < C; ++c) {
        const double *g = vals + (size_t)c * kRow + l, *e = ex0 + c * K;
#pragma unroll
        for (int k = 0; k < K; ++k) H[k] = fma(g[k * kLanes], e[k], H[k]);
    }
    const double m = mx[l];
#pragma unroll 1
    for (int code = w; code < q.n_codes; code += nw) {
        const double *uz = u + code * K;
        double F = 0.0;
#pragma unroll
        for (int k = 0; k < K; ++k) F = fma(H[k], uz[k], F);
        if (live) q.G[(size_t)site * q.n_codes + code] = F > 0.0 ? m + log(F) : -INFINITY;
    }
}

// the queries of a call on the device
struct QueryDev {
    const uint8_t *codes;  // [Q][n_sites]
    const int32_t *map;    // [n_sites] p(s) (nullptr: the identity)
    const double *sw;      // [n_sites] (nullptr: 1)
    int64_t n_sites;
    int n_codes, n_chunks;
};

// part[q][chunk] = sum over the chunk's sites of sw_s G[p(s)][code_qs]: a thread adds its 8
// sites in ascending order, then a fixed 64-lane tree, then the four waves in order
__global__ void __launch_bounds__(kPlaceThreads) k_place_prescore(QueryDev d, int n_query,
                                                                  const double *__restrict__ G,
                                                                  double *__restrict__ part) {
    __shared__ double red[kPlaceThreads / 64];
    const int64_t blk = blockIdx.x;
    const int64_t qi = blk / d.n_chunks, chunk = blk - qi * d.n_chunks;
    if (qi >= n_query) return;
    const uint8_t *codes = d.codes + (size_t)qi * d.n_sites;
    const int64_t base = chunk * kPlaceChunk;
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < kPlaceChunk / kPlaceThreads; ++j) {
        const int64_t s = base + j * kPlaceThreads + threadIdx.x;
        if (s < d.n_sites) {
            const double wgt = d.sw ? d.sw[s] : 1.0;
            if (wgt != 0.0) {
                const int64_t p = d.map ? d.map[s] : s;
                acc += wgt * G[(size_t)p * d.n_codes + codes[s]];
            }
        }
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double r = 0.0;
        for (int k = 0; k < kPlaceThreads / 64; ++k) r += red[k];
        part[blk] = r;
    }
}

struct NewtonArgsP {
    const int32_t *list;  // [n] the queries of this launch (nullptr: 0..n-1)
    const double *W, *m, *u, *evals, *rates;
    int C;
    double l0, tol;
    int max_iter;
    double *out;  // [n][5]: l*, lnL(l*), dlnL/dl, d2lnL/dl2, steps
};

// One workgroup per query: the Newton rule (pu_newton.h) on the pendant length, every evaluation a
// pass of the workgroup's 1024 threads over the query's sites.  Per evaluation e^{lambda_k r_c l}
// and its factors (lambda_k r_c), (lambda_k r_c)^2 stand in LDS; a thread adds its sites in
// ascending order, then a fixed 64-lane tree, then the sixteen waves in order.  Every thread takes
// the same step from the same sums.
template <int K>
__global__ void __launch_bounds__(kNewtonThreads) k_place_newton(QueryDev d, NewtonArgsP n) {
    __shared__ __attribute__((aligned(16))) double u[kMaxCodes * K];
    __shared__ __attribute__((aligned(16))) double E[3][kPlaceMaxCK];
    __shared__ double red[3][kNewtonThreads / 64];
    constexpr int kPairUnroll = K > 4 ? 2 : K / 2;
    const int C = n.C, CK = n.C * K;
    const int64_t qi = n.list ? n.list[blockIdx.x] : blockIdx.x;
    const uint8_t *codes = d.codes + (size_t)qi * d.n_sites;
    for (int i = threadIdx.x; i < d.n_codes * K; i += blockDim.x) u[i] = n.u[i];

    // {lnL, dlnL/dl, d2lnL/dl2} at pendant length t
    auto eval = [&](double t, double (&r)[3]) {
        __syncthreads();  // the last evaluation's readers of E and red are done (and u is set)
        for (int idx = threadIdx.x; idx < CK; idx += blockDim.x) {
            const double lam = n.evals[idx % K] * n.rates[idx / K];
            const double e = exp(lam * t);
            E[0][idx] = e;
            E[1][idx] = e * lam;
            E[2][idx] = e * (lam * lam);
        }
        __syncthreads();
        double a0 = 0.0, a1 = 0.0, a2 = 0.0;
        for (int64_t s = threadIdx.x; s < d.n_sites; s += kNewtonThreads) {
            const double wgt = d.sw ? d.sw[s] : 1.0;
            if (wgt == 0.0) continue;
            const int64_t p = d.map ? d.map[s] : s;
            const double *Wp = n.W + (size_t)p * CK;
            const double *uz = u + (int)codes[s] * K;
            double F = 0.0, F1 = 0.0, F2 = 0.0;
#pragma unroll 1
            for (int c = 0; c < C; ++c) {
                const dbl2 *Wc = reinterpret_cast<const dbl2 *>(Wp + c * K);
                const double *e0 = E[0] + c * K, *e1 = E[1] + c * K, *e2 = E[2] + c * K;
#pragma unroll kPairUnroll
                for (int kp = 0; kp < K / 2; ++kp) {
                    const dbl2 wv = Wc[kp];
                    const double x0 = wv.x * uz[2 * kp], x1 = wv.y * uz[2 * kp + 1];
                    F = fma(x0, e0[2 * kp], F);
                    F1 = fma(x0, e1[2 * kp], F1);
                    F2 = fma(x0, e2[2 * kp], F2);
                    F = fma(x1, e0[2 * kp + 1], F);
                    F1 = fma(x1, e1[2 * kp + 1], F1);
                    F2 = fma(x1, e2[2 * kp + 1], F2);
                }
            }
            if (F > 0.0) {
                const double g1 = F1 / F;
                a0 += wgt * (n.m[p] + log(F));
                a1 += wgt * g1;
                a2 += wgt * (F2 / F - g1 * g1);
            } else {
                a0 = -INFINITY;  // a site of likelihood 0 and non-zero weight
            }
        }
        a0 = wave_sum(a0);
        a1 = wave_sum(a1);
        a2 = wave_sum(a2);
        if ((threadIdx.x & 63) == 0) {
            red[0][threadIdx.x >> 6] = a0;
            red[1][threadIdx.x >> 6] = a1;
            red[2][threadIdx.x >> 6] = a2;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double s = 0.0;
            for (int k = 0; k < kNewtonThreads / 64; ++k) s += red[j][k];
            r[j] = s;
        }
    };

    // every thread steps a state of its own from the same sums: no broadcast
    NewtonState s;
    newton_start(s, n.l0);
    while (!s.done) {
        double r[3];
        eval(s.tn, r);
        newton_step(s, r[0], r[1], r[2], n.tol, n.max_iter);
    }
    if (threadIdx.x == 0) {
        double *o = n.out + 5 * (size_t)blockIdx.x;
        o[0] = s.t;
        o[1] = s.lnl;
        o[2] = s.d1;
        o[3] = s.d2;
        o[4] = (double)s.it;
    }
}

size_t place_lds_bytes(int K, int C) { return PlaceLds(K, C).total * sizeof(double); }

// the largest C whose tables fit the LDS of a CU and a context can hold
int place_max_cat(int K) {
    return max_cat(K, place_lds_bytes, std::min(kCtxMaxCat, kPlaceMaxCK / K));
}

}  // namespace

// the placement buffers of a context: the tables of the edge the walk stands on, the chunk
// sums, and the times of the last launches when profiling
struct pu::PlaceState {
    double *d_W = nullptr, *d_m = nullptr, *d_G = nullptr, *d_u = nullptr, *d_part = nullptr;
    size_t W_cap = 0, m_cap = 0, G_cap = 0, u_cap = 0, part_cap = 0;
    LaunchTimer timer[3];  // table, prescore, newton
};

void pu::place_free(pu_ctx *c) {
    PlaceState *s = c->place;
    if (!s) return;
    dfree(s->d_W);
    dfree(s->d_m);
    dfree(s->d_G);
    dfree(s->d_u);
    dfree(s->d_part);
    for (LaunchTimer &t : s->timer) t.destroy();
    delete s;
    c->place = nullptr;
}

namespace {

// what every call needs of the context, and the host's copy of the eigen-system
int place_ready(pu_ctx *c, const char *what) {
    if (int rc = resident_ready(c, what, place_max_cat(c->K))) return rc;
    if (c->h_eig.size() != (size_t)(2 * c->K * c->K + c->K))
        return set_err(&c->err, PU_E_STATE, "%s: no eigen-system in the context", what);
    return PU_OK;
}

// the caller's queries: checked on the host, then uploaded once as temporaries of the call
struct QueryHost {
    int n_query;
    int64_t n_sites;
    const uint8_t *codes;
    const int32_t *map;
    const double *sw;
    int n_codes;
    const double *table;
    double l0;
};

int check_queries(pu_ctx *c, const char *fn, const QueryHost &h) {
    if (!h.codes || !h.table)
        return set_err(&c->err, PU_E_ARG, "%s: null query buffer", fn);
    if (h.n_query < 1 || h.n_sites < 1)
        return set_err(&c->err, PU_E_ARG, "%s: %d queries of %lld sites", fn, h.n_query,
                       (long long)h.n_sites);
    if (h.n_codes < 1 || h.n_codes > kMaxCodes)
        return set_err(&c->err, PU_E_ARG, "%s: n_codes %d outside [1, %d]", fn, h.n_codes,
                       kMaxCodes);
    if (!std::isfinite(h.l0) || h.l0 <= 0.0)
        return set_err(&c->err, PU_E_ARG, "%s: pendant length %g", fn, h.l0);
    if (!h.map && h.n_sites != c->S)
        return set_err(&c->err, PU_E_ARG, "%s: %lld sites on %lld patterns without a site map", fn,
                       (long long)h.n_sites, (long long)c->S);
    if (h.map)
        for (int64_t s = 0; s < h.n_sites; ++s)
            if (h.map[s] < 0 || h.map[s] >= c->S)
                return set_err(&c->err, PU_E_ARG, "%s: site_pattern[%lld] = %d outside [0, %lld)",
                               fn, (long long)s, h.map[s], (long long)c->S);
    const size_t n = (size_t)h.n_query * h.n_sites;
    for (size_t i = 0; i < n; ++i)
        if (h.codes[i] >= h.n_codes)
            return set_err(&c->err, PU_E_ARG, "%s: query %zu, site %zu: code %d of %d", fn,
                           i / h.n_sites, i % h.n_sites, h.codes[i], h.n_codes);
    return PU_OK;
}

// the queries and u(code) = V^-1 table[code] to the device; the context's buffers sized for
// them (with_G: the log table and the chunk sums of the pre-score)
int upload_queries(pu_ctx *c, const QueryHost &h, bool with_G, HostCall &hc, QueryDev &d) {
    if (!c->place) c->place = new PlaceState();
    PlaceState *s = c->place;
    const int K = c->K;
    const size_t S = (size_t)c->S, n = (size_t)h.n_query * h.n_sites;
    const int n_chunks = (int)((h.n_sites + kPlaceChunk - 1) / kPlaceChunk);
    int rc;
    if ((rc = ctx_grow(c, s->d_W, s->W_cap, S * c->C * K)) ||
        (rc = ctx_grow(c, s->d_m, s->m_cap, S)) ||
        (rc = ctx_grow(c, s->d_u, s->u_cap, (size_t)kMaxCodes * K)))
        return rc;
    if (with_G && ((rc = ctx_grow(c, s->d_G, s->G_cap, S * kMaxCodes)) ||
                   (rc = ctx_grow(c, s->d_part, s->part_cap, (size_t)h.n_query * n_chunks))))
        return rc;
    std::vector<double> u((size_t)h.n_codes * K);
    const double *iv = c->h_eig.data() + (size_t)K * K + K;
    for (int code = 0; code < h.n_codes; ++code)
        for (int k = 0; k < K; ++k) {
            double acc = 0.0;
            for (int j = 0; j < K; ++j) acc += iv[k * K + j] * h.table[(size_t)code * K + j];
            u[(size_t)code * K + k] = acc;
        }
    d.codes = hc.to_device(h.codes, n);
    d.map = hc.to_device(h.map, (size_t)h.n_sites);
    d.sw = hc.to_device(h.sw, (size_t)h.n_sites);
    d.n_sites = h.n_sites;
    d.n_codes = h.n_codes;
    d.n_chunks = n_chunks;
    hc.hip("hipMemcpyAsync", hipMemcpyAsync(s->d_u, u.data(), u.size() * sizeof(double),
                                            hipMemcpyHostToDevice, hc.st));
    return hc.finish("placement");  // u leaves scope
}

// after the stream has drained: the times of the last launches made while profiling
int place_stamp(pu_ctx *c) {
    for (LaunchTimer &t : c->place->timer)
        if (int rc = t.stamp(c)) return rc;
    return PU_OK;
}

template <int K>
void launch_table_k(hipStream_t st, const EdgeArgs &a, const TableArgs &q) {
    const dim3 grid((unsigned)a.n_tiles), block(64 * place_waves(a.C));
    hipLaunchKernelGGL(k_place_table<K>, grid, block, place_lds_bytes(K, a.C), st, a, q);
}

// k_place_table of edge (n, o) at length t, queued on the context's stream
int table_enqueue(pu_ctx *c, NodeSrc n, NodeSrc o, double t, const QueryHost &h, bool with_G) {
    PlaceState *s = c->place;
    EdgeArgs a;
    edge_fill_args(c, a);
    TableArgs q = {};
    q.n = n;
    q.o = o;
    q.half = 0.5 * t;
    q.l0 = h.l0;
    q.n_codes = h.n_codes;
    q.u = s->d_u;
    q.W = s->d_W;
    q.m = s->d_m;
    q.G = with_G ? s->d_G : nullptr;
    int rc;
    if ((rc = s->timer[0].begin(c))) return rc;
    dispatch_k(c->K, [&](auto k) { launch_table_k<k()>(c->stream, a, q); });
    HIPCHK(&c->err, hipGetLastError());
    return s->timer[0].end(c);
}

// the pre-score of all queries on the tables in place: score_dev[Q]
int prescore_enqueue(pu_ctx *c, const QueryDev &d, int n_query, double *score_dev) {
    PlaceState *s = c->place;
    const int64_t blocks = (int64_t)n_query * d.n_chunks;
    if (blocks > 0x7fffffffLL)
        return set_err(&c->err, PU_E_ARG, "placement: %d queries x %d chunks exceed one launch",
                       n_query, d.n_chunks);
    int rc;
    if ((rc = s->timer[1].begin(c))) return rc;
    hipLaunchKernelGGL(k_place_prescore, dim3((unsigned)blocks), dim3(kPlaceThreads), 0, c->stream,
                       d, n_query, s->d_G, s->d_part);
    HIPCHK(&c->err, hipGetLastError());
    if ((rc = s->timer[1].end(c))) return rc;
    launch_row_sums(c->stream, s->d_part, n_query, d.n_chunks, score_dev);
    HIPCHK(&c->err, hipGetLastError());
    return PU_OK;
}

// k_place_newton for n queries (list_dev, nullptr: 0..n-1) on the tables in place: out_dev[n][5]
int newton_enqueue(pu_ctx *c, const QueryDev &d, const int32_t *list_dev, int n, double l0,
                   double tol, int max_iter, double *out_dev) {
    PlaceState *s = c->place;
    NewtonArgsP a = {};
    a.list = list_dev;
    a.W = s->d_W;
    a.m = s->d_m;
    a.u = s->d_u;
    a.evals = c->d_evals;
    a.rates = c->d_rates;
    a.C = c->C;
    a.l0 = l0;
    a.tol = tol;
    a.max_iter = max_iter;
    a.out = out_dev;
    int rc;
    if ((rc = s->timer[2].begin(c))) return rc;
    const dim3 grid((unsigned)n), block(kNewtonThreads);
    dispatch_k(c->K, [&](auto k) {
        hipLaunchKernelGGL(k_place_newton<k()>, grid, block, 0, c->stream, d, a);
    });
    HIPCHK(&c->err, hipGetLastError());
    return s->timer[2].end(c);
}

}  // namespace

extern "C" {

int pu_place_max_cat(int n_states) {
    return max_cat_call("pu_place_max_cat", n_states, place_max_cat);
}

int pu_place_edge(pu_ctx *c, int node, int other, double length, int n_query, int64_t n_sites,
                  const uint8_t *query_codes, const int32_t *site_pattern,
                  const double *site_weight, int n_codes, const double *code_table, double l0,
                  double tol, int max_iter, double *score_out, double *pendant_out,
                  double *lnl_out, double *derivs_out) {
    if (!c) return set_err(nullptr, PU_E_ARG, "null context");
    if (!score_out || !pendant_out || !lnl_out || !derivs_out)
        return set_err(&c->err, PU_E_ARG, "pu_place_edge: null buffer");
    const QueryHost h = {n_query, n_sites, query_codes, site_pattern, site_weight,
                         n_codes, code_table, l0};
    int rc = place_ready(c, "placement");  // the context's state first: S below is then final
    if (rc || (rc = check_queries(c, "pu_place_edge", h))) return rc;
    if (!std::isfinite(length) || length <= 0.0)
        return set_err(&c->err, PU_E_ARG, "pu_place_edge: length %g", length);
    if (max_iter < 0 || !(tol >= 0.0))
        return set_err(&c->err, PU_E_ARG, "pu_place_edge: tol %g, max_iter %d", tol, max_iter);
    DeviceGuard g(c->device);
    int key;
    NodeSrc sn, so;
    if ((rc = edge_key(c, node, other, &key)) || (rc = edge_node_src(c, node, &sn)) ||
        (rc = edge_node_src(c, other, &so)))
        return rc;
    HostCall hc(c->stream, &c->err);
    QueryDev d;
    if ((rc = upload_queries(c, h, true, hc, d))) return rc;
    const size_t Q = (size_t)n_query;
    std::vector<double> nt(max_iter ? 5 * Q : 0);
    double *d_score = hc.alloc<double>(Q), *d_nt = hc.alloc<double>(nt.size());
    if (!hc.rc) hc.rc = table_enqueue(c, sn, so, length, h, true);
    if (!hc.rc) hc.rc = prescore_enqueue(c, d, n_query, d_score);
    if (!hc.rc && max_iter)
        hc.rc = newton_enqueue(c, d, nullptr, n_query, l0, tol, max_iter, d_nt);
    hc.to_host(score_out, d_score, Q);
    hc.to_host(nt.data(), d_nt, nt.size());
    if ((rc = hc.finish("pu_place_edge")) || (rc = place_stamp(c))) return rc;
    if (!max_iter) {  // the pre-score alone
        for (size_t i = 0; i < Q; ++i) {
            pendant_out[i] = l0;
            lnl_out[i] = score_out[i];
            derivs_out[2 * i] = derivs_out[2 * i + 1] = NAN;
        }
        return PU_OK;
    }
    for (size_t i = 0; i < Q; ++i) {
        pendant_out[i] = nt[5 * i];
        lnl_out[i] = nt[5 * i + 1];
        derivs_out[2 * i] = nt[5 * i + 2];
        derivs_out[2 * i + 1] = nt[5 * i + 3];
    }
    return PU_OK;
}

int pu_place_prescore(pu_ctx *c, int n_rows, const int32_t *rows, int n_query, int64_t n_sites,
                      const uint8_t *query_codes, const int32_t *site_pattern,
                      const double *site_weight, int n_codes, const double *code_table, double l0,
                      int32_t *edges_out, double *lengths_out, double *score_out,
                      int *n_edges_out) {
    if (!c) return set_err(nullptr, PU_E_ARG, "null context");
    if (n_rows < 1 || !rows || !edges_out || !lengths_out || !score_out || !n_edges_out)
        return set_err(&c->err, PU_E_ARG, "pu_place_prescore: no rows or a null buffer");
    const QueryHost h = {n_query, n_sites, query_codes, site_pattern, site_weight,
                         n_codes, code_table, l0};
    int rc = place_ready(c, "placement");
    if (rc || (rc = check_queries(c, "pu_place_prescore", h))) return rc;
    const int cap = 2 * c->n_tips - 3;
    int n_edges = 0;
    for (int r = 0; r < n_rows; ++r) n_edges += rows[5 * (size_t)r + 3] >= 0;
    if (n_edges > cap)
        return set_err(&c->err, PU_E_ARG, "pu_place_prescore: more than 2 n_tips - 3 = %d edges "
                       "in the rows", cap);
    DeviceGuard g(c->device);
    HostCall hc(c->stream, &c->err);
    QueryDev d;
    if ((rc = upload_queries(c, h, true, hc, d))) return rc;
    const size_t Q = (size_t)n_query;
    // the scores of all edges stay on the device until the walk is over
    double *d_score = hc.alloc<double>((size_t)n_edges * Q);
    if (hc.rc) return hc.rc;
    size_t count = 0;
    return resident_walk(
        c, n_rows, rows,
        [&](int, const int32_t *row, int key) {
            NodeSrc sn, so;
            int e;
            if ((e = edge_node_src(c, row[3], &sn)) || (e = edge_node_src(c, row[4], &so)))
                return e;
            const double t = c->up_len[key];
            if ((e = table_enqueue(c, sn, so, t, h, true)) ||
                (e = prescore_enqueue(c, d, n_query, d_score + count * Q)))
                return e;
            edges_out[2 * count] = row[3];
            edges_out[2 * count + 1] = row[4];
            lengths_out[count++] = t;
            return PU_OK;
        },
        [&] {
            hc.to_host(score_out, d_score, count * Q);
            if (const int e = hc.finish("pu_place_prescore")) return e;
            *n_edges_out = (int)count;
            return place_stamp(c);
        });
}

int pu_place_refine(pu_ctx *c, int n_rows, const int32_t *rows, int n_query, int64_t n_sites,
                    const uint8_t *query_codes, const int32_t *site_pattern,
                    const double *site_weight, int n_codes, const double *code_table, double l0,
                    double tol, int max_iter, int n_edges, const int64_t *cand_off,
                    const int32_t *cand_query, double *pendant_out, double *lnl_out,
                    double *derivs_out, int32_t *iters_out) {
    if (!c) return set_err(nullptr, PU_E_ARG, "null context");
    if (n_rows < 1 || !rows || !cand_off || !pendant_out || !lnl_out || !derivs_out || !iters_out)
        return set_err(&c->err, PU_E_ARG, "pu_place_refine: no rows or a null buffer");
    const QueryHost h = {n_query, n_sites, query_codes, site_pattern, site_weight,
                         n_codes, code_table, l0};
    int rc = place_ready(c, "placement");
    if (rc || (rc = check_queries(c, "pu_place_refine", h))) return rc;
    if (max_iter < 0 || !(tol >= 0.0))
        return set_err(&c->err, PU_E_ARG, "pu_place_refine: tol %g, max_iter %d", tol, max_iter);
    if (n_edges < 0 || cand_off[0] != 0)
        return set_err(&c->err, PU_E_ARG, "pu_place_refine: n_edges %d, cand_off[0] %lld", n_edges,
                       n_edges < 0 ? 0LL : (long long)cand_off[0]);
    for (int e = 0; e < n_edges; ++e)
        if (cand_off[e + 1] < cand_off[e] || cand_off[e + 1] - cand_off[e] > 0x7fffffffLL)
            return set_err(&c->err, PU_E_ARG, "pu_place_refine: cand_off decreases at edge %d", e);
    const size_t n_cand = (size_t)cand_off[n_edges];
    if (n_cand && !cand_query)
        return set_err(&c->err, PU_E_ARG, "pu_place_refine: null candidate list");
    for (size_t i = 0; i < n_cand; ++i)
        if (cand_query[i] < 0 || cand_query[i] >= n_query)
            return set_err(&c->err, PU_E_ARG, "pu_place_refine: candidate %zu names query %d of "
                           "%d", i, cand_query[i], n_query);
    int walk_edges = 0;
    for (int r = 0; r < n_rows; ++r) walk_edges += rows[5 * (size_t)r + 3] >= 0;
    if (walk_edges > n_edges)
        return set_err(&c->err, PU_E_ARG, "pu_place_refine: %d edges in the rows, cand_off holds "
                       "%d", walk_edges, n_edges);
    DeviceGuard g(c->device);
    HostCall hc(c->stream, &c->err);
    QueryDev d;
    if ((rc = upload_queries(c, h, false, hc, d))) return rc;
    const int32_t *d_list = hc.to_device(cand_query, n_cand);
    double *d_nt = hc.alloc<double>(5 * n_cand);
    if (hc.rc) return hc.finish("pu_place_refine");
    int count = 0;
    return resident_walk(
        c, n_rows, rows,
        [&](int, const int32_t *row, int key) {
            const int64_t lo = cand_off[count], n = cand_off[count + 1] - lo;
            ++count;
            if (n == 0) return PU_OK;
            NodeSrc sn, so;
            int e;
            if ((e = edge_node_src(c, row[3], &sn)) || (e = edge_node_src(c, row[4], &so)) ||
                (e = table_enqueue(c, sn, so, c->up_len[key], h, false)))
                return e;
            return newton_enqueue(c, d, d_list + lo, (int)n, l0, tol, max_iter, d_nt + 5 * lo);
        },
        [&] {
            std::vector<double> nt(5 * n_cand);
            hc.to_host(nt.data(), d_nt, nt.size());
            int e;
            if ((e = hc.finish("pu_place_refine")) || (e = place_stamp(c))) return e;
            // candidates of edges past the walk's last keep NaN
            for (size_t i = 0; i < n_cand; ++i) {
                const bool done = i < (size_t)cand_off[count];
                pendant_out[i] = done ? nt[5 * i] : NAN;
                lnl_out[i] = done ? nt[5 * i + 1] : NAN;
                derivs_out[2 * i] = done ? nt[5 * i + 2] : NAN;
                derivs_out[2 * i + 1] = done ? nt[5 * i + 3] : NAN;
                iters_out[i] = done ? (int32_t)nt[5 * i + 4] : -1;
            }
            return PU_OK;
        });
}

int pu_place_kernel_ms(pu_ctx *c, double *table_ms, double *prescore_ms, double *newton_ms) {
    if (!c || !table_ms || !prescore_ms || !newton_ms)
        return set_err(c ? &c->err : nullptr, PU_E_ARG, "null argument");
    const PlaceState *s = c->place;
    *table_ms = s ? (double)s->timer[0].ms : 0.0;
    *prescore_ms = s ? (double)s->timer[1].ms : 0.0;
    *newton_ms = s ? (double)s->timer[2].ms : 0.0;
    return PU_OK;
}

}  // extern "C"
