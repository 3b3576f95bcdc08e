// pu_spr.hip -- subtree pruning and regrafting on the device-resident CLVs of a context (DESIGN
// 4.20; the reference has no tree search): the gfx950 kernel that scores a pruned subtree joined
// at the midpoint of an edge of the rest tree, and its C ABI (include/phylo_hip.h):
//   pu_regraft_max_cat   the kernel's category limit per alphabet (host only)
//   pu_regraft_edge      one regraft score on the current partials
//   pu_spr_sweep         one pass of the optimising traversal; at every edge the caller's inner
//                        rows re-orient nodes of the rest tree, score regrafts and restore
//   pu_spr_kernel_ms     the kernel time of the last launch under pu_ctx_profile
//
// Pruning the subtree on n's side of edge (n, o) dissolves o: its other neighbours x and y are
// joined by one edge of length t_x + t_y, which leaves the rest tree R.  With A, B the directed
// vectors of R at the two ends of an edge of length t (neither holds the subtree), S the vector
// at n pointing at o, sA, sB, sS their log scalers and l the pendant length len(n, o), the
// subtree joined at the midpoint scores
//   g_pc      = sum_i pi_i [P_c(t/2) A_pc](i) [P_c(t/2) B_pc](i) [P_c(l) S_pc](i)
//   sigma_pc  = sA_pc + sB_pc + sS_pc,  m_p = max_c sigma_pc  (over the categories with g_pc > 0)
//   score     = sum_p w_p (m_p + log sum_c w_c e^{sigma_pc - m_p} g_pc)
// the lnL of the rearranged tree at unchanged lengths (pulley principle).  It is k_place_table's
// three-way join with a dense third vector, and what pu_update_partials of o's slot from
// (A @ t/2, B @ t/2) followed by pu_edge_lnl(n, o) computes in two launches through a whole
// partial written and read back.
//
// k_regraft (k_ancestral's mapping: a workgroup is one 64-pattern tile, a lane a pattern, wave w
// owns categories w, w + nw, ...) builds P_c(t/2) and P_c(l) in LDS, forms the three products
// row by row and leaves g and sigma of its categories in LDS; wave 0 mixes them and writes the
// tile's weighted sum with a fixed lane tree.  k_row_sums, one thread per scored row, adds a
// row's tiles in ascending order.  Every sum runs in a fixed order and nothing written is read
// by another workgroup of the same launch: a score is bitwise repeatable and depends only on
// (A, B, S, t, l) and the pattern count.  The kernels only read the context's partials.
#include <math.h>

#include <cmath>
#include <vector>

#include "pu_ctx.h"
#include "pu_edge_dev.h"
#include "pu_resident.h"
#include "pu_service.h"

using namespace pu;

namespace {

constexpr int kSprMaxWaves = 8;  // k_regraft

__host__ __device__ inline int spr_waves(int C) { return C < kSprMaxWaves ? C : kSprMaxWaves; }

struct RegraftArgs {
    NodeSrc a, b, s;  // the two ends of the edge of R, the pruned subtree
    double half;      // t / 2
    double l;         // the pendant length
    double *part;     // [n_tiles] the tiles' weighted sums of this row
};

// LDS of one workgroup (doubles): the model (ModelLds), then [e^{lambda r t/2} C*K][e^{lambda r
// l} C*K][P(t/2) C*K*K][P(l) C*K*K][per (category, pattern): g, sigma: C*2*64]
struct SprLds : ModelLds {
    size_t ex, exl, P, Pl, vals, total;
    __host__ __device__ SprLds(int K, int C) : ModelLds(K, C) {
        ex = body;
        exl = ex + (size_t)C * K;
        P = exl + (size_t)C * K;
        Pl = P + (size_t)C * K * K;
        vals = Pl + (size_t)C * K * K;
        total = vals + (size_t)C * 2 * kLanes;
    }
};

template <int K>
__global__ void __launch_bounds__(64 * kSprMaxWaves) k_regraft(EdgeArgs a, RegraftArgs q) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int C = a.C;
    const SprLds L(K, C);
    const int tile = blockIdx.x, l = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nw = blockDim.x >> 6;
    const int64_t site = (int64_t)tile * kLanes + l;
    const int64_t site_c = site < a.S ? site : a.S - 1;
    const double *ev = lds + L.evecs, *iv = lds + L.ivecs, *el = lds + L.evals,
                 *pi = lds + L.pi, *rt = lds + L.rates, *ex = lds + L.ex, *exl = lds + L.exl,
                 *P = lds + L.P, *Pl = lds + L.Pl;
    double *vals = lds + L.vals;

    load_model<K>(a, lds, L);
    __syncthreads();
    const double t2[2] = {q.half, q.l};  // ex, exl: adjacent tables
    exp_tables<K>(lds + L.ex, el, rt, C, 2, t2);
    __syncthreads();
    // p_tables<K, false> of both tables, a thread forming entry (i, j) of P_c(t/2) and of P_c(l)
    // from one read of U and U^-1 (dealt one entry per turn, the K = 20 kernel took 6 % longer)
    for (int idx = threadIdx.x; idx < C * K * K; idx += blockDim.x) {
        const int ij = idx % (K * K), c = idx / (K * K);
        const int i = ij / K, j = ij - i * K;
        const double p = p_entry<K>(ev, iv, ex + c * K, i, j);
        const double pl = p_entry<K>(ev, iv, exl + c * K, i, j);
        lds[L.P + idx] = p;
        lds[L.Pl + idx] = pl;
    }
    __syncthreads();

    // K = 20: the row loop stays rolled (k_ancestral's way: the rows of the two P are read from
    // LDS where they are used, the three vectors wait in registers)
    constexpr int kRowUnroll = K > 4 ? 1 : K;
    for (int c = w; c < C; c += nw) {
        double A[K], B[K], V[K], sA, sB, sS;
        node_vec<K>(a, q.a, c, tile, l, site_c, A, sA);
        node_vec<K>(a, q.b, c, tile, l, site_c, B, sB);
        node_vec<K>(a, q.s, c, tile, l, site_c, V, sS);
        const double *Pc = P + (size_t)c * K * K, *Plc = Pl + (size_t)c * K * K;
        double g = 0.0;
#pragma unroll kRowUnroll
        for (int i = 0; i < K; ++i) {
            double ya = 0.0, yb = 0.0, ys = 0.0;
#pragma unroll
            for (int j = 0; j < K; ++j) {
                ya = fma(Pc[i * K + j], A[j], ya);
                yb = fma(Pc[i * K + j], B[j], yb);
                ys = fma(Plc[i * K + j], V[j], ys);
            }
            g = fma((pi[i] * ya) * yb, ys, g);
        }
        vals[(size_t)(2 * c) * kLanes + l] = g;
        vals[(size_t)(2 * c + 1) * kLanes + l] = (sA + sB) + sS;
    }
    __syncthreads();
    if (w != 0) return;

    // wave 0 mixes the categories of its 64 patterns on g
    double v0 = 0.0;
    if (site < a.S) {
        const double *vs = vals + l;
        const double m = mix_max(vs, vs + kLanes, 2 * kLanes, C);
        double Z = 0.0;
        for (int c = 0; c < C; ++c) {
            const double g = vs[(size_t)(2 * c) * kLanes];
            if (mix_takes_part(g))
                Z += mix_weight(a.weights[c], vs[(size_t)(2 * c + 1) * kLanes], m) * g;
        }
        const double pw = a.pattern_w[site];
        if (pw != 0.0) v0 = mix_lnl(pw, m, Z);  // (weight 0 adds +0, not 0 x lnL)
    }
    v0 = wave_sum(v0);
    if (l == 0) q.part[blockIdx.x] = v0;
}

size_t spr_lds_bytes(int K, int C) { return SprLds(K, C).total * sizeof(double); }

// the largest C whose two sets of P matrices and mix area fit the LDS of a CU, and a context can
// hold (K = 2: 64, 4: 64, 20: 20)
int spr_max_cat(int K) { return max_cat(K, spr_lds_bytes); }

}  // namespace

// the regraft buffers of a context: the tiles' sums of the rows scored at one edge of the walk,
// the scores of a call, and the time of the last k_regraft launch when profiling
struct pu::SprState {
    double *d_part = nullptr, *d_score = nullptr;
    size_t part_cap = 0, score_cap = 0;
    LaunchTimer timer;
};

void pu::spr_free(pu_ctx *c) {
    SprState *s = c->spr;
    if (!s) return;
    dfree(s->d_part);
    dfree(s->d_score);
    s->timer.destroy();
    delete s;
    c->spr = nullptr;
}

namespace {

bool good_len(double t) { return std::isfinite(t) && t > 0.0; }

// room for n_part rows of tile sums and n_score scores
int spr_buffers(pu_ctx *c, size_t n_part, size_t n_score) {
    if (!c->spr) c->spr = new SprState();
    SprState *s = c->spr;
    if (int rc = ctx_grow(c, s->d_part, s->part_cap, n_part * (size_t)c->n_tiles)) return rc;
    return ctx_grow(c, s->d_score, s->score_cap, n_score);
}

template <int K>
void launch_regraft_k(hipStream_t st, const EdgeArgs &a, const RegraftArgs &q) {
    const dim3 grid((unsigned)a.n_tiles), block(64 * spr_waves(a.C));
    hipLaunchKernelGGL(k_regraft<K>, grid, block, spr_lds_bytes(K, a.C), st, a, q);
}

// k_regraft of (na, nb, ns) at (t, l) into the k-th row of the tile sums, queued on the
// context's stream
int regraft_enqueue(pu_ctx *c, int na, int nb, int ns, double t, double l, size_t k) {
    SprState *s = c->spr;
    EdgeArgs a;
    edge_fill_args(c, a);
    RegraftArgs q = {};
    int rc;
    if ((rc = edge_node_src(c, na, &q.a)) || (rc = edge_node_src(c, nb, &q.b)) ||
        (rc = edge_node_src(c, ns, &q.s)))
        return rc;
    q.half = 0.5 * t;
    q.l = l;
    q.part = s->d_part + k * (size_t)c->n_tiles;
    if ((rc = s->timer.begin(c))) return rc;
    dispatch_k(c->K, [&](auto k) { launch_regraft_k<k()>(c->stream, a, q); });
    HIPCHK(&c->err, hipGetLastError());
    return s->timer.end(c);
}

// the first n rows of the tile sums into score_dev[n]
int sum_enqueue(pu_ctx *c, int n, double *score_dev) {
    launch_row_sums(c->stream, c->spr->d_part, n, c->n_tiles, score_dev);
    HIPCHK(&c->err, hipGetLastError());
    return PU_OK;
}

int check_scored(pu_ctx *c, const char *fn, long long row, int na, int nb, int ns, double t,
                 double l) {
    const int n = c->n_nodes;
    if (na < 0 || na >= n || nb < 0 || nb >= n || ns < 0 || ns >= n)
        return set_err(&c->err, PU_E_ARG, "%s: row %lld scores nodes (%d, %d, %d) outside [0, %d)",
                       fn, row, na, nb, ns, n);
    if (na == nb || na == ns || nb == ns)
        return set_err(&c->err, PU_E_ARG, "%s: row %lld scores (%d, %d, %d): repeated node", fn,
                       row, na, nb, ns);
    if (!good_len(t) || !good_len(l))
        return set_err(&c->err, PU_E_ARG, "%s: row %lld: edge length %g, pendant length %g", fn,
                       row, t, l);
    return PU_OK;
}

}  // namespace

extern "C" {

int pu_regraft_max_cat(int n_states) {
    return max_cat_call("pu_regraft_max_cat", n_states, spr_max_cat);
}

int pu_regraft_edge(pu_ctx *c, int a, int b, int s, double t, double l, double *score_out) {
    if (!c) return set_err(nullptr, PU_E_ARG, "null context");
    if (!score_out) return set_err(&c->err, PU_E_ARG, "pu_regraft_edge: null buffer");
    int rc = resident_ready(c, "pu_regraft_edge", spr_max_cat(c->K));
    if (rc || (rc = check_scored(c, "pu_regraft_edge", 0, a, b, s, t, l))) return rc;
    DeviceGuard g(c->device);
    if ((rc = spr_buffers(c, 1, 1))) return rc;
    HostCall hc(c->stream, &c->err);
    if (!hc.rc) hc.rc = regraft_enqueue(c, a, b, s, t, l, 0);
    if (!hc.rc) hc.rc = sum_enqueue(c, 1, c->spr->d_score);
    hc.to_host(score_out, c->spr->d_score, 1);
    rc = hc.finish("pu_regraft_edge");
    return rc ? rc : c->spr->timer.stamp(c);
}

int pu_spr_sweep(pu_ctx *c, int n_rows, const int32_t *rows, const int64_t *inner_off,
                 const int32_t *inner_rows, const double *inner_len, double *scores_out,
                 double *lnl_out) {
    if (!c) return set_err(nullptr, PU_E_ARG, "null context");
    if (n_rows < 1 || !rows || !inner_off)
        return set_err(&c->err, PU_E_ARG, "pu_spr_sweep: no rows or a null buffer");
    int rc = resident_ready(c, "pu_spr_sweep", spr_max_cat(c->K));
    if (rc) return rc;
    // every refusal over all rows before any launch
    if (inner_off[0] != 0)
        return set_err(&c->err, PU_E_ARG, "pu_spr_sweep: inner_off[0] = %lld",
                       (long long)inner_off[0]);
    size_t most = 0;  // scored rows at one edge of the walk
    for (int r = 0; r < n_rows; ++r) {
        const int64_t n = inner_off[r + 1] - inner_off[r];
        if (n < 0 || n > 0x7fffffffLL)
            return set_err(&c->err, PU_E_ARG, "pu_spr_sweep: inner_off decreases at row %d", r);
        if (n > 0 && rows[5 * (size_t)r + 3] < 0)
            return set_err(&c->err, PU_E_ARG, "pu_spr_sweep: row %d names no edge and has %lld "
                           "inner rows", r, (long long)n);
    }
    const size_t n_inner = (size_t)inner_off[n_rows];
    if (n_inner && (!inner_rows || !inner_len || !scores_out))
        return set_err(&c->err, PU_E_ARG, "pu_spr_sweep: null inner rows or score buffer");
    size_t n_scored = 0;
    for (int r = 0; r < n_rows; ++r) {
        size_t here = 0;
        for (int64_t i = inner_off[r]; i < inner_off[r + 1]; ++i) {
            const int32_t *x = inner_rows + 6 * (size_t)i;
            const double *len = inner_len + 4 * (size_t)i;
            if (x[0] >= 0) {
                if (x[0] >= c->n_nodes || x[1] < 0 || x[1] >= c->n_nodes || x[2] < 0 ||
                    x[2] >= c->n_nodes)
                    return set_err(&c->err, PU_E_ARG, "pu_spr_sweep: inner row %lld updates "
                                   "(%d, %d, %d) outside [0, %d)", (long long)i, x[0], x[1], x[2],
                                   c->n_nodes);
                if (!good_len(len[0]) || !good_len(len[1]))
                    return set_err(&c->err, PU_E_ARG, "pu_spr_sweep: inner row %lld: update "
                                   "lengths %g, %g", (long long)i, len[0], len[1]);
            }
            if (x[3] < 0) continue;
            if ((rc = check_scored(c, "pu_spr_sweep", (long long)i, x[3], x[4], x[5], len[2],
                                   len[3])))
                return rc;
            if (x[0] >= 0 && (x[0] == x[3] || x[0] == x[4] || x[0] == x[5]))
                return set_err(&c->err, PU_E_ARG, "pu_spr_sweep: inner row %lld updates node %d "
                               "and scores it", (long long)i, x[0]);
            ++here;
        }
        most = std::max(most, here);
        n_scored += here;
    }
    DeviceGuard g(c->device);
    if ((rc = spr_buffers(c, most, n_scored))) return rc;
    SprState *s = c->spr;
    HostCall hc(c->stream, &c->err);
    // Every kept partial is first rewritten by the update kernel from its children, one launch
    // each as the rows below do it: a restore then reproduces the bits it replaces whichever
    // kernel wrote the node last, and a score does not depend on which other rows ran
    for (int o = 0; o < c->n_ops && !rc; ++o) {
        const int32_t *op = c->ops_in.data() + 3 * (size_t)o;
        const double bl[2] = {c->up_len[op[1]], c->up_len[op[2]]};
        rc = edge_update_ops(c, 1, op, bl);
    }
    if (rc) return walk_close(c, rc, false, nullptr);
    size_t done = 0;  // scored rows so far: the compact index into d_score
    std::vector<int64_t> where;  // inner row of every scored row
    where.reserve(n_scored);
    return resident_walk(
        c, n_rows, rows,
        [&](int r, const int32_t *, int) {
            size_t k = 0;
            for (int64_t i = inner_off[r]; i < inner_off[r + 1]; ++i) {
                const int32_t *x = inner_rows + 6 * (size_t)i;
                const double *len = inner_len + 4 * (size_t)i;
                int e;
                if (x[0] >= 0 && (e = edge_update_ops(c, 1, x, len))) return e;
                if (x[3] < 0) continue;
                if ((e = regraft_enqueue(c, x[3], x[4], x[5], len[2], len[3], k))) return e;
                ++k;
                where.push_back(i);
            }
            if (!k) return PU_OK;
            const int e = sum_enqueue(c, (int)k, s->d_score + done);
            done += k;
            return e;
        },
        [&] {
            std::vector<double> sc(done);
            hc.to_host(sc.data(), s->d_score, done);
            if (const int e = hc.finish("pu_spr_sweep")) return e;
            for (size_t i = 0; i < n_inner; ++i) scores_out[i] = NAN;
            for (size_t i = 0; i < done; ++i) scores_out[where[i]] = sc[i];
            return s->timer.stamp(c);
        },
        false, lnl_out);
}

int pu_spr_kernel_ms(pu_ctx *c, double *regraft_ms) {
    if (!c || !regraft_ms) return set_err(c ? &c->err : nullptr, PU_E_ARG, "null argument");
    *regraft_ms = c->spr ? (double)c->spr->timer.ms : 0.0;
    return PU_OK;
}

}  // extern "C"
