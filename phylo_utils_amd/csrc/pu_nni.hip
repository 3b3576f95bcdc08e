// pu_nni.hip -- nearest-neighbour interchange on the device-resident CLVs of a context
// (DESIGN 4.15): the gfx950 kernel that scores the three arrangements of a quartet of
// subtrees, and its C ABI (include/phylo_hip.h):
//   pu_quartet_max_cat   the kernel's category limit per alphabet (host only)
//   pu_quartet_derivs    lnL, dlnL/dt, d2lnL/dt2 of the three arrangements of four nodes
//   pu_nni_sweep         one pass of the optimising traversal that scores every internal edge,
//                        the central length of each arrangement optimised by Newton
//   pu_quartet_site_lnl  pu_quartet_derivs plus the per-pattern lnL of the three arrangements
//   pu_branch_support    pu_nni_sweep's pass with aLRT, aBayes and SH-aLRT of every scored edge
//                        (the RELL product is pu_rell.hip)
//
// Arrangement (a,b | c,d) of nodes x0..x3 with pendant lengths l0..l3 and central length t:
//   L = clv(P(l_a), P(l_b), a, b), R = clv(P(l_c), P(l_d), c, d) -- the engine's update with
//   its rescale rule (pu_edge_dev.h rescale) on the nodes' current partials and scalers --
//   then what EDGE_DERIV (pu_edge.hip) defines for ends L, R at length t.
//
// Everything runs in the eigen-basis of the model, P(t r) = V diag(e^{lambda r t}) V^-1:
//   y_i = V (e^{lambda r l_i} o (V^-1 x_i))           the four pendant products, shared by the
//                                                     three arrangements, computed once
//   c_k = [V^T (pi o L)]_k [V^-1 R]_k                 K coefficients per arrangement
//   f = sum_k c_k e^{lambda_k r t}, f' = sum_k c_k (lambda_k r) e^{..}, f'' likewise
// (the sum table of k_edge_newton), so no K x K transition matrix is ever built: LDS holds V,
// V^-1 and 13 K exponentials per category, whatever the lengths.
//
// Mapping (k_edge's): a workgroup is one 64-site tile, a lane a site, wave w owns
// rate categories w, w + nw, ...; the categories of a site meet in LDS, where wave k mixes
// arrangement k exactly as k_edge mixes its edge (mix_derivs).  Every workgroup writes its 9
// sums; a one-workgroup second launch adds them in a fixed order (k_tile_sums), bitwise
// repeatable.
#include <math.h>

#include <algorithm>
#include <vector>

#include "pu_ctx.h"
#include "pu_edge_dev.h"
#include "pu_newton.h"
#include "pu_resident.h"
#include "pu_service.h"

using namespace pu;

namespace {

struct QuartetArgs {
    NodeSrc x[4];
    double l[4];   // pendant lengths
    double t[3];   // central length of each arrangement
    double *part;  // [grid][9] per-workgroup sums
    double *site;  // k_quartet<K, true>: [3][site_ld] unweighted per-pattern lnL
    int64_t site_ld;
};

// waves per workgroup at most: K = 20 holds four K-vectors and two more per arrangement in
// registers (about 300 VGPRs), so one wave per SIMD
__host__ __device__ constexpr int quartet_max_waves(int K) { return K == 20 ? 4 : 8; }
__host__ __device__ inline int quartet_waves(int K, int C) {
    return C < quartet_max_waves(K) ? C : quartet_max_waves(K);
}

// LDS of one workgroup (doubles): the model (ModelLds), then [pendant exponentials 4*C*K]
// [central exponentials and their two derivative factors 3*3*C*K][per-(arrangement, category,
// site) f, f', f'', log scaler: 3*4*C*64]
struct QuartetLds : ModelLds {
    size_t ex, eg, vals, total;
    __host__ __device__ QuartetLds(int K, int C) : ModelLds(K, C) {
        ex = body;
        eg = ex + (size_t)4 * C * K;
        vals = eg + (size_t)9 * C * K;
        total = vals + (size_t)12 * C * kLanes;
    }
};

// the other two nodes of arrangement k = (x0, x_{k+1} | x_c, x_d)
__host__ __device__ constexpr int arr_c(int k) { return k == 0 ? 2 : 1; }
__host__ __device__ constexpr int arr_d(int k) { return k == 2 ? 2 : 3; }

// SITES: the mix stage also stores the unweighted lnL of its 64 patterns under arrangement k,
// smax + log(Ls) (-inf where no category has f > 0), to q.site + k * q.site_ld + site: one
// coalesced 8-byte store per lane; the sums are formed as without it
template <int K, bool SITES = false>
__global__ void __launch_bounds__(64 * quartet_max_waves(K)) k_quartet(EdgeArgs a, QuartetArgs q) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int C = a.C;
    const QuartetLds L(K, C);
    const int tile = blockIdx.x, l = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nw = blockDim.x >> 6;
    const int64_t site = (int64_t)tile * kLanes + l;
    const int64_t site_c = site < a.S ? site : a.S - 1;
    const double *ev = lds + L.evecs, *iv = lds + L.ivecs, *el = lds + L.evals,
                 *pi = lds + L.pi, *rt = lds + L.rates, *ex = lds + L.ex, *eg = lds + L.eg;
    double *vals = lds + L.vals;

    load_model<K>(a, lds, L);
    __syncthreads();
    // e^{lambda (l r)} of the four pendant edges: [node][category][state]
    exp_tables<K>(lds + L.ex, el, rt, C, 4, q.l);
    // central edge of arrangement k: e, (lambda r) e, (lambda r)^2 e at [k][order][category][state]
    for (int idx = threadIdx.x; idx < 3 * C * K; idx += blockDim.x) {
        const int j = idx % K, kc = idx / K, c = kc % C, k = kc / C;
        const double lam = el[j], r = rt[c], e = exp_lrt(lam, r, q.t[k]);
        double *g = lds + L.eg + (size_t)3 * k * C * K + (size_t)c * K + j;
        g[0] = e;
        g[(size_t)C * K] = exp_lrt_d(e, lam, r, 1);
        g[(size_t)2 * C * K] = exp_lrt_d(e, lam, r, 2);
    }
    __syncthreads();

    // the loops over the eigen index run rolled for K = 20, so that the rows and columns of V
    // and V^-1 are read from LDS where they are used (unrolled, they are hoisted and spill)
    constexpr int kEigUnroll = K > 4 ? 1 : K;
    for (int c = w; c < C; c += nw) {
        // y_i = V (e o (V^-1 x_i)): the four pendant products of this (site, category)
        double y[4][K], s[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            double v[K];
            node_vec<K>(a, q.x[i], c, tile, l, site_c, v, s[i]);
            const double *e = ex + (size_t)(i * C + c) * K;
#pragma unroll
            for (int m = 0; m < K; ++m) y[i][m] = 0.0;
#pragma unroll kEigUnroll
            for (int j = 0; j < K; ++j) {
                double u = 0.0;
#pragma unroll
                for (int m = 0; m < K; ++m) u = fma(iv[j * K + m], v[m], u);
                u *= e[j];
#pragma unroll
                for (int m = 0; m < K; ++m) y[i][m] = fma(ev[m * K + j], u, y[i][m]);
            }
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int nb = k + 1, nc = arr_c(k), nd = arr_d(k);
            double Lv[K], Rv[K], sL, sR;
#pragma unroll
            for (int i = 0; i < K; ++i) {
                Lv[i] = y[0][i] * y[nb][i];
                Rv[i] = y[nc][i] * y[nd][i];
            }
            rescale<K>(Lv, s[0], s[nb], sL);
            rescale<K>(Rv, s[nc], s[nd], sR);
#pragma unroll
            for (int i = 0; i < K; ++i) Lv[i] = pi[i] * Lv[i];
            // c_j = [V^T (pi o L)]_j [V^-1 R]_j, summed against the central exponentials as it
            // is formed
            const double *g = eg + (size_t)3 * k * C * K + (size_t)c * K;
            double f = 0.0, f1 = 0.0, f2 = 0.0;
#pragma unroll kEigUnroll
            for (int j = 0; j < K; ++j) {
                double A = 0.0, B = 0.0;
#pragma unroll
                for (int i = 0; i < K; ++i) {
                    A = fma(Lv[i], ev[i * K + j], A);
                    B = fma(iv[j * K + i], Rv[i], B);
                }
                const double cj = A * B;
                f = fma(cj, g[j], f);
                f1 = fma(cj, g[(size_t)C * K + j], f1);
                f2 = fma(cj, g[(size_t)2 * C * K + j], f2);
            }
            double *o = vals + (size_t)4 * k * C * kLanes + (size_t)c * kLanes + l;
            o[0] = f;
            o[(size_t)C * kLanes] = f1;
            o[(size_t)2 * C * kLanes] = f2;
            o[(size_t)3 * C * kLanes] = sL + sR;
        }
    }
    __syncthreads();
    // wave k mixes the categories of arrangement k
    for (int k = w; k < 3; k += nw) {
        double v0 = 0.0, v1 = 0.0, v2 = 0.0;
        if (site < a.S) {
            const double sl = mix_derivs(vals + (size_t)4 * k * C * kLanes + l, C, a.weights,
                                         a.pattern_w[site], v0, v1, v2);
            if constexpr (SITES) q.site[(int64_t)k * q.site_ld + site] = sl;
        }
        v0 = wave_sum(v0);
        v1 = wave_sum(v1);
        v2 = wave_sum(v2);
        if (l == 0) {
            double *p = q.part + 9 * (size_t)blockIdx.x + 3 * k;
            p[0] = v0;
            p[1] = v1;
            p[2] = v2;
        }
    }
}

size_t quartet_lds_bytes(int K, int C) { return QuartetLds(K, C).total * sizeof(double); }

// the largest C whose tables and mix area fit the LDS of a CU (K = 2: 25, 4: 24, 20: 19)
int quartet_max_cat(int K) { return max_cat(K, quartet_lds_bytes, INT_MAX); }

int node_is_tip(const pu_ctx *c, int node) { return c->tip_slot[node] >= 0; }

// what every quartet call needs of the context, its partial sums and its mapped result buffer
int quartet_ready(pu_ctx *c) {
    int rc = resident_ready(c, "quartet scoring", quartet_max_cat(c->K));
    if (rc || (rc = ctx_grow(c, c->d_q_part, c->q_part_cap, 9 * (size_t)c->n_tiles))) return rc;
    if (!c->h_q_res) {
        HIPCHK(&c->err, hipHostMalloc((void **)&c->h_q_res, 9 * sizeof(double),
                                      hipHostMallocMapped));
        HIPCHK(&c->err, hipHostGetDevicePointer((void **)&c->d_q_res_host, c->h_q_res, 0));
    }
    return PU_OK;
}

template <int K>
void launch_quartet_k(hipStream_t st, const EdgeArgs &a, const QuartetArgs &q) {
    const dim3 grid((unsigned)a.n_tiles), block(64 * quartet_waves(K, a.C));
    if (q.site)
        hipLaunchKernelGGL((k_quartet<K, true>), grid, block, quartet_lds_bytes(K, a.C), st, a, q);
    else
        hipLaunchKernelGGL(k_quartet<K>, grid, block, quartet_lds_bytes(K, a.C), st, a, q);
}

// one evaluation: out9[3][3] (null: not wanted, and nothing is waited for) of the three
// arrangements of x[4] at central lengths t[3]; d_site (nullable) [3][site_ld] receives the
// unweighted per-pattern lnL of the three (k_quartet<K, true>)
int quartet_eval(pu_ctx *c, const NodeSrc *x, const double *l, const double *t, double *out9,
                 double *d_site = nullptr, int64_t site_ld = 0) {
    EdgeArgs a;
    edge_fill_args(c, a);
    QuartetArgs q;
    for (int i = 0; i < 4; ++i) {
        q.x[i] = x[i];
        q.l[i] = l[i];
    }
    for (int k = 0; k < 3; ++k) q.t[k] = t[k];
    q.part = c->d_q_part;
    q.site = d_site;
    q.site_ld = site_ld;
    int rc;
    if ((rc = c->q_timer.begin(c))) return rc;
    dispatch_k(c->K, [&](auto k) { launch_quartet_k<k()>(c->stream, a, q); });
    HIPCHK(&c->err, hipGetLastError());
    if ((rc = c->q_timer.end(c))) return rc;
    if (!out9) return c->q_timer.stamp(c);
    hipLaunchKernelGGL(k_tile_sums<9>, dim3(1), dim3(256), 0, c->stream, c->d_q_part, c->n_tiles,
                       c->d_q_res_host, 0.0);
    HIPCHK(&c->err, hipGetLastError());
    HIPCHK(&c->err, hipStreamSynchronize(c->stream));
    if ((rc = c->q_timer.stamp(c))) return rc;
    for (int k = 0; k < 9; ++k) out9[k] = c->h_q_res[k];
    return PU_OK;
}

// ---- branch support -----------------------------------------------------------

// the pattern weights as a weight row of the RELL product (integers, checked on the host)
__global__ void __launch_bounds__(256)
    k_weight_row(const double *__restrict__ w, int64_t S, uint32_t *__restrict__ row) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s < S) row[s] = (uint32_t)w[s];
}

// one workgroup per edge e: sums [1 + n_rep][V] holds B of the pattern weights (row 0: l_k) and
// of every replicate at vectors 3 e + k.  count[e] = #{r : d > g_r + eps}, d = l_0 - max(l_1,
// l_2), g_r the gap between the largest and the second largest centred sum c_k = B_k - l_k; an
// arrangement whose l_k is not finite has c_k = -inf and never wins.  Integer counts.
__global__ void __launch_bounds__(256)
    k_support_counts(const double *__restrict__ sums, int n_rep, int V, double eps,
                     int32_t *__restrict__ count) {
    __shared__ int red[4];
    const int e = (int)blockIdx.x;
    const double *l = sums + 3 * (size_t)e;
    const double l0 = l[0], l1 = l[1], l2 = l[2];
    const double d = l0 - fmax(l1, l2);
    int cnt = 0;
    for (int r = (int)threadIdx.x; r < n_rep; r += 256) {
        const double *b = sums + (size_t)(r + 1) * V + 3 * (size_t)e;
        const double c0 = isfinite(l0) ? b[0] - l0 : -INFINITY;
        const double c1 = isfinite(l1) ? b[1] - l1 : -INFINITY;
        const double c2 = isfinite(l2) ? b[2] - l2 : -INFINITY;
        const double hi = fmax(c0, fmax(c1, c2));
        const double mid = fmax(fmin(c0, c1), fmin(fmax(c0, c1), c2));
        cnt += d > (hi - mid) + eps ? 1 : 0;
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) cnt += __shfl_xor(cnt, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) count[e] = red[0] + red[1] + red[2] + red[3];
}

int quartet_call(pu_ctx *c, const char *fn, const int32_t *nodes, const double *lens,
                 const double *t, double *site_out, double *out9);
int sweep_check(pu_ctx *c, const char *fn, int n_rows, const int32_t *rows, double tol,
                int max_iter, const double *scores_out, const int32_t *quartets_out,
                const int *n_scored_out);
int sweep_walk(pu_ctx *c, const char *fn, int n_rows, const int32_t *rows, double tol,
               int max_iter, double *scores_out, int32_t *quartets_out, int *n_scored_out,
               double *d_site, int64_t site_ld);

}  // namespace

extern "C" {

int pu_quartet_max_cat(int n_states) {
    return max_cat_call("pu_quartet_max_cat", n_states, quartet_max_cat);
}

int pu_quartet_derivs(pu_ctx *c, const int32_t *nodes, const double *lens, const double *t,
                      double *out9) {
    if (!c) return set_err(nullptr, PU_E_ARG, "null context");
    if (!out9) return set_err(&c->err, PU_E_ARG, "pu_quartet_derivs: null buffer");
    return quartet_call(c, "pu_quartet_derivs", nodes, lens, t, nullptr, out9);
}

int pu_quartet_site_lnl(pu_ctx *c, const int32_t *nodes, const double *lens, const double *t,
                        double *site_out, double *out9) {
    if (!c) return set_err(nullptr, PU_E_ARG, "null context");
    if (!site_out) return set_err(&c->err, PU_E_ARG, "pu_quartet_site_lnl: null buffer");
    double tmp9[9];
    return quartet_call(c, "pu_quartet_site_lnl", nodes, lens, t, site_out, out9 ? out9 : tmp9);
}

int pu_nni_sweep(pu_ctx *c, int n_rows, const int32_t *rows, double tol, int max_iter,
                 double *scores_out, int32_t *quartets_out, int *n_scored_out) {
    if (!c) return set_err(nullptr, PU_E_ARG, "null context");
    int rc = sweep_check(c, "pu_nni_sweep", n_rows, rows, tol, max_iter, scores_out, quartets_out,
                         n_scored_out);
    if (rc) return rc;
    DeviceGuard g(c->device);
    return sweep_walk(c, "pu_nni_sweep", n_rows, rows, tol, max_iter, scores_out, quartets_out,
                      n_scored_out, nullptr, 0);
}

int pu_branch_support(pu_ctx *c, int n_rows, const int32_t *rows, double tol, int max_iter,
                      uint64_t seed, int64_t first_rep, int n_rep, double epsilon,
                      double *scores_out, int32_t *quartets_out, double *support_out,
                      double *rell_out, int *n_scored_out) {
    const char *fn = "pu_branch_support";
    if (!c) return set_err(nullptr, PU_E_ARG, "null context");
    if (!support_out) return set_err(&c->err, PU_E_ARG, "%s: null buffer", fn);
    if (n_rep < 1) return set_err(&c->err, PU_E_ARG, "%s: n_rep = %d", fn, n_rep);
    if (first_rep < 0 || first_rep + n_rep > ((int64_t)1 << 32))
        return set_err(&c->err, PU_E_ARG, "%s: replicates %lld .. %lld are outside [0, 2^32)", fn,
                       (long long)first_rep, (long long)(first_rep + n_rep - 1));
    if (!(epsilon >= 0.0) || !std::isfinite(epsilon))
        return set_err(&c->err, PU_E_ARG, "%s: epsilon = %g", fn, epsilon);
    int rc = sweep_check(c, fn, n_rows, rows, tol, max_iter, scores_out, quartets_out,
                         n_scored_out);
    if (rc) return rc;
    if ((int64_t)c->h_pattern_w.size() != c->S)
        return set_err(&c->err, PU_E_STATE, "%s: the context has no pattern weights", fn);
    int64_t N = 0;
    for (int64_t s = 0; s < c->S; ++s) {
        const double w = c->h_pattern_w[s];
        if (!(w >= 0.0) || !(w <= 2147483647.0) || w != floor(w))
            return set_err(&c->err, PU_E_ARG, "%s: pattern weight %lld = %g is not an integer in "
                           "[0, 2^31 - 1]", fn, (long long)s, w);
        N = std::min<int64_t>(N + (int64_t)w, (int64_t)1 << 32);
    }
    if (N < 1 || N > 0x7fffffff)
        return set_err(&c->err, PU_E_ARG, "%s: the pattern weights sum to %s, outside "
                       "[1, 2^31 - 1]", fn, N < 1 ? "0" : "more than 2^31 - 1");
    DeviceGuard g(c->device);
    const int cap = std::max(c->n_tips - 3, 1);
    const int64_t S = c->S, ld = (S + 63) & ~(int64_t)63;
    HostCall h(c->stream, &c->err);  // frees the pass's device buffers on every way out
    // the site buffer [edge][3][ld]: the largest allocation of the pass, asked for first
    double *d_site = h.alloc<double>((size_t)cap * 3 * ld);
    if (h.rc) return h.rc;
    h.rc = sweep_walk(c, fn, n_rows, rows, tol, max_iter, scores_out, quartets_out, n_scored_out,
                      d_site, ld);
    const int E = h.rc ? 0 : *n_scored_out, V = 3 * E;
    if (h.rc || E == 0) return h.finish(fn);
    // W in ranges of replicates (256 MiB); row 0 holds the pattern weights themselves
    const int64_t RC = std::min<int64_t>(
        n_rep, std::max<int64_t>(1, (int64_t)(((size_t)256 << 20) / (4 * (size_t)ld)) - 1));
    uint32_t *d_W = h.alloc<uint32_t>((size_t)(RC + 1) * ld);
    double *d_sums = h.alloc<double>((size_t)(n_rep + 1) * V);
    int32_t *d_cnt = h.alloc<int32_t>((size_t)E);
    if (h.rc) return h.finish(fn);
    hipLaunchKernelGGL(k_weight_row, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, c->stream,
                       c->d_pattern_w, S, d_W);
    h.hip(fn, hipGetLastError());
    for (int64_t r0 = 0; r0 < n_rep && !h.rc; r0 += RC) {
        const int nr = (int)std::min<int64_t>(RC, n_rep - r0);
        h.rc = pu_boot_weights_device(c->device, c->stream, seed, first_rep + r0, nr, S,
                                      c->d_pattern_w, d_W + ld, ld);
        if (h.rc) {
            c->err = g_err;
            break;
        }
        // the first range takes row 0 along
        const int lead = r0 == 0 ? 1 : 0;
        h.rc = pu_rell_sums_device(c->device, c->stream, V, S, d_site, ld, nr + lead,
                                   d_W + (1 - lead) * ld, ld, d_sums + (size_t)(r0 + 1 - lead) * V,
                                   V);
        if (h.rc) c->err = g_err;
    }
    if (h.rc) return h.finish(fn);
    hipLaunchKernelGGL(k_support_counts, dim3((unsigned)E), dim3(256), 0, c->stream, d_sums, n_rep,
                       V, epsilon, d_cnt);
    h.hip(fn, hipGetLastError());
    std::vector<double> sums((size_t)(n_rep + 1) * V);
    std::vector<int32_t> cnt((size_t)E);
    h.to_host(sums.data(), d_sums, sums.size());
    h.to_host(cnt.data(), d_cnt, cnt.size());
    if ((rc = h.finish(fn))) return rc;
    for (int e = 0; e < E; ++e) {
        const double *l = sums.data() + 3 * (size_t)e;
        double *o = support_out + 4 * (size_t)e;
        if (!std::isfinite(l[0])) {
            o[0] = o[1] = o[2] = o[3] = NAN;
        } else {
            const double d = l[0] - std::max(l[1], l[2]);
            o[0] = 2.0 * std::max(d, 0.0);
            o[1] = erf(sqrt(o[0] / 2.0));
            o[2] = 1.0 / (1.0 + exp(l[1] - l[0]) + exp(l[2] - l[0]));
            o[3] = (double)cnt[e] / (double)n_rep;
        }
        if (rell_out)
            for (int r = 0; r <= n_rep; ++r)
                for (int k = 0; k < 3; ++k)
                    rell_out[((size_t)e * (n_rep + 1) + r) * 3 + k] =
                        sums[(size_t)r * V + 3 * e + k];
    }
    return PU_OK;
}

}  // extern "C"

namespace {

// pu_quartet_derivs and pu_quartet_site_lnl: the checks, then one evaluation; site_out (host,
// nullable) [3][S]
int quartet_call(pu_ctx *c, const char *fn, const int32_t *nodes, const double *lens,
                 const double *t, double *site_out, double *out9) {
    if (!nodes || !lens) return set_err(&c->err, PU_E_ARG, "%s: null buffer", fn);
    int rc = quartet_ready(c);
    if (rc) return rc;
    DeviceGuard g(c->device);
    NodeSrc x[4];
    for (int i = 0; i < 4; ++i) {
        for (int j = 0; j < i; ++j)
            if (nodes[i] == nodes[j])
                return set_err(&c->err, PU_E_ARG, "%s: node %d repeated", fn, nodes[i]);
        if ((rc = edge_node_src(c, nodes[i], &x[i]))) return rc;
    }
    for (int i = 0; i < 5; ++i)
        if (!(lens[i] > 0.0) || !std::isfinite(lens[i]))
            return set_err(&c->err, PU_E_ARG, "%s: length %d = %g", fn, i, lens[i]);
    double tt[3] = {lens[4], lens[4], lens[4]};
    if (t)
        for (int k = 0; k < 3; ++k) {
            if (!(t[k] > 0.0) || !std::isfinite(t[k]))
                return set_err(&c->err, PU_E_ARG, "%s: central length %d = %g", fn, k, t[k]);
            tt[k] = t[k];
        }
    if (!site_out) return quartet_eval(c, x, lens, tt, out9);
    HostCall h(c->stream, &c->err);
    double *d_site = h.alloc<double>(3 * (size_t)c->S);
    if (!h.rc) h.rc = quartet_eval(c, x, lens, tt, out9, d_site, c->S);
    h.to_host(site_out, d_site, 3 * (size_t)c->S);
    return h.finish(fn);
}

// the argument rules and refusals of a scoring pass
int sweep_check(pu_ctx *c, const char *fn, int n_rows, const int32_t *rows, double tol,
                int max_iter, const double *scores_out, const int32_t *quartets_out,
                const int *n_scored_out) {
    if (n_rows < 1 || !rows || !scores_out || !quartets_out || !n_scored_out)
        return set_err(&c->err, PU_E_ARG, "%s: no rows or a null buffer", fn);
    if (!(tol > 0.0) || max_iter < 0)
        return set_err(&c->err, PU_E_ARG, "%s: tol %g, max_iter %d", fn, tol, max_iter);
    return quartet_ready(c);
}

// the scoring pass of pu_nni_sweep; with d_site, every scored edge also leaves the per-pattern
// lnL of its three arrangements at their optimised lengths in d_site [edge][3][site_ld]
int sweep_walk(pu_ctx *c, const char *fn, int n_rows, const int32_t *rows, double tol,
               int max_iter, double *scores_out, int32_t *quartets_out, int *n_scored_out,
               double *d_site, int64_t site_ld) {
    // the children of every internal node, in the caller's order (pu_set_schedule's ops)
    std::vector<int> child(2 * (size_t)c->n_nodes, -1);
    for (int o = 0; o < c->n_ops; ++o) {
        child[2 * (size_t)c->ops_in[3 * o]] = c->ops_in[3 * o + 1];
        child[2 * (size_t)c->ops_in[3 * o] + 1] = c->ops_in[3 * o + 2];
    }
    const int cap = c->n_tips - 3;
    int n_scored = 0;
    auto score = [&](int, const int32_t *row, int kc) -> int {
        int rc;
        const int nod = row[3], par = row[4];
        if (node_is_tip(c, nod) || node_is_tip(c, par)) return PU_OK;
        // the quartet (children of NOD | SIB, GPA); on the root edge both are PAR's children
        const int nodes[4] = {child[2 * (size_t)nod], child[2 * (size_t)nod + 1],
                              row[0] >= 0 ? row[1] : child[2 * (size_t)par],
                              row[0] >= 0 ? row[2] : child[2 * (size_t)par + 1]};
        if (n_scored >= cap)
            return set_err(&c->err, PU_E_ARG, "%s: more than n_tips - 3 = %d internal "
                           "edges in the rows", fn, cap);
        NodeSrc x[4];
        double l[4];
        for (int i = 0; i < 4; ++i) {
            int key;
            if (nodes[i] < 0)
                return set_err(&c->err, PU_E_ARG, "%s: node %d has no children in the "
                               "schedule", fn, i < 2 ? nod : par);
            if ((rc = edge_node_src(c, nodes[i], &x[i])) ||
                (rc = edge_key(c, nodes[i], i < 2 ? nod : par, &key)))
                return rc;
            l[i] = c->up_len[key];
        }
        // the rule of pu_newton.h, three of them advancing on one launch per step; a finished
        // one is evaluated along at its optimum (tn == t)
        NewtonState nt[3];
        double t[3], out9[9];
        for (int k = 0; k < 3; ++k) t[k] = newton_start(nt[k], c->up_len[kc]);
        while (!(nt[0].done && nt[1].done && nt[2].done)) {
            if ((rc = quartet_eval(c, x, l, t, out9))) return rc;
            for (int k = 0; k < 3; ++k) {
                const double *r = out9 + 3 * k;
                if (!nt[k].done) newton_step(nt[k], r[0], r[1], r[2], tol, max_iter);
                t[k] = nt[k].tn;
            }
        }
        for (int k = 0; k < 3; ++k) {
            double *s = scores_out + 12 * (size_t)n_scored + 4 * k;
            s[0] = nt[k].t;
            s[1] = nt[k].lnl;
            s[2] = nt[k].d1;
            s[3] = (double)nt[k].evals;
        }
        int32_t *qo = quartets_out + 6 * (size_t)n_scored;
        qo[0] = nod;
        qo[1] = par;
        for (int i = 0; i < 4; ++i) qo[2 + i] = nodes[i];
        if (d_site) {  // one more launch at (t*_0, t*_1, t*_2); nothing comes back to the host
            for (int k = 0; k < 3; ++k) t[k] = nt[k].t;
            if ((rc = quartet_eval(c, x, l, t, nullptr, d_site + (size_t)n_scored * 3 * site_ld,
                                   site_ld)))
                return rc;
        }
        ++n_scored;
        return PU_OK;
    };
    // every score came back to the host with its evaluation: nothing is left to collect
    return resident_walk(c, n_rows, rows, score, [&] {
        *n_scored_out = n_scored;
        return PU_OK;
    });
}

}  // namespace

extern "C" {

int pu_quartet_kernel_ms(pu_ctx *c, double *ms_out) {
    if (!c || !ms_out) return set_err(c ? &c->err : nullptr, PU_E_ARG, "null argument");
    *ms_out = (double)c->q_timer.ms;
    return PU_OK;
}

}  // extern "C"
