// pu_counts.hip -- per-edge joint count matrices on the device-resident CLVs of a context
// (the reference has none): the gfx950 kernel that turns the two partials at the
// ends of an edge into the derivative of lnL with respect to every entry of the edge's
// transition matrices, and its C ABI (include/phylo_hip.h):
//   pu_counts_max_cat     the kernel's category limit per alphabet (host only)
//   pu_edge_counts        the count matrices of one edge on the current partials
//   pu_counts_sweep       one pass of the optimising traversal over every edge
//   pu_counts_kernel_ms   the kernel time of the last launch under pu_ctx_profile
//
// While the optimising traversal stands on edge (n, o), partials[n] holds the subtree below n
// and partials[o], re-oriented, everything else (pu_ancestral.hip).  With A, B the two vectors of
// (site s, category c), sigma_c = sA_c + sB_c, m = max_c sigma_c, F_c = sum_i pi_i A_c(i)
// (P_c(t) B_c)(i), Z = sum_c w_c e^{sigma_c - m} F_c the mixed site likelihood and pw the
// pattern weight:
//   M[c][i][j] = sum_s pw_s (w_c e^{sigma_sc - m_s} / Z_s) A_sc(i) B_sc(j)
// i the state at n, j the state at o.  M carries no pi and no P: it is dlnL / d(pi_j P_c[j][i]),
// from which the host derives the gradient of lnL in every model parameter and every length.
// The kernel only reads the context.
//
// Mapping: a workgroup takes tiles b, b + G, b + 2G, ... of 64 sites (G workgroups, a function
// of the tile count alone), a lane a site, wave w owns rate categories w, w + nw, ...  Per tile
// the first half is k_ancestral's (y = P_c B, F_c, the mix by wave 0), which leaves coef_sc =
// pw w_c e^{..} / Z in LDS; the second half adds coef A(i) B(j).
//   K = 2, 4: a lane keeps the K x K sums of one category in registers across all its tiles
//     and the wave adds them with one wave_sum per entry at the end.  More categories than
//     waves (8; K = 20: 4) are taken in rounds, one category per wave and round; a round
//     repeats the first half (the usual C <= 4 is one round).
//   K = 20: sum_s (coef A)[s][i] B[s][j] is a [K x 64] . [64 x K] product per tile.  The wave
//     stages coef A and B in LDS ([state][site], pitch 66) and runs it on the fp64 matrix cores
//     (v_mfma_f64_16x16x4_f64, 20 padded to 32: four 16 x 16 accumulators, 16 k-steps of 4
//     sites per tile).  The VALU product on the same staging, a lane owning 4 x 2 entries, is
//     kept for the measurement behind it (PU_COUNTS_VALU=1 selects it).
// Sum order: sites ascending within a lane (tiles ascending), a fixed lane tree (K <= 4) or
// the matrix core's fixed k order (K = 20), then a one-workgroup second launch that adds the
// workgroups' matrices in index order and the lnL sums in tile_sums' order.  Nothing depends
// on timing: two runs are bitwise equal.
#include <math.h>
#include <stdlib.h>

#include <cmath>

#include "pu_ctx.h"
#include "pu_edge_dev.h"
#include "pu_resident.h"
#include "pu_service.h"

using namespace pu;

namespace {

struct CntArgs {
    NodeSrc n, o;  // the two ends of the edge: i is n's state, j is o's
    double t;      // the edge length
    double *part;  // [grid][C][K][K] partial matrices, then [grid] weighted lnL sums
};

typedef double d4 __attribute__((ext_vector_type(4)));

// waves of a workgroup: K = 20 stays at four, one per SIMD, which leaves a wave the whole
// register file (eight, two per SIMD, spill the product's operands)
__host__ __device__ constexpr int cnt_max_waves(int K) { return K == 20 ? 4 : 8; }
constexpr int kCntPitch = 66;  // K = 20 staging: doubles per state row (64 sites + 2: the 16
                               // rows of an MFMA operand read fall in distinct LDS banks)
__host__ __device__ inline int cnt_waves(int K, int C) {
    return C < cnt_max_waves(K) ? C : cnt_max_waves(K);
}
// workgroups of a launch: a function of the tile count alone
__host__ __device__ inline int cnt_grid(int K, int n_tiles) {
    (void)K;
    return n_tiles < 256 ? n_tiles : 256;  // one workgroup per CU of an MI355X
}

// LDS of one workgroup (doubles): the model (ModelLds), then [exponentials C*K][P C*K*K][per
// category: F, sigma -- later coef: 2*64][K = 20, per category: coef A and B staged [K][66] each]
struct CntLds : ModelLds {
    size_t ex, P, vals, stage, total;
    __host__ __device__ CntLds(int K, int C) : ModelLds(K, C) {
        ex = body;
        P = ex + (size_t)C * K;
        vals = P + (size_t)C * K * K;
        stage = vals + (size_t)C * 2 * kLanes;
        total = stage + (K == 20 ? (size_t)C * 2 * K * kCntPitch : 0);
    }
};

template <int K, bool MFMA>
__global__ void __launch_bounds__(64 * cnt_max_waves(K)) k_counts(EdgeArgs a, CntArgs q) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int C = a.C;
    const CntLds L(K, C);
    const int l = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nw = blockDim.x >> 6;
    const double *ev = lds + L.evecs, *iv = lds + L.ivecs, *el = lds + L.evals,
                 *pi = lds + L.pi, *rt = lds + L.rates, *ex = lds + L.ex, *P = lds + L.P;
    double *vals = lds + L.vals;
    constexpr int kRow = 2 * kLanes;  // doubles per category in vals: F, then sigma / coef
    constexpr int kKK = K * K;

    load_model<K>(a, lds, L);
    __syncthreads();
    exp_tables<K>(lds + L.ex, el, rt, C, 1, &q.t);
    __syncthreads();
    p_tables<K, true>(lds + L.P, ev, iv, ex, rt, C);
    __syncthreads();

    const int n_rounds = (C + nw - 1) / nw;
    double lnl_acc = 0.0;                    // wave 0: this lane's pw x lnL_s over its tiles
    for (int r = 0; r < n_rounds; ++r) {
        const int c_own = w + r * nw;  // the category whose sums this wave keeps this round
        const bool own = c_own < C;
        // K <= 4: acc[i * K + j]; K = 20, MFMA: four 16 x 16 accumulators (row (l >> 4) + 4 reg,
        // column l & 15 of block (I, J) in m[2 I + J]); VALU: 4 x 2 entries in v
        double acc[K <= 4 ? kKK : 1] = {};
        d4 m[4] = {};
        double v[8] = {};
        for (int tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
            const int64_t site = (int64_t)tile * kLanes + l;
            const int64_t site_c = site < a.S ? site : a.S - 1;
            double kA[K <= 4 ? K : 1], kB[K <= 4 ? K : 1];  // K <= 4: the own category's A, B
            for (int c = w; c < C; c += nw) {
                double A[K], B[K], sA, sB;
                node_vec<K>(a, q.n, c, tile, l, site_c, A, sA);
                node_vec<K>(a, q.o, c, tile, l, site_c, B, sB);
                const double *Pc = P + (size_t)c * K * K;
                double F = 0.0;
                if constexpr (K == 20) {
                    // the rows of P are read from LDS where they are used; y_i waits in the
                    // lane's own column of the staging area (k_ancestral's way round spills)
                    double *y = lds + L.stage + (size_t)c * 2 * K * kCntPitch + l;
#pragma unroll 1
                    for (int i = 0; i < K; ++i) {
                        double yi = 0.0;
#pragma unroll
                        for (int j = 0; j < K; ++j) yi = fma(Pc[i * K + j], B[j], yi);
                        y[i * kCntPitch] = yi;
                    }
#pragma unroll
                    for (int i = 0; i < K; ++i) F += (pi[i] * A[i]) * y[i * kCntPitch];
                    // A and B wait in the staging area (kept in registers across the mix, the
                    // 80 registers spill)
#pragma unroll
                    for (int i = 0; i < K; ++i) {
                        y[i * kCntPitch] = A[i];
                        y[(K + i) * kCntPitch] = B[i];
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < K; ++i) {
                        double yi = 0.0;
#pragma unroll
                        for (int j = 0; j < K; ++j) yi = fma(Pc[i * K + j], B[j], yi);
                        F += (pi[i] * A[i]) * yi;
                    }
                }
                vals[(size_t)c * kRow + l] = F;
                vals[(size_t)c * kRow + kLanes + l] = sA + sB;
                if (K <= 4 && c == c_own) {
#pragma unroll
                    for (int i = 0; i < K; ++i) {
                        kA[i] = A[i];
                        kB[i] = B[i];
                    }
                }
            }
            __syncthreads();
            if (w == 0) {
                // wave 0 mixes the categories of its 64 sites.  coef_c = pw w_c e^{sigma_c - m} / Z
                // replaces sigma_c; exactly 0 where pw = 0 and past the last pattern
                double *vs = vals + l;
                const double pw = site < a.S ? a.pattern_w[site] : 0.0;
                const double mx = mix_max(vs, vs + kLanes, kRow, C);
                const double Z = mix_weights(vs, vs + kLanes, kRow, C, a.weights, mx);
                for (int c = 0; c < C; ++c) {
                    const double we = vs[(size_t)c * kRow + kLanes];
                    vs[(size_t)c * kRow + kLanes] = pw != 0.0 ? pw * we / Z : 0.0;
                }
                if (r == 0) {  // mix_lnl's rule, written out: the product contracts into the sum
                    if (Z > 0.0)
                        lnl_acc += pw * (mx + log(Z));
                    else if (pw != 0.0)
                        lnl_acc = -INFINITY;
                }
            }
            __syncthreads();
            if constexpr (K == 20) {
                double *xa = lds + L.stage + (size_t)(own ? c_own : 0) * 2 * K * kCntPitch;
                double *xb = xa + K * kCntPitch;
                if (own) {
                    const double coef = vals[(size_t)c_own * kRow + kLanes + l];
                    const bool nz = coef != 0.0;
#pragma unroll 4
                    for (int i = 0; i < K; ++i) {
                        xa[i * kCntPitch + l] = nz ? coef * xa[i * kCntPitch + l] : 0.0;
                        xb[i * kCntPitch + l] = nz ? xb[i * kCntPitch + l] : 0.0;
                    }
                }
                __syncthreads();
                if (own) {
                    if constexpr (MFMA) {
                        // A operand: row l & 15 (state i), k = l >> 4 (site); B operand: k =
                        // l >> 4, column l & 15 (state j).  States 20..31 of the second block
                        // are zeros
                        const int g = l >> 4, n = l & 15;
                        const bool hi = n < 4;
                        const double *a0p = xa + n * kCntPitch + g;
                        const double *a1p = xa + (16 + (hi ? n : 3)) * kCntPitch + g;
                        const double *b0p = xb + n * kCntPitch + g;
                        const double *b1p = xb + (16 + (hi ? n : 3)) * kCntPitch + g;
#pragma unroll 4
                        for (int s0 = 0; s0 < kLanes; s0 += 4) {
                            const double a0 = a0p[s0], b0 = b0p[s0];
                            const double a1 = hi ? a1p[s0] : 0.0, b1 = hi ? b1p[s0] : 0.0;
                            m[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, m[0], 0, 0, 0);
                            m[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, m[1], 0, 0, 0);
                            m[2] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, m[2], 0, 0, 0);
                            m[3] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, m[3], 0, 0, 0);
                        }
                    } else if (l < 50) {
                        // lane (ib, jb) owns states i = 4 ib .. 4 ib + 3, j = 2 jb, 2 jb + 1
                        const double *ap = xa + (4 * (l / 10)) * kCntPitch;
                        const double *bp = xb + (2 * (l % 10)) * kCntPitch;
#pragma unroll 4
                        for (int s = 0; s < kLanes; ++s) {
                            const double b0 = bp[s], b1 = bp[kCntPitch + s];
#pragma unroll
                            for (int i = 0; i < 4; ++i) {
                                const double ai = ap[i * kCntPitch + s];
                                v[2 * i] = fma(ai, b0, v[2 * i]);
                                v[2 * i + 1] = fma(ai, b1, v[2 * i + 1]);
                            }
                        }
                    }
                }
            } else if (own) {
                const double coef = vals[(size_t)c_own * kRow + kLanes + l];
                const bool nz = coef != 0.0;
#pragma unroll
                for (int i = 0; i < K; ++i) {
                    const double xa = nz ? coef * kA[i] : 0.0;
#pragma unroll
                    for (int j = 0; j < K; ++j)
                        acc[i * K + j] = fma(xa, nz ? kB[j] : 0.0, acc[i * K + j]);
                }
            }
            __syncthreads();  // vals and the staging area are rewritten by the next tile
        }
        if (!own) continue;
        double *out = q.part + ((size_t)blockIdx.x * C + c_own) * kKK;
        if constexpr (K == 20) {
            if constexpr (MFMA) {
                const int g = l >> 4, n = l & 15;
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const int j = 16 * (b & 1) + n;
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg) {
                        const int i = 16 * (b >> 1) + g + 4 * reg;
                        if (i < K && j < K) out[i * K + j] = m[b][reg];
                    }
                }
            } else if (l < 50) {
                const int i0 = 4 * (l / 10), j0 = 2 * (l % 10);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    out[(i0 + i) * K + j0] = v[2 * i];
                    out[(i0 + i) * K + j0 + 1] = v[2 * i + 1];
                }
            }
        } else {
#pragma unroll
            for (int e = 0; e < kKK; ++e) {
                const double s = wave_sum(acc[e]);
                if (l == 0) out[e] = s;
            }
        }
    }
    if (w == 0) {
        const double s = wave_sum(lnl_acc);
        if (l == 0) q.part[(size_t)gridDim.x * C * kKK + blockIdx.x] = s;
    }
}

// second launch, one workgroup: entry e of the result is the workgroups' entries e added in
// index order; the lnL is their sums in tile_sums' order
__global__ void __launch_bounds__(256) k_counts_sum(const double *__restrict__ part, int n,
                                                    int n_entries, double *__restrict__ counts,
                                                    double *__restrict__ lnl) {
    for (int e = threadIdx.x; e < n_entries; e += blockDim.x) {
        double s = 0.0;
        for (int b = 0; b < n; ++b) s += part[(size_t)b * n_entries + e];
        counts[e] = s;
    }
    tile_sums<1>(part + (size_t)n * n_entries, n, lnl);
}

size_t cnt_lds_bytes(int K, int C) { return CntLds(K, C).total * sizeof(double); }

// the largest C whose tables fit the LDS of a CU and a context can hold (K = 2: 64, 4: 64,
// 20: 6)
int cnt_max_cat(int K) { return max_cat(K, cnt_lds_bytes); }

size_t cnt_part_doubles(const pu_ctx *c) {
    return (size_t)cnt_grid(c->K, c->n_tiles) * ((size_t)c->C * c->K * c->K + 1);
}

// what every call needs of the context, and the workgroups' partials
int counts_ready(pu_ctx *c, const char *what) {
    const int rc = resident_ready(c, what, cnt_max_cat(c->K));
    return rc ? rc : ctx_grow(c, c->d_c_part, c->c_part_cap, cnt_part_doubles(c));
}

template <int K, bool MFMA>
void launch_counts_k(hipStream_t st, const EdgeArgs &a, const CntArgs &q) {
    const dim3 grid((unsigned)cnt_grid(K, a.n_tiles)), block(64 * cnt_waves(K, a.C));
    hipLaunchKernelGGL((k_counts<K, MFMA>), grid, block, cnt_lds_bytes(K, a.C), st, a, q);
}

// the K = 20 product on the VALU instead of the matrix cores: the slower of the two mappings
// measured, kept so that the measurement can be repeated
bool counts_valu() {
    static const bool on = [] {
        const char *e = getenv("PU_COUNTS_VALU");
        return e && e[0] == '1';
    }();
    return on;
}

// one k_counts launch and its sum, queued on the context's stream; the matrices land in
// counts_dev [C][K][K] and the weighted lnL sum in *lnl_dev (device memory)
int counts_enqueue(pu_ctx *c, CntArgs q, double *counts_dev, double *lnl_dev) {
    EdgeArgs a;
    edge_fill_args(c, a);
    q.part = c->d_c_part;
    int rc;
    if ((rc = c->c_timer.begin(c))) return rc;
    dispatch_k(c->K, [&](auto k) {
        if constexpr (k() == 20) {
            if (!counts_valu()) return launch_counts_k<20, true>(c->stream, a, q);
        }
        launch_counts_k<k(), false>(c->stream, a, q);
    });
    HIPCHK(&c->err, hipGetLastError());
    if ((rc = c->c_timer.end(c))) return rc;
    hipLaunchKernelGGL(k_counts_sum, dim3(1), dim3(256), 0, c->stream, c->d_c_part,
                       cnt_grid(c->K, c->n_tiles), c->C * c->K * c->K, counts_dev, lnl_dev);
    HIPCHK(&c->err, hipGetLastError());
    return PU_OK;
}

}  // namespace

extern "C" {

int pu_counts_max_cat(int n_states) {
    return max_cat_call("pu_counts_max_cat", n_states, cnt_max_cat);
}

int pu_edge_counts(pu_ctx *c, int node, int other, double length, double *counts_out,
                   double *lnl_out) {
    if (!c) return set_err(nullptr, PU_E_ARG, "null context");
    if (!counts_out || !lnl_out)
        return set_err(&c->err, PU_E_ARG, "pu_edge_counts: null buffer");
    int rc = counts_ready(c, "edge counts");
    if (rc) return rc;
    DeviceGuard g(c->device);
    int key;
    CntArgs q = {};
    if ((rc = edge_key(c, node, other, &key)) || (rc = edge_node_src(c, node, &q.n)) ||
        (rc = edge_node_src(c, other, &q.o)))
        return rc;
    if (!std::isfinite(length) || length == 0.0)
        return set_err(&c->err, PU_E_ARG, "pu_edge_counts: length %g", length);
    q.t = length < 0.0 ? c->up_len[key] : length;
    const size_t n = (size_t)c->C * c->K * c->K;
    HostCall h(c->stream, &c->err);
    double *d_out = h.alloc<double>(n + 1);  // the matrices, then the lnL
    if (!h.rc) h.rc = counts_enqueue(c, q, d_out, d_out + n);
    h.to_host(counts_out, d_out, n);
    h.to_host(lnl_out, d_out + n, 1);
    rc = h.finish("pu_edge_counts");
    return rc ? rc : c->c_timer.stamp(c);
}

int pu_counts_sweep(pu_ctx *c, int n_rows, const int32_t *rows, int32_t *edges_out,
                    double *lengths_out, double *counts_out, double *edge_lnl_out,
                    int *n_edges_out) {
    if (!c) return set_err(nullptr, PU_E_ARG, "null context");
    if (n_rows < 1 || !rows || !edges_out || !lengths_out || !counts_out || !edge_lnl_out ||
        !n_edges_out)
        return set_err(&c->err, PU_E_ARG, "pu_counts_sweep: no rows or a null buffer");
    int rc = counts_ready(c, "edge counts");
    if (rc) return rc;
    DeviceGuard g(c->device);
    const int cap = 2 * c->n_tips - 3;
    size_t n_edges = 0;
    for (int r = 0; r < n_rows; ++r) n_edges += rows[5 * (size_t)r + 3] >= 0;
    if (n_edges > (size_t)cap)
        return set_err(&c->err, PU_E_ARG, "pu_counts_sweep: more than 2 n_tips - 3 = %d edges in "
                       "the rows", cap);
    const size_t n = (size_t)c->C * c->K * c->K;
    // the results of all edges stay on the device until the walk is over
    HostCall h(c->stream, &c->err);
    double *d_counts = h.alloc<double>(n_edges * n), *d_lnl = h.alloc<double>(n_edges);
    if (h.rc) return h.rc;
    size_t count = 0;
    return resident_walk(
        c, n_rows, rows,
        [&](int, const int32_t *row, int key) {
            // i the state at NOD (its subtree), j the state at PAR (everything else)
            CntArgs q = {};
            int e;
            if ((e = edge_node_src(c, row[3], &q.n)) || (e = edge_node_src(c, row[4], &q.o)))
                return e;
            q.t = c->up_len[key];
            if ((e = counts_enqueue(c, q, d_counts + count * n, d_lnl + count))) return e;
            edges_out[2 * count] = row[3];
            edges_out[2 * count + 1] = row[4];
            lengths_out[count++] = q.t;
            return PU_OK;
        },
        [&] {
            h.to_host(counts_out, d_counts, count * n);
            h.to_host(edge_lnl_out, d_lnl, count);
            if (const int e = h.finish("pu_counts_sweep")) return e;
            *n_edges_out = (int)count;
            return c->c_timer.stamp(c);
        });
}

int pu_counts_kernel_ms(pu_ctx *c, double *ms_out) {
    if (!c || !ms_out) return set_err(c ? &c->err : nullptr, PU_E_ARG, "null argument");
    *ms_out = (double)c->c_timer.ms;
    return PU_OK;
}

}  // extern "C"
