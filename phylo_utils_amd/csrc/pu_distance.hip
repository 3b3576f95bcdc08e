// pu_distance.hip -- pairwise maximum-likelihood distances and their variances for all taxon
// pairs of a coded alignment, and the C ABI of it (pu_pair_counts, pu_pair_distances,
// pu_pair_distances_device).
//
// Reference behaviour (paths relative to the reference repository root):
//   optimise(model, partials_a, partials_b, min_brlen, max_brlen)  phylo_utils/likelihood.py:226-236
//   returns (t, -1 / lnL''(t)) of the two-sequence likelihood; brent_optimise / scipy_optimise
//   beside it.  That module needs the missing `likcalc` and cannot run upstream; what it
//   computes is restated here (normative):
//     lnL_ab(t) = sum_{u,v} N_ab[u][v] log F_uv(t)
//     N_ab[u][v] = sum_s w_s [code_a(s) = u][code_b(s) = v]
//     F_uv(t)   = sum_m L[u][m] R[v][m] g_m(t),  L[u][m] = sum_i pi_i x_u[i] E[i][m],
//                                                R[v][m] = sum_j E^-1[m][j] x_v[j]
//     g_m = sum_c q_c e^{l_m r_c t}, g'_m = sum_c q_c (l_m r_c) e^{..}, g''_m = sum_c q_c (l_m r_c)^2 e^{..}
//   F is evaluated as F_uv(0) + sum_m L[u][m] R[v][m] h_m(t), h_m = g_m(t) - g_m(0) = sum_c q_c
//   expm1(l_m r_c t) and F_uv(0) = (sum_c q_c) sum_i pi_i x_u[i] x_v[i] (E E^-1 = 1): at short
//   lengths a mismatch bin's F is of order t, and the plain sum loses it among terms of order 1
//   and F' = F'' = 0 exactly for a bin whose code u or v has a constant tip vector (gap, N, X:
//   F does not depend on t there).
//
//   k_pair_counts  one wave per workgroup; the workgroup owns P consecutive pairs of the pair
//                  list (for the default list, all i < j row-major, that is a strip of the
//                  taxa x taxa triangle: one row taxon against P consecutive column taxa) and
//                  one segment of the sites.  It stages 128-site chunks of its 2 P code rows and
//                  of the weights in LDS with coalesced row reads, then lane p walks the chunk
//                  for pair p alone and adds each weight into pair p's own n_codes^2 fp64 bins
//                  in LDS: every bin has one writer, so there are no atomics, no lanes meeting
//                  on DNA's few hot bins, and the adds of a bin run in site order.  The bins
//                  are written once, as the segment's slab; k_pair_merge adds the slabs of a
//                  pair in segment order.  The segmentation depends on n_sites alone, so the
//                  counts do not depend on the pair chunking, the grid or the run.
//   k_pair_newton  one wave per pair, four pairs per workgroup; L, R, the eigenvalues, rates and
//                  category weights in LDS, the pair's counts in registers (16 bins per lane).
//                  Each evaluation: lanes m < K build g, g', g'' (C exponentials each) and pass
//                  them through LDS to every lane's registers; the lanes run over their non-zero
//                  bins; a fixed-order butterfly adds the three sums.  The safeguarded Newton
//                  loop on lnL'(t) = 0 is wave-uniform and runs to the end inside the launch.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdlib.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "pu_ctx.h"
#include "pu_service.h"

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "pu_distance.hip: gfx950 only, as the other kernel files of this library"
#endif

using namespace pu;

namespace {

constexpr int kMaxCat = PU_PAIR_MAX_CAT;            // rates and weights in LDS
constexpr size_t kCountLds = 40 * 1024;             // LDS of one k_pair_counts workgroup
constexpr size_t kDistWsBytes = (size_t)256 << 20;  // count matrices (and slabs) of one chunk
constexpr int kNW = 4;                              // k_pair_newton: pairs (waves) per workgroup
constexpr int kBinsPerLane = kMaxCodes * kMaxCodes / 64;

struct CountArgs {
    const uint8_t *codes;  // [n_taxa][ld]
    int64_t ld, S;
    const double *w;       // [S] or null: 1
    const int32_t *pairs;  // [n_pairs][2], this launch's
    int64_t n_pairs;
    int n_codes, P;        // P: pairs per workgroup
    int64_t seg;           // sites per segment (a multiple of kCH); blockIdx.y: the segment
    double *out;           // [segments][n_pairs][n_codes^2]
};

__host__ inline size_t count_lds(int n_codes, int P) {
    return ((size_t)P * bin_stride(n_codes) + kCH) * 8 + (size_t)2 * P * kRow;
}

__global__ void __launch_bounds__(64) k_pair_counts(CountArgs a) {
    extern __shared__ double lds[];
    const int lane = (int)threadIdx.x;
    const int n = a.n_codes, nb = n * n, bs = bin_stride(n);
    double *bins = lds;                    // [P][bs]
    double *wl = bins + (size_t)a.P * bs;  // [kCH]
    uint8_t *st = reinterpret_cast<uint8_t *>(wl + kCH);  // [2 P][kRow]
    const int64_t p0 = (int64_t)blockIdx.x * a.P;
    const int np = (int)min((int64_t)a.P, a.n_pairs - p0);
    const int64_t s_lo = (int64_t)blockIdx.y * a.seg, s_hi = min(a.S, s_lo + a.seg);
    for (int i = lane; i < np * bs; i += 64) bins[i] = 0.0;
    const int32_t *rows = a.pairs + 2 * p0;  // staged row r = 2 p + side is taxon rows[r]
    double *mine = bins + (size_t)lane * bs;
    const uint32_t *sa = reinterpret_cast<const uint32_t *>(st + (size_t)2 * lane * kRow);
    const uint32_t *sb = reinterpret_cast<const uint32_t *>(st + (size_t)(2 * lane + 1) * kRow);
    for (int64_t s0 = s_lo; s0 < s_hi; s0 += kCH) {
        const int m = (int)min((int64_t)kCH, s_hi - s0);
        __syncthreads();  // the previous chunk has been consumed
        for (int r = 0; r < 2 * np; ++r) {
            const uint8_t *src = a.codes + (int64_t)rows[r] * a.ld + s0;
            for (int c = lane; c < kCH; c += 64) st[r * kRow + c] = c < m ? src[c] : (uint8_t)255;
        }
        for (int c = lane; c < kCH; c += 64) wl[c] = c < m ? (a.w ? a.w[s0 + c] : 1.0) : 0.0;
        __syncthreads();
        if (lane < np) {
            for (int c4 = 0; c4 < (m + 3) / 4; ++c4) {
                uint32_t ua = sa[c4], ub = sb[c4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int u = (int)(ua & 255u), v = (int)(ub & 255u);
                    ua >>= 8;
                    ub >>= 8;
                    // a code outside the table (the padding's 255 too) counts nowhere
                    if (u < n && v < n) mine[u * n + v] += wl[4 * c4 + k];
                }
            }
        }
    }
    __syncthreads();
    double *out = a.out + ((size_t)blockIdx.y * a.n_pairs + p0) * nb;
    for (int p = 0; p < np; ++p)
        for (int i = lane; i < nb; i += 64) out[(size_t)p * nb + i] = bins[(size_t)p * bs + i];
}

// counts[e] = slab_0[e] + slab_1[e] + ... in segment order
__global__ void __launch_bounds__(256)
    k_pair_merge(const double *__restrict__ slabs, int n_seg, size_t n, double *__restrict__ out) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    double acc = slabs[e];
    for (int g = 1; g < n_seg; ++g) acc = __dadd_rn(acc, slabs[(size_t)g * n + e]);
    out[e] = acc;
}

struct NewtonPairArgs {
    const double *model;   // L [n_codes][K], R [n_codes][K], evals [K], rates [C], weights [C],
                           // F(0) [n_codes][n_codes]
    const double *counts;  // [n_pairs][n_codes^2]
    const double *t0;      // [n_pairs] or null
    double *out5;          // [n_pairs][5]
    int64_t n_pairs;
    int n_codes, C;
    uint32_t flat;         // bit u: the tip vector of code u is constant
    double lo, hi, tol;
    int max_iter;
};

__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) x = __dadd_rn(x, __shfl_xor(x, o, 64));
    return x;  // a + b == b + a bit for bit: every lane holds the same sum
}

template <int K>
__global__ void __launch_bounds__(64 * kNW) k_pair_newton(NewtonPairArgs a) {
    __shared__ double sL[kMaxCodes * K], sR[kMaxCodes * K], slam[K], sr[kMaxCat], sq[kMaxCat];
    __shared__ double sg[kNW][3][K], sF0[kMaxCodes * kMaxCodes];
    const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int n = a.n_codes, nb = n * n, C = a.C;
    for (int i = tid; i < n * K; i += 64 * kNW) {
        sL[i] = a.model[i];
        sR[i] = a.model[n * K + i];
    }
    if (tid < K) slam[tid] = a.model[2 * n * K + tid];
    for (int i = tid; i < C; i += 64 * kNW) {
        sr[i] = a.model[2 * n * K + K + i];
        sq[i] = a.model[2 * n * K + K + C + i];
    }
    for (int i = tid; i < nb; i += 64 * kNW) sF0[i] = a.model[2 * n * K + K + 2 * C + i];
    __syncthreads();
    const int64_t pair = (int64_t)blockIdx.x * kNW + w;
    if (pair >= a.n_pairs) return;  // whole waves leave; nothing below synchronises workgroups

    // this lane's bins: b = lane + 64 i
    double N[kBinsPerLane];
    int uv[kBinsPerLane];
    const double *cnt = a.counts + (size_t)pair * nb;
#pragma unroll
    for (int i = 0; i < kBinsPerLane; ++i) {
        const int b = lane + 64 * i;
        N[i] = b < nb ? cnt[b] : 0.0;
        const int u = b < nb ? b / n : 0, v = b < nb ? b - u * n : 0;
        uv[i] = (u * K) | ((v * K) << 10) | ((((a.flat >> u) | (a.flat >> v)) & 1u) << 20);
    }

    double l, d1, d2;  // the last evaluation's sums (wave-uniform)
    int evals = 0;
    auto eval = [&](double t) {
        if (lane < K) {
            const double lam = slam[lane];
            double g0 = 0.0, g1 = 0.0, g2 = 0.0;
            for (int c = 0; c < C; ++c) {
                const double x = lam * sr[c], e = sq[c] * exp(x * t);
                g0 = fma(sq[c], expm1(x * t), g0);
                g1 = fma(x, e, g1);
                g2 = fma(x * x, e, g2);
            }
            sg[w][0][lane] = g0;
            sg[w][1][lane] = g1;
            sg[w][2][lane] = g2;
        }
        // one wave: its LDS accesses complete in program order; keep the compiler to it
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
        double g[3][K];
#pragma unroll
        for (int m = 0; m < K; ++m) {
            g[0][m] = sg[w][0][m];
            g[1][m] = sg[w][1][m];
            g[2][m] = sg[w][2][m];
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
        double al = 0.0, a1 = 0.0, a2 = 0.0;
        int bad = 0;
#pragma unroll
        for (int i = 0; i < kBinsPerLane; ++i) {
            if (N[i] == 0.0) continue;
            const double *Lu = sL + (uv[i] & 1023), *Rv = sR + ((uv[i] >> 10) & 1023);
            double F = sF0[lane + 64 * i], F1 = 0.0, F2 = 0.0;
#pragma unroll
            for (int m = 0; m < K; ++m) {
                const double lr = Lu[m] * Rv[m];
                F = fma(lr, g[0][m], F);
                F1 = fma(lr, g[1][m], F1);
                F2 = fma(lr, g[2][m], F2);
            }
            if ((uv[i] >> 20) & 1) F1 = F2 = 0.0;
            if (!(F > 0.0)) {
                bad = 1;
                continue;
            }
            al = fma(N[i], log(F), al);
            a1 = fma(N[i], F1 / F, a1);
            a2 = fma(N[i], (F2 * F - F1 * F1) / (F * F), a2);
        }
        l = wave_sum(al);
        d1 = wave_sum(a1);
        d2 = wave_sum(a2);
        if (__any(bad)) l = -INFINITY;
        ++evals;
    };
    double *out = a.out5 + 5 * pair;
    auto finish = [&](double t) {
        if (lane == 0) {
            const bool ok = l > -INFINITY;  // a bin with N > 0 and F <= 0: lnL = -inf, no optimum
            out[0] = ok ? t : NAN;
            out[1] = l;
            out[2] = ok ? d1 : NAN;
            out[3] = ok ? d2 : NAN;
            out[4] = (double)evals;
        }
    };
    const double lo = a.lo, hi = a.hi;
    double t = a.t0 ? a.t0[pair] : sqrt(lo * hi);
    if (a.max_iter == 0) {
        eval(t);
        return finish(t);
    }
    eval(lo);
    if (!(l > -INFINITY) || d1 <= 0.0) return finish(lo);
    eval(hi);
    if (!(l > -INFINITY) || d1 >= 0.0) return finish(hi);
    double ba = lo, bb = hi;  // lnL'(ba) > 0 > lnL'(bb)
    if (!(t > ba && t < bb)) t = sqrt(lo * hi);
    for (int it = 0; it < a.max_iter; ++it) {
        eval(t);
        if (!(l > -INFINITY) || d1 == 0.0) break;
        if (d1 > 0.0) ba = t;
        else bb = t;
        double tn = d2 < 0.0 ? t - d1 / d2 : NAN;
        // closed bounds: t is an end of the bracket by now and its step points inwards; at the
        // root the step falls below t's spacing and tn == t must count as a step of zero
        if (!(tn >= ba && tn <= bb)) tn = 0.5 * (ba + bb);
        const double step = tn - t;
        if (fabs(step) < a.tol) {  // the step is taken and the result evaluated where it lands
            t = tn;
            eval(t);
            break;
        }
        if (it + 1 < a.max_iter) t = tn;  // out of iterations: the last evaluated point stands
    }
    finish(t);
}

// ---- host side ---------------------------------------------------------------------------

// per-device buffers of the pair calls and their host staging copies (DevState: pu_service.h)
struct DistState : DevState {
    PairList pairs;
    DevBuf<double> t0, model, counts, slabs;
    std::vector<double> h_t0, h_model;
    ChunkProfile prof;
};
DistState g_dist[64];

struct ModelIn {
    int K, C;
    const double *table, *evecs, *evals, *ivecs, *freqs, *rates, *cw;
};
struct Opt {
    const double *t0;
    double lo, hi, tol;
    int max_iter;
};

int check_model(const char *fn, const ModelIn &m, const Opt &o, int64_t n_pairs) {
    if (!m.table || !m.evecs || !m.evals || !m.ivecs || !m.freqs || !m.rates || !m.cw)
        return set_err(nullptr, PU_E_ARG, "%s: null model buffer", fn);
    if (m.K != 2 && m.K != 4 && m.K != 20)
        return set_err(nullptr, PU_E_ARG, "%s: K = %d is not supported (2, 4, 20)", fn, m.K);
    if (m.C < 1 || m.C > kMaxCat)
        return set_err(nullptr, PU_E_ARG, "%s: n_cat = %d is outside [1, %d]", fn, m.C, kMaxCat);
    if (!(0.0 < o.lo && o.lo < o.hi) || !(o.hi < INFINITY))
        return set_err(nullptr, PU_E_ARG, "%s: bounds need 0 < lo < hi (%g, %g)", fn, o.lo, o.hi);
    if (!(o.tol > 0.0) || o.max_iter < 0)
        return set_err(nullptr, PU_E_ARG, "%s: tol = %g, max_iter = %d", fn, o.tol, o.max_iter);
    if (o.t0)
        for (int64_t p = 0; p < n_pairs; ++p)
            if (!(o.t0[p] >= o.lo && o.t0[p] <= o.hi))
                return set_err(nullptr, PU_E_ARG, "%s: t0[%lld] = %g is outside [%g, %g]", fn,
                               (long long)p, o.t0[p], o.lo, o.hi);
    return PU_OK;
}

// the model as k_pair_newton reads it: L [n][K], R [n][K], evals [K], rates [C], weights [C],
// F(0) [n][n]; returns the mask of the codes whose tip vector is constant
uint32_t pack_model(const ModelIn &m, int n, std::vector<double> &h) {
    const int K = m.K, C = m.C;
    uint32_t flat = 0;
    h.assign((size_t)2 * n * K + K + 2 * C + (size_t)n * n, 0.0);
    double *L = h.data(), *R = L + (size_t)n * K;
    for (int u = 0; u < n; ++u) {
        const double *x = m.table + (size_t)u * K;
        bool same = true;
        for (int i = 1; i < K; ++i) same = same && x[i] == x[0];
        if (same) flat |= 1u << u;
        for (int k = 0; k < K; ++k) {
            double accl = 0.0, accr = 0.0;
            for (int i = 0; i < K; ++i) {
                accl += m.freqs[i] * x[i] * m.evecs[(size_t)i * K + k];
                accr += m.ivecs[(size_t)k * K + i] * x[i];
            }
            L[(size_t)u * K + k] = accl;
            R[(size_t)u * K + k] = accr;
        }
    }
    std::copy(m.evals, m.evals + K, R + (size_t)n * K);
    std::copy(m.rates, m.rates + C, R + (size_t)n * K + K);
    std::copy(m.cw, m.cw + C, R + (size_t)n * K + K + C);
    double Q = 0.0, *F0 = R + (size_t)n * K + K + 2 * C;
    for (int c = 0; c < C; ++c) Q += m.cw[c];
    for (int u = 0; u < n; ++u)
        for (int v = 0; v < n; ++v) {
            double acc = 0.0;
            for (int i = 0; i < K; ++i)
                acc += m.freqs[i] * m.table[(size_t)u * K + i] * m.table[(size_t)v * K + i];
            F0[(size_t)u * n + v] = Q * acc;
        }
    return flat;
}

// sites per segment of k_pair_counts: a function of n_sites alone (at most 32 segments)
int64_t seg_sites(int64_t S) {
    const int64_t per = ((S + 31) / 32 + kCH - 1) / kCH * kCH;
    return std::max<int64_t>(2 * kCH, per);
}

// pairs per chunk: count matrices and slabs within kDistWsBytes, or PU_DIST_CHUNK
int64_t pair_chunk(int n_codes, int n_seg, int64_t n_pairs) {
    const size_t per = (size_t)n_codes * n_codes * 8 * (size_t)(1 + (n_seg > 1 ? n_seg : 0));
    const int64_t chunk = std::max<int64_t>(1, (int64_t)(kDistWsBytes / per));
    return std::min(env_cap("PU_DIST_CHUNK", chunk), n_pairs);
}

// the model packed into the state's buffer, uploaded on st, and what k_pair_newton's arguments
// take from it and from the options; counts, t0, out5 and n_pairs are the launch's own
int newton_args(DistState &D, hipStream_t st, const ModelIn &m, int n, const Opt &o,
                NewtonPairArgs *q) {
    q->flat = pack_model(m, n, D.h_model);
    if (int rc = D.model.reserve(D.h_model.size())) return rc;
    HIPCHK(nullptr, hipMemcpyAsync(D.model.p, D.h_model.data(), D.h_model.size() * 8,
                                   hipMemcpyHostToDevice, st));
    q->model = D.model.p;
    q->t0 = nullptr;
    q->n_codes = n;
    q->C = m.C;
    q->lo = o.lo;
    q->hi = o.hi;
    q->tol = o.tol;
    q->max_iter = o.max_iter;
    return PU_OK;
}

int launch_newton(const NewtonPairArgs &q, int K, hipStream_t st) {
    const dim3 grid((unsigned)((q.n_pairs + kNW - 1) / kNW));
    if (K == 2) hipLaunchKernelGGL(k_pair_newton<2>, grid, dim3(64 * kNW), 0, st, q);
    else if (K == 4) hipLaunchKernelGGL(k_pair_newton<4>, grid, dim3(64 * kNW), 0, st, q);
    else hipLaunchKernelGGL(k_pair_newton<20>, grid, dim3(64 * kNW), 0, st, q);
    HIPCHK(nullptr, hipGetLastError());
    return PU_OK;
}

// the work of every pair call, queued on st: counts of each chunk of pairs into the state's
// buffer, then -- with a model -- k_pair_newton on them into d_out5, or -- without -- the counts
// copied to counts_host.  d_codes / d_w are device buffers.
int run_pairs(int device, hipStream_t st, const Shape &s, const uint8_t *d_codes, int64_t ld,
              const double *d_w, const ModelIn *m, const Opt *o, double *d_out5,
              double *counts_host) {
    DistState &D = g_dist[device];
    StateScope scope(D, st);
    int rc;
    if ((rc = scope.rc)) return rc;
    const int n = s.n_codes, nb = n * n;
    if ((rc = D.pairs.upload(st, s.n_taxa, s.n_pairs, s.pairs))) return rc;
    NewtonPairArgs q;
    if (m) {
        if ((rc = newton_args(D, st, *m, n, *o, &q))) return rc;
        if (o->t0) {
            D.h_t0.assign(o->t0, o->t0 + s.n_pairs);
            if ((rc = D.t0.reserve(D.h_t0.size()))) return rc;
            HIPCHK(nullptr, hipMemcpyAsync(D.t0.p, D.h_t0.data(), D.h_t0.size() * 8,
                                           hipMemcpyHostToDevice, st));
        }
    }
    const int64_t seg = seg_sites(s.n_sites);
    const int n_seg = (int)((s.n_sites + seg - 1) / seg);
    const int64_t chunk = pair_chunk(n, n_seg, s.n_pairs);
    if ((rc = D.counts.reserve((size_t)chunk * nb))) return rc;
    if (n_seg > 1 && (rc = D.slabs.reserve((size_t)n_seg * chunk * nb))) return rc;
    const int P = (int)std::min<size_t>(64, kCountLds / ((size_t)bin_stride(n) * 8 + 2 * kRow));
    if ((rc = D.prof.reserve((s.n_pairs + chunk - 1) / chunk))) return rc;
    for (int64_t p0 = 0; p0 < s.n_pairs; p0 += chunk) {
        const int64_t np = std::min(chunk, s.n_pairs - p0);
        if ((rc = D.prof.mark(0, st))) return rc;
        CountArgs a;
        a.codes = d_codes;
        a.ld = ld;
        a.S = s.n_sites;
        a.w = d_w;
        a.pairs = D.pairs.d.p + 2 * p0;
        a.n_pairs = np;
        a.n_codes = n;
        a.P = P;
        a.seg = seg;
        a.out = n_seg > 1 ? D.slabs.p : D.counts.p;
        const dim3 grid((unsigned)((np + P - 1) / P), (unsigned)n_seg);
        hipLaunchKernelGGL(k_pair_counts, grid, dim3(64), count_lds(n, P), st, a);
        HIPCHK(nullptr, hipGetLastError());
        if (n_seg > 1) {
            const size_t ne = (size_t)np * nb;
            hipLaunchKernelGGL(k_pair_merge, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, st,
                               D.slabs.p, n_seg, ne, D.counts.p);
            HIPCHK(nullptr, hipGetLastError());
        }
        if ((rc = D.prof.mark(1, st))) return rc;
        if (m) {
            q.counts = D.counts.p;
            q.t0 = o->t0 ? D.t0.p + p0 : nullptr;
            q.out5 = d_out5 + 5 * p0;
            q.n_pairs = np;
            if ((rc = launch_newton(q, m->K, st))) return rc;
        } else {
            HIPCHK(nullptr, hipMemcpyAsync(counts_host + (size_t)p0 * nb, D.counts.p,
                                           (size_t)np * nb * 8, hipMemcpyDeviceToHost, st));
        }
        if ((rc = D.prof.mark(2, st))) return rc;
    }
    return PU_OK;
}

}  // namespace

// ---- for pu_bootstrap.hip: the Newton step on count matrices that are already on the device

namespace pu {

int pair_check_model(const char *fn, const PairModel &pm, double lo, double hi, double tol,
                     int max_iter) {
    if (pm.n_codes < 1 || pm.n_codes > kMaxCodes)
        return set_err(nullptr, PU_E_ARG, "%s: n_codes = %d is outside [1, %d]", fn, pm.n_codes,
                       kMaxCodes);
    const ModelIn m{pm.K, pm.C, pm.table, pm.evecs, pm.evals, pm.ivecs, pm.freqs, pm.rates, pm.cw};
    const Opt o{nullptr, lo, hi, tol, max_iter};
    return check_model(fn, m, o, 0);
}

// k_pair_newton over d_counts [n_batch][rows][n_codes^2], queued on st; the row of (b, i) lands
// at d_out5 + 5 (b out_stride + i).  The start is sqrt(lo hi), as in a pair call without t0.
int pair_newton_device(int device, hipStream_t st, const PairModel &pm, double lo, double hi,
                       double tol, int max_iter, const double *d_counts, int64_t n_batch,
                       int64_t rows, double *d_out5, int64_t out_stride) {
    DistState &D = g_dist[device];
    StateScope scope(D, st);
    int rc;
    if ((rc = scope.rc)) return rc;
    const ModelIn m{pm.K, pm.C, pm.table, pm.evecs, pm.evals, pm.ivecs, pm.freqs, pm.rates, pm.cw};
    const int n = pm.n_codes;
    NewtonPairArgs q;
    if ((rc = newton_args(D, st, m, n, Opt{nullptr, lo, hi, tol, max_iter}, &q))) return rc;
    const bool one = out_stride == rows;  // the rows of all batches are one list
    const int64_t n_launch = one ? 1 : n_batch;
    q.n_pairs = one ? n_batch * rows : rows;
    for (int64_t b = 0; b < n_launch; ++b) {
        q.counts = d_counts + (size_t)b * rows * n * n;
        q.out5 = d_out5 + 5 * b * out_stride;
        if ((rc = launch_newton(q, m.K, st))) return rc;
    }
    return PU_OK;
}

}  // namespace pu

extern "C" {

int pu_pair_counts(int device, const uint8_t *codes, int n_taxa, int64_t n_sites, int n_codes,
                   const double *site_weights, int64_t n_pairs, const int32_t *pairs,
                   double *counts_out) {
    const char *fn = "pu_pair_counts";
    const Shape s{n_taxa, n_codes, n_sites, n_pairs, pairs, 1};
    int rc;
    if ((rc = check_shape(fn, s, !codes))) return rc;
    if (!counts_out) return set_err(nullptr, PU_E_ARG, "%s: null output", fn);
    if ((rc = check_codes(fn, codes, n_taxa, n_sites, n_codes))) return rc;
    if ((rc = check_device(device))) return rc;
    DeviceGuard g(device);
    HostCall h(device);
    const uint8_t *d_codes = h.to_device(codes, (size_t)n_taxa * n_sites);
    const double *d_w = h.to_device(site_weights, (size_t)n_sites);
    if (!h.rc)
        h.rc = run_pairs(device, h.st, s, d_codes, n_sites, d_w, nullptr, nullptr, nullptr,
                         counts_out);
    return h.finish(fn);
}

int pu_pair_distances_device(int device, void *stream, int n_states, int n_cat, int n_codes,
                             const double *code_table, const double *evecs, const double *evals,
                             const double *ivecs, const double *freqs, const double *rates,
                             const double *cat_weights, const uint8_t *d_codes, int64_t ld,
                             int n_taxa, int64_t n_sites, const double *d_site_weights,
                             int64_t n_pairs, const int32_t *pairs, const double *t0, double lo,
                             double hi, double tol, int max_iter, double *d_out5) {
    const char *fn = "pu_pair_distances_device";
    const Shape s{n_taxa, n_codes, n_sites, n_pairs, pairs, 1};
    const ModelIn m{n_states, n_cat, code_table, evecs, evals, ivecs, freqs, rates, cat_weights};
    const Opt o{t0, lo, hi, tol, max_iter};
    int rc;
    if ((rc = check_shape(fn, s, !d_codes))) return rc;
    if (!d_out5) return set_err(nullptr, PU_E_ARG, "%s: null output", fn);
    if (ld < n_sites)
        return set_err(nullptr, PU_E_ARG, "%s: row stride %lld below n_sites = %lld", fn,
                       (long long)ld, (long long)n_sites);
    if ((rc = check_model(fn, m, o, n_pairs))) return rc;
    if ((rc = check_device(device))) return rc;
    DeviceGuard g(device);
    return run_pairs(device, (hipStream_t)stream, s, d_codes, ld, d_site_weights, &m, &o, d_out5,
                     nullptr);
}

int pu_pair_distances(int device, int n_states, int n_cat, int n_codes, const double *code_table,
                      const double *evecs, const double *evals, const double *ivecs,
                      const double *freqs, const double *rates, const double *cat_weights,
                      const uint8_t *codes, int n_taxa, int64_t n_sites,
                      const double *site_weights, int64_t n_pairs, const int32_t *pairs,
                      const double *t0, double lo, double hi, double tol, int max_iter,
                      double *out5) {
    const char *fn = "pu_pair_distances";
    const Shape s{n_taxa, n_codes, n_sites, n_pairs, pairs, 1};
    const ModelIn m{n_states, n_cat, code_table, evecs, evals, ivecs, freqs, rates, cat_weights};
    const Opt o{t0, lo, hi, tol, max_iter};
    int rc;
    if ((rc = check_shape(fn, s, !codes))) return rc;
    if (!out5) return set_err(nullptr, PU_E_ARG, "%s: null output", fn);
    if ((rc = check_model(fn, m, o, n_pairs))) return rc;
    if ((rc = check_codes(fn, codes, n_taxa, n_sites, n_codes))) return rc;
    if ((rc = check_device(device))) return rc;
    DeviceGuard g(device);
    HostCall h(device);
    const uint8_t *d_codes = h.to_device(codes, (size_t)n_taxa * n_sites);
    const double *d_w = h.to_device(site_weights, (size_t)n_sites);
    double *d_out = h.alloc<double>(5 * (size_t)n_pairs);
    if (!h.rc) h.rc = run_pairs(device, h.st, s, d_codes, n_sites, d_w, &m, &o, d_out, nullptr);
    h.to_host(out5, d_out, 5 * (size_t)n_pairs);
    return h.finish(fn);
}

int pu_pair_profile(int device, int on) { return profile_set(g_dist, device, on); }

int pu_pair_kernel_ms(int device, double *counts_ms, double *newton_ms) {
    return profile_ms("pu_pair_kernel_ms", g_dist, device, counts_ms, newton_ms);
}

}  // extern "C"
