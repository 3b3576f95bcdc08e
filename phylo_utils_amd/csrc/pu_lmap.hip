// pu_lmap.hip -- likelihood mapping on the GPU: the quartets of a mapping, the
// weighted code 4-tuple counts of every quartet, and the maximum-likelihood score of the three
// four-taxon trees of every quartet with all five lengths optimised; and the C ABI of it
// (pu_lmap_quartets, pu_lmap_bins, pu_lmap_scores, pu_lmap_scores_device, pu_lmap_profile,
// pu_lmap_kernel_ms).
//
// The reference has no likelihood mapping; the rule is this project's own (DESIGN 4.30,
// normative; tests/lmap_reference.py restates it on the oracle).  Topology tau of quartet
// (a, b, c, d) has tips (p, q | r, s) = (a, b | c, d), (a, c | b, d), (a, d | b, c) and lengths
// (l_p, l_q, l_r, l_s, l_i):
//     L_s = sum_c q_c sum_i pi_i (P_c(l_p) x_p)_i (P_c(l_q) x_q)_i
//                     sum_j P_c(l_i)[i][j] (P_c(l_r) x_r)_j (P_c(l_s) x_s)_j,   lnL = sum_s w_s log L_s
// with no scaler.  A round optimises p, q, r, s, i in turn by the rule of pu_newton.h.
//
//   k_lmap_quartets  a lane per quartet: the unranked combination (all quartets), the mixed-radix
//                    member indices (all quartets of four clusters) or the Philox draws.
//   k_lmap_bins      a workgroup per (quartet, segment of patterns): the weights of the patterns
//                    whose four codes are the tuple (u_a, u_b, u_c, u_d) of codes in use, added in
//                    unsigned 64-bit integers into LDS bins and from there into the quartet's
//                    n_used^4 global bins, both with integer atomics: no order to depend on.
//   k_lmap_opt<K>    a workgroup per (quartet, topology) runs the whole schedule: it keeps in LDS
//                    the model, the tip tables T_e[c][u][.] = P_c(l_e) x_u of the four tip edges
//                    and P_c(l_i), and rebuilds per evaluation only what the edge in hand
//                    changes: its own table with the two derivative tables (a tip edge), or K C
//                    exponentials (the internal edge, which is evaluated in the eigen-basis:
//                    sum_m (X E)_m (E^-1 W)_m e^{l_m r_c t} (l_m r_c)^o).  The items are the
//                    patterns (a lane takes patterns tid, tid + T, ... in ascending order) or
//                    the non-zero bins (likewise, in ascending bin index); a lane's sums are added
//                    by a 64-lane butterfly and the waves' sums in wave order.  Every thread
//                    steps its own copy of the NewtonState on the same sums.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "pu_ctx.h"
#include "pu_newton.h"
#include "pu_philox.h"
#include "pu_service.h"

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "pu_lmap.hip: gfx950 only, as the other kernel files of this library"
#endif

using namespace pu;

namespace {

constexpr int kMaxCat = PU_PAIR_MAX_CAT;
constexpr size_t kWsBytes = (size_t)256 << 20;  // the bins of one chunk of quartets
constexpr size_t kLdsCap = 160 * 1024;          // LDS one workgroup may have
constexpr int kMaxBins = 4096;                  // n_used^4 of the bins feed
constexpr int kTBPat = 256;                     // threads of k_lmap_opt over patterns
constexpr int kTBBin = 64;                      // ... over bins: a few hundred items, one wave
constexpr int kTB = 256;                        // k_lmap_quartets, k_lmap_bins

// ---- quartets ---------------------------------------------------------------------------------

struct QuartetArgs {
    int n;                   // taxa (no clusters)
    int clustered, all;      // all: every quartet in order, nothing drawn
    int32_t size[4], off[4];  // clusters: members [off[k], off[k] + size[k]) of `members`
    const int32_t *members;  // ascending within a cluster
    uint64_t seed;
    int64_t Q;
    int32_t *out;  // [Q][4]
};

__device__ __forceinline__ int64_t choose(int64_t x, int r) {  // C(x, r), r <= 3, in range here
    if (x < r) return 0;
    if (r == 0) return 1;
    if (r == 1) return x;
    if (r == 2) return x * (x - 1) / 2;
    return x * (x - 1) / 2 * (x - 2) / 3;
}

__global__ void __launch_bounds__(kTB) k_lmap_quartets(QuartetArgs a) {
    const int64_t g = (int64_t)blockIdx.x * kTB + threadIdx.x;
    if (g >= a.Q) return;
    int32_t t[4];
    if (a.clustered) {
        int64_t rest = g;
        for (int k = 3; k >= 0; --k) {
            const int64_t s = a.size[k];
            int64_t idx;
            if (a.all) {
                idx = k ? rest % s : rest;
                rest /= s;
            } else {
                idx = (int64_t)floor(philox_u(a.seed, (uint64_t)g, (uint32_t)(4 + k), 3u) * (double)s);
            }
            idx = min(idx, s - 1);
            t[k] = a.members[a.off[k] + idx];
        }
    } else if (a.all) {  // the g-th of all a < b < c < d in lexicographic order
        int64_t rest = g;
        int v = 0;
        for (int k = 0; k < 4; ++k) {
            for (;; ++v) {
                const int64_t with_v = choose(a.n - 1 - v, 3 - k);
                if (rest < with_v || v >= a.n - 1) break;
                rest -= with_v;
            }
            t[k] = v++;
        }
    } else {  // four draws without replacement, kept in draw order
        int32_t sorted[4];
        for (int k = 0; k < 4; ++k) {
            const int left = a.n - k;
            const double u = philox_u(a.seed, (uint64_t)g, (uint32_t)k, 3u);
            int v = min((int)floor(u * (double)left), left - 1);
            int pos = 0;
            for (; pos < k && sorted[pos] <= v; ++pos) ++v;
            for (int j = k; j > pos; --j) sorted[j] = sorted[j - 1];
            sorted[pos] = v;
            t[k] = v;
        }
    }
    for (int k = 0; k < 4; ++k) a.out[4 * g + k] = t[k];
}

// ---- bins -------------------------------------------------------------------------------------

struct BinArgs {
    const uint8_t *codes;  // [n_taxa][ld]
    int64_t ld, S;
    const double *w;          // [S] non-negative integers, or null: 1
    const int32_t *quartets;  // [nq][4], this launch's
    int n_taxa, nu, nbins;    // nbins = nu^4 <= kMaxBins
    uint8_t remap[kMaxCodes];  // code -> its index among the codes in use, or 255
    int64_t seg;              // patterns per blockIdx.y
    unsigned long long *out;  // [nq][nbins], zeroed
};

__global__ void __launch_bounds__(kTB) k_lmap_bins(BinArgs a) {
    extern __shared__ unsigned long long sbins[];
    const int tid = (int)threadIdx.x;
    for (int i = tid; i < a.nbins; i += kTB) sbins[i] = 0ull;
    __syncthreads();
    const int32_t *tx = a.quartets + 4 * (int64_t)blockIdx.x;
    bool ok = true;
    for (int k = 0; k < 4; ++k) ok = ok && (unsigned)tx[k] < (unsigned)a.n_taxa;
    const int64_t s_lo = (int64_t)blockIdx.y * a.seg, s_hi = min(a.S, s_lo + a.seg);
    if (ok)
        for (int64_t s = s_lo + tid; s < s_hi; s += kTB) {
            const unsigned long long w = a.w ? (unsigned long long)a.w[s] : 1ull;
            int b = 0;
            bool in = w != 0ull;
            for (int k = 0; k < 4; ++k) {
                const int u = a.remap[a.codes[(int64_t)tx[k] * a.ld + s] & (kMaxCodes - 1)];
                in = in && u < a.nu;
                b = b * a.nu + u;
            }
            if (in) atomicAdd(&sbins[b], w);
        }
    __syncthreads();
    unsigned long long *out = a.out + (int64_t)blockIdx.x * a.nbins;
    for (int i = tid; i < a.nbins; i += kTB)
        if (sbins[i]) atomicAdd(&out[i], sbins[i]);
}

// ---- the optimiser ----------------------------------------------------------------------------

struct OptArgs {
    const double *model;  // E [K][K], E^-1 [K][K], evals [K], pi [K], rates [C], weights [C],
                          // table [n][K]
    const uint8_t *codes;  // patterns feed: [n_taxa][ld]; null: the bins feed
    int64_t ld, S;
    const double *w;                 // [S] or null: 1
    const unsigned long long *bins;  // bins feed: [nq][nbins] over the n codes of `table`
    int nbins;
    const int32_t *quartets;  // [nq][4], this launch's
    int n_taxa, n, C;         // n: rows of table
    double t0[5], tol, min_gain;
    int max_iter, max_rounds;
    double *out;     // [nq][3][8]
    double *derivs;  // [nq][3][5][2] or null
};

// the doubles of LDS a workgroup of k_lmap_opt takes
__host__ __device__ inline size_t opt_lds_doubles(int K, int C, int n) {
    return (size_t)2 * K * K + 2 * K + 2 * C + (size_t)n * K + (size_t)6 * C * n * K +
           (size_t)C * K * K + (size_t)3 * C * K + 24;
}

template <int K>
__global__ void __launch_bounds__(kTBPat) k_lmap_opt(OptArgs a) {
    extern __shared__ double lds[];
    const int tid = (int)threadIdx.x, nt = (int)blockDim.x, lane = tid & 63, wave = tid >> 6;
    const int C = a.C, n = a.n, CK = C * K, CnK = C * n * K;
    double *sE = lds, *sEi = sE + K * K, *slam = sEi + K * K, *spi = slam + K, *sr = spi + K;
    double *sq = sr + C, *sR = sq + C, *sT = sR + n * K, *sD = sT + 4 * CnK, *sP = sD + 2 * CnK;
    double *sex = sP + C * K * K, *red = sex + 3 * CK, *slen = red + 16;
    for (int i = tid; i < 2 * K * K + 2 * K + 2 * C; i += nt) lds[i] = a.model[i];
    __syncthreads();
    {  // R[u][m] = sum_j E^-1[m][j] x_u[j]
        const double *table = a.model + 2 * K * K + 2 * K + 2 * C;
        for (int idx = tid; idx < n * K; idx += nt) {
            const int u = idx / K, m = idx - u * K;
            double acc = 0.0;
            for (int j = 0; j < K; ++j) acc = fma(sEi[m * K + j], table[u * K + j], acc);
            sR[idx] = acc;
        }
    }
    const int64_t quartet = (int64_t)blockIdx.x / 3;
    const int tau = (int)(blockIdx.x - 3 * quartet);
    // tips (p, q, r, s) as positions in (a, b, c, d): p is a; in scalars, as the lengths below
    const int pq = tau == 0 ? 1 : (tau == 1 ? 2 : 3), pr = tau == 0 ? 2 : 1, ps = tau == 2 ? 2 : 3;
    const int32_t *tx = a.quartets + 4 * quartet;
    const int32_t t_p = tx[0], t_q = tx[pq], t_r = tx[pr], t_s = tx[ps];
    // the bound keeps a wrong index inside the rows
    const bool rows_ok = (unsigned)t_p < (unsigned)a.n_taxa && (unsigned)t_q < (unsigned)a.n_taxa &&
                         (unsigned)t_r < (unsigned)a.n_taxa && (unsigned)t_s < (unsigned)a.n_taxa;
    const int64_t row_p = rows_ok ? t_p * a.ld : 0, row_q = rows_ok ? t_q * a.ld : 0;
    const int64_t row_r = rows_ok ? t_r * a.ld : 0, row_s = rows_ok ? t_s * a.ld : 0;
    const unsigned long long *bins = a.bins ? a.bins + quartet * a.nbins : nullptr;
    // bin b = ((u_a n + u_b) n + u_c) n + u_d: the weight of a tip's digit
    auto digit = [&](int pos) { return pos == 3 ? 1 : (pos == 2 ? n : (pos == 1 ? n * n : n * n * n)); };
    const int div_p = n * n * n, div_q = digit(pq), div_r = digit(pr), div_s = digit(ps);

    // ex[o][c][m] = (l_m r_c)^o e^{l_m r_c t}
    auto build_ex = [&](double t) {
        for (int idx = tid; idx < CK; idx += nt) {
            const int c = idx / K, m = idx - c * K;
            const double x = slam[m] * sr[c], e = exp(slam[m] * (t * sr[c]));
            sex[idx] = e;
            sex[CK + idx] = x * e;
            sex[2 * CK + idx] = (x * x) * e;
        }
    };
    // the table of tip edge e out of ex, with its derivative tables where orders = 3
    auto build_tip = [&](int e, int orders) {
        for (int idx = tid; idx < orders * CnK; idx += nt) {
            const int o = idx / CnK, rem = idx - o * CnK;
            const int c = rem / (n * K), ui = rem - c * n * K, u = ui / K, i = ui - u * K;
            const double *ex = sex + o * CK + c * K;
            double acc = 0.0;
#pragma unroll
            for (int m = 0; m < K; ++m) acc = fma(sE[i * K + m] * ex[m], sR[u * K + m], acc);
            (o == 0 ? sT + e * CnK : sD + (o - 1) * CnK)[rem] = acc;
        }
    };
    auto build_P = [&]() {
        for (int idx = tid; idx < C * K * K; idx += nt) {
            const int c = idx / (K * K), ij = idx - c * K * K, i = ij / K, j = ij - i * K;
            double acc = 0.0;
#pragma unroll
            for (int m = 0; m < K; ++m) acc = fma(sE[i * K + m] * sex[c * K + m], sEi[m * K + j], acc);
            sP[idx] = acc;
        }
    };

    double lnl = 0.0, d1 = 0.0, d2 = 0.0;  // the last evaluation's sums, the same in every thread
    double al, a1, a2;
    int bad;
    // what one item (a pattern, a bin) of weight w with codes u of (p, q, r, s) adds; h: the
    // edge in hand, whose table (a tip) or exponentials (the internal edge) stand at the abscissa
    auto item = [&](int h, const int (&u)[4], double w) {
        double L0 = 0.0, L1 = 0.0, L2 = 0.0;
        for (int c = 0; c < C; ++c) {
            const double *Tp = sT + ((0 * C + c) * n + u[0]) * K, *Tq = sT + ((1 * C + c) * n + u[1]) * K;
            const double *Tr = sT + ((2 * C + c) * n + u[2]) * K, *Ts = sT + ((3 * C + c) * n + u[3]) * K;
            const double *Pc = sP + c * K * K;
            double f0 = 0.0, f1 = 0.0, f2 = 0.0;
            if (h == 4) {
                double am[K], W[K];
#pragma unroll
                for (int m = 0; m < K; ++m) am[m] = 0.0;
#pragma unroll
                for (int i = 0; i < K; ++i) {
                    const double X = spi[i] * Tp[i] * Tq[i];
                    W[i] = Tr[i] * Ts[i];
#pragma unroll
                    for (int m = 0; m < K; ++m) am[m] = fma(X, sE[i * K + m], am[m]);
                }
                const double *ex = sex + c * K;
#pragma unroll
                for (int m = 0; m < K; ++m) {
                    double bm = 0.0;
#pragma unroll
                    for (int j = 0; j < K; ++j) bm = fma(sEi[m * K + j], W[j], bm);
                    const double g = am[m] * bm;
                    f0 = fma(g, ex[m], f0);
                    f1 = fma(g, ex[CK + m], f1);
                    f2 = fma(g, ex[2 * CK + m], f2);
                }
            } else if (h < 2) {
                const double *other = h == 0 ? Tq : Tp, *H0 = h == 0 ? Tp : Tq;
                const double *H1 = sD + (c * n + (h == 0 ? u[0] : u[1])) * K, *H2 = H1 + CnK;
                double W[K];
#pragma unroll
                for (int j = 0; j < K; ++j) W[j] = Tr[j] * Ts[j];
#pragma unroll
                for (int i = 0; i < K; ++i) {
                    double z = 0.0;
#pragma unroll
                    for (int j = 0; j < K; ++j) z = fma(Pc[i * K + j], W[j], z);
                    const double U = spi[i] * other[i] * z;
                    f0 = fma(U, H0[i], f0);
                    f1 = fma(U, H1[i], f1);
                    f2 = fma(U, H2[i], f2);
                }
            } else {
                const double *other = h == 2 ? Ts : Tr, *H0 = h == 2 ? Tr : Ts;
                const double *H1 = sD + (c * n + (h == 2 ? u[2] : u[3])) * K, *H2 = H1 + CnK;
                double Y[K];
#pragma unroll
                for (int j = 0; j < K; ++j) Y[j] = 0.0;
#pragma unroll
                for (int i = 0; i < K; ++i) {
                    const double X = spi[i] * Tp[i] * Tq[i];
#pragma unroll
                    for (int j = 0; j < K; ++j) Y[j] = fma(X, Pc[i * K + j], Y[j]);
                }
#pragma unroll
                for (int j = 0; j < K; ++j) {
                    const double U = Y[j] * other[j];
                    f0 = fma(U, H0[j], f0);
                    f1 = fma(U, H1[j], f1);
                    f2 = fma(U, H2[j], f2);
                }
            }
            L0 = fma(sq[c], f0, L0);
            L1 = fma(sq[c], f1, L1);
            L2 = fma(sq[c], f2, L2);
        }
        if (!(L0 > 0.0)) {
            bad = 1;
            return;
        }
        al = fma(w, log(L0), al);
        a1 = fma(w, L1 / L0, a1);
        a2 = fma(w, (L2 * L0 - L1 * L1) / (L0 * L0), a2);
    };
    // lnL and its derivatives in the length of edge h at t, the other lengths as the tables hold
    // them; the table of a tip edge h is left at t
    auto eval = [&](int h, double t) {
        build_ex(t);
        __syncthreads();
        if (h < 4) {
            build_tip(h, 3);
            __syncthreads();
        }
        al = a1 = a2 = 0.0;
        bad = rows_ok ? 0 : 1;
        if (bins) {
            for (int b = tid; b < a.nbins && rows_ok; b += nt) {
                const unsigned long long cnt = bins[b];
                if (!cnt) continue;
                const int u[4] = {(b / div_p) % n, (b / div_q) % n, (b / div_r) % n,
                                  (b / div_s) % n};
                item(h, u, (double)cnt);
            }
        } else {
            for (int64_t s = tid; s < a.S && rows_ok; s += nt) {
                const double w = a.w ? a.w[s] : 1.0;
                if (w == 0.0) continue;
                const int u[4] = {a.codes[row_p + s], a.codes[row_q + s], a.codes[row_r + s],
                                  a.codes[row_s + s]};
                if (!(u[0] < n && u[1] < n && u[2] < n && u[3] < n)) {  // a code outside the table has no likelihood
                    bad = 1;
                    continue;
                }
                item(h, u, w);
            }
        }
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            al = __dadd_rn(al, __shfl_xor(al, o, 64));
            a1 = __dadd_rn(a1, __shfl_xor(a1, o, 64));
            a2 = __dadd_rn(a2, __shfl_xor(a2, o, 64));
        }
        bad = __any(bad) ? 1 : 0;
        if (lane == 0) {
            red[4 * wave] = al;
            red[4 * wave + 1] = a1;
            red[4 * wave + 2] = a2;
            red[4 * wave + 3] = (double)bad;
        }
        __syncthreads();
        double s0 = red[0], s1 = red[1], s2 = red[2], sb = red[3];
        for (int v = 1; v < nt / 64; ++v) {
            s0 = __dadd_rn(s0, red[4 * v]);
            s1 = __dadd_rn(s1, red[4 * v + 1]);
            s2 = __dadd_rn(s2, red[4 * v + 2]);
            sb += red[4 * v + 3];
        }
        __syncthreads();  // red and ex are free again
        lnl = sb != 0.0 ? -INFINITY : s0;
        d1 = s1;
        d2 = s2;
    };
    // the tables of edge h at t, after its length has been settled
    auto settle = [&](int h, double t) {
        build_ex(t);
        __syncthreads();
        if (h < 4) build_tip(h, 1);
        else build_P();
        __syncthreads();
    };

    // the five lengths live in LDS: registers indexed by the edge in hand would go to scratch
    if (tid < 5) slen[tid] = newton_clamp(a.t0[tid]);
    __syncthreads();
    for (int h = 0; h < 5; ++h) settle(h, slen[h]);
    int rounds = 0, evals = 1;
    eval(0, slen[0]);
    double cur = lnl;
    for (int r = 1; r <= a.max_rounds && isfinite(cur); ++r) {
        const double before = cur;
        for (int h = 0; h < 5 && isfinite(cur); ++h) {
            NewtonState s;
            double t = newton_start(s, slen[h]);
            while (!s.done) {
                eval(h, t);
                ++evals;
                t = newton_step(s, lnl, d1, d2, a.tol, a.max_iter);
            }
            if (tid == 0) slen[h] = s.t;  // settle's barriers publish it
            cur = s.lnl;
            settle(h, s.t);
        }
        rounds = r;
        if (a.min_gain >= 0.0 && cur - before <= a.min_gain) break;
    }
    const int64_t slot = (int64_t)blockIdx.x;
    if (tid == 0) {
        double *out = a.out + 8 * slot;
        out[0] = cur;
        for (int h = 0; h < 5; ++h) out[1 + h] = slen[h];
        out[6] = (double)rounds;
        out[7] = (double)evals;
    }
    if (a.derivs) {
        for (int h = 0; h < 5; ++h) {
            const bool ok = isfinite(cur);
            if (ok) eval(h, slen[h]);
            if (tid == 0) {
                a.derivs[(slot * 5 + h) * 2] = ok && isfinite(lnl) ? d1 : NAN;
                a.derivs[(slot * 5 + h) * 2 + 1] = ok && isfinite(lnl) ? d2 : NAN;
            }
        }
    }
}

// ---- host side --------------------------------------------------------------------------------

struct LmapState : DevState {
    DevBuf<double> model;
    DevBuf<int32_t> quartets, members;
    DevBuf<unsigned long long> bins;
    std::vector<double> h_model;
    std::vector<int32_t> h_quartets;
    ChunkProfile prof;
};
LmapState g_lmap[64];

struct ModelIn {
    int K, C;
    const double *table, *evecs, *evals, *ivecs, *freqs, *rates, *cw;
};
struct Opt {
    const double *t0;  // [5] or null: 0.1 each
    double tol, min_gain;
    int max_iter, max_rounds;
};
struct Aln {
    int n_taxa, n_codes;
    int64_t n_sites;
};
// the codes the bins run over: `used` ascending, nu of them
struct Used {
    int nu = 0;
    uint8_t code[kMaxCodes];
    uint8_t remap[kMaxCodes];
    void set_all(int n_codes) {
        nu = n_codes;
        for (int c = 0; c < kMaxCodes; ++c) {
            code[c] = (uint8_t)c;
            remap[c] = c < n_codes ? (uint8_t)c : (uint8_t)255;
        }
    }
    void set_from(const bool *seen, int n_codes) {
        nu = 0;
        for (int c = 0; c < kMaxCodes; ++c) {
            remap[c] = 255;
            if (c < n_codes && seen[c]) {
                remap[c] = (uint8_t)nu;
                code[nu++] = (uint8_t)c;
            }
        }
    }
    bool fits() const { return nu >= 1 && nu <= 8; }  // nu^4 <= kMaxBins
    int nbins() const { return nu * nu * nu * nu; }
};

int check_aln(const char *fn, const Aln &s, bool null_buffer) {
    if (null_buffer) return set_err(nullptr, PU_E_ARG, "%s: null buffer", fn);
    if (s.n_taxa < 4 || s.n_sites <= 0)
        return set_err(nullptr, PU_E_ARG, "%s: n_taxa = %d (at least 4), n_sites = %lld", fn,
                       s.n_taxa, (long long)s.n_sites);
    if (s.n_codes < 1 || s.n_codes > kMaxCodes)
        return set_err(nullptr, PU_E_ARG, "%s: n_codes = %d is outside [1, %d]", fn, s.n_codes,
                       kMaxCodes);
    return PU_OK;
}

int check_quartets(const char *fn, int n_taxa, int64_t Q, const int32_t *quartets) {
    if (Q < 1) return set_err(nullptr, PU_E_ARG, "%s: n_quartets = %lld", fn, (long long)Q);
    if (!quartets) return set_err(nullptr, PU_E_ARG, "%s: null quartets", fn);
    for (int64_t q = 0; q < Q; ++q) {
        const int32_t *t = quartets + 4 * q;
        bool ok = true;
        for (int k = 0; k < 4; ++k) {
            ok = ok && t[k] >= 0 && t[k] < n_taxa;
            for (int j = 0; j < k; ++j) ok = ok && t[j] != t[k];
        }
        if (!ok)
            return set_err(nullptr, PU_E_ARG, "%s: quartet %lld = (%d, %d, %d, %d) of %d taxa", fn,
                           (long long)q, t[0], t[1], t[2], t[3], n_taxa);
    }
    return PU_OK;
}

int check_model(const char *fn, const ModelIn &m, const Opt &o, int n_codes) {
    if (!m.table || !m.evecs || !m.evals || !m.ivecs || !m.freqs || !m.rates || !m.cw)
        return set_err(nullptr, PU_E_ARG, "%s: null model buffer", fn);
    if (m.K != 2 && m.K != 4 && m.K != 20)
        return set_err(nullptr, PU_E_ARG, "%s: K = %d is not supported (2, 4, 20)", fn, m.K);
    if (m.C < 1 || m.C > kMaxCat)
        return set_err(nullptr, PU_E_ARG, "%s: n_cat = %d is outside [1, %d]", fn, m.C, kMaxCat);
    if (!(o.tol > 0.0) || o.max_iter < 0 || o.max_rounds < 0)
        return set_err(nullptr, PU_E_ARG, "%s: tol = %g, max_iter = %d, max_rounds = %d", fn, o.tol,
                       o.max_iter, o.max_rounds);
    if (o.min_gain != o.min_gain) return set_err(nullptr, PU_E_ARG, "%s: min_gain is NaN", fn);
    if (o.t0)
        for (int h = 0; h < 5; ++h)
            if (!(o.t0[h] >= kMinLen && o.t0[h] <= kMaxLen))
                return set_err(nullptr, PU_E_ARG, "%s: t0[%d] = %g is outside [%g, %g]", fn, h,
                               o.t0[h], kMinLen, kMaxLen);
    const size_t lds = opt_lds_doubles(m.K, m.C, n_codes) * 8;
    if (lds > kLdsCap)
        return set_err(nullptr, PU_E_ARG, "%s: %d states x %d categories x %d codes need %zu bytes "
                       "of LDS per workgroup, past %zu: the tables grow with n_cat x n_codes, so "
                       "use fewer rate categories or a code table with fewer rows", fn, m.K, m.C,
                       n_codes, lds, kLdsCap);
    return PU_OK;
}

// host forms: a weight is a finite number >= 0
int check_weights(const char *fn, const double *w, int64_t n) {
    if (w)
        for (int64_t s = 0; s < n; ++s)
            if (!(w[s] >= 0.0 && w[s] < INFINITY))
                return set_err(nullptr, PU_E_ARG, "%s: weight %g of pattern %lld is negative or "
                               "not finite", fn, w[s], (long long)s);
    return PU_OK;
}

// weights the bins can count: non-negative integers below 2^53
bool integer_weights(const double *w, int64_t n) {
    if (w)
        for (int64_t s = 0; s < n; ++s)
            if (!(w[s] >= 0.0 && w[s] < 0x1p53 && w[s] == floor(w[s]))) return false;
    return true;
}

// PU_LMAP_FEED, read at each call: +1 bins, -1 patterns, 0 unset
int feed_env() {
    const char *f = getenv("PU_LMAP_FEED");
    if (f && !strcmp(f, "bins")) return 1;
    if (f && !strcmp(f, "patterns")) return -1;
    return 0;
}

int64_t quartet_chunk(int64_t Q, int nbins) {
    int64_t chunk = Q;
    if (nbins) chunk = std::max<int64_t>(1, (int64_t)(kWsBytes / ((size_t)nbins * 8)));
    chunk = std::min<int64_t>(chunk, (int64_t)0x7fffffff / 3);  // blockIdx.x = 3 quartet + tau
    return std::min(env_cap("PU_LMAP_CHUNK", chunk), Q);
}

int upload_quartets(LmapState &D, hipStream_t st, int64_t Q, const int32_t *quartets) {
    D.h_quartets.assign(quartets, quartets + 4 * Q);
    if (int rc = D.quartets.reserve((size_t)4 * Q)) return rc;
    HIPCHK(nullptr, hipMemcpyAsync(D.quartets.p, D.h_quartets.data(), (size_t)16 * Q,
                                   hipMemcpyHostToDevice, st));
    return PU_OK;
}

int launch_bins(LmapState &D, hipStream_t st, const Aln &s, const uint8_t *d_codes, int64_t ld,
                const double *d_w, const Used &U, int64_t q0, int64_t nq) {
    const int nbins = U.nbins();
    HIPCHK(nullptr, hipMemsetAsync(D.bins.p, 0, (size_t)nq * nbins * 8, st));
    BinArgs b;
    b.codes = d_codes;
    b.ld = ld;
    b.S = s.n_sites;
    b.w = d_w;
    b.quartets = D.quartets.p + 4 * q0;
    b.n_taxa = s.n_taxa;
    b.nu = U.nu;
    b.nbins = nbins;
    memcpy(b.remap, U.remap, sizeof(b.remap));
    // a quartet's patterns are cut where there are few quartets; integer sums take any cut
    const int64_t tiles = (s.n_sites + 4 * kTB - 1) / (4 * kTB);
    const int64_t gy = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(tiles, 1024),
                                                              (4096 + nq - 1) / nq));
    b.seg = (s.n_sites + gy - 1) / gy;
    b.out = D.bins.p;
    hipLaunchKernelGGL(k_lmap_bins, dim3((unsigned)nq, (unsigned)gy), dim3(kTB), (size_t)nbins * 8,
                       st, b);
    HIPCHK(nullptr, hipGetLastError());
    return PU_OK;
}

// the model as k_lmap_opt reads it, the table cut to the rows `U` lists (null: all n_codes)
void pack_model(const ModelIn &m, int n_codes, const Used *U, std::vector<double> &h) {
    const int K = m.K, C = m.C, n = U ? U->nu : n_codes;
    h.clear();
    h.insert(h.end(), m.evecs, m.evecs + K * K);
    h.insert(h.end(), m.ivecs, m.ivecs + K * K);
    h.insert(h.end(), m.evals, m.evals + K);
    h.insert(h.end(), m.freqs, m.freqs + K);
    h.insert(h.end(), m.rates, m.rates + C);
    h.insert(h.end(), m.cw, m.cw + C);
    for (int u = 0; u < n; ++u) {
        const double *x = m.table + (size_t)(U ? U->code[u] : u) * K;
        h.insert(h.end(), x, x + K);
    }
}

// The work of every call, queued on st.  d_codes / d_w / d_out / d_derivs are device buffers,
// quartets a host list.  U: the codes of the bins feed, or null: the patterns feed.  Without a
// model the bins of every quartet are copied to bins_host.
int run_lmap(int device, hipStream_t st, const Aln &s, const uint8_t *d_codes, int64_t ld,
             const double *d_w, int64_t Q, const int32_t *quartets, const Used *U,
             const ModelIn *m, const Opt *o, double *d_out, double *d_derivs,
             unsigned long long *bins_host) {
    LmapState &D = g_lmap[device];
    StateScope scope(D, st);
    int rc;
    if ((rc = scope.rc)) return rc;
    if ((rc = upload_quartets(D, st, Q, quartets))) return rc;
    const int nbins = U ? U->nbins() : 0;
    const int64_t chunk = quartet_chunk(Q, nbins);
    if (U && (rc = D.bins.reserve((size_t)chunk * nbins))) return rc;
    OptArgs a{};
    if (m) {
        pack_model(*m, s.n_codes, U, D.h_model);
        if ((rc = D.model.reserve(D.h_model.size()))) return rc;
        HIPCHK(nullptr, hipMemcpyAsync(D.model.p, D.h_model.data(), D.h_model.size() * 8,
                                       hipMemcpyHostToDevice, st));
        a.model = D.model.p;
        a.codes = U ? nullptr : d_codes;
        a.ld = ld;
        a.S = s.n_sites;
        a.w = d_w;
        a.bins = U ? D.bins.p : nullptr;
        a.nbins = nbins;
        a.n_taxa = s.n_taxa;
        a.n = U ? U->nu : s.n_codes;
        a.C = m->C;
        for (int h = 0; h < 5; ++h) a.t0[h] = o->t0 ? o->t0[h] : 0.1;
        a.tol = o->tol;
        a.min_gain = o->min_gain;
        a.max_iter = o->max_iter;
        a.max_rounds = o->max_rounds;
    }
    if ((rc = D.prof.reserve((Q + chunk - 1) / chunk))) return rc;
    for (int64_t q0 = 0; q0 < Q; q0 += chunk) {
        const int64_t nq = std::min(chunk, Q - q0);
        if ((rc = D.prof.mark(0, st))) return rc;
        if (U && (rc = launch_bins(D, st, s, d_codes, ld, d_w, *U, q0, nq))) return rc;
        if ((rc = D.prof.mark(1, st))) return rc;
        if (m) {
            a.quartets = D.quartets.p + 4 * q0;
            a.out = d_out + 24 * q0;
            a.derivs = d_derivs ? d_derivs + 30 * q0 : nullptr;
            const dim3 grid((unsigned)(3 * nq)), block(U ? kTBBin : kTBPat);
            const size_t lds = opt_lds_doubles(m->K, m->C, a.n) * 8;
            if (m->K == 2) hipLaunchKernelGGL(k_lmap_opt<2>, grid, block, lds, st, a);
            else if (m->K == 4) hipLaunchKernelGGL(k_lmap_opt<4>, grid, block, lds, st, a);
            else hipLaunchKernelGGL(k_lmap_opt<20>, grid, block, lds, st, a);
            HIPCHK(nullptr, hipGetLastError());
        } else {
            HIPCHK(nullptr, hipMemcpyAsync(bins_host + (size_t)q0 * nbins, D.bins.p,
                                           (size_t)nq * nbins * 8, hipMemcpyDeviceToHost, st));
        }
        if ((rc = D.prof.mark(2, st))) return rc;
    }
    return PU_OK;
}

// m = C(n, 4) or the product of the cluster sizes against Q, without overflow
bool at_most(unsigned __int128 m, int64_t Q) { return m <= (unsigned __int128)Q; }

}  // namespace

extern "C" {

int pu_lmap_quartets(int device, int n_taxa, const int32_t *cluster, int64_t n_quartets,
                     uint64_t seed, int32_t *quartets_out, int64_t *n_out) {
    const char *fn = "pu_lmap_quartets";
    if (n_taxa < 4) return set_err(nullptr, PU_E_ARG, "%s: n_taxa = %d (at least 4)", fn, n_taxa);
    if (n_quartets < 1)
        return set_err(nullptr, PU_E_ARG, "%s: n_quartets = %lld", fn, (long long)n_quartets);
    if (!quartets_out || !n_out) return set_err(nullptr, PU_E_ARG, "%s: null output", fn);
    QuartetArgs a{};
    a.n = n_taxa;
    a.seed = seed;
    std::vector<int32_t> members;
    unsigned __int128 m;
    if (cluster) {
        a.clustered = 1;
        int64_t size[4] = {0, 0, 0, 0};
        for (int t = 0; t < n_taxa; ++t) {
            if (cluster[t] < -1 || cluster[t] > 3)
                return set_err(nullptr, PU_E_ARG, "%s: cluster[%d] = %d is outside -1..3", fn, t,
                               cluster[t]);
            if (cluster[t] >= 0) ++size[cluster[t]];
        }
        m = 1;
        for (int k = 0; k < 4; ++k) {
            if (!size[k]) return set_err(nullptr, PU_E_ARG, "%s: cluster %d is empty", fn, k);
            a.size[k] = (int32_t)size[k];
            a.off[k] = k ? a.off[k - 1] + a.size[k - 1] : 0;
            m *= (unsigned __int128)size[k];
            for (int t = 0; t < n_taxa; ++t)
                if (cluster[t] == k) members.push_back(t);
        }
    } else {
        const unsigned __int128 n = (unsigned __int128)n_taxa;
        m = n * (n - 1) / 2 * (n - 2) / 3 * (n - 3) / 4;
    }
    a.all = at_most(m, n_quartets) ? 1 : 0;
    a.Q = a.all ? (int64_t)m : n_quartets;
    *n_out = a.Q;
    int rc;
    if ((rc = check_device(device))) return rc;
    DeviceGuard g(device);
    HostCall h(device);
    a.members = cluster ? h.to_device(members.data(), members.size()) : nullptr;
    a.out = h.alloc<int32_t>((size_t)4 * a.Q);
    if (!h.rc) {
        hipLaunchKernelGGL(k_lmap_quartets, dim3((unsigned)((a.Q + kTB - 1) / kTB)), dim3(kTB), 0,
                           h.st, a);
        h.hip(fn, hipGetLastError());
    }
    h.to_host(quartets_out, a.out, (size_t)4 * a.Q);
    return h.finish(fn);
}

int pu_lmap_bins(int device, const uint8_t *codes, int n_taxa, int64_t n_sites, int n_codes,
                 const double *site_weights, int64_t n_quartets, const int32_t *quartets,
                 int n_used, const uint8_t *used, uint64_t *bins_out) {
    const char *fn = "pu_lmap_bins";
    const Aln s{n_taxa, n_codes, n_sites};
    int rc;
    if ((rc = check_aln(fn, s, !codes))) return rc;
    if ((rc = check_quartets(fn, n_taxa, n_quartets, quartets))) return rc;
    if (!bins_out) return set_err(nullptr, PU_E_ARG, "%s: null output", fn);
    Used U;
    if (used) {
        bool seen[kMaxCodes] = {};
        for (int i = 0; i < n_used; ++i) {
            if (used[i] >= n_codes || (i && used[i] <= used[i - 1]))
                return set_err(nullptr, PU_E_ARG, "%s: used[%d] = %d (ascending codes below %d)",
                               fn, i, (int)used[i], n_codes);
            seen[used[i]] = true;
        }
        U.set_from(seen, n_codes);
    } else {
        U.set_all(n_codes);
    }
    if (!U.fits())
        return set_err(nullptr, PU_E_ARG, "%s: %d codes in use: n_used^4 must be in [1, %d]", fn,
                       U.nu, kMaxBins);
    if (!integer_weights(site_weights, n_sites))
        return set_err(nullptr, PU_E_ARG, "%s: the bins need non-negative integer weights below "
                       "2^53", fn);
    if ((rc = check_codes(fn, codes, n_taxa, n_sites, n_codes))) return rc;
    for (int64_t i = 0; i < (int64_t)n_taxa * n_sites; ++i)
        if (U.remap[codes[i]] == 255)
            return set_err(nullptr, PU_E_ARG, "%s: taxon %lld site %lld: code %d is not in `used`",
                           fn, (long long)(i / n_sites), (long long)(i % n_sites), (int)codes[i]);
    if ((rc = check_device(device))) return rc;
    DeviceGuard g(device);
    HostCall h(device);
    const uint8_t *d_codes = h.to_device(codes, (size_t)n_taxa * n_sites);
    const double *d_w = h.to_device(site_weights, (size_t)n_sites);
    if (!h.rc)
        h.rc = run_lmap(device, h.st, s, d_codes, n_sites, d_w, n_quartets, quartets, &U, nullptr,
                        nullptr, nullptr, nullptr, reinterpret_cast<unsigned long long *>(bins_out));
    return h.finish(fn);
}

int pu_lmap_scores_device(int device, void *stream, int n_states, int n_cat, int n_codes,
                          const double *code_table, const double *evecs, const double *evals,
                          const double *ivecs, const double *freqs, const double *rates,
                          const double *cat_weights, const uint8_t *d_codes, int64_t ld,
                          int n_taxa, int64_t n_sites, const double *d_site_weights,
                          int64_t n_quartets, const int32_t *quartets, const double *t0,
                          double tol, int max_iter, int max_rounds, double min_gain,
                          double *d_out, double *d_derivs) {
    const char *fn = "pu_lmap_scores_device";
    const Aln s{n_taxa, n_codes, n_sites};
    const ModelIn m{n_states, n_cat, code_table, evecs, evals, ivecs, freqs, rates, cat_weights};
    const Opt o{t0, tol, min_gain, max_iter, max_rounds};
    int rc;
    if ((rc = check_aln(fn, s, !d_codes))) return rc;
    if ((rc = check_quartets(fn, n_taxa, n_quartets, quartets))) return rc;
    if (!d_out) return set_err(nullptr, PU_E_ARG, "%s: null output", fn);
    if (ld < n_sites)
        return set_err(nullptr, PU_E_ARG, "%s: row stride %lld below n_sites = %lld", fn,
                       (long long)ld, (long long)n_sites);
    if ((rc = check_model(fn, m, o, n_codes))) return rc;
    // the bins take integer weights and n_codes^4 <= 4096 as the caller's word: without weights
    // they are the default, with weights PU_LMAP_FEED=bins states it
    Used U;
    U.set_all(n_codes);
    const int feed = feed_env();
    const bool bins = U.fits() && (d_site_weights ? feed > 0 : feed >= 0);
    if ((rc = check_device(device))) return rc;
    DeviceGuard g(device);
    return run_lmap(device, (hipStream_t)stream, s, d_codes, ld, d_site_weights, n_quartets,
                    quartets, bins ? &U : nullptr, &m, &o, d_out, d_derivs, nullptr);
}

int pu_lmap_scores(int device, int n_states, int n_cat, int n_codes, const double *code_table,
                   const double *evecs, const double *evals, const double *ivecs,
                   const double *freqs, const double *rates, const double *cat_weights,
                   const uint8_t *codes, int n_taxa, int64_t n_sites, const double *site_weights,
                   int64_t n_quartets, const int32_t *quartets, const double *t0, double tol,
                   int max_iter, int max_rounds, double min_gain, double *out, double *derivs) {
    const char *fn = "pu_lmap_scores";
    const Aln s{n_taxa, n_codes, n_sites};
    const ModelIn m{n_states, n_cat, code_table, evecs, evals, ivecs, freqs, rates, cat_weights};
    const Opt o{t0, tol, min_gain, max_iter, max_rounds};
    int rc;
    if ((rc = check_aln(fn, s, !codes))) return rc;
    if ((rc = check_quartets(fn, n_taxa, n_quartets, quartets))) return rc;
    if (!out) return set_err(nullptr, PU_E_ARG, "%s: null output", fn);
    if ((rc = check_model(fn, m, o, n_codes))) return rc;
    if ((rc = check_codes(fn, codes, n_taxa, n_sites, n_codes))) return rc;
    if ((rc = check_weights(fn, site_weights, n_sites))) return rc;
    bool seen[kMaxCodes] = {};
    for (int64_t i = 0; i < (int64_t)n_taxa * n_sites; ++i) seen[codes[i]] = true;
    Used U;
    U.set_from(seen, n_codes);
    const bool bins = U.fits() && feed_env() >= 0 && integer_weights(site_weights, n_sites);
    if ((rc = check_device(device))) return rc;
    DeviceGuard g(device);
    HostCall h(device);
    const uint8_t *d_codes = h.to_device(codes, (size_t)n_taxa * n_sites);
    const double *d_w = h.to_device(site_weights, (size_t)n_sites);
    double *d_out = h.alloc<double>(24 * (size_t)n_quartets);
    double *d_der = derivs ? h.alloc<double>(30 * (size_t)n_quartets) : nullptr;
    if (!h.rc)
        h.rc = run_lmap(device, h.st, s, d_codes, n_sites, d_w, n_quartets, quartets,
                        bins ? &U : nullptr, &m, &o, d_out, d_der, nullptr);
    h.to_host(out, d_out, 24 * (size_t)n_quartets);
    if (derivs) h.to_host(derivs, d_der, 30 * (size_t)n_quartets);
    return h.finish(fn);
}

int pu_lmap_profile(int device, int on) { return profile_set(g_lmap, device, on); }

int pu_lmap_kernel_ms(int device, double *bins_ms, double *opt_ms) {
    return profile_ms("pu_lmap_kernel_ms", g_lmap, device, bins_ms, opt_ms);
}

}  // extern "C"
