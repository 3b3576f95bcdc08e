// pu_edge_dev.h -- device helpers shared by the kernels that read the resident CLVs of a
// context through EdgeArgs (pu_edge.hip, pu_nni.hip, pu_ancestral.hip, pu_counts.hip,
// pu_place.hip, pu_spr.hip): site vectors in the tiled slot layout of pu_kernels.hip, a node's
// vector and scaler by NodeSrc, the engine's rescale rule and the 64-lane sum; the model in LDS
// and the transition matrices built from it; the category mix of a site; the second-launch sums
// (DESIGN 4.25).  Each is stated here once.  Not part of the public ABI.
#pragma once
#include <math.h>

#include "pu_internal.h"

namespace pu {

namespace {

constexpr double kScaleThreshold = 0x1p-128;  // numba_likelihood_engine.py:7
constexpr int kLanes = 64;

typedef double dbl2 __attribute__((ext_vector_type(2)));

// ---- site vectors in the tiled slot layout (pu_kernels.hip k_untile / k_untile_aa) ----
template <int K>
__device__ __forceinline__ int tiled_index(int i, int l) {
    if constexpr (K == 20) {  // [wave 4][aa_row_off]: lane (g, s16) of wave w, rows g, g+4..
        const int w = l >> 4, s16 = l & 15;
        const int g = i < 16 ? (i & 3) : i - 16, r = i < 16 ? (i >> 2) : 4;
        return w * 5 * 64 + aa_row_off(r, g * 16 + s16);
    } else {  // [K/2][64][2]
        return (i >> 1) * 128 + 2 * l + (i & 1);
    }
}

template <int K>
__device__ __forceinline__ void load_site(const double *row, int l, double (&v)[K]) {
    if constexpr (K == 20) {
#pragma unroll
        for (int i = 0; i < K; ++i) v[i] = row[tiled_index<K>(i, l)];
    } else {
        const dbl2 *q = reinterpret_cast<const dbl2 *>(row) + l;
#pragma unroll
        for (int i = 0; i < K / 2; ++i) {
            const dbl2 t = q[i * kLanes];
            v[2 * i] = t.x;
            v[2 * i + 1] = t.y;
        }
    }
}

template <int K>
__device__ __forceinline__ void store_site(double *row, int l, const double (&v)[K]) {
    if constexpr (K == 20) {
#pragma unroll
        for (int i = 0; i < K; ++i) row[tiled_index<K>(i, l)] = v[i];
    } else {
        dbl2 *q = reinterpret_cast<dbl2 *>(row) + l;
#pragma unroll
        for (int i = 0; i < K / 2; ++i) q[i * kLanes] = dbl2{v[2 * i], v[2 * i + 1]};
    }
}

// the K-vector and scaler of one node at (site, category)
template <int K>
__device__ __forceinline__ void node_vec(const EdgeArgs &a, NodeSrc n, int cat, int tile, int l,
                                         int64_t site_c, double (&v)[K], double &s) {
    if (n.kind == SRC_SLOT) {
        const size_t row = layout_row(K, a.C, a.tile_pitch, cat, tile);
        load_site<K>(a.clv + (size_t)n.idx * a.slot_stride + row * K * kLanes, l, v);
        s = a.scale[(size_t)n.idx * a.sstride + row * kLanes + l];
        return;
    }
    const double *src = n.kind == SRC_CODED
                            ? a.table + (size_t)a.codes[(size_t)n.idx * a.code_stride + site_c] * K
                            : a.tips + ((size_t)n.idx * a.S + site_c) * K;
#pragma unroll
    for (int i = 0; i < K; ++i) v[i] = src[i];
    s = 0.0;
}

template <int K>
__device__ __forceinline__ void rescale(double (&out)[K], double sa, double sb, double &cml) {
    double m = out[0];  // np.max: NaN propagates
#pragma unroll
    for (int i = 1; i < K; ++i) m = (out[i] > m || out[i] != out[i]) ? out[i] : m;
    const double base = sa + sb;
    if (m < kScaleThreshold && m > 0.0) {
        cml = base + log(m);
#pragma unroll
        for (int i = 0; i < K; ++i) out[i] = out[i] / m;
    } else {
        cml = base;
    }
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// ---- the model in LDS, and P_c(t) = U diag(e^{lambda t r_c}) U^-1 out of it --------------------

// The head of every kernel's LDS (doubles): [evecs K*K][ivecs K*K][evals K][pi K][rates C]; the
// kernel's own tables follow from `body`, 16-byte aligned.  k_edge reads pi from global memory
// and keeps no slot for it (with_pi = false).
struct ModelLds {
    size_t evecs, ivecs, evals, pi, rates, body;
    __host__ __device__ ModelLds(int K, int C, bool with_pi = true) {
        evecs = 0;
        ivecs = evecs + (size_t)K * K;
        evals = ivecs + (size_t)K * K;
        pi = evals + K;
        rates = pi + (with_pi ? K : 0);
        body = (rates + C + 1) & ~size_t(1);
    }
};

// the eigen-system of the context into the head, by every thread of the workgroup; the caller's
// barrier follows
template <int K, bool PI = true>
__device__ __forceinline__ void load_model(const EdgeArgs &a, double *lds, const ModelLds &L) {
    for (int i = threadIdx.x; i < K * K; i += blockDim.x) {
        lds[L.evecs + i] = a.evecs[i];
        lds[L.ivecs + i] = a.ivecs[i];
    }
    for (int i = threadIdx.x; i < K; i += blockDim.x) {
        lds[L.evals + i] = a.evals[i];
        if constexpr (PI) lds[L.pi + i] = a.pi[i];
    }
    for (int i = threadIdx.x; i < a.C; i += blockDim.x) lds[L.rates + i] = a.rates[i];
}

// e^{lambda (t r)} (k_pmatrix's arithmetic: P(t) is bit-identical to the traversal's), and the
// factor of its t-derivative of order 1 or 2: x^ord e, x = lambda r
__device__ __forceinline__ double exp_lrt(double lam, double r, double t) {
    return exp(lam * (t * r));
}
__device__ __forceinline__ double exp_lrt_d(double e, double lam, double r, int ord) {
    const double x = lam * r;
    return ord == 1 ? x * e : (x * x) * e;
}

// ex[m][c][k] = x^ord[m] e^{lambda_k (t[m] r_c)} for n lengths (ord null: all of order 0), the
// entries dealt to the threads of the workgroup.  No barrier: the caller's own follows.
template <int K>
__device__ __forceinline__ void exp_tables(double *ex, const double *el, const double *rt, int C,
                                           int n, const double *t, const int *ord = nullptr) {
    for (int idx = threadIdx.x; idx < n * C * K; idx += blockDim.x) {
        const int k = idx % K, mc = idx / K, m = n == 1 ? 0 : mc / C, c = mc - m * C;
        const double r = rt[c];
        double e = exp_lrt(el[k], r, t[m]);
        if (ord && ord[m] > 0) e = exp_lrt_d(e, el[k], r, ord[m]);
        ex[idx] = e;
    }
}

// entry (i, j) of U diag(e) U^-1: sum_k (U[i][k] e[k]) U^-1[k][j], one fma chain
template <int K>
__device__ __forceinline__ double p_entry(const double *ev, const double *iv, const double *e,
                                          int i, int j) {
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k) acc = fma(ev[i * K + k] * e[k], iv[k * K + j], acc);
    return acc;
}

// P[m][c] = U diag(ex[m][c]) U^-1 of the n tables above, likewise dealt and barrier-free.
// RATE0_I: a category of rate 0 (+I) gets I itself at order 0 instead of U U^-1, which is I
// plus rounding of either sign.  true in k_edge, whose updates write partials that
// must equal the traversal's (exact products of tip rows, F_0 exactly 0 at a variable pattern),
// and in k_ancestral and k_counts, where a noise F_0 > 0 passed the mix and reached cat_post and
// M_0.  false in k_place_table and k_regraft, which only add F_0 to a pattern's likelihood: on
// exact partials that is 1e-16 relative, which their tests bound.  k_quartet forms no matrix and
// keeps its own exponentials at rate 0 for the same reason.
template <int K, bool RATE0_I>
__device__ __forceinline__ void p_tables(double *P, const double *ev, const double *iv,
                                         const double *ex, const double *rt, int C, int n = 1,
                                         const int *ord = nullptr) {
    for (int idx = threadIdx.x; idx < n * C * K * K; idx += blockDim.x) {
        const int ij = idx % (K * K), mc = idx / (K * K);
        const int i = ij / K, j = ij - i * K;
        double acc = p_entry<K>(ev, iv, ex + mc * K, i, j);
        if constexpr (RATE0_I) {
            const int m = n == 1 ? 0 : mc / C, c = mc - m * C;
            if (rt[c] == 0.0 && (!ord || ord[m] == 0)) acc = i == j ? 1.0 : 0.0;
        }
        P[idx] = acc;
    }
}

// ---- the category mix of a site ----------------------------------------------------------------
// L = sum_c w_c F_c e^{sigma_c} = e^m sum_c w_c e^{sigma_c - m} F_c, F_c the category's linear
// likelihood and sigma_c its log scaler (equal across categories unless a child was rescaled, so
// the exponential is usually skipped).  Only categories with F_c > 0 take part (lnl_node's -inf
// for the others, numba_likelihood_engine.py:82-87): an all-zero vector keeps an unrescaled
// scaler, which must not set m and underflow every other category's weight (an invariable
// category at a variable pattern).  F and sigma of category c stand at [c * stride].
__device__ __forceinline__ bool mix_takes_part(double F) { return F > 0.0; }

__device__ __forceinline__ double mix_max(const double *F, const double *sigma, size_t stride,
                                          int C) {
    double m = -INFINITY;
    for (int c = 0; c < C; ++c)
        if (mix_takes_part(F[c * stride])) m = fmax(m, sigma[c * stride]);
    return m;
}

// the weight of a category that takes part
__device__ __forceinline__ double mix_weight(double w, double sigma, double m) {
    return w * (sigma == m ? 1.0 : exp(sigma - m));
}

// every category's weight (0: takes no part) in place of its sigma; returns Z = sum_c weight F_c
__device__ __forceinline__ double mix_weights(const double *F, double *sigma, size_t stride, int C,
                                              const double *w, double m) {
    double Z = 0.0;
    for (int c = 0; c < C; ++c) {
        const double Fc = F[c * stride];
        const double we = mix_takes_part(Fc) ? mix_weight(w[c], sigma[c * stride], m) : 0.0;
        sigma[c * stride] = we;
        Z += we * Fc;
    }
    return Z;
}

// what a pattern of weight pw adds to a lnL: -inf where no category takes part, which a weight
// of 0 does not see
__device__ __forceinline__ double mix_lnl(double pw, double m, double Z) {
    if (Z > 0.0) return pw * (m + log(Z));
    return pw != 0.0 ? -INFINITY : 0.0;
}

// The mix of f, f', f'' (EDGE_DERIV, the quartet's arrangements): v[(o * C + c) * 64], o = 0..3:
// f, f', f'', sigma.  dlnL/dt = sum_c w_c f'_c e^{..} / sum_c w_c f_c e^{..}, likewise d2: one
// log and two divisions per site.  v1, v2 stay as they are where no category takes part; returns
// the pattern's own lnL.
__device__ __forceinline__ double mix_derivs(const double *v, int C, const double *w, double pw,
                                             double &v0, double &v1, double &v2) {
    const double *sigma = v + 3 * C * kLanes;
    const double m = mix_max(v, sigma, kLanes, C);
    double Ls = 0.0, N1 = 0.0, N2 = 0.0;
    for (int c = 0; c < C; ++c) {
        if (!mix_takes_part(v[c * kLanes])) continue;
        const double we = mix_weight(w[c], sigma[c * kLanes], m);
        Ls += we * v[c * kLanes];
        N1 += we * v[(C + c) * kLanes];
        N2 += we * v[(2 * C + c) * kLanes];
    }
    v0 = mix_lnl(pw, m, Ls);
    if (Ls > 0.0) {
        const double d1 = N1 / Ls;
        v1 = pw * d1;
        v2 = pw * (N2 / Ls - d1 * d1);
    }
    return Ls > 0.0 ? m + log(Ls) : -INFINITY;
}

// ---- second launches: the workgroups' partial sums in a fixed order ---------------------------

// result[k] = sum_b part[b][k], k < N, by one workgroup of 256 threads: partial b by thread
// b % 256, a 64-lane tree, the four waves in order -- the order does not depend on timing.
// seq != 0: result is mapped host memory that the host polls at result[N] instead of
// synchronising the stream; the sums reach it before the sequence number does.
template <int N>
__device__ __forceinline__ void tile_sums(const double *__restrict__ part, int n,
                                          double *__restrict__ result, double seq = 0.0) {
    __shared__ double red[N * 4];
    double s[N];
#pragma unroll
    for (int k = 0; k < N; ++k) s[k] = 0.0;
    for (int b = threadIdx.x; b < n; b += blockDim.x)
#pragma unroll
        for (int k = 0; k < N; ++k) s[k] += part[N * (size_t)b + k];
    const int w = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        s[k] = wave_sum(s[k]);
        if ((threadIdx.x & 63) == 0) red[N * w + k] = s[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < N; ++k) {
            double r = 0.0;
            for (int j = 0; j < 4; ++j) r += red[N * j + k];
            result[k] = r;
        }
        if (seq != 0.0) {
            __threadfence_system();
            __hip_atomic_store(result + N, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

template <int N>
__global__ void __launch_bounds__(256) k_tile_sums(const double *__restrict__ part, int n,
                                                   double *__restrict__ result, double seq) {
    tile_sums<N>(part, n, result, seq);
}

// out[r] = sum_k part[r][k], a thread per row, the row's entries in ascending order
constexpr int kRowSumThreads = 256;
template <class T>
__global__ void __launch_bounds__(kRowSumThreads) k_row_sums(const T *__restrict__ part, int n_rows,
                                                             int n_cols, T *__restrict__ out) {
    const int64_t r = (int64_t)blockIdx.x * kRowSumThreads + threadIdx.x;
    if (r >= n_rows) return;
    T s = 0.0;
    for (int k = 0; k < n_cols; ++k) s += part[(size_t)r * n_cols + k];
    out[r] = s;
}

template <class T>
void launch_row_sums(hipStream_t st, const T *part, int n_rows, int n_cols, T *out) {
    const dim3 grid((unsigned)((n_rows + kRowSumThreads - 1) / kRowSumThreads));
    hipLaunchKernelGGL(k_row_sums<T>, grid, dim3(kRowSumThreads), 0, st, part, n_rows, n_cols, out);
}

}  // namespace

}  // namespace pu
