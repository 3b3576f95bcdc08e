// pu_edge_dev.h -- device helpers shared by the kernels that read the resident CLVs of a
// context through EdgeArgs (pu_edge.hip: edge operations; pu_nni.hip: quartet scoring): site
// vectors in the tiled slot layout of pu_kernels.hip, a node's vector and scaler by NodeSrc,
// the engine's rescale rule and the 64-lane sum.  Not part of the public ABI.
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

}  // namespace

}  // namespace pu
