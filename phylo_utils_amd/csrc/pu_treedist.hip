// pu_treedist.hip -- sets of trees with branch lengths compared on the GPU: weighted
// Robinson-Foulds and branch-score distances, topological and weighted path-difference
// distances, and the per-split and per-tip sums of the lengths; and the C ABI of it (pu_treedist,
// pu_treedist_profile, pu_treedist_kernel_ms).
//
// The reference compares no trees; the rule is this project's own (normative;
// tests/treedist_reference.py restates it).  The trees, their forms, their edge orders, the
// splits and their ids are pu_treeset.hip's: this file runs that file's stages
// through pu_treeset_stages.h and reads the id arrays they leave.  Every tree has lengths
// [2n-3], fp64, in its form's edge order.  Keyed lengths: pendant key i = the edge at tip i,
// split key u = the edge whose split has id u, a key a tree does not hold = 0.
//
//   k_td_keys      one thread per (tree, op-order edge): the edge's length goes to vec[t][c] when
//                  its child end c is a tip, else to cl_len[t][c - n] (edge -> cluster of
//                  pu_treeset.hip).  vec [T][2n-3]: the n pendant lengths by tip, then room for the
//                  n - 3 split lengths in ascending id.
//   k_td_sort      one workgroup per tree: its (id, length) pairs sorted by id in LDS (bitonic,
//                  padded with INT32_MAX to a power of two; a tree holds an id once, so the order
//                  is unique): sid [T][n-3] and vec[t][n..].
//   k_td_weighted  a tile of 16 row trees x 16 column trees per workgroup, one lane per pair, as
//                  k_ts_rf.  The lane adds the n pendant terms in tip order, then walks the two
//                  sorted lists and adds the terms of the union in ascending id: wRF += |la - lb|,
//                  KF2 += (la - lb)^2, the square rounded on its own (__dmul_rn, __dadd_rn).  The
//                  32 vectors and id lists are staged in LDS while they fit the 160 KiB
//                  (32 (20 n - 36) bytes: n <= 257), else read from memory.
//   k_td_sums      split_sum[u] = the lengths of the edges that carry u, added serially over the
//                  trees in ascending tree index (the positions first[u] .. of perm, which the
//                  stable sort left in tree order); tip_sum[i] likewise over vec[t][i].
//   k_td_root      one thread per tree: parent, depth and the length of the edge to the parent
//                  for every node of the tree rooted at tip 0.  The device form is rooted at X (the
//                  last op's cluster, y hung below it); the path tip 0 .. X is reversed; the other
//                  nodes take their depth from their parent in descending node order, in which a
//                  parent always comes first.
//   k_td_paths     one thread per (tree, pair i < j, row-major): it walks up from the deeper of
//                  the two ends until they meet, counting the edges (e, uint16) and adding the
//                  lengths of each side serially from the tip's pendant edge (h_i, h_j);
//                  p = h_i + h_j.  No subtraction.  Kept: this walk, O(depth) per pair; counting
//                  the splits that separate i and j was not written.  The arrays are read from
//                  memory at every n: there is no LDS tier here.
//   k_td_path2     a tile of 16 x 16 trees per workgroup, one lane per pair; the pair axis streams
//                  through LDS in chunks (1024 uint16 or 256 fp64 per tree).  Integers: the
//                  squared differences, four per 64-bit LDS read, summed in uint64.  fp64: the
//                  squares are rounded on their own and added serially in pair order; after every
//                  2048 pairs (8 chunks) the segment's sum is added to the total and reset (the
//                  segment rule of DESIGN 4.17), so the result depends on the two trees and n
//                  alone.
//
// Memory.  Beside pu_treeset.hip's buffers (T (n - 3) (8 nw + 44) bytes): vec, cl_len and sid,
// T (28 n - 60) bytes; for the path distances parent, depth and length per node, T (2n - 2) 16
// bytes, the integer paths T ceil4(n (n - 1) / 2) 2 bytes and, for wpath2, T n (n - 1) / 2 8 bytes
// more.  Nothing is chunked; PU_E_NOMEM where it does not fit.
#include <hip/hip_runtime.h>

#include <limits.h>
#include <math.h>
#include <stdlib.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "pu_ctx.h"
#include "pu_service.h"
#include "pu_treeset_stages.h"

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "pu_treedist.hip: gfx950 only, as the other kernel files of this library"
#endif

using namespace pu;

namespace {

constexpr size_t kLdsCap = 160 * 1024;  // LDS one workgroup may have
constexpr int kTB = 256;
constexpr int kTT = 16;      // row trees and column trees of a tile
constexpr int kChunkI = 1024;  // k_td_path2: pairs per staged chunk, integers
constexpr int kChunkD = 256;   // ... fp64; 8 chunks make a segment of 2048 pairs
constexpr int kSegChunks = 2048 / kChunkD;

inline unsigned blocks(int64_t n) { return (unsigned)((n + kTB - 1) / kTB); }

// ---- keyed lengths ----------------------------------------------------------------------------

__global__ void __launch_bounds__(kTB)
    k_td_keys(const int32_t *__restrict__ cj, const int32_t *__restrict__ y,
              const int32_t *__restrict__ emap, const double *__restrict__ lengths, int n, int64_t T,
              double *__restrict__ vec, double *__restrict__ cl_len) {
    const int E = 2 * n - 3, ns = n - 3;
    const int64_t i = (int64_t)blockIdx.x * kTB + threadIdx.x;
    if (i >= T * E) return;
    const int64_t t = i / E;
    const int k = (int)(i - t * E);
    const int c = k < E - 1 ? cj[t * (int64_t)(n - 2) * 2 + k] : y[t];
    const double len = lengths[t * E + (emap ? emap[i] : k)];
    if (c >= 0 && c < n) vec[t * E + c] = len;
    else if (c >= n && c - n < ns) cl_len[t * ns + (c - n)] = len;
}

// sid [T][ns], vec[t][n + .]: every tree's (id, length) pairs by ascending id
__global__ void __launch_bounds__(kTB)
    k_td_sort(const int32_t *__restrict__ split_id, const double *__restrict__ cl_len, int n, int P,
              int32_t *__restrict__ sid, double *__restrict__ vec) {
    extern __shared__ double lds_d[];
    double *val = lds_d;                                      // [P]
    int32_t *key = reinterpret_cast<int32_t *>(lds_d + P);    // [P]
    const int tid = (int)threadIdx.x, ns = n - 3, E = 2 * n - 3;
    const int64_t base = (int64_t)blockIdx.x * ns;
    for (int i = tid; i < P; i += kTB) {
        key[i] = i < ns ? split_id[base + i] : INT_MAX;
        val[i] = i < ns ? cl_len[base + i] : 0.0;
    }
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += kTB) {
                const int l = i ^ j;
                if (l > i) {
                    const int32_t x = key[i], z = key[l];
                    const bool up = (i & k) == 0;
                    if ((x > z) == up) {
                        const double vx = val[i], vz = val[l];
                        key[i] = z;
                        key[l] = x;
                        val[i] = vz;
                        val[l] = vx;
                    }
                }
            }
            __syncthreads();
        }
    for (int i = tid; i < ns; i += kTB) {
        sid[base + i] = key[i];
        vec[(int64_t)blockIdx.x * E + n + i] = val[i];
    }
}

// ---- weighted RF and branch score -------------------------------------------------------------

struct WeightedArgs {
    const int32_t *sid;  // [T][ns]
    const double *vec;   // [T][E]
    int n, T, n_rows;
    int in_lds;          // the tile's 32 vectors and lists are staged
    double *wrf, *kf2;   // [n_rows][T], nullable each
};

__host__ __device__ inline int sid_stride(int ns) { return ns | 1; }
__host__ inline size_t weighted_lds(int n) {
    return (size_t)2 * kTT * ((size_t)(2 * n - 3) * 8 + (size_t)sid_stride(n - 3) * 4);
}

__global__ void __launch_bounds__(kTB) k_td_weighted(WeightedArgs a) {
    extern __shared__ double lds_d[];
    const int tid = (int)threadIdx.x, n = a.n, ns = n - 3, E = 2 * n - 3, ss = sid_stride(ns);
    const int r0 = (int)blockIdx.y * kTT, c0 = (int)blockIdx.x * kTT;
    const int nr = min(kTT, a.n_rows - r0), nc = min(kTT, a.T - c0);
    int32_t *lds_i = reinterpret_cast<int32_t *>(lds_d + (size_t)2 * kTT * E);
    if (a.in_lds) {  // lists 0..15: the rows, 16..31: the columns
        for (int i = tid; i < 2 * kTT * E; i += kTB) {
            const int l = i / E, k = i - l * E;
            const int t = l < kTT ? r0 + l : c0 + l - kTT;
            const bool live = l < kTT ? l < nr : l - kTT < nc;
            if (live) lds_d[i] = a.vec[(int64_t)t * E + k];
        }
        for (int i = tid; i < 2 * kTT * ns; i += kTB) {
            const int l = i / ns, k = i - l * ns;
            const int t = l < kTT ? r0 + l : c0 + l - kTT;
            const bool live = l < kTT ? l < nr : l - kTT < nc;
            if (live) lds_i[(size_t)l * ss + k] = a.sid[(int64_t)t * ns + k];
        }
        __syncthreads();
    }
    const int i = tid / kTT, j = tid - i * kTT;
    if (i >= nr || j >= nc) return;
    const double *A = a.in_lds ? lds_d + (size_t)i * E : a.vec + (int64_t)(r0 + i) * E;
    const double *B = a.in_lds ? lds_d + (size_t)(kTT + j) * E : a.vec + (int64_t)(c0 + j) * E;
    const int32_t *IA = a.in_lds ? lds_i + (size_t)i * ss : a.sid + (int64_t)(r0 + i) * ns;
    const int32_t *IB = a.in_lds ? lds_i + (size_t)(kTT + j) * ss : a.sid + (int64_t)(c0 + j) * ns;
    double w = 0.0, q = 0.0;
    for (int k = 0; k < n; ++k) {
        const double d = __dsub_rn(A[k], B[k]);
        w = __dadd_rn(w, fabs(d));
        q = __dadd_rn(q, __dmul_rn(d, d));
    }
    int pa = 0, pb = 0;
    while (pa < ns || pb < ns) {
        const int32_t x = pa < ns ? IA[pa] : INT_MAX, z = pb < ns ? IB[pb] : INT_MAX;
        const double la = x <= z ? A[n + pa] : 0.0, lb = z <= x ? B[n + pb] : 0.0;
        const double d = __dsub_rn(la, lb);
        w = __dadd_rn(w, fabs(d));
        q = __dadd_rn(q, __dmul_rn(d, d));
        pa += x <= z ? 1 : 0;
        pb += z <= x ? 1 : 0;
    }
    const int64_t o = (int64_t)(r0 + i) * a.T + c0 + j;
    if (a.wrf) a.wrf[o] = w;
    if (a.kf2) a.kf2[o] = q;
}

// ---- length sums ------------------------------------------------------------------------------

__global__ void __launch_bounds__(kTB)
    k_td_split_sums(const uint32_t *__restrict__ perm, const uint32_t *__restrict__ first,
                    const int64_t *__restrict__ n_unique, const double *__restrict__ cl_len,
                    int64_t N, double *__restrict__ split_sum) {
    const int64_t u = (int64_t)blockIdx.x * kTB + threadIdx.x, U = *n_unique;
    if (u >= U || u >= N) return;
    const int64_t end = u + 1 < U ? (int64_t)first[u + 1] : N;
    double s = 0.0;
    for (int64_t p = first[u]; p < end; ++p) s = __dadd_rn(s, cl_len[perm[p]]);
    split_sum[u] = s;
}

__global__ void __launch_bounds__(kTB)
    k_td_tip_sums(const double *__restrict__ vec, int n, int64_t T, double *__restrict__ tip_sum) {
    const int i = (int)(blockIdx.x * kTB + threadIdx.x), E = 2 * n - 3;
    if (i >= n) return;
    double s = 0.0;
    for (int64_t t = 0; t < T; ++t) s = __dadd_rn(s, vec[t * E + i]);
    tip_sum[i] = s;
}

// ---- paths of one tree ------------------------------------------------------------------------

// par, dep [T][2n-2], nlen [T][2n-2]: the tree rooted at tip 0 (par = -1, dep = 0 there)
__global__ void __launch_bounds__(64)
    k_td_root(const int32_t *__restrict__ cj, const int32_t *__restrict__ y,
              const int32_t *__restrict__ emap, const double *__restrict__ lengths, int n, int64_t T,
              int32_t *__restrict__ par_, int32_t *__restrict__ dep_, double *__restrict__ nlen_) {
    const int64_t t = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (t >= T) return;
    const int E = 2 * n - 3, V = 2 * n - 2, X = 2 * n - 3;
    int32_t *par = par_ + t * V, *dep = dep_ + t * V;
    double *nlen = nlen_ + t * V;
    const int32_t *c2 = cj + t * (int64_t)(n - 2) * 2;
    const double *len = lengths + t * E;
    const int32_t *em = emap ? emap + t * E : nullptr;
    for (int v = 0; v < V; ++v) {
        par[v] = -1;
        dep[v] = -1;
        nlen[v] = 0.0;
    }
    for (int k = 0; k < E; ++k) {
        const int c = k < E - 1 ? c2[k] : y[t];
        if (c < 0 || c >= X) continue;  // not the device form: nothing is written
        par[c] = k < E - 1 ? n + (k >> 1) : X;
        nlen[c] = len[em ? em[k] : k];
    }
    // the path tip 0 .. X, turned round
    int v = 0, p = par[0], d = 0;
    double lv = nlen[0];
    par[0] = -1;
    nlen[0] = 0.0;
    dep[0] = 0;
    for (int guard = 0; p >= 0 && guard < V; ++guard) {
        const int next = par[p];
        const double ln = nlen[p];
        par[p] = v;
        nlen[p] = lv;
        dep[p] = ++d;
        v = p;
        p = next;
        lv = ln;
    }
    // a node off that path hangs below a larger-numbered cluster or a node of the path
    for (int u = V - 1; u >= 0; --u)
        if (dep[u] < 0) {
            const int q = par[u];
            dep[u] = q >= 0 && dep[q] >= 0 ? dep[q] + 1 : 0;
        }
}

// row-major index of pair (i, j), i < j, among the n (n - 1) / 2
__device__ inline int64_t pair_row_start(int64_t i, int n) { return i * (2 * (int64_t)n - i - 1) / 2; }

template <bool WANT_P>
__global__ void __launch_bounds__(kTB)
    k_td_paths(const int32_t *__restrict__ par_, const int32_t *__restrict__ dep_,
               const double *__restrict__ nlen_, int n, int64_t P, int64_t Pe,
               uint16_t *__restrict__ e16, double *__restrict__ p64) {
    const int64_t nb = (Pe + kTB - 1) / kTB, t = (int64_t)blockIdx.x / nb;
    const int64_t q = ((int64_t)blockIdx.x - t * nb) * kTB + threadIdx.x;
    if (q >= Pe) return;
    if (q >= P) {  // the padding of a row of e16
        e16[t * Pe + q] = 0;
        return;
    }
    const int V = 2 * n - 2;
    const int32_t *par = par_ + t * V, *dep = dep_ + t * V;
    const double *nlen = nlen_ + t * V;
    const double b2 = 2.0 * n - 1.0;
    int64_t i = (int64_t)((b2 - sqrt(b2 * b2 - 8.0 * (double)q)) * 0.5);
    i = max((int64_t)0, min(i, (int64_t)n - 2));
    while (i + 1 < n - 1 && pair_row_start(i + 1, n) <= q) ++i;
    while (i > 0 && pair_row_start(i, n) > q) --i;
    const int j = (int)(q - pair_row_start(i, n) + i + 1);
    int a = (int)i, b = j, da = dep[a], db = dep[b], e = 0;
    double ha = 0.0, hb = 0.0;
    for (int guard = 0; a != b && guard < 2 * V; ++guard) {
        const bool ua = da >= db, ub = db >= da;
        if (ua) {
            if (WANT_P) ha = __dadd_rn(ha, nlen[a]);
            a = par[a];
            --da;
            ++e;
        }
        if (ub) {
            if (WANT_P) hb = __dadd_rn(hb, nlen[b]);
            b = par[b];
            --db;
            ++e;
        }
        if (a < 0 || b < 0) break;  // not a tree: nothing more is read
    }
    e16[t * Pe + q] = (uint16_t)e;
    if (WANT_P) p64[t * P + q] = __dadd_rn(ha, hb);
}

// ---- path distances ---------------------------------------------------------------------------

struct Path2Args {
    const void *paths;  // [T][ld]: uint16 (ld a multiple of 4) or fp64
    int64_t P, ld;
    int T, n_rows;
    void *out;          // [n_rows][T]: uint64 or fp64
};

constexpr int kStrideI = kChunkI / 4 + 1;  // 64-bit words of a staged row of uint16
constexpr int kStrideD = kChunkD + 1;

__global__ void __launch_bounds__(kTB) k_td_path2_int(Path2Args a) {
    extern __shared__ double lds_d[];
    uint64_t *rows = reinterpret_cast<uint64_t *>(lds_d);  // [32][kStrideI]
    const int tid = (int)threadIdx.x;
    const int r0 = (int)blockIdx.y * kTT, c0 = (int)blockIdx.x * kTT;
    const int nr = min(kTT, a.n_rows - r0), nc = min(kTT, a.T - c0);
    const int i = tid / kTT, j = tid - i * kTT;
    const bool live = i < nr && j < nc;
    const uint64_t *src = static_cast<const uint64_t *>(a.paths);
    const int64_t ld4 = a.ld / 4;  // 64-bit words of a row: four pairs each, the tail zero
    uint64_t acc = 0;
    for (int64_t w0 = 0; w0 < ld4; w0 += kChunkI / 4) {
        const int kc = (int)min((int64_t)(kChunkI / 4), ld4 - w0);
        for (int x = tid; x < 2 * kTT * (kChunkI / 4); x += kTB) {
            const int l = x / (kChunkI / 4), k = x - l * (kChunkI / 4);
            const int t = l < kTT ? r0 + l : c0 + l - kTT;
            const bool ok = (l < kTT ? l < nr : l - kTT < nc) && k < kc;
            if (ok) rows[l * kStrideI + k] = src[(int64_t)t * ld4 + w0 + k];
        }
        __syncthreads();
        if (live) {
            const uint64_t *A = rows + i * kStrideI, *B = rows + (kTT + j) * kStrideI;
            for (int k = 0; k < kc; ++k) {
                const uint64_t x = A[k], z = B[k];
                uint32_t s = 0;
#pragma unroll
                for (int h = 0; h < 4; ++h) {
                    const int d = (int)((x >> (16 * h)) & 0xffffu) - (int)((z >> (16 * h)) & 0xffffu);
                    s += (uint32_t)(d * d);  // < 2^28 each
                }
                acc += s;
            }
        }
        __syncthreads();
    }
    if (live) static_cast<uint64_t *>(a.out)[(int64_t)(r0 + i) * a.T + c0 + j] = acc;
}

__global__ void __launch_bounds__(kTB) k_td_path2_f64(Path2Args a) {
    extern __shared__ double lds_d[];
    double *rows = lds_d;  // [32][kStrideD]
    const int tid = (int)threadIdx.x;
    const int r0 = (int)blockIdx.y * kTT, c0 = (int)blockIdx.x * kTT;
    const int nr = min(kTT, a.n_rows - r0), nc = min(kTT, a.T - c0);
    const int i = tid / kTT, j = tid - i * kTT;
    const bool live = i < nr && j < nc;
    const double *src = static_cast<const double *>(a.paths);
    double total = 0.0, seg = 0.0;
    int in_seg = 0;
    for (int64_t q0 = 0; q0 < a.P; q0 += kChunkD) {
        const int kc = (int)min((int64_t)kChunkD, a.P - q0);
        for (int x = tid; x < 2 * kTT * kChunkD; x += kTB) {
            const int l = x / kChunkD, k = x - l * kChunkD;
            const int t = l < kTT ? r0 + l : c0 + l - kTT;
            const bool ok = (l < kTT ? l < nr : l - kTT < nc) && k < kc;
            if (ok) rows[l * kStrideD + k] = src[(int64_t)t * a.ld + q0 + k];
        }
        __syncthreads();
        if (live) {
            const double *A = rows + i * kStrideD, *B = rows + (kTT + j) * kStrideD;
            for (int k = 0; k < kc; ++k) {
                const double d = __dsub_rn(A[k], B[k]);
                seg = __dadd_rn(seg, __dmul_rn(d, d));
            }
            if (++in_seg == kSegChunks) {  // 2048 pairs: the segment's sum joins the total
                total = __dadd_rn(total, seg);
                seg = 0.0;
                in_seg = 0;
            }
        }
        __syncthreads();
    }
    if (live) {
        if (in_seg) total = __dadd_rn(total, seg);
        static_cast<double *>(a.out)[(int64_t)(r0 + i) * a.T + c0 + j] = total;
    }
}

// ---- host side --------------------------------------------------------------------------------

// profiling events of the last call per device: start, after the tree-set stages, after the
// weighted stage (keys, sort, merge, sums), after the paths per tree, after the integer
// reduction, after the fp64 reduction
constexpr int kEvents = 6;
struct TreedistState {
    std::mutex mu;
    bool prof_on = false, have = false;
    hipEvent_t ev[kEvents] = {};
};
TreedistState g_td[64];

int mark(TreedistState &S, int i, hipStream_t st) {
    std::lock_guard<std::mutex> lk(S.mu);
    if (!S.prof_on) return PU_OK;
    if (i == 0) S.have = false;
    if (!S.ev[i]) HIPCHK(nullptr, hipEventCreate(&S.ev[i]));
    HIPCHK(nullptr, hipEventRecord(S.ev[i], st));
    if (i == kEvents - 1) S.have = true;
    return PU_OK;
}

}  // namespace

extern "C" {

int pu_treedist(int device, int n, int n_trees, int form, const int32_t *trees,
                const int32_t *roots, const double *lengths, int n_rows, double *wrf_out,
                double *kf2_out, uint64_t *path2_out, double *wpath2_out, int64_t *n_unique_out,
                double *split_len_sum_out, double *tip_len_sum_out) {
    const char *fn = "pu_treedist";
    int rc;
    if ((rc = treeset_check_args(fn, n, n_trees, form, trees, roots, n_rows))) return rc;
    if (!lengths) return set_err(nullptr, PU_E_ARG, "%s: null lengths", fn);
    const int64_t T = n_trees;
    const int E = 2 * n - 3, ns = n - 3, V = 2 * n - 2;
    for (int64_t t = 0; t < T; ++t)
        for (int k = 0; k < E; ++k) {
            const double x = lengths[t * E + k];
            if (!(x >= 0.0) || !std::isfinite(x))
                return set_err(nullptr, PU_E_ARG, "%s: tree %lld edge %d: length %g is not a "
                               "finite number >= 0", fn, (long long)t, k, x);
        }
    TreesetForm f;
    if ((rc = treeset_device_form(fn, n, n_trees, form, trees, roots, f))) return rc;
    if ((rc = check_device(device))) return rc;
    if (device < 0 || device >= 64) return set_err(nullptr, PU_E_ARG, "%s: device %d", fn, device);
    DeviceGuard g(device);
    HostCall h(device);
    TreedistState &S = g_td[device];
    const size_t N = (size_t)T * ns;
    const int64_t P = (int64_t)n * (n - 1) / 2, Pe = (P + 3) & ~(int64_t)3;
    const bool want_w = n_rows > 0 && (wrf_out || kf2_out);
    const bool want_i = n_rows > 0 && path2_out, want_d = n_rows > 0 && wpath2_out;
    const bool want_keys = want_w || split_len_sum_out || tip_len_sum_out;
    const size_t M = (size_t)n_rows * T;

    const int32_t *d_cj = h.to_device(f.cj.data(), f.cj.size());
    const int32_t *d_y = h.to_device(f.y.data(), f.y.size());
    const int32_t *d_emap = f.emap.empty() ? nullptr : h.to_device(f.emap.data(), f.emap.size());
    const double *d_len = h.to_device(lengths, (size_t)T * E);
    // every buffer before the first launch: the call is not chunked
    TreesetOut o;
    o.edge_ids = h.alloc<int32_t>((size_t)T * E);
    o.n_unique = h.alloc<int64_t>(1);
    o.uniq_bits = nullptr;
    o.count = nullptr;
    o.rf = nullptr;
    double *vec = want_keys ? h.alloc<double>((size_t)T * E) : nullptr;
    double *cl_len = want_keys && N ? h.alloc<double>(N) : nullptr;
    int32_t *sid = want_w && N ? h.alloc<int32_t>(N) : nullptr;
    double *d_wrf = want_w && wrf_out ? h.alloc<double>(M) : nullptr;
    double *d_kf2 = want_w && kf2_out ? h.alloc<double>(M) : nullptr;
    double *d_ssum = split_len_sum_out && N ? h.alloc<double>(N) : nullptr;
    double *d_tsum = tip_len_sum_out ? h.alloc<double>((size_t)n) : nullptr;
    const bool want_paths = want_i || want_d;
    if (want_paths && T * ((Pe + kTB - 1) / kTB) > (int64_t)INT_MAX)
        return set_err(nullptr, PU_E_NOMEM, "%s: the paths of %lld trees of %d tips do not fit the "
                       "device", fn, (long long)T, n);
    int32_t *par = want_paths ? h.alloc<int32_t>((size_t)T * V) : nullptr;
    int32_t *dep = want_paths ? h.alloc<int32_t>((size_t)T * V) : nullptr;
    double *nlen = want_paths ? h.alloc<double>((size_t)T * V) : nullptr;
    uint16_t *e16 = want_paths ? h.alloc<uint16_t>((size_t)T * Pe) : nullptr;
    double *p64 = want_d ? h.alloc<double>((size_t)T * P) : nullptr;
    uint64_t *d_p2 = want_i ? h.alloc<uint64_t>(M) : nullptr;
    double *d_wp2 = want_d ? h.alloc<double>(M) : nullptr;

    hipStream_t st = h.st;
    TreesetIds ids;
    if (!h.rc) h.rc = mark(S, 0, st);
    // the splits and their ids are needed for the split keys only
    const bool want_ids = want_w || split_len_sum_out || n_unique_out;
    if (!h.rc && want_ids)
        h.rc = treeset_run(device, st, n, T, d_cj, d_y, d_emap, 0, o, &ids);
    if (!h.rc) h.rc = mark(S, 1, st);

    if (!h.rc && want_keys) {
        hipLaunchKernelGGL(k_td_keys, dim3(blocks(T * E)), dim3(kTB), 0, st, d_cj, d_y, d_emap, d_len,
                           n, T, vec, cl_len);
        if (want_w) {
            if (N) {
                int Pw = 1;
                while (Pw < ns) Pw <<= 1;
                hipLaunchKernelGGL(k_td_sort, dim3((unsigned)T), dim3(kTB), (size_t)Pw * 12, st,
                                   ids.split_id, cl_len, n, Pw, sid, vec);
            }
            WeightedArgs a;
            a.sid = sid;
            a.vec = vec;
            a.n = n;
            a.T = (int)T;
            a.n_rows = n_rows;
            a.in_lds = weighted_lds(n) <= kLdsCap ? 1 : 0;
            a.wrf = d_wrf;
            a.kf2 = d_kf2;
            const dim3 grid((unsigned)((T + kTT - 1) / kTT),
                            (unsigned)((n_rows + kTT - 1) / kTT));
            hipLaunchKernelGGL(k_td_weighted, grid, dim3(kTB), a.in_lds ? weighted_lds(n) : 0, st, a);
        }
        if (d_ssum)
            hipLaunchKernelGGL(k_td_split_sums, dim3(blocks((int64_t)N)), dim3(kTB), 0, st, ids.perm,
                               ids.first, o.n_unique, cl_len, (int64_t)N, d_ssum);
        if (d_tsum)
            hipLaunchKernelGGL(k_td_tip_sums, dim3(blocks(n)), dim3(kTB), 0, st, vec, n, T, d_tsum);
        h.hip(fn, hipGetLastError());
    }
    if (!h.rc) h.rc = mark(S, 2, st);

    if (!h.rc && want_paths) {
        hipLaunchKernelGGL(k_td_root, dim3((unsigned)((T + 63) / 64)), dim3(64), 0, st, d_cj, d_y,
                           d_emap, d_len, n, T, par, dep, nlen);
        const dim3 grid((unsigned)(T * ((Pe + kTB - 1) / kTB)));
        if (want_d)
            hipLaunchKernelGGL(k_td_paths<true>, grid, dim3(kTB), 0, st, par, dep, nlen, n, P, Pe,
                               e16, p64);
        else
            hipLaunchKernelGGL(k_td_paths<false>, grid, dim3(kTB), 0, st, par, dep, nlen, n, P, Pe,
                               e16, p64);
        h.hip(fn, hipGetLastError());
    }
    if (!h.rc) h.rc = mark(S, 3, st);
    const dim3 tiles((unsigned)((T + kTT - 1) / kTT), (unsigned)((n_rows + kTT - 1) / kTT));
    if (!h.rc && want_i) {
        Path2Args a;
        a.paths = e16;
        a.P = P;
        a.ld = Pe;
        a.T = (int)T;
        a.n_rows = n_rows;
        a.out = d_p2;
        hipLaunchKernelGGL(k_td_path2_int, tiles, dim3(kTB), (size_t)2 * kTT * kStrideI * 8, st, a);
        h.hip(fn, hipGetLastError());
    }
    if (!h.rc) h.rc = mark(S, 4, st);
    if (!h.rc && want_d) {
        Path2Args a;
        a.paths = p64;
        a.P = P;
        a.ld = P;
        a.T = (int)T;
        a.n_rows = n_rows;
        a.out = d_wp2;
        hipLaunchKernelGGL(k_td_path2_f64, tiles, dim3(kTB), (size_t)2 * kTT * kStrideD * 8, st, a);
        h.hip(fn, hipGetLastError());
    }
    if (!h.rc) h.rc = mark(S, 5, st);

    if (d_wrf) h.to_host(wrf_out, d_wrf, M);
    if (d_kf2) h.to_host(kf2_out, d_kf2, M);
    if (d_p2) h.to_host(path2_out, d_p2, M);
    if (d_wp2) h.to_host(wpath2_out, d_wp2, M);
    if (d_tsum) h.to_host(tip_len_sum_out, d_tsum, (size_t)n);
    int64_t U = 0;
    if (want_ids) h.to_host(&U, o.n_unique, 1);
    // U is known only now: the split sums follow in a second wave of copies
    if (!h.rc) h.hip(fn, hipStreamSynchronize(st));
    if (!h.rc) {
        if (n_unique_out) *n_unique_out = U;
        if (d_ssum) h.to_host(split_len_sum_out, d_ssum, (size_t)U);
    }
    return h.finish(fn);
}

int pu_treedist_profile(int device, int on) {
    if (device < 0 || device >= 64) return set_err(nullptr, PU_E_ARG, "device %d", device);
    std::lock_guard<std::mutex> lk(g_td[device].mu);
    g_td[device].prof_on = on != 0;
    g_td[device].have = false;
    return PU_OK;
}

int pu_treedist_kernel_ms(int device, double *ids_ms, double *weighted_ms, double *paths_ms,
                          double *path2_ms, double *wpath2_ms) {
    const char *fn = "pu_treedist_kernel_ms";
    if (device < 0 || device >= 64 || !ids_ms || !weighted_ms || !paths_ms || !path2_ms ||
        !wpath2_ms)
        return set_err(nullptr, PU_E_ARG, "%s: bad argument", fn);
    std::lock_guard<std::mutex> lk(g_td[device].mu);
    TreedistState &S = g_td[device];
    if (!S.have) return set_err(nullptr, PU_E_STATE, "%s: nothing recorded", fn);
    DeviceGuard g(device);
    HIPCHK(nullptr, hipEventSynchronize(S.ev[kEvents - 1]));
    float ms[kEvents - 1];
    for (int i = 0; i < kEvents - 1; ++i)
        HIPCHK(nullptr, hipEventElapsedTime(&ms[i], S.ev[i], S.ev[i + 1]));
    *ids_ms = ms[0];
    *weighted_ms = ms[1];
    *paths_ms = ms[2];
    *path2_ms = ms[3];
    *wpath2_ms = ms[4];
    return PU_OK;
}

}  // extern "C"
