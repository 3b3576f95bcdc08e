// pu_nj.hip -- neighbour joining (Saitou-Nei in the Studier-Keppler form) and BIONJ (Gascuel
// 1997, variances initialised to the distances) from a distance matrix or a batch of them, the
// scatter of pu_pair_distances_device rows into a matrix, and the C ABI of both (pu_nj,
// pu_nj_device, pu_nj_max_lds_n, pu_pair_matrix_device).
//
// The rule (normative).  Tips are clusters 0..n-1, the m-th join creates cluster
// n + m, r = n - m clusters are live.  State: D (and V = D for BIONJ), R_i = sum_k D_ik and
// RV_i = sum_k V_ik, summed once by one thread per row in increasing k and only updated after.
//   while r > 3:  the live pair a < b (ids) with the smallest Q_ab = (r-2) D_ab - R_a - R_b
//                 (product rounded, two subtractions left to right, no contraction), ties to the
//                 lexicographically smallest (a, b);
//                 l_a = D_ab/2 + (R_a - R_b) / (2 (r-2)),  l_b = D_ab - l_a;
//                 NJ     D_uk = (D_ak + D_bk - D_ab) / 2
//                 BIONJ  lam = 1/2 + (RV_b - RV_a) / (2 (r-2) V_ab) in [0, 1], 1/2 when V_ab = 0
//                        D_uk = lam (D_ak - l_a) + (1 - lam) (D_bk - l_b)
//                        V_uk = lam V_ak + (1 - lam) V_bk - lam (1 - lam) V_ab
//                 R_k <- R_k - D_ak - D_bk + D_uk;  R_u = sum_k D_uk in increasing id, one thread
//   r = 3:        a < b < c: join (a, b) with l_a = (D_ab + D_ac - D_bc)/2,
//                 l_b = (D_ab + D_bc - D_ac)/2; root edge (2n-3, c) of (D_ac + D_bc - D_ab)/2.
//
// Storage.  A cluster lives in a slot of the matrix; a new cluster takes the slot of its child a.
// The live slots are kept as a list in increasing cluster id (the new cluster has the largest
// id, so it is appended), two copies written in turn.  Pairs of list positions p < q are then
// pairs of ids a < b, and the tie rule is the smallest (p, q).
//
//   k_nj_lds      tier A: one workgroup of 1024 threads per matrix, the upper triangle of D (and
//                 of V) in LDS, all n - 3 joins and the last step in one launch.  Wave w takes
//                 the list rows q = w + 1, w + 17, ..., its lanes the p < q; the workgroup
//                 reduces (Q, p, q) through shuffles and 16 LDS slots.
//   k_nj_copy / k_nj_sums / k_nj_partial / k_nj_join / k_nj_last
//                 tier B: the matrix stays in memory, symmetric.  Per join k_nj_partial (up to
//                 256 workgroups of 4 waves, rows strided over all waves) writes one (Q, p, q)
//                 per workgroup and k_nj_join (one workgroup) reduces them, joins and updates.
//                 r is known to the host, so every launch is queued up front; no workgroup
//                 waits on another.
//   k_pair_matrix [n_pairs][5] rows of pu_pair_distances_device -> a symmetric [n][n] matrix.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdlib.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "pu_ctx.h"
#include "pu_service.h"

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "pu_nj.hip: gfx950 only, as the other kernel files of this library"
#endif

// every product and sum below rounds on its own (the rule's Q, lengths and updates)
#pragma clang fp contract(off)

using namespace pu;

namespace {

constexpr int kNjMaxN = PU_NJ_MAX_N;      // the working copies are n^2 doubles
constexpr size_t kLdsCap = 160 * 1024;    // LDS one workgroup may have
constexpr int kTA = 1024, kWA = kTA / 64; // tier A / k_nj_join: threads, waves
constexpr int kTP = 256, kWP = kTP / 64;  // k_nj_partial
constexpr int kMaxPart = 256;             // workgroups of k_nj_partial
constexpr uint32_t kNone = 0xffffffffu;

__host__ __device__ inline size_t tri(int n) { return (size_t)n * (n - 1) / 2; }

// tier A's LDS: the triangles and row sums, the reduction slots, two live lists and the ids
__host__ inline size_t nj_lds_bytes(int n, int method) {
    return ((size_t)(1 + method) * (tri(n) + n) + kWA) * 8 + ((size_t)3 * n + kWA) * 4;
}

__host__ inline int nj_max_lds_n(int method) {
    int n = 3;
    while (n < kNjMaxN && nj_lds_bytes(n + 1, method) <= kLdsCap) ++n;
    return n;
}

struct NjOut {
    int32_t *joins;   // [n_mat][n-2][2]
    double *lens;     // [n_mat][n-2][2]
    int32_t *root;    // [n_mat][2]
    double *root_len; // [n_mat]
    double *q;        // [n_mat][n-3] or null
};

__device__ __forceinline__ bool better(double q, uint32_t k, double bq, uint32_t bk) {
    return q < bq || (q == bq && k < bk);
}

// the smallest (Q, key) of the workgroup, in every thread; red_q / red_k: one slot per wave.
// The caller separates two calls by a barrier.
__device__ __forceinline__ void block_argmin(double &q, uint32_t &k, double *red_q,
                                             uint32_t *red_k, int n_waves) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double oq = __shfl_xor(q, o, 64);
        const uint32_t ok = (uint32_t)__shfl_xor((int)k, o, 64);
        if (better(oq, ok, q, k)) {
            q = oq;
            k = ok;
        }
    }
    const int lane = (int)threadIdx.x & 63, w = (int)threadIdx.x >> 6;
    if (lane == 0) {
        red_q[w] = q;
        red_k[w] = k;
    }
    __syncthreads();
    q = red_q[0];
    k = red_k[0];
    for (int i = 1; i < n_waves; ++i)
        if (better(red_q[i], red_k[i], q, k)) {
            q = red_q[i];
            k = red_k[i];
        }
}

// what a join needs of its pair
struct Join {
    double dab, la, lb, lam, oml, c;
};

__device__ __forceinline__ Join make_join(int method, int r, double dab, double ra, double rb,
                                          double vab, double rva, double rvb) {
    Join j;
    const double den = 2.0 * (double)(r - 2);
    j.dab = dab;
    j.la = 0.5 * dab + (ra - rb) / den;
    j.lb = dab - j.la;
    j.lam = 0.5;
    if (method && vab != 0.0) {
        double lam = 0.5 + (rvb - rva) / (den * vab);
        lam = lam < 0.0 ? 0.0 : (lam > 1.0 ? 1.0 : lam);
        j.lam = lam;
    }
    j.oml = 1.0 - j.lam;
    j.c = (j.lam * j.oml) * vab;
    return j;
}

__device__ __forceinline__ double new_d(int method, const Join &j, double dak, double dbk) {
    if (!method) return 0.5 * ((dak + dbk) - j.dab);
    return j.lam * (dak - j.la) + j.oml * (dbk - j.lb);
}

__device__ __forceinline__ double new_v(const Join &j, double vak, double vbk) {
    return (j.lam * vak + j.oml * vbk) - j.c;
}

// old list position of new list position i once positions p < q have left
__device__ __forceinline__ int old_pos(int i, int p, int q) {
    if (i >= p) ++i;
    if (i >= q) ++i;
    return i;
}

// the last step, r = 3, by one thread: slots a, b, c in increasing id
__device__ __forceinline__ void last_step(int n, double dab, double dac, double dbc, int ida,
                                          int idb, int idc, const NjOut &o, int64_t mat) {
    const int m = n - 3;
    int32_t *jo = o.joins + ((int64_t)mat * (n - 2) + m) * 2;
    double *lo = o.lens + ((int64_t)mat * (n - 2) + m) * 2;
    jo[0] = ida;
    jo[1] = idb;
    lo[0] = 0.5 * ((dab + dac) - dbc);
    lo[1] = 0.5 * ((dab + dbc) - dac);
    o.root[2 * mat] = 2 * n - 3;
    o.root[2 * mat + 1] = idc;
    o.root_len[mat] = 0.5 * ((dac + dbc) - dab);
}

// ---- tier A -------------------------------------------------------------------------------

struct LdsArgs {
    const double *D;  // [n_mat][n][ld]
    int64_t ld;
    int n;
    NjOut out;
};

__device__ __forceinline__ int tri_at(int i, int j) {
    const int lo = min(i, j), hi = max(i, j);
    return hi * (hi - 1) / 2 + lo;
}

template <int METHOD>
__global__ void __launch_bounds__(kTA) k_nj_lds(LdsArgs a) {
    extern __shared__ double lds[];
    const int n = a.n, tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int nt = (int)tri(n);
    double *D = lds, *V = METHOD ? D + nt : D;
    double *R = D + (size_t)(1 + METHOD) * nt, *RV = METHOD ? R + n : R;
    double *red_q = R + (size_t)(1 + METHOD) * n;
    uint32_t *red_k = reinterpret_cast<uint32_t *>(red_q + kWA);
    int *live0 = reinterpret_cast<int *>(red_k + kWA), *live1 = live0 + n, *id = live1 + n;
    const int64_t mat = blockIdx.x;
    const double *src = a.D + mat * n * a.ld;

    for (int e = tid; e < n * n; e += kTA) {
        const int i = e / n, j = e - i * n;
        if (i < j) {
            const double d = src[(int64_t)i * a.ld + j];
            D[tri_at(i, j)] = d;
            if (METHOD) V[tri_at(i, j)] = d;
        }
    }
    if (tid < n) {
        live0[tid] = tid;
        id[tid] = tid;
    }
    __syncthreads();
    if (tid < n) {
        double s = 0.0;
        for (int k = 0; k < n; ++k)
            if (k != tid) s = s + D[tri_at(tid, k)];
        R[tid] = s;
        if (METHOD) RV[tid] = s;  // V = D: the same adds
    }
    __syncthreads();

    for (int m = 0; m + 3 < n; ++m) {
        const int r = n - m;
        const int *cur = (m & 1) ? live1 : live0;
        int *nxt = (m & 1) ? live0 : live1;
        const double mult = (double)(r - 2);
        double bq = INFINITY;
        uint32_t bk = kNone;
        for (int q = w + 1; q < r; q += kWA) {
            const int sq = cur[q];
            const double rq = R[sq];
            for (int p = lane; p < q; p += 64) {
                const int sp = cur[p];
                const double Q = (mult * D[tri_at(sp, sq)] - R[sp]) - rq;
                const uint32_t key = ((uint32_t)p << 16) | (uint32_t)q;
                if (better(Q, key, bq, bk)) {
                    bq = Q;
                    bk = key;
                }
            }
        }
        block_argmin(bq, bk, red_q, red_k, kWA);
        if (bk == kNone) bk = 1u;  // nothing compared below +inf (NaN input): positions (0, 1)
        const int p = (int)(bk >> 16), q = (int)(bk & 0xffffu);
        const int sa = cur[p], sb = cur[q];
        const int ab = tri_at(sa, sb);
        const Join j = make_join(METHOD, r, D[ab], R[sa], R[sb], V[ab], RV[sa], RV[sb]);
        if (tid == 0) {
            int32_t *jo = a.out.joins + (mat * (n - 2) + m) * 2;
            double *lo = a.out.lens + (mat * (n - 2) + m) * 2;
            jo[0] = id[sa];
            jo[1] = id[sb];
            lo[0] = j.la;
            lo[1] = j.lb;
            if (a.out.q) a.out.q[mat * (n - 3) + m] = bq;
        }
        for (int pos = tid; pos < r; pos += kTA) {
            if (pos == p || pos == q) continue;
            const int sk = cur[pos];
            const int ak = tri_at(sa, sk), bk2 = tri_at(sb, sk);
            const double dak = D[ak], dbk = D[bk2];
            const double duk = new_d(METHOD, j, dak, dbk);
            D[ak] = duk;
            R[sk] = ((R[sk] - dak) - dbk) + duk;
            if (METHOD) {
                const double vak = V[ak], vbk = V[bk2];
                const double vuk = new_v(j, vak, vbk);
                V[ak] = vuk;
                RV[sk] = ((RV[sk] - vak) - vbk) + vuk;
            }
        }
        for (int i = tid; i < r - 1; i += kTA) nxt[i] = i == r - 2 ? sa : cur[old_pos(i, p, q)];
        __syncthreads();
        if (tid == 0) {
            double s = 0.0;
            for (int i = 0; i < r - 2; ++i) s = s + D[tri_at(sa, nxt[i])];
            R[sa] = s;
            id[sa] = n + m;
        }
        if (METHOD && tid == 64) {
            double s = 0.0;
            for (int i = 0; i < r - 2; ++i) s = s + V[tri_at(sa, nxt[i])];
            RV[sa] = s;
        }
        __syncthreads();
    }
    if (tid == 0) {
        const int *cur = ((n - 3) & 1) ? live1 : live0;
        const int sa = cur[0], sb = cur[1], sc = cur[2];
        last_step(n, D[tri_at(sa, sb)], D[tri_at(sa, sc)], D[tri_at(sb, sc)], id[sa], id[sb],
                  id[sc], a.out, mat);
    }
}

// ---- tier B -------------------------------------------------------------------------------

struct MemState {
    double *D, *V;     // [n][n] symmetric working copies (V: BIONJ)
    double *R, *RV;    // [n]
    double *pq;        // [kMaxPart]
    uint32_t *pk;      // [kMaxPart]
    int *live[2], *id; // [n] each
    int n;
};

__global__ void __launch_bounds__(256)
    k_nj_copy(MemState s, int method, const double *__restrict__ src, int64_t ld) {
    const int n = s.n;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)n * n) return;
    const int i = (int)(e / n), j = (int)(e - (int64_t)i * n);
    const double d = i == j ? 0.0 : src[(int64_t)min(i, j) * ld + max(i, j)];
    s.D[e] = d;
    if (method) s.V[e] = d;
    if (e < n) {
        s.live[0][e] = (int)e;
        s.id[e] = (int)e;
    }
}

__global__ void __launch_bounds__(256) k_nj_sums(MemState s, int method) {
    const int n = s.n, i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= n) return;
    double acc = 0.0;
    for (int k = 0; k < n; ++k)
        if (k != i) acc = acc + s.D[(size_t)k * n + i];  // = D[i][k]: the copy is symmetric
    s.R[i] = acc;
    if (method) s.RV[i] = acc;
}

__global__ void __launch_bounds__(kTP) k_nj_partial(MemState s, int m) {
    __shared__ double red_q[kWP];
    __shared__ uint32_t red_k[kWP];
    const int n = s.n, r = n - m;
    const int *cur = s.live[m & 1];
    const int lane = (int)threadIdx.x & 63;
    const int gw = (int)blockIdx.x * kWP + ((int)threadIdx.x >> 6), n_gw = (int)gridDim.x * kWP;
    const double mult = (double)(r - 2);
    double bq = INFINITY;
    uint32_t bk = kNone;
    for (int q = gw + 1; q < r; q += n_gw) {
        const int sq = cur[q];
        const double rq = s.R[sq];
        const double *row = s.D + (size_t)sq * n;
        for (int p = lane; p < q; p += 64) {
            const int sp = cur[p];
            const double Q = (mult * row[sp] - s.R[sp]) - rq;
            const uint32_t key = ((uint32_t)p << 16) | (uint32_t)q;
            if (better(Q, key, bq, bk)) {
                bq = Q;
                bk = key;
            }
        }
    }
    block_argmin(bq, bk, red_q, red_k, kWP);
    if (threadIdx.x == 0) {
        s.pq[blockIdx.x] = bq;
        s.pk[blockIdx.x] = bk;
    }
}

template <int METHOD>
__global__ void __launch_bounds__(kTA) k_nj_join(MemState s, int m, int n_part, NjOut out,
                                                 int64_t mat) {
    extern __shared__ double du[];  // [r - 2] D_uk in new list order, then [r - 2] V_uk
    __shared__ double red_q[kWA];
    __shared__ uint32_t red_k[kWA];
    const int n = s.n, r = n - m, tid = (int)threadIdx.x;
    const int *cur = s.live[m & 1];
    int *nxt = s.live[(m + 1) & 1];
    double *dv = du + (r - 2);
    double bq = tid < n_part ? s.pq[tid] : INFINITY;
    uint32_t bk = tid < n_part ? s.pk[tid] : kNone;
    block_argmin(bq, bk, red_q, red_k, kWA);
    if (bk == kNone) bk = 1u;
    const int p = (int)(bk >> 16), q = (int)(bk & 0xffffu);
    const int sa = cur[p], sb = cur[q];
    double *Da = s.D + (size_t)sa * n, *Db = s.D + (size_t)sb * n;
    double *Va = METHOD ? s.V + (size_t)sa * n : Da, *Vb = METHOD ? s.V + (size_t)sb * n : Db;
    const Join j = make_join(METHOD, r, Da[sb], s.R[sa], s.R[sb], Va[sb],
                             METHOD ? s.RV[sa] : 0.0, METHOD ? s.RV[sb] : 0.0);
    // the update below writes neither the pair's own entries nor its sums and id
    if (tid == 0) {
        int32_t *jo = out.joins + (mat * (n - 2) + m) * 2;
        double *lo = out.lens + (mat * (n - 2) + m) * 2;
        jo[0] = s.id[sa];
        jo[1] = s.id[sb];
        lo[0] = j.la;
        lo[1] = j.lb;
        if (out.q) out.q[mat * (n - 3) + m] = bq;
    }
    for (int pos = tid; pos < r; pos += kTA) {
        if (pos == p || pos == q) continue;
        const int sk = cur[pos];
        const int i = pos - (pos > p) - (pos > q);
        const double dak = Da[sk], dbk = Db[sk];
        const double duk = new_d(METHOD, j, dak, dbk);
        Da[sk] = duk;
        s.D[(size_t)sk * n + sa] = duk;
        s.R[sk] = ((s.R[sk] - dak) - dbk) + duk;
        du[i] = duk;
        if (METHOD) {
            const double vak = Va[sk], vbk = Vb[sk];
            const double vuk = new_v(j, vak, vbk);
            Va[sk] = vuk;
            s.V[(size_t)sk * n + sa] = vuk;
            s.RV[sk] = ((s.RV[sk] - vak) - vbk) + vuk;
            dv[i] = vuk;
        }
    }
    for (int i = tid; i < r - 1; i += kTA) nxt[i] = i == r - 2 ? sa : cur[old_pos(i, p, q)];
    __syncthreads();
    if (tid == 0) {
        double acc = 0.0;
        for (int i = 0; i < r - 2; ++i) acc = acc + du[i];
        s.R[sa] = acc;
        s.id[sa] = n + m;
    }
    if (METHOD && tid == 64) {
        double acc = 0.0;
        for (int i = 0; i < r - 2; ++i) acc = acc + dv[i];
        s.RV[sa] = acc;
    }
}

__global__ void k_nj_last(MemState s, NjOut out, int64_t mat) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int n = s.n;
    const int *cur = s.live[(n - 3) & 1];
    const int sa = cur[0], sb = cur[1], sc = cur[2];
    last_step(n, s.D[(size_t)sa * n + sb], s.D[(size_t)sa * n + sc], s.D[(size_t)sb * n + sc],
              s.id[sa], s.id[sb], s.id[sc], out, mat);
}

// ---- scatter ------------------------------------------------------------------------------

// without a pair list: one thread per matrix entry of every matrix of the batch; pair (i, j),
// i < j, is row i n - i (i + 1) / 2 + j - i - 1 of the matrix's out5 rows; the diagonal is zero
__global__ void __launch_bounds__(256)
    k_pair_matrix_all(int n_mat, int n, const double *__restrict__ out5, double *__restrict__ D,
                      int64_t ld) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x, nn = (int64_t)n * n;
    if (e >= nn * n_mat) return;
    const int64_t r = e / nn, k = e - r * nn;
    const int i = (int)(k / n), j = (int)(k - (int64_t)i * n);
    double d = 0.0;
    if (i != j) {
        const int64_t lo = min(i, j), hi = max(i, j), np = (nn - n) / 2;
        d = out5[5 * (r * np + lo * n - lo * (lo + 1) / 2 + hi - lo - 1)];
    }
    D[(r * n + i) * ld + j] = d;
}

// with a pair list: both entries of every listed pair; nothing else is written
__global__ void __launch_bounds__(256)
    k_pair_matrix_list(int64_t n_pairs, const int32_t *__restrict__ pairs,
                       const double *__restrict__ out5, double *__restrict__ D, int64_t ld) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n_pairs) return;
    const int64_t i = pairs[2 * p], j = pairs[2 * p + 1];
    const double d = out5[5 * p];
    D[i * ld + j] = d;
    D[j * ld + i] = d;
}

// ---- host side ---------------------------------------------------------------------------

// per-device buffers of tier B and of the scatter (DevState: pu_service.h)
struct NjState : DevState {
    DevBuf<double> ws;
    DevBuf<int32_t> iw;
    PairList pairs;
};
NjState g_nj[64];

int check_nj(const char *fn, int method, int n_mat, int n, const void *D, int64_t ld,
             const NjOut &o) {
    if (!D || !o.joins || !o.lens || !o.root || !o.root_len)
        return set_err(nullptr, PU_E_ARG, "%s: null buffer", fn);
    if (method != 0 && method != 1)
        return set_err(nullptr, PU_E_ARG, "%s: method = %d (0 NJ, 1 BIONJ)", fn, method);
    if (n < 3 || n > kNjMaxN)
        return set_err(nullptr, PU_E_ARG, "%s: n = %d is outside [3, %d]", fn, n, kNjMaxN);
    if (n_mat < 1) return set_err(nullptr, PU_E_ARG, "%s: n_mat = %d", fn, n_mat);
    if (ld < n)
        return set_err(nullptr, PU_E_ARG, "%s: row stride %lld below n = %d", fn, (long long)ld,
                       n);
    return PU_OK;
}

// PU_NJ_TIER=A|B forces a tier where n allows it
bool use_lds(int n, int method) {
    const bool fits = n <= nj_max_lds_n(method);
    if (const char *env = getenv("PU_NJ_TIER")) {
        if (env[0] == 'B' || env[0] == 'b') return false;
    }
    return fits;
}

int run_nj(int device, hipStream_t st, int method, int n_mat, int n, const double *d_D,
           int64_t ld, const NjOut &o) {
    NjState &S = g_nj[device];
    StateScope scope(S, st);
    if (scope.rc) return scope.rc;
    if (use_lds(n, method)) {
        LdsArgs a{d_D, ld, n, o};
        const size_t lds = nj_lds_bytes(n, method);
        if (method) hipLaunchKernelGGL(k_nj_lds<1>, dim3(n_mat), dim3(kTA), lds, st, a);
        else hipLaunchKernelGGL(k_nj_lds<0>, dim3(n_mat), dim3(kTA), lds, st, a);
        HIPCHK(nullptr, hipGetLastError());
    } else {
        const size_t nn = (size_t)n * n;
        int rc;
        if ((rc = S.ws.reserve((size_t)(1 + method) * (nn + n) + kMaxPart))) return rc;
        if ((rc = S.iw.reserve((size_t)3 * n + kMaxPart))) return rc;
        MemState s;
        s.n = n;
        s.D = S.ws.p;
        s.V = method ? s.D + nn : s.D;
        s.R = S.ws.p + (size_t)(1 + method) * nn;
        s.RV = method ? s.R + n : s.R;
        s.pq = s.R + (size_t)(1 + method) * n;
        s.live[0] = S.iw.p;
        s.live[1] = S.iw.p + n;
        s.id = S.iw.p + 2 * (size_t)n;
        s.pk = reinterpret_cast<uint32_t *>(S.iw.p + 3 * (size_t)n);
        for (int64_t mat = 0; mat < n_mat; ++mat) {
            hipLaunchKernelGGL(k_nj_copy, dim3((unsigned)((nn + 255) / 256)), dim3(256), 0, st, s,
                               method, d_D + mat * n * ld, ld);
            hipLaunchKernelGGL(k_nj_sums, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, s,
                               method);
            for (int m = 0; m + 3 < n; ++m) {
                const int r = n - m;
                const int n_part = std::max(1, std::min(kMaxPart, (r - 1 + kWP - 1) / kWP));
                hipLaunchKernelGGL(k_nj_partial, dim3(n_part), dim3(kTP), 0, st, s, m);
                const size_t lds = (size_t)(1 + method) * (r - 2) * 8;
                if (method)
                    hipLaunchKernelGGL(k_nj_join<1>, dim3(1), dim3(kTA), lds, st, s, m, n_part, o,
                                       mat);
                else
                    hipLaunchKernelGGL(k_nj_join<0>, dim3(1), dim3(kTA), lds, st, s, m, n_part, o,
                                       mat);
            }
            hipLaunchKernelGGL(k_nj_last, dim3(1), dim3(64), 0, st, s, o, mat);
            HIPCHK(nullptr, hipGetLastError());
        }
    }
    return PU_OK;
}

}  // namespace

int pu::pair_matrix_all(hipStream_t st, int n_mat, int n, const double *d_out5, double *d_D,
                        int64_t ld) {
    const int64_t ne = (int64_t)n_mat * n * n;
    hipLaunchKernelGGL(k_pair_matrix_all, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, st,
                       n_mat, n, d_out5, d_D, ld);
    HIPCHK(nullptr, hipGetLastError());
    return PU_OK;
}

extern "C" {

int pu_nj_max_lds_n(int method) {
    if (method != 0 && method != 1) return set_err(nullptr, PU_E_ARG, "method = %d", method);
    return nj_max_lds_n(method);
}

int pu_nj_device(int device, void *stream, int method, int n_mat, int n, const double *d_D,
                 int64_t ld, int32_t *d_joins, double *d_lens, int32_t *d_root,
                 double *d_root_len, double *d_q) {
    const NjOut o{d_joins, d_lens, d_root, d_root_len, d_q};
    int rc;
    if ((rc = check_nj("pu_nj_device", method, n_mat, n, d_D, ld, o))) return rc;
    if ((rc = check_device(device))) return rc;
    DeviceGuard g(device);
    return run_nj(device, (hipStream_t)stream, method, n_mat, n, d_D, ld, o);
}

int pu_nj(int device, int method, int n_mat, int n, const double *D, int32_t *joins_out,
          double *lens_out, int32_t *root_out, double *root_len_out, double *q_out) {
    const char *fn = "pu_nj";
    const NjOut ho{joins_out, lens_out, root_out, root_len_out, q_out};
    int rc;
    if ((rc = check_nj(fn, method, n_mat, n, D, n, ho))) return rc;
    for (int64_t b = 0; b < n_mat; ++b)
        for (int i = 0; i < n; ++i)
            for (int j = i + 1; j < n; ++j) {
                const double d = D[(b * n + i) * n + j];
                if (!(d >= 0.0) || !(d < INFINITY))
                    return set_err(nullptr, PU_E_ARG, "%s: matrix %lld entry (%d, %d) = %g", fn,
                                   (long long)b, i, j, d);
            }
    if ((rc = check_device(device))) return rc;
    DeviceGuard g(device);
    HostCall h(device);
    const size_t nD = (size_t)n_mat * n * n, nj = (size_t)n_mat * (n - 2) * 2;
    const size_t nq = (size_t)n_mat * (n - 3);
    const double *d_D = h.to_device(D, nD);
    double *d_f = h.alloc<double>(nj + n_mat + nq);          // lens, root_len, q
    int32_t *d_i = h.alloc<int32_t>(nj + 2 * (size_t)n_mat);  // joins, root
    if (!h.rc) {
        const NjOut o{d_i, d_f, d_i + nj, d_f + nj, q_out && nq ? d_f + nj + n_mat : nullptr};
        h.rc = run_nj(device, h.st, method, n_mat, n, d_D, n, o);
        h.to_host(joins_out, o.joins, nj);
        h.to_host(lens_out, o.lens, nj);
        h.to_host(root_out, o.root, (size_t)n_mat * 2);
        h.to_host(root_len_out, o.root_len, (size_t)n_mat);
        if (o.q) h.to_host(q_out, o.q, nq);
    }
    return h.finish(fn);
}

int pu_pair_matrix_device(int device, void *stream, int n_taxa, int64_t n_pairs,
                          const int32_t *pairs, const double *d_out5, double *d_D, int64_t ld) {
    const char *fn = "pu_pair_matrix_device";
    if (!d_out5 || !d_D) return set_err(nullptr, PU_E_ARG, "%s: null buffer", fn);
    if (n_taxa < 2 || n_taxa > kNjMaxN)
        return set_err(nullptr, PU_E_ARG, "%s: n_taxa = %d is outside [2, %d]", fn, n_taxa,
                       kNjMaxN);
    if (ld < n_taxa)
        return set_err(nullptr, PU_E_ARG, "%s: row stride %lld below n_taxa = %d", fn,
                       (long long)ld, n_taxa);
    int rc;
    if ((rc = check_pairs(fn, n_taxa, n_pairs, pairs))) return rc;
    if ((rc = check_device(device))) return rc;
    DeviceGuard g(device);
    hipStream_t st = (hipStream_t)stream;
    NjState &S = g_nj[device];
    StateScope scope(S, st);
    if ((rc = scope.rc)) return rc;
    if (!pairs) return pair_matrix_all(st, 1, n_taxa, d_out5, d_D, ld);
    if ((rc = S.pairs.upload(st, n_taxa, n_pairs, pairs))) return rc;
    hipLaunchKernelGGL(k_pair_matrix_list, dim3((unsigned)((n_pairs + 255) / 256)), dim3(256), 0,
                       st, n_pairs, S.pairs.d.p, d_out5, d_D, ld);
    HIPCHK(nullptr, hipGetLastError());
    return PU_OK;
}

}  // extern "C"
