// pu_bootstrap.hip -- nonparametric bootstrap (Felsenstein 1985) of distance trees on the GPU:
// resampled site weights, the pair count matrices of all replicates in one pass over the
// alignment, the replicates' distance matrices and trees, and the support of a reference tree's
// splits; and the C ABI of it (pu_boot_weights[_device], pu_boot_pair_counts,
// pu_boot_distances[_device], pu_split_support[_device], pu_bootstrap_nj).
//
// The reference has no tree builder and no bootstrap; the rule is this project's own
// (normative).  S site patterns with non-negative integer weights w_s (fp64; NULL:
// all 1), N = sum_s w_s in [1, 2^31 - 1].  Replicate r (a global number: first_rep continues a
// series) draws N columns j = 0..N-1:
//     (x0, x1, ..) = philox4x32_10(counter = (j lo, j hi, r, 1), key = (seed lo, seed hi))
//     u = ((x1 >> 5) * 2^26 + (x0 >> 6)) * 2^-53       the simulator's u; counter word 3 = 1
//                                                       keeps the two streams apart
//     c = min(floor(u * N), N - 1)                      one fp64 multiply
//     s = the first pattern whose inclusive integer prefix sum of w exceeds c
//     W[r][s] += 1                                      uint32
// The counts are integers: W does not depend on the grid, the order of the adds or on which
// other replicates the call asked for.  The scaled form (pu_boot_weights_scaled[_device], DESIGN
// 4.24) is the same rule with j = 0..n_draw-1 -- c still uses N --, so a row sums to n_draw and
// with n_draw = N it is the row above, bit for bit.  Replicate r's pair count matrices are
//     N_ab^(r)[u][v] = sum_s W[r][s] [code_a(s) = u][code_b(s) = v],
// integers again, so they are exact and equal, bit for bit, to what pu_pair_counts gives for
// site_weights = W[r]; the Newton step (pu_distance.hip k_pair_newton, unchanged) and the
// joining (pu_nj.hip, unchanged) then run on all replicates at once.  A split is the tip set of
// a cluster n + m, m = 0..n-4, of a tree in pu_nj's join form, as a bitset of ceil(n / 64)
// words, complemented when it holds tip 0; support[m] of a reference split is the share of the
// ok replicates (every upper-triangle distance finite) whose tree holds an equal bitset.
//
//   k_boot_prefix       one workgroup: the inclusive prefix sums of the weights (as integers) and
//                       their total N.  Each thread sums a contiguous range, thread 0 scans the
//                       1024 partial sums, each thread then writes its range.
//   k_boot_weights      one lane per (replicate, column): the draw, a binary search of the prefix
//                       sums (none for unit weights: s = c) and a 32-bit atomic add into
//                       W [n_rep][ldw].  Grid-stride: the grid does not need N on the host.  The
//                       number of columns is N, one n_draw for the launch or one per row.
//   k_boot_pair_counts  k_pair_counts with lane = replicate in place of lane = pair.  A
//                       workgroup owns P pairs (one wave each), a tile of T <= 64 replicates and
//                       a segment of the sites.  It stages 128-site chunks of the pairs' code
//                       rows -- read once for the whole tile, not once per replicate -- and of the
//                       tile's W rows, transposed, in LDS; then for each site every lane of a
//                       wave reads the same (u, v) as a broadcast and its own W[r][s] and adds
//                       into its own replicate's uint32 bins in LDS (odd stride between lanes).
//                       One writer per bin, no atomics, no divergence.  T and P follow from
//                       n_codes and the 160 KiB of LDS (DNA's 15 codes: T = 64, P = 2; 32 codes:
//                       T = 32, P = 1).  One segment: the bins are written as fp64
//                       [n_rep][n_pairs][n_codes^2], the layout k_pair_newton reads.
//   k_boot_merge        several segments: their uint32 slabs added as integers, then to fp64.
//   (pu_nj.hip)         k_pair_matrix_all: the t column of out5 [n_rep][n_pairs][5] as matrices
//                       [n_rep][n][ld].
//   k_boot_ok           one workgroup per replicate: ok[r] = every upper-triangle entry finite.
//   k_boot_splits       one workgroup per tree, thread w owns word w of every cluster's bitset:
//                       cluster n + m is the OR of its children's, in join order (a thread reads
//                       back only words it wrote itself); then the complement rule.
//   k_boot_support      one workgroup per reference split: full-word comparison with every
//                       split of every ok replicate, count / n_ok.
//
// Range.  The split kernels are written for the trees the LDS tier of pu_nj serves, up to a few
// hundred taxa (measured: 200 taxa x 100 replicates, 0.17 ms): k_boot_splits walks the n - 3
// joins of a tree serially per bitset word, and k_boot_support compares every reference split
// with all n_rep (n - 3) replicate splits, n^2 n_rep ceil(n / 64) word compares in all and no
// hash prefilter.  They are correct up to PU_NJ_MAX_N but have not been timed in the thousands.
// Memory.  Only the count matrices are chunked (256 MiB, the pair calls' policy).
// pu_bootstrap_nj holds the out5 rows, matrices and join arrays of all replicates at once,
// (1 + n_rep) (5 n (n - 1) / 2 + n^2 + 2 (n - 2) + 1) doubles, and W, n_rep n_sites words; where
// that does not fit it returns PU_E_NOMEM and the separate calls, over ranges of replicates
// (first_rep), still run.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdlib.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "pu_ctx.h"
#include "pu_service.h"
#include "pu_philox.h"

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "pu_bootstrap.hip: gfx950 only, as the other kernel files of this library"
#endif

using namespace pu;

namespace {

constexpr size_t kLdsCap = 160 * 1024;              // LDS one workgroup may have
constexpr int kMaxWaves = 4;                        // k_boot_pair_counts: pairs per workgroup
constexpr int kMinTile = 4;                         // replicates per tile, at least
constexpr size_t kBootWsBytes = (size_t)256 << 20;  // count matrices and slabs of one chunk
constexpr int kMaxSeg = 32;
constexpr int64_t kMaxN = 0x7fffffff;
constexpr int kPT = 1024;                           // k_boot_prefix threads

// ---- weights ------------------------------------------------------------------------------

__global__ void __launch_bounds__(kPT)
    k_boot_prefix(const double *__restrict__ w, int64_t S, uint32_t *__restrict__ prefix,
                  int64_t *__restrict__ total) {
    __shared__ int64_t part[kPT];
    const int t = (int)threadIdx.x;
    const int64_t per = (S + kPT - 1) / kPT;
    const int64_t lo = min(S, (int64_t)t * per), hi = min(S, lo + per);
    int64_t acc = 0;
    for (int64_t s = lo; s < hi; ++s) acc += (int64_t)w[s];
    part[t] = acc;
    __syncthreads();
    if (t == 0) {
        int64_t run = 0;
        for (int i = 0; i < kPT; ++i) {
            const int64_t x = part[i];
            part[i] = run;
            run += x;
        }
        *total = run;
    }
    __syncthreads();
    int64_t run = part[t];
    for (int64_t s = lo; s < hi; ++s) {
        run += (int64_t)w[s];
        prefix[s] = (uint32_t)run;
    }
}

struct WeightArgs {
    uint64_t seed;
    uint32_t first_rep;
    int n_rep;
    int64_t S;
    const uint32_t *prefix;  // [S] or null: unit weights
    const int64_t *total;    // N (with prefix)
    uint32_t *W;             // [n_rep][ldw], zeroed
    int64_t ldw;
    int64_t n_draw;          // columns of every row; 0: N
    const int64_t *n_draws;  // [n_rep] columns of each row, or null: n_draw
};

__global__ void __launch_bounds__(256) k_boot_weights(WeightArgs a) {
    const int64_t N = a.prefix ? *a.total : a.S;
    if (N < 1 || N > kMaxN) return;  // outside the rule: W stays zero
    const double dN = (double)N;
    for (int r = (int)blockIdx.y; r < a.n_rep; r += (int)gridDim.y) {
        uint32_t *row = a.W + (int64_t)r * a.ldw;
        const int64_t n = a.n_draws ? a.n_draws[r] : a.n_draw > 0 ? a.n_draw : N;
        if (n > kMaxN) continue;  // outside the rule: the row stays zero
        for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < n;
             j += (int64_t)gridDim.x * 256) {
            const double u = philox_u(a.seed, (uint64_t)j, a.first_rep + (uint32_t)r, 1u);
            int64_t c = (int64_t)__dmul_rn(u, dN);
            c = min(c, N - 1);
            int64_t s = c;
            if (a.prefix) {  // the first s with prefix[s] > c; prefix[S - 1] = N > c
                int64_t lo = 0, hi = a.S - 1;
                while (lo < hi) {
                    const int64_t mid = (lo + hi) >> 1;
                    if ((int64_t)a.prefix[mid] > c) hi = mid;
                    else lo = mid + 1;
                }
                s = lo;
            }
            atomicAdd(row + s, 1u);
        }
    }
}

// ---- pair counts of all replicates ----------------------------------------------------------

struct BootCountArgs {
    const uint8_t *codes;  // [n_taxa][ld]
    int64_t ld, S;
    const uint32_t *W;     // [n_rep][ldw]: this launch's replicates
    int64_t ldw;
    int n_rep;
    const int32_t *pairs;  // [n_pairs][2], this launch's
    int64_t n_pairs;
    int n_codes, P, T;     // pairs (waves) per workgroup, replicates per tile
    int64_t seg;           // sites per segment (a multiple of kCH); blockIdx.z: the segment
    double *out;           // [n_rep][n_pairs][n_codes^2] (one segment)
    uint32_t *slabs;       // [segments][n_rep][n_pairs][n_codes^2] or null
};

__host__ inline size_t count_lds(int n_codes, int P, int T) {
    return ((size_t)P * T * bin_stride(n_codes) + (size_t)kCH * (T + 1)) * 4 + (size_t)2 * P * kRow;
}

__global__ void __launch_bounds__(64 * kMaxWaves) k_boot_pair_counts(BootCountArgs a) {
    extern __shared__ uint32_t lds32[];
    const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6, nthr = (int)blockDim.x;
    const int n = a.n_codes, nb = n * n, bs = bin_stride(n), T = a.T, tw = T + 1;
    uint32_t *bins = lds32;                                    // [P][T][bs]
    uint32_t *wl = bins + (size_t)a.P * T * bs;                // [kCH][tw]: site-major
    uint8_t *st = reinterpret_cast<uint8_t *>(wl + kCH * tw);  // [2 P][kRow]
    const int64_t p0 = (int64_t)blockIdx.x * a.P;
    const int np = (int)min((int64_t)a.P, a.n_pairs - p0);
    const int r0 = (int)blockIdx.y * T, nr = min(T, a.n_rep - r0);
    const int64_t s_lo = (int64_t)blockIdx.z * a.seg, s_hi = min(a.S, s_lo + a.seg);
    for (int i = tid; i < a.P * T * bs; i += nthr) bins[i] = 0u;
    const int32_t *rows = a.pairs + 2 * p0;  // staged row 2 p + side is taxon rows[2 p + side]
    uint32_t *mine = bins + ((size_t)w * T + (lane < T ? lane : 0)) * bs;
    const uint32_t *sa = reinterpret_cast<const uint32_t *>(st + (size_t)2 * w * kRow);
    const uint32_t *sb = reinterpret_cast<const uint32_t *>(st + (size_t)(2 * w + 1) * kRow);
    const uint32_t *wm = wl + (lane < T ? lane : 0);
    for (int64_t s0 = s_lo; s0 < s_hi; s0 += kCH) {
        const int m = (int)min((int64_t)kCH, s_hi - s0);
        __syncthreads();  // the previous chunk has been consumed
        for (int r = 0; r < 2 * np; ++r) {
            const uint8_t *src = a.codes + (int64_t)rows[r] * a.ld + s0;
            for (int c = tid; c < kCH; c += nthr) st[r * kRow + c] = c < m ? src[c] : (uint8_t)255;
        }
        for (int i = tid; i < T * kCH; i += nthr) {
            const int r = i / kCH, c = i - r * kCH;
            wl[c * tw + r] = (r < nr && c < m) ? a.W[(int64_t)(r0 + r) * a.ldw + s0 + c] : 0u;
        }
        __syncthreads();
        if (w < np && lane < T) {
            for (int c4 = 0; c4 < (m + 3) / 4; ++c4) {
                uint32_t ua = sa[c4], ub = sb[c4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int u = (int)(ua & 255u), v = (int)(ub & 255u);
                    ua >>= 8;
                    ub >>= 8;
                    // a code outside the table (the padding's 255 too) counts nowhere
                    if (u < n && v < n) mine[u * n + v] += wm[(4 * c4 + k) * tw];
                }
            }
        }
    }
    __syncthreads();
    const size_t slab = (size_t)a.n_rep * a.n_pairs * nb;
    for (int p = 0; p < np; ++p)
        for (int i = tid; i < nr * nb; i += nthr) {
            const int r = i / nb, b = i - r * nb;
            const uint32_t x = bins[((size_t)p * T + r) * bs + b];
            const size_t e = ((size_t)(r0 + r) * a.n_pairs + p0 + p) * nb + b;
            if (a.slabs) a.slabs[(size_t)blockIdx.z * slab + e] = x;
            else a.out[e] = (double)x;
        }
}

__global__ void __launch_bounds__(256)
    k_boot_merge(const uint32_t *__restrict__ slabs, int n_seg, size_t n, double *__restrict__ out) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    uint64_t acc = 0;
    for (int g = 0; g < n_seg; ++g) acc += slabs[(size_t)g * n + e];
    out[e] = (double)acc;
}

// ---- matrices -----------------------------------------------------------------------------

__global__ void __launch_bounds__(256)
    k_boot_ok(int n, const double *__restrict__ D, int64_t ld, int32_t *__restrict__ ok) {
    const int64_t r = blockIdx.x;
    const double *M = D + r * n * ld;
    int bad = 0;
    for (int e = (int)threadIdx.x; e < n * n; e += 256) {
        const int i = e / n, j = e - i * n;
        if (i < j && !isfinite(M[(int64_t)i * ld + j])) bad = 1;
    }
    bad = __syncthreads_or(bad);
    if (threadIdx.x == 0) ok[r] = bad ? 0 : 1;
}

// ---- splits and their support ---------------------------------------------------------------

// bits [n_trees][n - 3][nw]: the canonical tip bitset of cluster n + m of every tree
__global__ void __launch_bounds__(64)
    k_boot_splits(const int32_t *__restrict__ joins, int n, int nw, uint64_t *bits) {
    extern __shared__ uint8_t flag[];  // [n - 3]: cluster m holds tip 0
    const int tid = (int)threadIdx.x, ns = n - 3;
    const int32_t *jo = joins + (int64_t)blockIdx.x * (n - 2) * 2;
    uint64_t *out = bits + (int64_t)blockIdx.x * ns * nw;
    for (int w = tid; w < nw; w += 64)
        for (int m = 0; m < ns; ++m) {
            uint64_t x = 0;
            for (int side = 0; side < 2; ++side) {
                const int c = jo[2 * m + side];
                if (c < 0 || c >= n + m) continue;  // not a join form: nothing is read for it
                if (c < n) {
                    if ((c >> 6) == w) x |= 1ull << (c & 63);
                } else {
                    x |= out[(int64_t)(c - n) * nw + w];  // written by this thread, earlier
                }
            }
            out[(int64_t)m * nw + w] = x;
        }
    __syncthreads();
    for (int m = tid; m < ns; m += 64) flag[m] = (uint8_t)(out[(int64_t)m * nw] & 1ull);
    __syncthreads();
    const uint64_t last = (n & 63) ? (1ull << (n & 63)) - 1ull : ~0ull;
    for (int w = tid; w < nw; w += 64)
        for (int m = 0; m < ns; ++m)
            if (flag[m]) {
                const uint64_t x = ~out[(int64_t)m * nw + w];
                out[(int64_t)m * nw + w] = w == nw - 1 ? x & last : x;
            }
}

__device__ __forceinline__ int block_sum_256(int x, int *red) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) x += __shfl_xor(x, o, 64);
    __syncthreads();  // red is free again
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// support[m] = (ok replicates whose tree holds reference split m) / n_ok; block 0 writes n_ok
__global__ void __launch_bounds__(256)
    k_boot_support(int n, int nw, int n_rep, const uint64_t *__restrict__ ref,
                   const uint64_t *__restrict__ bits, const int32_t *__restrict__ ok,
                   double *__restrict__ support, int32_t *__restrict__ n_ok) {
    __shared__ int red[4];
    const int tid = (int)threadIdx.x, ns = n - 3, m = (int)blockIdx.x;
    int nok = 0, cnt = 0;
    for (int r = tid; r < n_rep; r += 256) nok += ok ? (ok[r] != 0) : 1;
    if (m < ns) {
        const uint64_t *want = ref + (int64_t)m * nw;
        const int64_t all = (int64_t)n_rep * ns;
        for (int64_t e = tid; e < all; e += 256) {
            const int64_t r = e / ns;
            if (ok && !ok[r]) continue;
            const uint64_t *have = bits + e * nw;
            bool same = true;
            for (int w = 0; w < nw && same; ++w) same = have[w] == want[w];
            cnt += same ? 1 : 0;
        }
    }
    nok = block_sum_256(nok, red);
    cnt = block_sum_256(cnt, red);
    if (tid == 0) {
        if (m < ns) support[m] = (double)cnt / (double)nok;
        if (m == 0) *n_ok = nok;
    }
}

// ---- host side ---------------------------------------------------------------------------

// per-device buffers of the bootstrap calls (DevState: pu_service.h)
struct BootState : DevState {
    DevBuf<uint32_t> prefix, slabs;
    DevBuf<int64_t> total;
    PairList pairs;
    DevBuf<double> counts;
    DevBuf<uint64_t> bits;
    ChunkProfile prof;
};
BootState g_boot[64];

// N of host weights (NULL: n_sites), or an error: a weight that is negative, non-integer or
// non-finite, or N outside [1, 2^31 - 1]
int host_total(const char *fn, const double *w, int64_t S, int64_t *N) {
    int64_t acc = 0;
    if (!w) acc = S;
    else
        for (int64_t s = 0; s < S; ++s) {
            const double x = w[s];
            if (!(x >= 0.0) || !(x <= (double)kMaxN) || x != floor(x))
                return set_err(nullptr, PU_E_ARG, "%s: site weight %lld = %g is not an integer in "
                               "[0, 2^31 - 1]", fn, (long long)s, x);
            acc += (int64_t)x;
            if (acc > kMaxN) break;
        }
    if (acc < 1 || acc > kMaxN)
        return set_err(nullptr, PU_E_ARG, "%s: the weights sum to %s, outside [1, 2^31 - 1]", fn,
                       acc < 1 ? "0" : "more than 2^31 - 1");
    *N = acc;
    return PU_OK;
}

int check_reps(const char *fn, int64_t first_rep, int n_rep, int64_t n_sites) {
    if (n_rep < 1) return set_err(nullptr, PU_E_ARG, "%s: n_rep = %d", fn, n_rep);
    if (first_rep < 0 || first_rep + n_rep > ((int64_t)1 << 32))
        return set_err(nullptr, PU_E_ARG, "%s: replicates %lld .. %lld are outside [0, 2^32)", fn,
                       (long long)first_rep, (long long)(first_rep + n_rep - 1));
    if (n_sites < 1) return set_err(nullptr, PU_E_ARG, "%s: n_sites = %lld", fn, (long long)n_sites);
    return PU_OK;
}

// W of n_rep replicates queued on st; N_host: N when the host knows it (unit weights, host
// forms), else 0; n_draw columns per row (0: N), or d_n_draws [n_rep] of them (device), n_draw
// then only sizing the grid
int run_weights(int device, hipStream_t st, uint64_t seed, int64_t first_rep, int n_rep,
                int64_t S, const double *d_w, int64_t N_host, uint32_t *d_W, int64_t ldw,
                int64_t n_draw = 0, const int64_t *d_n_draws = nullptr) {
    BootState &B = g_boot[device];
    StateScope scope(B, st);
    int rc;
    if ((rc = scope.rc)) return rc;
    HIPCHK(nullptr, hipMemset2DAsync(d_W, (size_t)ldw * 4, 0, (size_t)S * 4, (size_t)n_rep, st));
    WeightArgs a;
    a.seed = seed;
    a.first_rep = (uint32_t)first_rep;
    a.n_rep = n_rep;
    a.S = S;
    a.prefix = nullptr;
    a.total = nullptr;
    a.W = d_W;
    a.ldw = ldw;
    a.n_draw = n_draw;
    a.n_draws = d_n_draws;
    if (d_w) {
        if ((rc = B.prefix.reserve((size_t)S))) return rc;
        if ((rc = B.total.reserve(1))) return rc;
        hipLaunchKernelGGL(k_boot_prefix, dim3(1), dim3(kPT), 0, st, d_w, S, B.prefix.p, B.total.p);
        HIPCHK(nullptr, hipGetLastError());
        a.prefix = B.prefix.p;
        a.total = B.total.p;
    }
    const int64_t cols = std::max(N_host > 0 ? N_host : S, n_draw);
    const dim3 grid((unsigned)std::min<int64_t>(1024, (cols + 255) / 256),
                    (unsigned)std::min(n_rep, 64));
    hipLaunchKernelGGL(k_boot_weights, grid, dim3(256), 0, st, a);
    HIPCHK(nullptr, hipGetLastError());
    return PU_OK;
}

// a replicate's W must itself be a weight vector of the rule: its sum within [1, 2^31 - 1]
int check_W(const char *fn, const uint32_t *W, int n_rep, int64_t S) {
    for (int r = 0; r < n_rep; ++r) {
        uint64_t acc = 0;
        for (int64_t s = 0; s < S; ++s) acc += W[(int64_t)r * S + s];
        if (acc < 1 || acc > (uint64_t)kMaxN)
            return set_err(nullptr, PU_E_ARG, "%s: the weights of replicate %d sum to %llu, "
                           "outside [1, 2^31 - 1]", fn, r, (unsigned long long)acc);
    }
    return PU_OK;
}

struct Opt {
    double lo, hi, tol;
    int max_iter;
};

// the counts of every replicate and pair, chunk by chunk, queued on st: then -- with a model --
// k_pair_newton on them into d_out5 [n_rep][n_pairs][5], or -- without -- copied to counts_host
int run_counts(int device, hipStream_t st, const Shape &s, const uint8_t *d_codes, int64_t ld,
               const uint32_t *d_W, int64_t ldw, const PairModel *pm, const Opt *o, double *d_out5,
               double *counts_host) {
    BootState &B = g_boot[device];
    StateScope scope(B, st);
    int rc;
    if ((rc = scope.rc)) return rc;
    const int n = s.n_codes, nb = n * n;
    if ((rc = B.pairs.upload(st, s.n_taxa, s.n_pairs, s.pairs))) return rc;
    // the tile: as many replicates as the call has, up to 64, while one pair's bins fit
    int T = 64;
    while (T > kMinTile && (count_lds(n, 1, T) > kLdsCap || T / 2 >= s.n_rep)) T >>= 1;
    int P = kMaxWaves;
    while (P > 1 && count_lds(n, P, T) > kLdsCap) --P;
    if (count_lds(n, P, T) > kLdsCap)
        return set_err(nullptr, PU_E_STATE, "pu_boot: no tile of %d codes fits the LDS", n);
    // segments: only as many as it takes to fill the device; the sums are integers, so the
    // counts do not depend on them
    const int64_t groups = (s.n_pairs + P - 1) / P * ((s.n_rep + T - 1) / T);
    int64_t n_seg = std::min<int64_t>({(int64_t)kMaxSeg, (1024 + groups - 1) / groups,
                                       std::max<int64_t>(1, s.n_sites / (2 * kCH))});
    const int64_t seg = ((s.n_sites + n_seg - 1) / n_seg + kCH - 1) / kCH * kCH;
    n_seg = (s.n_sites + seg - 1) / seg;
    // the chunk: whole tiles of replicates times all pairs where that fits, else one tile times
    // as many pairs as fit (PU_DIST_CHUNK caps the pairs, as in the pair calls, and
    // PU_BOOT_REP_CHUNK the replicates; no result depends on either)
    const size_t per = (size_t)nb * (8 + (n_seg > 1 ? 4 * (size_t)n_seg : 0));
    const int64_t room = std::max<int64_t>(1, (int64_t)(kBootWsBytes / per));
    int64_t pc = env_cap("PU_DIST_CHUNK", s.n_pairs), rc_n;
    if (room >= (int64_t)T * pc) rc_n = std::min<int64_t>(s.n_rep, room / pc / T * T);
    else {
        rc_n = std::min<int64_t>(s.n_rep, T);
        pc = std::max<int64_t>(1, std::min(pc, room / rc_n));
    }
    rc_n = env_cap("PU_BOOT_REP_CHUNK", rc_n);
    if ((rc = B.counts.reserve((size_t)rc_n * pc * nb))) return rc;
    if (n_seg > 1 && (rc = B.slabs.reserve((size_t)n_seg * rc_n * pc * nb))) return rc;
    if ((rc = B.prof.reserve((s.n_rep + rc_n - 1) / rc_n * ((s.n_pairs + pc - 1) / pc)))) return rc;
    for (int64_t r0 = 0; r0 < s.n_rep; r0 += rc_n) {
        const int64_t nr = std::min<int64_t>(rc_n, s.n_rep - r0);
        for (int64_t p0 = 0; p0 < s.n_pairs; p0 += pc) {
            const int64_t np = std::min(pc, s.n_pairs - p0);
            if ((rc = B.prof.mark(0, st))) return rc;
            BootCountArgs a;
            a.codes = d_codes;
            a.ld = ld;
            a.S = s.n_sites;
            a.W = d_W + r0 * ldw;
            a.ldw = ldw;
            a.n_rep = (int)nr;
            a.pairs = B.pairs.d.p + 2 * p0;
            a.n_pairs = np;
            a.n_codes = n;
            a.P = P;
            a.T = T;
            a.seg = seg;
            a.out = B.counts.p;
            a.slabs = n_seg > 1 ? B.slabs.p : nullptr;
            const dim3 grid((unsigned)((np + P - 1) / P), (unsigned)((nr + T - 1) / T),
                            (unsigned)n_seg);
            if (grid.y > 65535u)
                return set_err(nullptr, PU_E_STATE, "pu_boot: %u replicate tiles in one chunk",
                               grid.y);
            hipLaunchKernelGGL(k_boot_pair_counts, grid, dim3(64 * P), count_lds(n, P, T), st, a);
            HIPCHK(nullptr, hipGetLastError());
            const size_t ne = (size_t)nr * np * nb;
            if (n_seg > 1) {
                hipLaunchKernelGGL(k_boot_merge, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0,
                                   st, B.slabs.p, (int)n_seg, ne, B.counts.p);
                HIPCHK(nullptr, hipGetLastError());
            }
            if ((rc = B.prof.mark(1, st))) return rc;
            if (pm) {
                if ((rc = pair_newton_device(device, st, *pm, o->lo, o->hi, o->tol, o->max_iter,
                                             B.counts.p, nr, np,
                                             d_out5 + 5 * (r0 * s.n_pairs + p0), s.n_pairs)))
                    return rc;
            } else if (np == s.n_pairs) {
                HIPCHK(nullptr, hipMemcpyAsync(counts_host + (size_t)r0 * s.n_pairs * nb, B.counts.p,
                                               ne * 8, hipMemcpyDeviceToHost, st));
            } else {
                for (int64_t r = 0; r < nr; ++r)
                    HIPCHK(nullptr, hipMemcpyAsync(
                                        counts_host + ((size_t)(r0 + r) * s.n_pairs + p0) * nb,
                                        B.counts.p + (size_t)r * np * nb, (size_t)np * nb * 8,
                                        hipMemcpyDeviceToHost, st));
            }
            if ((rc = B.prof.mark(2, st))) return rc;
        }
    }
    return PU_OK;
}

int check_support(const char *fn, int n, int n_rep, const void *ref_joins, const void *ref_root,
                  const void *joins, const void *roots, const void *support, const void *n_ok) {
    if (!ref_joins || !ref_root || !joins || !roots || !support || !n_ok)
        return set_err(nullptr, PU_E_ARG, "%s: null buffer", fn);
    if (n < 3 || n > PU_NJ_MAX_N)
        return set_err(nullptr, PU_E_ARG, "%s: n = %d is outside [3, %d]", fn, n, PU_NJ_MAX_N);
    if (n_rep < 1) return set_err(nullptr, PU_E_ARG, "%s: n_rep = %d", fn, n_rep);
    return PU_OK;
}

// join form: the children of cluster n + m are distinct live clusters below n + m
int check_joins(const char *fn, const char *what, int64_t tree, int n, const int32_t *jo) {
    std::vector<char> used((size_t)2 * n, 0);
    for (int m = 0; m < n - 2; ++m)
        for (int side = 0; side < 2; ++side) {
            const int c = jo[2 * m + side];
            if (c < 0 || c >= n + m || used[c])
                return set_err(nullptr, PU_E_ARG, "%s: %s tree %lld join %d: cluster %d is not "
                               "live", fn, what, (long long)tree, m, c);
            used[c] = 1;
        }
    return PU_OK;
}

int run_support(int device, hipStream_t st, int n, int n_rep, const int32_t *d_ref_joins,
                const int32_t *d_joins, const int32_t *d_ok, double *d_support, int32_t *d_n_ok) {
    BootState &B = g_boot[device];
    StateScope scope(B, st);
    int rc;
    if ((rc = scope.rc)) return rc;
    const int ns = n - 3, nw = (n + 63) / 64;
    if ((rc = B.bits.reserve((size_t)(1 + n_rep) * std::max(ns, 1) * nw))) return rc;
    uint64_t *ref = B.bits.p, *bits = ref + (size_t)std::max(ns, 1) * nw;
    if (ns > 0) {
        hipLaunchKernelGGL(k_boot_splits, dim3(1), dim3(64), (size_t)ns, st, d_ref_joins, n, nw,
                           ref);
        hipLaunchKernelGGL(k_boot_splits, dim3((unsigned)n_rep), dim3(64), (size_t)ns, st, d_joins,
                           n, nw, bits);
        HIPCHK(nullptr, hipGetLastError());
    }
    hipLaunchKernelGGL(k_boot_support, dim3((unsigned)std::max(ns, 1)), dim3(256), 0, st, n, nw,
                       n_rep, ref, bits, d_ok, d_support, d_n_ok);
    HIPCHK(nullptr, hipGetLastError());
    return PU_OK;
}

}  // namespace

extern "C" {

int pu_boot_weights_device(int device, void *stream, uint64_t seed, int64_t first_rep, int n_rep,
                           int64_t n_sites, const double *d_site_weights, uint32_t *d_w,
                           int64_t ldw) {
    const char *fn = "pu_boot_weights_device";
    int rc;
    if (!d_w) return set_err(nullptr, PU_E_ARG, "%s: null output", fn);
    if ((rc = check_reps(fn, first_rep, n_rep, n_sites))) return rc;
    if (ldw < n_sites)
        return set_err(nullptr, PU_E_ARG, "%s: row stride %lld below n_sites = %lld", fn,
                       (long long)ldw, (long long)n_sites);
    if (!d_site_weights && n_sites > kMaxN)
        return set_err(nullptr, PU_E_ARG, "%s: N = %lld is outside [1, 2^31 - 1]", fn,
                       (long long)n_sites);
    if ((rc = check_device(device))) return rc;
    DeviceGuard g(device);
    return run_weights(device, (hipStream_t)stream, seed, first_rep, n_rep, n_sites,
                       d_site_weights, d_site_weights ? 0 : n_sites, d_w, ldw);
}

int pu_boot_weights(int device, uint64_t seed, int64_t first_rep, int n_rep, int64_t n_sites,
                    const double *site_weights, uint32_t *w_out) {
    const char *fn = "pu_boot_weights";
    int rc;
    int64_t N = 0;
    if (!w_out) return set_err(nullptr, PU_E_ARG, "%s: null output", fn);
    if ((rc = check_reps(fn, first_rep, n_rep, n_sites))) return rc;
    if ((rc = host_total(fn, site_weights, n_sites, &N))) return rc;
    if ((rc = check_device(device))) return rc;
    DeviceGuard g(device);
    HostCall h(device);
    const size_t nW = (size_t)n_rep * n_sites;
    const double *d_sw = h.to_device(site_weights, (size_t)n_sites);
    uint32_t *d_W = h.alloc<uint32_t>(nW);
    if (!h.rc)
        h.rc = run_weights(device, h.st, seed, first_rep, n_rep, n_sites, d_sw, N, d_W, n_sites);
    h.to_host(w_out, d_W, nW);
    return h.finish(fn);
}

int pu_boot_weights_scaled_device(int device, void *stream, uint64_t seed, int64_t first_rep,
                                  int n_rep, int64_t n_sites, const double *d_site_weights,
                                  int64_t n_draw, const int64_t *d_n_draws, uint32_t *d_w,
                                  int64_t ldw) {
    const char *fn = "pu_boot_weights_scaled_device";
    int rc;
    if (!d_w) return set_err(nullptr, PU_E_ARG, "%s: null output", fn);
    if ((rc = check_reps(fn, first_rep, n_rep, n_sites))) return rc;
    if (ldw < n_sites)
        return set_err(nullptr, PU_E_ARG, "%s: row stride %lld below n_sites = %lld", fn,
                       (long long)ldw, (long long)n_sites);
    if (!d_site_weights && n_sites > kMaxN)
        return set_err(nullptr, PU_E_ARG, "%s: N = %lld is outside [1, 2^31 - 1]", fn,
                       (long long)n_sites);
    if (!d_n_draws && (n_draw < 1 || n_draw > kMaxN))
        return set_err(nullptr, PU_E_ARG, "%s: n_draw = %lld is outside [1, 2^31 - 1]", fn,
                       (long long)n_draw);
    if ((rc = check_device(device))) return rc;
    DeviceGuard g(device);
    return run_weights(device, (hipStream_t)stream, seed, first_rep, n_rep, n_sites,
                       d_site_weights, d_site_weights ? 0 : n_sites, d_w, ldw,
                       std::max<int64_t>(n_draw, 0), d_n_draws);
}

int pu_boot_weights_scaled(int device, uint64_t seed, int64_t first_rep, int n_rep,
                           int64_t n_sites, const double *site_weights, int64_t n_draw,
                           const int64_t *n_draws, uint32_t *w_out) {
    const char *fn = "pu_boot_weights_scaled";
    int rc;
    int64_t N = 0, most = n_draw;
    if (!w_out) return set_err(nullptr, PU_E_ARG, "%s: null output", fn);
    if ((rc = check_reps(fn, first_rep, n_rep, n_sites))) return rc;
    if ((rc = host_total(fn, site_weights, n_sites, &N))) return rc;
    for (int r = 0; r < (n_draws ? n_rep : 0); ++r) {
        if (n_draws[r] < 1 || n_draws[r] > kMaxN)
            return set_err(nullptr, PU_E_ARG, "%s: n_draws[%d] = %lld is outside [1, 2^31 - 1]",
                           fn, r, (long long)n_draws[r]);
        most = r ? std::max(most, n_draws[r]) : n_draws[r];
    }
    if (!n_draws && (n_draw < 1 || n_draw > kMaxN))
        return set_err(nullptr, PU_E_ARG, "%s: n_draw = %lld is outside [1, 2^31 - 1]", fn,
                       (long long)n_draw);
    if ((rc = check_device(device))) return rc;
    DeviceGuard g(device);
    HostCall h(device);
    const size_t nW = (size_t)n_rep * n_sites;
    const double *d_sw = h.to_device(site_weights, (size_t)n_sites);
    const int64_t *d_nd = h.to_device(n_draws, (size_t)n_rep);
    uint32_t *d_W = h.alloc<uint32_t>(nW);
    // the grid is sized for the longest row; its stride loop covers any other
    if (!h.rc)
        h.rc = run_weights(device, h.st, seed, first_rep, n_rep, n_sites, d_sw, N, d_W, n_sites,
                           most, d_nd);
    h.to_host(w_out, d_W, nW);
    return h.finish(fn);
}

int pu_boot_pair_counts(int device, const uint8_t *codes, int n_taxa, int64_t n_sites, int n_codes,
                        const uint32_t *W, int n_rep, int64_t n_pairs, const int32_t *pairs,
                        double *counts_out) {
    const char *fn = "pu_boot_pair_counts";
    const Shape s{n_taxa, n_codes, n_sites, n_pairs, pairs, n_rep};
    int rc;
    if ((rc = check_shape(fn, s, !codes || !W))) return rc;
    if (!counts_out) return set_err(nullptr, PU_E_ARG, "%s: null output", fn);
    if ((rc = check_codes(fn, codes, n_taxa, n_sites, n_codes))) return rc;
    if ((rc = check_W(fn, W, n_rep, n_sites))) return rc;
    if ((rc = check_device(device))) return rc;
    DeviceGuard g(device);
    HostCall h(device);
    const uint8_t *d_codes = h.to_device(codes, (size_t)n_taxa * n_sites);
    const uint32_t *d_W = h.to_device(W, (size_t)n_rep * n_sites);
    if (!h.rc)
        h.rc = run_counts(device, h.st, s, d_codes, n_sites, d_W, n_sites, nullptr, nullptr,
                          nullptr, counts_out);
    return h.finish(fn);
}

int pu_boot_distances_device(int device, void *stream, int n_states, int n_cat, int n_codes,
                             const double *code_table, const double *evecs, const double *evals,
                             const double *ivecs, const double *freqs, const double *rates,
                             const double *cat_weights, const uint8_t *d_codes, int64_t ld,
                             int n_taxa, int64_t n_sites, const uint32_t *d_W, int64_t ldw,
                             int n_rep, int64_t n_pairs, const int32_t *pairs, double lo, double hi,
                             double tol, int max_iter, double *d_out5, double *d_D, int64_t ldd) {
    const char *fn = "pu_boot_distances_device";
    const Shape s{n_taxa, n_codes, n_sites, n_pairs, pairs, n_rep};
    const PairModel pm{n_states, n_cat, n_codes, code_table, evecs, evals, ivecs, freqs, rates,
                       cat_weights};
    const Opt o{lo, hi, tol, max_iter};
    int rc;
    if ((rc = check_shape(fn, s, !d_codes || !d_W))) return rc;
    if (!d_out5) return set_err(nullptr, PU_E_ARG, "%s: null output", fn);
    if (ld < n_sites || ldw < n_sites)
        return set_err(nullptr, PU_E_ARG, "%s: row strides %lld, %lld below n_sites = %lld", fn,
                       (long long)ld, (long long)ldw, (long long)n_sites);
    if (d_D && (pairs || ldd < n_taxa || n_taxa > PU_NJ_MAX_N))
        return set_err(nullptr, PU_E_ARG, "%s: the matrices need all pairs (no list), a row stride "
                       ">= n_taxa = %d (%lld) and n_taxa <= %d", fn, n_taxa, (long long)ldd,
                       PU_NJ_MAX_N);
    if ((rc = pair_check_model(fn, pm, lo, hi, tol, max_iter))) return rc;
    if ((rc = check_device(device))) return rc;
    DeviceGuard g(device);
    hipStream_t st = (hipStream_t)stream;
    if ((rc = run_counts(device, st, s, d_codes, ld, d_W, ldw, &pm, &o, d_out5, nullptr))) return rc;
    if (d_D) return pair_matrix_all(st, n_rep, n_taxa, d_out5, d_D, ldd);
    return PU_OK;
}

int pu_boot_distances(int device, int n_states, int n_cat, int n_codes, const double *code_table,
                      const double *evecs, const double *evals, const double *ivecs,
                      const double *freqs, const double *rates, const double *cat_weights,
                      const uint8_t *codes, int n_taxa, int64_t n_sites, const uint32_t *W,
                      int n_rep, int64_t n_pairs, const int32_t *pairs, double lo, double hi,
                      double tol, int max_iter, double *out5_out) {
    const char *fn = "pu_boot_distances";
    const Shape s{n_taxa, n_codes, n_sites, n_pairs, pairs, n_rep};
    const PairModel pm{n_states, n_cat, n_codes, code_table, evecs, evals, ivecs, freqs, rates,
                       cat_weights};
    const Opt o{lo, hi, tol, max_iter};
    int rc;
    if ((rc = check_shape(fn, s, !codes || !W))) return rc;
    if (!out5_out) return set_err(nullptr, PU_E_ARG, "%s: null output", fn);
    if ((rc = pair_check_model(fn, pm, lo, hi, tol, max_iter))) return rc;
    if ((rc = check_codes(fn, codes, n_taxa, n_sites, n_codes))) return rc;
    if ((rc = check_W(fn, W, n_rep, n_sites))) return rc;
    if ((rc = check_device(device))) return rc;
    DeviceGuard g(device);
    HostCall h(device);
    const size_t n_out = 5 * (size_t)n_rep * n_pairs;
    const uint8_t *d_codes = h.to_device(codes, (size_t)n_taxa * n_sites);
    const uint32_t *d_W = h.to_device(W, (size_t)n_rep * n_sites);
    double *d_out = h.alloc<double>(n_out);
    if (!h.rc)
        h.rc = run_counts(device, h.st, s, d_codes, n_sites, d_W, n_sites, &pm, &o, d_out, nullptr);
    h.to_host(out5_out, d_out, n_out);
    return h.finish(fn);
}

int pu_split_support_device(int device, void *stream, int n, int n_rep, const int32_t *d_ref_joins,
                            const int32_t *d_ref_root, const int32_t *d_joins,
                            const int32_t *d_roots, const int32_t *d_ok, double *d_support,
                            int32_t *d_n_ok) {
    const char *fn = "pu_split_support_device";
    int rc;
    if ((rc = check_support(fn, n, n_rep, d_ref_joins, d_ref_root, d_joins, d_roots, d_support,
                            d_n_ok)))
        return rc;
    if ((rc = check_device(device))) return rc;
    DeviceGuard g(device);
    return run_support(device, (hipStream_t)stream, n, n_rep, d_ref_joins, d_joins, d_ok,
                       d_support, d_n_ok);
}

int pu_split_support(int device, int n, int n_rep, const int32_t *ref_joins,
                     const int32_t *ref_root, const int32_t *joins, const int32_t *roots,
                     const int32_t *ok, double *support_out, int32_t *n_ok_out) {
    const char *fn = "pu_split_support";
    int rc;
    if ((rc = check_support(fn, n, n_rep, ref_joins, ref_root, joins, roots, support_out,
                            n_ok_out)))
        return rc;
    if ((rc = check_joins(fn, "reference", 0, n, ref_joins))) return rc;
    for (int64_t r = 0; r < n_rep; ++r)
        if ((rc = check_joins(fn, "replicate", r, n, joins + r * (n - 2) * 2))) return rc;
    if ((rc = check_device(device))) return rc;
    DeviceGuard g(device);
    HostCall h(device);
    const size_t nj = (size_t)(n - 2) * 2;
    const int32_t *d_ref = h.to_device(ref_joins, nj), *d_jo = h.to_device(joins, nj * n_rep);
    const int32_t *d_ok = h.to_device(ok, (size_t)n_rep);
    double *d_sup = h.alloc<double>((size_t)std::max(n - 3, 1));
    int32_t *d_nok = h.alloc<int32_t>(1);
    if (!h.rc) h.rc = run_support(device, h.st, n, n_rep, d_ref, d_jo, d_ok, d_sup, d_nok);
    h.to_host(support_out, d_sup, (size_t)(n - 3));
    h.to_host(n_ok_out, d_nok, 1);
    return h.finish(fn);
}

int pu_bootstrap_nj(int device, int method, int n_states, int n_cat, int n_codes,
                    const double *code_table, const double *evecs, const double *evals,
                    const double *ivecs, const double *freqs, const double *rates,
                    const double *cat_weights, const uint8_t *codes, int n_taxa, int64_t n_sites,
                    const double *site_weights, uint64_t seed, int n_rep, double lo, double hi,
                    double tol, int max_iter, int32_t *ref_joins_out, double *ref_lens_out,
                    int32_t *ref_root_out, double *ref_root_len_out, double *support_out,
                    int32_t *n_ok_out, int32_t *rep_joins_out, int32_t *rep_roots_out) {
    const char *fn = "pu_bootstrap_nj";
    const int n = n_taxa;
    const PairModel pm{n_states, n_cat, n_codes, code_table, evecs, evals, ivecs, freqs, rates,
                       cat_weights};
    int rc;
    int64_t N = 0;
    if (!codes || !ref_joins_out || !ref_lens_out || !ref_root_out || !ref_root_len_out ||
        !support_out || !n_ok_out)
        return set_err(nullptr, PU_E_ARG, "%s: null buffer", fn);
    if (method != 0 && method != 1)
        return set_err(nullptr, PU_E_ARG, "%s: method = %d (0 NJ, 1 BIONJ)", fn, method);
    if (n < 3 || n > PU_NJ_MAX_N)
        return set_err(nullptr, PU_E_ARG, "%s: n_taxa = %d is outside [3, %d]", fn, n,
                       PU_NJ_MAX_N);
    if ((rc = check_reps(fn, 0, n_rep, n_sites))) return rc;
    if ((rc = pair_check_model(fn, pm, lo, hi, tol, max_iter))) return rc;
    if ((rc = host_total(fn, site_weights, n_sites, &N))) return rc;
    if ((rc = check_codes(fn, codes, n, n_sites, n_codes))) return rc;
    if ((rc = check_device(device))) return rc;
    DeviceGuard g(device);
    HostCall h(device);
    hipStream_t st = h.st;
    const int64_t np = (int64_t)n * (n - 1) / 2;
    const size_t nj = (size_t)(n - 2) * 2, nn = (size_t)n * n, R = (size_t)n_rep;
    const uint8_t *d_codes = h.to_device(codes, (size_t)n * n_sites);
    const double *d_sw = h.to_device(site_weights, (size_t)n_sites);
    uint32_t *d_W = h.alloc<uint32_t>(R * n_sites);
    const size_t n_f = (1 + R) * (5 * (size_t)np + nn + nj + 1) + (size_t)n;
    double *d_f = h.alloc<double>(n_f);                            // every fp64 buffer of the call
    int32_t *d_i = h.alloc<int32_t>((1 + R) * (nj + 2) + R + 1);  // every int32 buffer
    if (!h.rc) {
        int &rc = h.rc;  // the chain below stops at the call's first error
        double *o5_ref = d_f, *o5 = o5_ref + 5 * np, *D_ref = o5 + 5 * np * R, *D = D_ref + nn;
        double *len_ref = D + nn * R, *len = len_ref + nj, *rl_ref = len + nj * R, *rl = rl_ref + 1;
        double *sup = rl + R;
        int32_t *jo_ref = d_i, *jo = jo_ref + nj, *ro_ref = jo + nj * R, *ro = ro_ref + 2;
        int32_t *ok = ro + 2 * R, *nok = ok + R;
        // the reference tree, from the weights as they are
        rc = pu_pair_distances_device(device, st, n_states, n_cat, n_codes, code_table, evecs,
                                      evals, ivecs, freqs, rates, cat_weights, d_codes, n_sites, n,
                                      n_sites, d_sw, np, nullptr, nullptr, lo, hi, tol, max_iter,
                                      o5_ref);
        if (!rc) rc = pu_pair_matrix_device(device, st, n, np, nullptr, o5_ref, D_ref, n);
        if (!rc) rc = pu_nj_device(device, st, method, 1, n, D_ref, n, jo_ref, len_ref, ro_ref,
                                   rl_ref, nullptr);
        // the replicates
        if (!rc) rc = run_weights(device, st, seed, 0, n_rep, n_sites, d_sw, N, d_W, n_sites);
        if (!rc) rc = pu_boot_distances_device(device, st, n_states, n_cat, n_codes, code_table,
                                               evecs, evals, ivecs, freqs, rates, cat_weights,
                                               d_codes, n_sites, n, n_sites, d_W, n_sites, n_rep,
                                               np, nullptr, lo, hi, tol, max_iter, o5, D, n);
        if (!rc) {
            hipLaunchKernelGGL(k_boot_ok, dim3((unsigned)n_rep), dim3(256), 0, st, n, D, (int64_t)n,
                               ok);
            if (hipGetLastError() != hipSuccess)
                rc = set_err(nullptr, PU_E_HIP, "%s: k_boot_ok launch failed", fn);
        }
        if (!rc) rc = pu_nj_device(device, st, method, n_rep, n, D, n, jo, len, ro, rl, nullptr);
        if (!rc) rc = run_support(device, st, n, n_rep, jo_ref, jo, ok, sup, nok);
        h.to_host(ref_joins_out, jo_ref, nj);
        h.to_host(ref_lens_out, len_ref, nj);
        h.to_host(ref_root_out, ro_ref, 2);
        h.to_host(ref_root_len_out, rl_ref, 1);
        h.to_host(support_out, sup, (size_t)(n - 3));
        h.to_host(n_ok_out, nok, 1);
        if (rep_joins_out) h.to_host(rep_joins_out, jo, nj * R);
        if (rep_roots_out) h.to_host(rep_roots_out, ro, 2 * R);
    }
    return h.finish(fn);
}

int pu_boot_profile(int device, int on) { return profile_set(g_boot, device, on); }

int pu_boot_kernel_ms(int device, double *counts_ms, double *newton_ms) {
    return profile_ms("pu_boot_kernel_ms", g_boot, device, counts_ms, newton_ms);
}

}  // extern "C"
