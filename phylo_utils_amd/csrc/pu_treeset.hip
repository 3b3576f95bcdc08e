// pu_treeset.hip -- sets of trees compared on the GPU: the table of their distinct splits, a
// split id per edge of every tree, the number of trees that hold each split and the
// Robinson-Foulds distances between the trees; and the C ABI of it (pu_treeset_compare,
// pu_treeset_profile, pu_treeset_kernel_ms).
//
// The reference has no tree comparison; the rule is this project's own (normative;
// tests/treeset_reference.py restates it).  T trees over the same n tips, tips 0..n-1, internal
// nodes n..2n-3.  The split of an edge is the set of tips on the side of it that does not hold
// tip 0, a bitset of nw = ceil(n / 64) words, tip i at bit i & 63 of word i >> 6.  A split of 1
// or n - 1 tips (a pendant edge) is trivial and has no id; a binary tree has exactly n - 3
// others, one per internal edge.  U is the table of the distinct non-trivial splits of all
// trees in ascending order as unsigned integers of 64 nw bits (word nw - 1 the most
// significant); the id of a split is its index in U; count[u] is the number of trees that hold
// split u; RF(a, b) = 2 (n - 3) - 2 |ids(a) & ids(b)|.  Two splits are equal only if all nw
// words are: nothing here hashes.
//
// The host checks the trees and brings every form to one device form (`cj`, below); the rest
// runs on the device.  The argument rules, the form conversion and the device stages are also
// offered to pu_treedist.hip (pu_treeset_stages.h), which reads the id arrays they leave.
//
//   device form       cj [T][n-2][2]: op m of a tree makes cluster n + m from two children, a tip
//                     (< n) or an earlier cluster n + m' (m' < m) -- pu_nj's join form, to which
//                     an op list comes by renaming every parent to n + (its op index).  y [T]:
//                     the end of the root edge that is not the last op's parent, in the same
//                     naming.
//   edge -> cluster   The edges of a tree in op order are 2 m + side = (child, parent of op m)
//                     and, last, the root edge.  In a post-order nothing is made after the last
//                     op, so its parent X has no parent: X is one end of the root edge, y the
//                     other.  Hence edge 2 m + side is internal iff its child c >= n, and its
//                     split is cluster c - n; the root edge is internal iff y >= n, and its split
//                     is cluster y - n (the clusters of X and y are complements: one split).  A
//                     cluster that is a child or y is never the last one, so the splits of the
//                     n - 3 internal edges are exactly clusters 0..n-4, each once, and cluster
//                     n - 3 (X) is never built.
//   k_ts_splits       bits [T][n-3][nw].  A thread owns one word of one tree and ORs the
//                     children's words in op order, reading back only words it wrote itself.
//                     Kept: one tree per 64-lane workgroup, as k_boot_splits, but with the op
//                     list and the clusters in LDS while they fit the 160 KiB (n <= 1088; else a
//                     workgroup of 64 or 128 threads, one per word, keeps the clusters in
//                     place in memory).
//                     Measured against it (PU_TREESET_GROUP=g, read at each call): g trees share
//                     the workgroup, up to 64 / (nw rounded up to a power of two), so that
//                     n <= 64 fills the wave with 64 trees -- slower at every shape timed (DESIGN
//                     4.27): the op chain is as long, its LDS reads now collide between trees,
//                     and 64 lanes stage and write out what 64 workgroups did.  Then the
//                     canonical side: a cluster with tip 0 is complemented and the last word
//                     masked to n bits.
//   ids               perm = 0..N-1 (N = T (n - 3)) sorted by rocPRIM's stable 64-bit radix sort,
//                     one pass per word from word 0 (least significant) upward, the keys gathered
//                     through perm before each pass (k_ts_gather): an exact lexicographic sort.
//                     k_ts_flag marks a position whose nw words differ from its predecessor's,
//                     rocPRIM's inclusive scan of the flags numbers the splits, k_ts_uniq writes
//                     id per (tree, cluster), the first position of every id and U's rows,
//                     k_ts_count the counts (next first position - own: a tree holds a split
//                     once), k_ts_edge_ids the ids per edge through edge -> cluster.
//   k_ts_sort_lists   one workgroup per tree: its n - 3 ids sorted in LDS (bitonic, padded with
//                     INT32_MAX to a power of two).
//   k_ts_rf           a workgroup takes a tile of 16 row trees x 16 column trees, stages their 32
//                     sorted lists in LDS (odd stride) while they fit, and counts the
//                     intersection of every pair.  Kept: one lane per pair, a two-pointer merge
//                     (256 pairs = 256 lanes).  Measured against it: one wave per pair, the
//                     lanes binary-searching the row list's ids in the column list
//                     (PU_TREESET_RF=wave, read at each call; DESIGN 4.27 has both times).
//
// Memory.  The call is not chunked: bits, two key arrays, two permutations and five N-word
// arrays, N (8 nw + 44) bytes and rocPRIM's temporaries, are held at once; where they do not
// fit the call returns PU_E_NOMEM.
#include <hip/hip_runtime.h>

#include <limits.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <new>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "pu_ctx.h"
#include "pu_service.h"
#include "pu_treeform.h"
#include "pu_treeset_stages.h"

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "pu_treeset.hip: gfx950 only, as the other kernel files of this library"
#endif

using namespace pu;

namespace {

constexpr size_t kLdsCap = 160 * 1024;  // LDS one workgroup may have
constexpr int kTB = 256;
constexpr int kTile = 16;               // k_ts_rf: row trees and column trees of a tile

// ---- splits -----------------------------------------------------------------------------------

struct SplitArgs {
    const int32_t *cj;  // [T][n-2][2]
    int n, nw, T;
    int G, tpt;         // trees per workgroup, threads per tree
    int in_lds;         // the clusters of the G trees live in LDS
    uint64_t *bits;     // [T][n-3][nw]
};

__host__ inline size_t split_lds(int n, int nw, int G, bool in_lds) {
    const size_t ns = (size_t)(n - 3);
    return (in_lds ? (size_t)G * ns * nw * 8 : 0) + (size_t)G * ns * 8 + (((size_t)G * ns + 7) & ~(size_t)7);
}

__global__ void __launch_bounds__(kTB) k_ts_splits(SplitArgs a) {
    extern __shared__ uint64_t lds64[];
    const int tid = (int)threadIdx.x, nthr = (int)blockDim.x;
    const int n = a.n, nw = a.nw, ns = n - 3, G = a.G;
    const int64_t t0 = (int64_t)blockIdx.x * G;
    const int nt = (int)min((int64_t)G, (int64_t)a.T - t0);  // trees of this workgroup
    uint64_t *cl_lds = lds64;                                 // [G][ns][nw] (in_lds)
    int32_t *jl = reinterpret_cast<int32_t *>(lds64 + (a.in_lds ? (size_t)G * ns * nw : 0));
    uint8_t *flag = reinterpret_cast<uint8_t *>(jl + (size_t)G * ns * 2);  // [G][ns]
    // the first n - 3 ops of every tree (the last one's cluster is never needed)
    for (int i = tid; i < nt * ns * 2; i += nthr) {
        const int tt = i / (ns * 2), r = i - tt * ns * 2;
        jl[i] = a.cj[(t0 + tt) * (int64_t)(n - 2) * 2 + r];
    }
    __syncthreads();
    const int g = tid / a.tpt, w0 = tid - g * a.tpt;
    uint64_t *cl = nullptr;
    if (g < nt)
        cl = a.in_lds ? cl_lds + (size_t)g * ns * nw : a.bits + (t0 + g) * (int64_t)ns * nw;
    if (cl) {
        const int32_t *jo = jl + (size_t)g * ns * 2;
        for (int w = w0; w < nw; w += a.tpt)
            for (int m = 0; m < ns; ++m) {
                uint64_t x = 0;
#pragma unroll
                for (int side = 0; side < 2; ++side) {
                    const int c = jo[2 * m + side];
                    if (c < 0 || c >= n + m) continue;  // not the device form: nothing is read
                    if (c < n) {
                        if ((c >> 6) == w) x |= 1ull << (c & 63);
                    } else {
                        x |= cl[(int64_t)(c - n) * nw + w];  // written by this thread, earlier
                    }
                }
                cl[(int64_t)m * nw + w] = x;
            }
    }
    __syncthreads();
    // the canonical side: word 0 belongs to another thread, so the flags are taken first
    for (int i = tid; i < nt * ns; i += nthr) {
        const int tt = i / ns, m = i - tt * ns;
        const uint64_t *c0 = a.in_lds ? cl_lds + (size_t)tt * ns * nw
                                      : a.bits + (t0 + tt) * (int64_t)ns * nw;
        flag[i] = (uint8_t)(c0[(int64_t)m * nw] & 1ull);
    }
    __syncthreads();
    const uint64_t last = (n & 63) ? (1ull << (n & 63)) - 1ull : ~0ull;
    if (a.in_lds) {
        // the workgroup's trees are neighbours in bits: one coalesced sweep
        uint64_t *out = a.bits + t0 * (int64_t)ns * nw;
        const int64_t all = (int64_t)nt * ns * nw;
        for (int64_t e = tid; e < all; e += nthr) {
            const int w = (int)(e % nw);
            uint64_t x = cl_lds[e];
            if (flag[e / nw]) {
                x = ~x;
                if (w == nw - 1) x &= last;
            }
            out[e] = x;
        }
    } else if (cl) {
        for (int w = w0; w < nw; w += a.tpt)
            for (int m = 0; m < ns; ++m)
                if (flag[(size_t)g * ns + m]) {
                    const uint64_t x = ~cl[(int64_t)m * nw + w];
                    cl[(int64_t)m * nw + w] = w == nw - 1 ? x & last : x;
                }
    }
}

// ---- ids --------------------------------------------------------------------------------------

__global__ void __launch_bounds__(kTB) k_ts_iota(uint32_t *__restrict__ perm, int64_t N) {
    const int64_t i = (int64_t)blockIdx.x * kTB + threadIdx.x;
    if (i < N) perm[i] = (uint32_t)i;
}

__global__ void __launch_bounds__(kTB)
    k_ts_gather(const uint64_t *__restrict__ bits, const uint32_t *__restrict__ perm, int w, int nw,
                int64_t N, uint64_t *__restrict__ key) {
    const int64_t i = (int64_t)blockIdx.x * kTB + threadIdx.x;
    if (i < N) key[i] = bits[(int64_t)perm[i] * nw + w];
}

// flag[p] = the split at sorted position p differs from its predecessor's in some word
__global__ void __launch_bounds__(kTB)
    k_ts_flag(const uint64_t *__restrict__ bits, const uint32_t *__restrict__ perm, int nw,
              int64_t N, uint32_t *__restrict__ flag) {
    const int64_t p = (int64_t)blockIdx.x * kTB + threadIdx.x;
    if (p >= N) return;
    uint32_t f = 1u;
    if (p > 0) {
        const uint64_t *x = bits + (int64_t)perm[p] * nw, *y = bits + (int64_t)perm[p - 1] * nw;
        f = 0u;
        for (int w = 0; w < nw; ++w) f |= x[w] != y[w] ? 1u : 0u;
    }
    flag[p] = f;
}

// num = the inclusive scan of flag: id = num - 1 per (tree, cluster), the first sorted position
// of every id, U's rows (nullable) and U itself
__global__ void __launch_bounds__(kTB)
    k_ts_uniq(const uint64_t *__restrict__ bits, const uint32_t *__restrict__ perm,
              const uint32_t *__restrict__ flag, const uint32_t *__restrict__ num, int nw, int64_t N,
              int32_t *__restrict__ split_id, uint32_t *__restrict__ first,
              uint64_t *__restrict__ uniq_bits, int64_t *__restrict__ n_unique) {
    const int64_t p = (int64_t)blockIdx.x * kTB + threadIdx.x;
    if (p >= N) return;
    const uint32_t id = num[p] - 1u, src = perm[p];
    split_id[src] = (int32_t)id;
    if (flag[p]) {
        first[id] = (uint32_t)p;
        if (uniq_bits)
            for (int w = 0; w < nw; ++w) uniq_bits[(int64_t)id * nw + w] = bits[(int64_t)src * nw + w];
    }
    if (p == N - 1) *n_unique = (int64_t)num[p];
}

__global__ void __launch_bounds__(kTB)
    k_ts_count(const uint32_t *__restrict__ first, const int64_t *__restrict__ n_unique, int64_t N,
               int32_t *__restrict__ count) {
    const int64_t u = (int64_t)blockIdx.x * kTB + threadIdx.x, U = *n_unique;
    if (u >= U) return;
    const int64_t next = u + 1 < U ? (int64_t)first[u + 1] : N;
    count[u] = (int32_t)(next - (int64_t)first[u]);
}

// edge_ids [T][2n-3] through edge -> cluster; emap (nullable) [T][2n-3]: where the edge of op
// order k stands in the caller's own edge order
__global__ void __launch_bounds__(kTB)
    k_ts_edge_ids(const int32_t *__restrict__ cj, const int32_t *__restrict__ y,
                  const int32_t *__restrict__ emap, const int32_t *__restrict__ split_id, int n,
                  int64_t T, int32_t *__restrict__ edge_ids) {
    const int E = 2 * n - 3, ns = n - 3;
    const int64_t i = (int64_t)blockIdx.x * kTB + threadIdx.x;
    if (i >= T * E) return;
    const int64_t t = i / E;
    const int k = (int)(i - t * E);
    const int c = k < E - 1 ? cj[t * (int64_t)(n - 2) * 2 + k] : y[t];
    int32_t id = -1;
    if (c >= n && c - n < ns) id = split_id[t * ns + (c - n)];
    edge_ids[t * E + (emap ? emap[i] : k)] = id;
}

// sorted [T][n-3]: every tree's ids ascending; P = n - 3 rounded up to a power of two
__global__ void __launch_bounds__(kTB)
    k_ts_sort_lists(const int32_t *__restrict__ split_id, int ns, int P, int32_t *__restrict__ sorted) {
    extern __shared__ int32_t lds32[];
    const int tid = (int)threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * ns;
    for (int i = tid; i < P; i += kTB) lds32[i] = i < ns ? split_id[base + i] : INT_MAX;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += kTB) {
                const int l = i ^ j;
                if (l > i) {
                    const int32_t x = lds32[i], z = lds32[l];
                    const bool up = (i & k) == 0;
                    if ((x > z) == up) {
                        lds32[i] = z;
                        lds32[l] = x;
                    }
                }
            }
            __syncthreads();
        }
    for (int i = tid; i < ns; i += kTB) sorted[base + i] = lds32[i];
}

// ---- RF ---------------------------------------------------------------------------------------

struct RfArgs {
    const int32_t *sorted;  // [T][ns]
    int ns, T, n_rows;
    int stride;             // of a staged list in LDS (odd), or 0: the lists are read from memory
    int32_t *rf;            // [n_rows][T]
};

template <bool WAVE>
__global__ void __launch_bounds__(kTB) k_ts_rf(RfArgs a) {
    extern __shared__ int32_t lds32[];
    const int tid = (int)threadIdx.x, ns = a.ns;
    const int r0 = (int)blockIdx.y * kTile, c0 = (int)blockIdx.x * kTile;
    const int nr = min(kTile, a.n_rows - r0), nc = min(kTile, a.T - c0);
    if (a.stride) {  // lists 0..15: the rows, 16..31: the columns
        for (int i = tid; i < 2 * kTile * ns; i += kTB) {
            const int l = i / ns, k = i - l * ns;
            const int t = l < kTile ? r0 + l : c0 + l - kTile;
            const bool live = l < kTile ? l < nr : l - kTile < nc;
            if (live) lds32[(size_t)l * a.stride + k] = a.sorted[(int64_t)t * ns + k];
        }
        __syncthreads();
    }
    if (!WAVE) {
        const int i = tid / kTile, j = tid - i * kTile;
        if (i >= nr || j >= nc) return;
        const int32_t *A = a.stride ? lds32 + (size_t)i * a.stride : a.sorted + (int64_t)(r0 + i) * ns;
        const int32_t *B = a.stride ? lds32 + (size_t)(kTile + j) * a.stride
                                    : a.sorted + (int64_t)(c0 + j) * ns;
        int pa = 0, pb = 0, common = 0;
        while (pa < ns && pb < ns) {
            const int32_t x = A[pa], z = B[pb];
            common += x == z ? 1 : 0;
            pa += x <= z ? 1 : 0;
            pb += z <= x ? 1 : 0;
        }
        a.rf[(int64_t)(r0 + i) * a.T + c0 + j] = 2 * (ns - common);
    } else {
        const int lane = tid & 63, wv = tid >> 6;
        for (int q = wv; q < kTile * kTile; q += kTB / 64) {  // wave-uniform
            const int i = q / kTile, j = q - i * kTile;
            if (i >= nr || j >= nc) continue;
            const int32_t *A = a.stride ? lds32 + (size_t)i * a.stride
                                        : a.sorted + (int64_t)(r0 + i) * ns;
            const int32_t *B = a.stride ? lds32 + (size_t)(kTile + j) * a.stride
                                        : a.sorted + (int64_t)(c0 + j) * ns;
            int common = 0;
            for (int k = lane; k < ns; k += 64) {
                const int32_t x = A[k];
                int lo = 0, hi = ns;  // the first position of B with an id >= x
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (B[mid] < x) lo = mid + 1;
                    else hi = mid;
                }
                common += (lo < ns && B[lo] == x) ? 1 : 0;
            }
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) common += __shfl_xor(common, o, 64);
            if (lane == 0) a.rf[(int64_t)(r0 + i) * a.T + c0 + j] = 2 * (ns - common);
        }
    }
}

// ---- host side --------------------------------------------------------------------------------

// per-device buffers of the tree-set calls (DevState: pu_service.h)
struct TreesetState : DevState {
    DevBuf<uint64_t> bits, key_a, key_b;
    DevBuf<uint32_t> perm_a, perm_b, flag, num, first;
    DevBuf<int32_t> split_id, sorted;
    DevBuf<uint8_t> sort_tmp, scan_tmp;
    bool prof_on = false, have = false;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
};
TreesetState g_ts[64];

inline unsigned blocks(int64_t n) { return (unsigned)((n + kTB - 1) / kTB); }

int mark(TreesetState &S, int i, hipStream_t st) {
    if (!S.prof_on) return PU_OK;
    if (!S.ev[i]) HIPCHK(nullptr, hipEventCreate(&S.ev[i]));
    HIPCHK(nullptr, hipEventRecord(S.ev[i], st));
    if (i == 3) S.have = true;
    return PU_OK;
}

// everything on the device, queued on st; ids (nullable): pu_treeset_stages.h
int run_compare(int device, hipStream_t st, int n, int64_t T, const int32_t *d_cj,
                const int32_t *d_y, const int32_t *d_emap, int n_rows, const TreesetOut &o,
                TreesetIds *ids) {
    TreesetState &S = g_ts[device];
    if (ids) *ids = TreesetIds();
    StateScope scope(S, st);
    int rc;
    if ((rc = scope.rc)) return rc;
    const int ns = n - 3, nw = (n + 63) / 64, E = 2 * n - 3;
    const int64_t N = T * ns;
    S.have = false;
    if ((rc = mark(S, 0, st))) return rc;
    if (N == 0) {  // three tips: no split, every edge pendant, every distance 0
        HIPCHK(nullptr, hipMemsetAsync(o.edge_ids, 0xff, (size_t)T * E * 4, st));
        HIPCHK(nullptr, hipMemsetAsync(o.n_unique, 0, 8, st));
        if (o.rf && n_rows) HIPCHK(nullptr, hipMemsetAsync(o.rf, 0, (size_t)n_rows * T * 4, st));
        for (int i = 1; i < 4; ++i)
            if ((rc = mark(S, i, st))) return rc;
        return PU_OK;
    }
    // the workspace, all of it before the first launch: the call is not chunked
    size_t sort_need = 0, scan_need = 0;
    HIPCHK(nullptr, rocprim::radix_sort_pairs(nullptr, sort_need, (const uint64_t *)nullptr,
                                              (uint64_t *)nullptr, (const uint32_t *)nullptr,
                                              (uint32_t *)nullptr, (size_t)N, 0u, 64u, st));
    HIPCHK(nullptr, rocprim::inclusive_scan(nullptr, scan_need, (uint32_t *)nullptr,
                                            (uint32_t *)nullptr, (size_t)N,
                                            rocprim::plus<uint32_t>(), st));
    if ((rc = S.bits.reserve((size_t)N * nw)) || (rc = S.key_a.reserve((size_t)N)) ||
        (rc = S.key_b.reserve((size_t)N)) || (rc = S.perm_a.reserve((size_t)N)) ||
        (rc = S.perm_b.reserve((size_t)N)) || (rc = S.flag.reserve((size_t)N)) ||
        (rc = S.num.reserve((size_t)N)) || (rc = S.first.reserve((size_t)N)) ||
        (rc = S.split_id.reserve((size_t)N)) || (rc = S.sorted.reserve((size_t)N)) ||
        (rc = S.sort_tmp.reserve(std::max<size_t>(sort_need, 1))) ||
        (rc = S.scan_tmp.reserve(std::max<size_t>(scan_need, 1))))
        return rc;

    // splits
    SplitArgs a;
    a.cj = d_cj;
    a.n = n;
    a.nw = nw;
    a.T = (int)T;
    a.bits = S.bits.p;
    int tpt = 1;
    while (tpt < nw && tpt < kTB) tpt <<= 1;
    unsigned threads = 64;
    if (tpt <= 64) {
        // one tree per workgroup unless PU_TREESET_GROUP asks for more (timing; no result
        // depends on it)
        const char *env = getenv("PU_TREESET_GROUP");
        a.G = std::max(1, std::min(64 / tpt, env ? atoi(env) : 1));
        a.in_lds = 1;
        while (a.G > 1 && split_lds(n, nw, a.G, true) > kLdsCap) a.G >>= 1;
        if (split_lds(n, nw, a.G, true) > kLdsCap) a.in_lds = 0;
    } else {
        a.G = 1;
        a.in_lds = 0;
    }
    if (!a.in_lds) {  // one tree, the clusters in place in memory, a thread per word (nw <= 128)
        a.G = 1;
        threads = (unsigned)std::min(kTB, (nw + 63) / 64 * 64);
        tpt = (int)threads;
    }
    a.tpt = tpt;
    hipLaunchKernelGGL(k_ts_splits, dim3((unsigned)((T + a.G - 1) / a.G)), dim3(threads),
                       split_lds(n, nw, a.G, a.in_lds != 0), st, a);
    HIPCHK(nullptr, hipGetLastError());
    if ((rc = mark(S, 1, st))) return rc;

    // ids
    uint32_t *perm = S.perm_a.p, *other = S.perm_b.p;
    hipLaunchKernelGGL(k_ts_iota, dim3(blocks(N)), dim3(kTB), 0, st, perm, N);
    for (int w = 0; w < nw; ++w) {
        hipLaunchKernelGGL(k_ts_gather, dim3(blocks(N)), dim3(kTB), 0, st, S.bits.p, perm, w, nw, N,
                           S.key_a.p);
        // the last word holds n & 63 bits only
        const unsigned end = (w == nw - 1 && (n & 63)) ? (unsigned)(((n & 63) + 7) / 8 * 8) : 64u;
        size_t tb = S.sort_tmp.cap;
        HIPCHK(nullptr, rocprim::radix_sort_pairs((void *)S.sort_tmp.p, tb, (const uint64_t *)S.key_a.p,
                                                  S.key_b.p, (const uint32_t *)perm, other,
                                                  (size_t)N, 0u, end, st));
        std::swap(perm, other);
    }
    hipLaunchKernelGGL(k_ts_flag, dim3(blocks(N)), dim3(kTB), 0, st, S.bits.p, perm, nw, N, S.flag.p);
    {
        size_t sb = S.scan_tmp.cap;
        HIPCHK(nullptr, rocprim::inclusive_scan((void *)S.scan_tmp.p, sb, S.flag.p, S.num.p,
                                                (size_t)N, rocprim::plus<uint32_t>(), st));
    }
    hipLaunchKernelGGL(k_ts_uniq, dim3(blocks(N)), dim3(kTB), 0, st, S.bits.p, perm, S.flag.p,
                       S.num.p, nw, N, S.split_id.p, S.first.p, o.uniq_bits, o.n_unique);
    if (o.count)
        hipLaunchKernelGGL(k_ts_count, dim3(blocks(N)), dim3(kTB), 0, st, S.first.p, o.n_unique, N,
                           o.count);
    hipLaunchKernelGGL(k_ts_edge_ids, dim3(blocks(T * E)), dim3(kTB), 0, st, d_cj, d_y, d_emap,
                       S.split_id.p, n, T, o.edge_ids);
    HIPCHK(nullptr, hipGetLastError());
    if ((rc = mark(S, 2, st))) return rc;
    if (ids) {
        ids->split_id = S.split_id.p;
        ids->perm = perm;
        ids->first = S.first.p;
    }

    // RF
    if (o.rf && n_rows > 0) {
        int P = 1;
        while (P < ns) P <<= 1;
        hipLaunchKernelGGL(k_ts_sort_lists, dim3((unsigned)T), dim3(kTB), (size_t)P * 4, st,
                           S.split_id.p, ns, P, S.sorted.p);
        RfArgs r;
        r.sorted = S.sorted.p;
        r.ns = ns;
        r.T = (int)T;
        r.n_rows = n_rows;
        r.stride = ns | 1;
        r.rf = o.rf;
        size_t lds = (size_t)2 * kTile * r.stride * 4;
        if (lds > kLdsCap) {
            r.stride = 0;
            lds = 0;
        }
        const dim3 grid((unsigned)((T + kTile - 1) / kTile), (unsigned)((n_rows + kTile - 1) / kTile));
        const char *env = getenv("PU_TREESET_RF");
        if (env && !strcmp(env, "wave"))
            hipLaunchKernelGGL(k_ts_rf<true>, grid, dim3(kTB), lds, st, r);
        else
            hipLaunchKernelGGL(k_ts_rf<false>, grid, dim3(kTB), lds, st, r);
        HIPCHK(nullptr, hipGetLastError());
    }
    return mark(S, 3, st);
}

}  // namespace

// the names of this file's constants (kTile) mean other things in namespace pu: the stages stay
// outside it, behind this door
int pu::treeset_run(int device, hipStream_t st, int n, int64_t T, const int32_t *d_cj,
                    const int32_t *d_y, const int32_t *d_emap, int n_rows, const TreesetOut &o,
                    TreesetIds *ids) {
    return run_compare(device, st, n, T, d_cj, d_y, d_emap, n_rows, o, ids);
}

int pu::treeset_check_args(const char *fn, int n, int n_trees, int form, const int32_t *trees,
                           const int32_t *roots, int n_rows) {
    if (!trees) return set_err(nullptr, PU_E_ARG, "%s: null buffer", fn);
    if (form != PU_TREES_OPS && form != PU_TREES_JOINS && form != PU_TREES_EDGES)
        return set_err(nullptr, PU_E_ARG, "%s: form = %d (PU_TREES_OPS, _JOINS, _EDGES)", fn, form);
    if (form != PU_TREES_EDGES && !roots)
        return set_err(nullptr, PU_E_ARG, "%s: the ops and joins forms need the root edges", fn);
    if (n < 3 || n > PU_NJ_MAX_N)
        return set_err(nullptr, PU_E_ARG, "%s: n = %d is outside [3, %d]", fn, n, PU_NJ_MAX_N);
    if (n_trees < 1) return set_err(nullptr, PU_E_ARG, "%s: n_trees = %d", fn, n_trees);
    if ((int64_t)n_trees * (n - 3) >= ((int64_t)1 << 31))
        return set_err(nullptr, PU_E_ARG, "%s: %d trees of %d splits: 2^31 or more", fn, n_trees,
                       n - 3);
    if (n_rows < 0 || n_rows > n_trees)
        return set_err(nullptr, PU_E_ARG, "%s: n_rows = %d is outside [0, %d]", fn, n_rows, n_trees);
    return PU_OK;
}

// every form to the device form (header comment); a set too large for the host's memory is
// refused like one too large for the device's
int pu::treeset_device_form(const char *fn, int n, int n_trees, int form, const int32_t *trees,
                            const int32_t *roots, TreesetForm &f) {
    int rc;
    const int64_t T = n_trees;
    const int n_ops = n - 2, E = 2 * n - 3;
    std::vector<int32_t> &cj = f.cj, &y = f.y, &emap = f.emap;
    try {
        cj.resize((size_t)T * n_ops * 2);
        y.resize((size_t)T);
        emap.clear();
        if (form == PU_TREES_EDGES) emap.resize((size_t)T * E);
        std::vector<int32_t> ops((size_t)n_ops * 3), slot((size_t)E), where((size_t)2 * n - 2);
        std::vector<char> state;
        EdgeTree et;
        int32_t root[2];
        for (int64_t t = 0; t < T; ++t) {
            const int32_t *op = ops.data();
            if (form == PU_TREES_OPS) {
                op = trees + t * n_ops * 3;
                root[0] = roots[2 * t];
                root[1] = roots[2 * t + 1];
            } else if (form == PU_TREES_JOINS) {
                for (int m = 0; m < n_ops; ++m) {
                    ops[3 * m] = n + m;
                    ops[3 * m + 1] = trees[(t * n_ops + m) * 2];
                    ops[3 * m + 2] = trees[(t * n_ops + m) * 2 + 1];
                }
                root[0] = roots[2 * t];
                root[1] = roots[2 * t + 1];
            } else {
                if ((rc = et.build(fn, t, n, trees + t * E * 2))) return rc;
                et.schedule(ops.data(), root, slot.data());
                for (int k = 0; k < E; ++k) emap[(size_t)t * E + k] = slot[k] >> 1;
            }
            if ((rc = check_ops(fn, t, n, op, root, state))) return rc;
            for (int m = 0; m < n_ops; ++m) where[op[3 * m]] = m;
            auto name = [&](int v) { return v < n ? v : n + where[v]; };
            for (int m = 0; m < n_ops; ++m) {
                cj[((size_t)t * n_ops + m) * 2] = name(op[3 * m + 1]);
                cj[((size_t)t * n_ops + m) * 2 + 1] = name(op[3 * m + 2]);
            }
            const int X = op[3 * (n_ops - 1)];
            y[(size_t)t] = name(root[0] == X ? root[1] : root[0]);
        }
    } catch (const std::bad_alloc &) {
        return set_err(nullptr, PU_E_NOMEM, "%s: the host cannot hold %lld trees of %d tips", fn,
                       (long long)T, n);
    }
    return PU_OK;
}

extern "C" {

int pu_treeset_compare(int device, int n, int n_trees, int form, const int32_t *trees,
                       const int32_t *roots, int n_rows, int32_t *edge_ids_out,
                       int64_t *n_unique_out, uint64_t *uniq_bits_out, int32_t *uniq_count_out,
                       int32_t *rf_out) {
    const char *fn = "pu_treeset_compare";
    int rc;
    if (!trees || !edge_ids_out || !n_unique_out)
        return set_err(nullptr, PU_E_ARG, "%s: null buffer", fn);
    if ((rc = treeset_check_args(fn, n, n_trees, form, trees, roots, n_rows))) return rc;
    const int64_t T = n_trees;
    const int E = 2 * n - 3;
    TreesetForm f;
    if ((rc = treeset_device_form(fn, n, n_trees, form, trees, roots, f))) return rc;
    const std::vector<int32_t> &cj = f.cj, &y = f.y, &emap = f.emap;
    if ((rc = check_device(device))) return rc;
    DeviceGuard g(device);
    HostCall h(device);
    const size_t N = (size_t)T * (n - 3), nw = (size_t)(n + 63) / 64;
    const int32_t *d_cj = h.to_device(cj.data(), cj.size());
    const int32_t *d_y = h.to_device(y.data(), y.size());
    const int32_t *d_emap = emap.empty() ? nullptr : h.to_device(emap.data(), emap.size());
    TreesetOut o;
    o.edge_ids = h.alloc<int32_t>((size_t)T * E);
    o.n_unique = h.alloc<int64_t>(1);
    o.uniq_bits = uniq_bits_out ? h.alloc<uint64_t>(N * nw) : nullptr;
    o.count = uniq_count_out ? h.alloc<int32_t>(N) : nullptr;
    o.rf = rf_out && n_rows ? h.alloc<int32_t>((size_t)n_rows * T) : nullptr;
    if (!h.rc) h.rc = treeset_run(device, h.st, n, T, d_cj, d_y, d_emap, n_rows, o, nullptr);
    h.to_host(edge_ids_out, o.edge_ids, (size_t)T * E);
    h.to_host(n_unique_out, o.n_unique, 1);
    if (o.rf) h.to_host(rf_out, o.rf, (size_t)n_rows * T);
    // U is known only now: its rows follow in a second wave of copies
    if (!h.rc) h.hip(fn, hipStreamSynchronize(h.st));
    if (!h.rc) {
        const size_t U = (size_t)*n_unique_out;
        if (o.uniq_bits) h.to_host(uniq_bits_out, o.uniq_bits, U * nw);
        if (o.count) h.to_host(uniq_count_out, o.count, U);
    }
    return h.finish(fn);
}

int pu_treeset_profile(int device, int on) {
    if (device < 0 || device >= 64) return set_err(nullptr, PU_E_ARG, "device %d", device);
    std::lock_guard<std::mutex> lk(g_ts[device].mu);
    g_ts[device].prof_on = on != 0;
    g_ts[device].have = false;
    return PU_OK;
}

int pu_treeset_kernel_ms(int device, double *splits_ms, double *ids_ms, double *rf_ms) {
    const char *fn = "pu_treeset_kernel_ms";
    if (device < 0 || device >= 64 || !splits_ms || !ids_ms || !rf_ms)
        return set_err(nullptr, PU_E_ARG, "%s: bad argument", fn);
    std::lock_guard<std::mutex> lk(g_ts[device].mu);
    TreesetState &S = g_ts[device];
    if (!S.have) return set_err(nullptr, PU_E_STATE, "%s: nothing recorded", fn);
    DeviceGuard g(device);
    HIPCHK(nullptr, hipEventSynchronize(S.ev[3]));
    float ms[3];
    for (int i = 0; i < 3; ++i) HIPCHK(nullptr, hipEventElapsedTime(&ms[i], S.ev[i], S.ev[i + 1]));
    *splits_ms = ms[0];
    *ids_ms = ms[1];
    *rf_ms = ms[2];
    return PU_OK;
}

}  // extern "C"
