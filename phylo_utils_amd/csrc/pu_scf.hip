// pu_scf.hip -- site concordance factors on the GPU: per internal branch of a tree
// the quartets drawn around it and, per quartet, the weighted number of decisive site patterns
// that support each of its three resolutions; and the C ABI of it (pu_scf_counts, pu_scf_profile,
// pu_scf_kernel_ms).
//
// The reference has no concordance factors; the rule is this project's own (DESIGN 4.29,
// normative; tests/concordance_reference.py restates it).  The tree is an edge list of DESIGN
// 4.22's form.  Edge e = (x, y) is internal iff both ends are internal nodes; x's other two edges
// in increasing edge id lead to clades A and B, y's to C and D; a clade is the set of tips beyond
// its edge in ascending row order.  With m = |A||B||C||D| <= Q the branch has all m quartets in
// mixed-radix order (D fastest), else Q quartets whose clade k takes the tip at index
// min(floor(u |X|), |X| - 1), u = philox_u(seed, q, 4 e + k, 3rd counter word 2).  A pattern is
// decisive for a quartet iff all four codes have exactly one state; it adds its weight to n1
// (ab|cd), n2 (ac|bd) or n3 (ad|bc) where two pairs of equal states differ from each other.
//
//   host             checks the alignment and the tree, roots the tree on edge 0 and builds the
//                    tips below every node as bitsets of nw = ceil(n / 64) words: a clade is one
//                    of them or its complement, so no tip list per branch exists anywhere.
//   k_scf_picks      one lane per (branch, quartet, clade): the index by the rule above, then a
//                    rank/select on the clade's bitset.
//   k_scf_states     every (taxon, pattern) code as one byte: the single state, or 0xFF where
//                    the state set is no singleton; rows padded to the pattern tile with 0xFF,
//                    so the hot loop has no bound to check.
//   k_scf_counts     a workgroup takes a block of quartets and walks pattern tiles of 256 PPL
//                    patterns; a lane owns PPL neighbouring patterns of the tile, keeps their
//                    weights in registers and reads its PPL bytes of each of the quartet's four
//                    rows in one load.  Three 64-bit sums per lane, a wave reduction, one 64-bit
//                    LDS atomic per (wave, quartet, count), and at the end of the workgroup one
//                    global 64-bit atomic per (quartet, count) that is not zero.
//                    Kept: the rows read straight from memory, where L2 serves the re-reads
//                    (PPL = 8, the tile 2048 patterns, blocks of 64 quartets).  Measured against
//                    it (PU_SCF_FEED=lds, read at each call; DESIGN 4.29 has both times): the
//                    tile of all n rows staged in LDS once per block of 512 quartets (PPL = 8, 4
//                    or 2, the widest whose n rows fit the 160 KiB beside the counters; none
//                    fits n > 296 and the rows are read from memory) -- 3.4 and 7.3 times
//                    slower at 50 taxa x 100k and 200 taxa x 10k patterns: one workgroup per
//                    CU, few blocks, and a staged row is used only 4 * 512 / n times.  No
//                    result depends on the feed.
//
// Every sum is an unsigned 64-bit integer: no result depends on the launch shape, the feed, the
// order or the chunking.
//
// Memory.  The device holds the whole coded alignment, as the parsimony calls do, and a
// workspace of at most 256 MiB (PU_SCF_WS=bytes lowers it): one half for the picks and counts of
// a chunk of branches (40 bytes per quartet), the other for the state bytes of a chunk of
// patterns.  The call is cut into chunks of branches (PU_SCF_CHUNK=n caps them) and, inside
// each, of patterns.  A chunk of patterns is never less than one tile of 2048: a PU_SCF_WS below
// 2 * 2048 n_taxa bytes (16 MB at 4000 taxa) is exceeded by that much and no further.
#include <hip/hip_runtime.h>

#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "pu_ctx.h"
#include "pu_philox.h"
#include "pu_service.h"
#include "pu_treeform.h"

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "pu_scf.hip: gfx950 only, as the other kernel files of this library"
#endif

using namespace pu;

namespace {

constexpr int kTB = 256;
constexpr int kPatTile = 2048;             // the widest pattern tile (PPL = 8): rows are padded to it
constexpr size_t kLdsCap = 160 * 1024;  // LDS one workgroup may have
constexpr size_t kWsCap = (size_t)256 << 20;
constexpr int kMaxStates = 32;
constexpr int kQbGlobal = 64;   // quartets of a workgroup, rows from memory
constexpr int kQbLds = 512;     // quartets of a workgroup, rows in LDS: they are staged once per block
constexpr uint8_t kNone = 0xFF;  // no single state

// ---- picks ------------------------------------------------------------------------------------

struct PickArgs {
    const uint64_t *below;  // [2n-2][nw] tips below every node, the tree rooted on edge 0
    const int32_t *clade;   // [nb][4][3] = (node, complement?, size) of clades A, B, C, D
    const int32_t *binfo;   // [nb][3] = (edge id, nq, exhaustive?)
    int n, nw, Q;
    int64_t total;  // nb * Q * 4
    uint64_t seed;
    int32_t *taxa;  // [nb][Q][4]
};

__global__ void __launch_bounds__(kTB) k_scf_picks(PickArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kTB + threadIdx.x;
    if (i >= a.total) return;
    const int64_t b = i / (4 * (int64_t)a.Q);
    const int64_t r = i - b * 4 * (int64_t)a.Q;
    const int64_t q = r >> 2;
    const int k = (int)(r & 3);
    const int32_t *bi = a.binfo + 3 * b;
    if (q >= bi[1]) {
        a.taxa[i] = -1;
        return;
    }
    const int32_t *cl = a.clade + b * 12;
    const int size = cl[3 * k + 2];
    int64_t idx;
    if (bi[2]) {  // all quartets, mixed radix with D fastest
        int64_t t = q;
        idx = 0;
        for (int kk = 3; kk >= 0; --kk) {
            const int64_t s = cl[3 * kk + 2];
            const int64_t d = kk ? t % s : t;
            t /= s;
            if (kk == k) idx = d;
        }
    } else {
        const double u = philox_u(a.seed, (uint64_t)q, (uint32_t)(4 * bi[0] + k), 2u);
        idx = (int64_t)floor(u * (double)size);
    }
    idx = min(idx, (int64_t)size - 1);
    const uint64_t *bits = a.below + (int64_t)cl[3 * k] * a.nw;
    const bool comp = cl[3 * k + 1] != 0;
    const uint64_t last = (a.n & 63) ? (1ull << (a.n & 63)) - 1ull : ~0ull;
    int32_t tip = -1;
    for (int w = 0; w < a.nw; ++w) {
        uint64_t x = comp ? ~bits[w] : bits[w];
        if (w == a.nw - 1) x &= last;
        const int c = __popcll(x);
        if (idx < c) {
            for (int j = 0; j < (int)idx; ++j) x &= x - 1;
            tip = w * 64 + (__ffsll((unsigned long long)x) - 1);
            break;
        }
        idx -= c;
    }
    a.taxa[i] = tip;
}

// ---- states -----------------------------------------------------------------------------------

struct StateArgs {
    const uint8_t *codes;  // [n][n_pat]
    int64_t n_pat, p0, n_cols, pitch;
    uint8_t single[kMaxCodes];
    uint8_t *sb;  // [n][pitch]
};

__global__ void __launch_bounds__(kTB) k_scf_states(StateArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kTB + threadIdx.x;
    if (i >= a.pitch) return;
    const int64_t t = blockIdx.y;
    uint8_t s = kNone;
    if (i < a.n_cols) s = a.single[a.codes[t * a.n_pat + a.p0 + i] & (kMaxCodes - 1)];
    a.sb[t * a.pitch + i] = s;
}

// ---- counts -----------------------------------------------------------------------------------

struct CountArgs {
    const uint8_t *sb;   // [n][pitch], pitch a multiple of kPatTile
    const uint64_t *w;   // [n_pat] or null: all 1
    const int32_t *taxa;  // [nqt][4]
    int64_t pitch, p0, n_cols, nqt;
    int n_taxa, qb, n_tiles;
    uint64_t *counts;  // [nqt][3]
};

__device__ inline unsigned long long wave_sum(unsigned long long v) {
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

template <int PPL>
__device__ inline uint64_t load_bytes(const uint8_t *p) {
    if (PPL == 8) return *reinterpret_cast<const uint64_t *>(p);
    if (PPL == 4) return *reinterpret_cast<const uint32_t *>(p);
    return *reinterpret_cast<const uint16_t *>(p);
}

__host__ __device__ inline size_t acc_bytes(int qb) { return ((size_t)qb * 24 + 15) / 16 * 16; }

template <int PPL, bool LDS>
__global__ void __launch_bounds__(kTB) k_scf_counts(CountArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int TILE = kTB * PPL;
    unsigned long long *acc = reinterpret_cast<unsigned long long *>(smem);  // [qb][3]
    uint8_t *rows = smem + acc_bytes(a.qb);                                  // [n][TILE] (LDS)
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int64_t q0 = (int64_t)blockIdx.x * a.qb;
    const int nq = (int)min((int64_t)a.qb, a.nqt - q0);
    for (int i = tid; i < nq * 3; i += kTB) acc[i] = 0ull;
    __syncthreads();
    for (int t = (int)blockIdx.y; t < a.n_tiles; t += (int)gridDim.y) {
        const int64_t col0 = (int64_t)t * TILE + (int64_t)tid * PPL;
        unsigned long long wv[PPL];
#pragma unroll
        for (int j = 0; j < PPL; ++j)
            wv[j] = col0 + j < a.n_cols ? (a.w ? a.w[a.p0 + col0 + j] : 1ull) : 0ull;
        if (LDS) {
            __syncthreads();  // the tile before this one has been read
            constexpr int V = TILE / 16;
            for (int i = tid; i < a.n_taxa * V; i += kTB) {
                const int r = i / V, c = i - r * V;
                reinterpret_cast<uint4 *>(rows)[i] = *reinterpret_cast<const uint4 *>(
                    a.sb + (int64_t)r * a.pitch + (int64_t)t * TILE + (int64_t)c * 16);
            }
            __syncthreads();
        }
        for (int q = 0; q < nq; ++q) {
            const int4 tx = *reinterpret_cast<const int4 *>(a.taxa + (q0 + q) * 4);
            // a slot past the branch's quartets; the bound keeps a wrong pick inside the rows
            if ((unsigned)tx.x >= (unsigned)a.n_taxa || (unsigned)tx.y >= (unsigned)a.n_taxa ||
                (unsigned)tx.z >= (unsigned)a.n_taxa || (unsigned)tx.w >= (unsigned)a.n_taxa)
                continue;
            uint64_t ra, rb, rc, rd;
            if (LDS) {
                const uint8_t *base = rows + tid * PPL;
                ra = load_bytes<PPL>(base + (size_t)tx.x * TILE);
                rb = load_bytes<PPL>(base + (size_t)tx.y * TILE);
                rc = load_bytes<PPL>(base + (size_t)tx.z * TILE);
                rd = load_bytes<PPL>(base + (size_t)tx.w * TILE);
            } else {
                const uint8_t *base = a.sb + col0;
                ra = load_bytes<PPL>(base + (int64_t)tx.x * a.pitch);
                rb = load_bytes<PPL>(base + (int64_t)tx.y * a.pitch);
                rc = load_bytes<PPL>(base + (int64_t)tx.z * a.pitch);
                rd = load_bytes<PPL>(base + (int64_t)tx.w * a.pitch);
            }
            unsigned long long n1 = 0ull, n2 = 0ull, n3 = 0ull;
#pragma unroll
            for (int j = 0; j < PPL; ++j) {
                const unsigned sa = (unsigned)(ra >> (8 * j)) & 0xFFu, sb = (unsigned)(rb >> (8 * j)) & 0xFFu;
                const unsigned sc = (unsigned)(rc >> (8 * j)) & 0xFFu, sd = (unsigned)(rd >> (8 * j)) & 0xFFu;
                const bool dec = ((sa | sb | sc | sd) & 0x80u) == 0u;  // states are below 32
                n1 += (dec && sa == sb && sc == sd && sa != sc) ? wv[j] : 0ull;
                n2 += (dec && sa == sc && sb == sd && sa != sb) ? wv[j] : 0ull;
                n3 += (dec && sa == sd && sb == sc && sa != sb) ? wv[j] : 0ull;
            }
            n1 = wave_sum(n1);
            n2 = wave_sum(n2);
            n3 = wave_sum(n3);
            if (lane == 0) {
                if (n1) atomicAdd(&acc[3 * q], n1);
                if (n2) atomicAdd(&acc[3 * q + 1], n2);
                if (n3) atomicAdd(&acc[3 * q + 2], n3);
            }
        }
    }
    __syncthreads();
    unsigned long long *out = reinterpret_cast<unsigned long long *>(a.counts) + q0 * 3;
    for (int i = tid; i < nq * 3; i += kTB)
        if (acc[i]) atomicAdd(&out[i], acc[i]);
}

// ---- host side --------------------------------------------------------------------------------

enum { T_PICKS = 0, T_STATES = 1, T_COUNTS = 2 };

struct ScfState : DevState {
    DevBuf<uint8_t> sb;
    DevBuf<uint64_t> counts;
    DevBuf<int32_t> taxa;
    bool prof = false, have_ms = false;
    double ms[3] = {0.0, 0.0, 0.0};
    std::vector<hipEvent_t> ev;  // pairs around every launch of the chunk in flight
    std::vector<int> what;
    size_t n_ev = 0;
};
ScfState g_scf[64];

// events around one launch while profiling; like the events of the other per-device states
// they live as long as the process
struct Span {
    ScfState &S;
    hipStream_t st;
    bool on;
    Span(ScfState &s, hipStream_t stream, int what) : S(s), st(stream), on(s.prof) {
        if (!on) return;
        while (S.ev.size() < 2 * (S.n_ev + 1)) {
            hipEvent_t e = nullptr;
            if (hipEventCreate(&e) != hipSuccess) {
                on = false;
                return;
            }
            S.ev.push_back(e);
        }
        if (S.what.size() <= S.n_ev) S.what.resize(S.n_ev + 1);
        S.what[S.n_ev] = what;
        (void)hipEventRecord(S.ev[2 * S.n_ev], st);
    }
    ~Span() {
        if (!on) return;
        (void)hipEventRecord(S.ev[2 * S.n_ev + 1], st);
        ++S.n_ev;
    }
};

// after a wait for the stream: the spans of the chunk into ms
void add_spans(ScfState &S) {
    for (size_t i = 0; i < S.n_ev; ++i) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, S.ev[2 * i], S.ev[2 * i + 1]) == hipSuccess)
            S.ms[S.what[i]] += ms;
    }
    S.n_ev = 0;
}

// pu_fitch_lengths' alignment rules (pu_parsimony.hip: check_aln), with n_taxa >= 4, and the
// single state of every code
int check_aln(const char *fn, const uint8_t *codes, int n_taxa, int64_t n_pat, int n_codes, int K,
              const double *table, const int64_t *weights, uint8_t *single) {
    if (!codes || !table) return set_err(nullptr, PU_E_ARG, "%s: null buffer", fn);
    if (n_taxa < 4 || n_taxa > PU_PARS_MAX_TAXA)
        return set_err(nullptr, PU_E_ARG, "%s: n_taxa = %d is outside [4, %d]", fn, n_taxa,
                       PU_PARS_MAX_TAXA);
    if (n_pat < 1) return set_err(nullptr, PU_E_ARG, "%s: n_pat = %lld", fn, (long long)n_pat);
    if (K < 1 || K > kMaxStates)
        return set_err(nullptr, PU_E_ARG, "%s: n_states = %d is outside [1, %d]", fn, K,
                       kMaxStates);
    if (n_codes < 1 || n_codes > kMaxCodes)
        return set_err(nullptr, PU_E_ARG, "%s: n_codes = %d is outside [1, %d]", fn, n_codes,
                       kMaxCodes);
    std::fill(single, single + kMaxCodes, kNone);
    for (int c = 0; c < n_codes; ++c) {
        int n_set = 0, state = 0;
        for (int k = 0; k < K; ++k)
            if (table[(size_t)c * K + k] > 0.0) {
                ++n_set;
                state = k;
            }
        if (!n_set)
            return set_err(nullptr, PU_E_ARG, "%s: code %d allows no state (an all-zero table row)",
                           fn, c);
        if (n_set == 1) single[c] = (uint8_t)state;
    }
    if (int rc = check_codes(fn, codes, n_taxa, n_pat, n_codes)) return rc;
    if (weights) {
        const uint64_t lim = ((uint64_t)1 << 63) / (2 * (uint64_t)n_taxa);
        uint64_t sum = 0;
        for (int64_t p = 0; p < n_pat; ++p) {
            if (weights[p] < 0)
                return set_err(nullptr, PU_E_ARG, "%s: weight %lld of pattern %lld is negative", fn,
                               (long long)weights[p], (long long)p);
            if ((uint64_t)weights[p] > lim - sum)
                return set_err(nullptr, PU_E_ARG, "%s: the weights sum past 2^63 / (2 n_taxa)", fn);
            sum += (uint64_t)weights[p];
        }
    }
    return PU_OK;
}

// The branches of a call on the host: the tips below every node of the tree rooted on edge 0,
// and per internal edge its four clades
struct Branches {
    int n = 0, nw = 0;
    std::vector<uint64_t> below;   // [2n-2][nw]
    std::vector<int32_t> internal;  // edge ids
    std::vector<int32_t> clade;    // [nb][4][3]
    std::vector<int32_t> binfo;    // [nb][3]

    void build(EdgeTree &et, int n_taxa, const int32_t *edges, int64_t Q) {
        n = n_taxa;
        nw = (n + 63) / 64;
        const int n_nodes = 2 * n - 2, n_edges = 2 * n - 3;
        std::vector<int32_t> ops((size_t)(n - 2) * 3), slot((size_t)n_edges), par((size_t)n_nodes, -1);
        int32_t root[2];
        et.schedule(ops.data(), root, slot.data());
        below.assign((size_t)n_nodes * nw, 0ull);
        for (int i = 0; i < n; ++i) below[(size_t)i * nw + (i >> 6)] = 1ull << (i & 63);
        for (int i = 0; i < n - 2; ++i) {
            const int v = ops[3 * i];
            for (int c = 1; c <= 2; ++c) {
                const int ch = ops[3 * i + c];
                par[ch] = v;
                for (int w = 0; w < nw; ++w) below[(size_t)v * nw + w] |= below[(size_t)ch * nw + w];
            }
        }
        par[root[0]] = root[1];
        par[root[1]] = root[0];
        std::vector<int32_t> size((size_t)n_nodes);
        for (int v = 0; v < n_nodes; ++v) {
            int c = 0;
            for (int w = 0; w < nw; ++w) c += __builtin_popcountll(below[(size_t)v * nw + w]);
            size[v] = c;
        }
        for (int e = 0; e < n_edges; ++e) {
            const int x = edges[2 * e], y = edges[2 * e + 1];
            if (x < n || y < n) continue;
            internal.push_back(e);
            int64_t m = 1;
            for (int end : {x, y})
                for (int j = 0; j < 3; ++j) {  // adj is in increasing edge id
                    const int f = et.adj[(size_t)end * 6 + 2 * j], g = et.adj[(size_t)end * 6 + 2 * j + 1];
                    if (g == e) continue;
                    // beyond edge g seen from `end`: below f where f hangs under `end`, else
                    // everything that is not below `end`
                    const bool down = par[f] == end;
                    const int s = down ? size[f] : n - size[end];
                    clade.push_back(down ? f : end);
                    clade.push_back(down ? 0 : 1);
                    clade.push_back(s);
                    m *= s;  // at most 4000^4 / 256 < 2^63
                }
            binfo.push_back(e);
            binfo.push_back((int32_t)std::min<int64_t>(m, Q));
            binfo.push_back(m <= Q ? 1 : 0);
        }
    }
};

template <int PPL, bool LDS>
void launch_counts(dim3 grid, size_t lds, hipStream_t st, const CountArgs &a) {
    hipLaunchKernelGGL((k_scf_counts<PPL, LDS>), grid, dim3(kTB), lds, st, a);
}

}  // namespace

extern "C" {

int pu_scf_counts(int device, int n_taxa, int64_t n_pat, int n_codes, int n_states,
                  const uint8_t *codes, const double *code_table, const int64_t *weights,
                  const int32_t *edges, int n_quartets, uint64_t seed, uint64_t *counts_out,
                  int32_t *nq_out, int32_t *taxa_out) {
    const char *fn = "pu_scf_counts";
    int rc;
    StateArgs sa{};
    if ((rc = check_aln(fn, codes, n_taxa, n_pat, n_codes, n_states, code_table, weights,
                        sa.single)))
        return rc;
    if (n_quartets < 1) return set_err(nullptr, PU_E_ARG, "%s: n_quartets = %d", fn, n_quartets);
    const int64_t Q = n_quartets;
    const size_t cap = (size_t)env_cap("PU_SCF_WS", (int64_t)kWsCap);
    const size_t per_branch = (size_t)Q * 40;  // counts [Q][3] uint64 and taxa [Q][4] int32
    if (per_branch > cap / 2)
        return set_err(nullptr, PU_E_ARG, "%s: n_quartets = %d: the counts and picks of one branch "
                       "(%zu bytes) pass half the workspace of %zu bytes", fn, n_quartets,
                       per_branch, cap);
    if (!edges || !counts_out || !nq_out) return set_err(nullptr, PU_E_ARG, "%s: null buffer", fn);
    EdgeTree et;
    if ((rc = et.build(fn, 0, n_taxa, edges))) return rc;
    const int n_edges = 2 * n_taxa - 3;
    Branches B;
    B.build(et, n_taxa, edges, Q);
    const int64_t nb_all = (int64_t)B.internal.size();
    std::fill(counts_out, counts_out + (size_t)n_edges * Q * 3, (uint64_t)0);
    std::fill(nq_out, nq_out + n_edges, 0);
    if (taxa_out) std::fill(taxa_out, taxa_out + (size_t)n_edges * Q * 4, -1);
    for (int64_t b = 0; b < nb_all; ++b) nq_out[B.internal[b]] = B.binfo[3 * b + 1];

    if ((rc = check_device(device))) return rc;
    DeviceGuard g(device);
    HostCall h(device);
    if (h.rc) return h.rc;
    ScfState &S = g_scf[device];
    StateScope scope(S, h.st);
    if (scope.rc) return scope.rc;
    S.have_ms = false;  // until this call has ended well
    S.ms[0] = S.ms[1] = S.ms[2] = 0.0;
    S.n_ev = 0;

    // the cut: branches per chunk, patterns per chunk (a multiple of the widest tile)
    const int64_t bc = env_cap("PU_SCF_CHUNK",
                               std::max<int64_t>(1, std::min<int64_t>(nb_all, (int64_t)(cap / 2 / per_branch))));
    const int64_t padded = (n_pat + kPatTile - 1) / kPatTile * kPatTile;
    int64_t pc = padded;
    if ((size_t)n_taxa * (size_t)pc > cap / 2)
        pc = std::max<int64_t>(kPatTile, (int64_t)(cap / 2 / (size_t)n_taxa) / kPatTile * kPatTile);

    // the feed: rows in LDS at the widest tile whose n rows fit, or from memory
    const char *feed = getenv("PU_SCF_FEED");
    const bool want_lds = feed && !strcmp(feed, "lds");
    int ppl = 8, qb = kQbGlobal;
    bool lds = false;
    if (want_lds)
        for (int p : {8, 4, 2})
            if (acc_bytes(kQbLds) + (size_t)n_taxa * kTB * p <= kLdsCap) {
                ppl = p;
                qb = kQbLds;
                lds = true;
                break;
            }

    const uint8_t *d_codes = h.to_device(codes, (size_t)n_taxa * n_pat);
    const uint64_t *d_w =
        reinterpret_cast<const uint64_t *>(h.to_device(weights, weights ? (size_t)n_pat : 0));
    const uint64_t *d_below = h.to_device(B.below.data(), B.below.size());
    const int32_t *d_clade = h.to_device(B.clade.data(), B.clade.size());
    const int32_t *d_binfo = h.to_device(B.binfo.data(), B.binfo.size());
    if (!h.rc && nb_all) {
        if ((rc = S.sb.reserve((size_t)n_taxa * pc)) || (rc = S.counts.reserve((size_t)bc * Q * 3)) ||
            (rc = S.taxa.reserve((size_t)bc * Q * 4)))
            h.rc = rc;
    }
    std::vector<uint64_t> h_counts;
    std::vector<int32_t> h_taxa;
    if (!h.rc && nb_all) {
        h_counts.resize((size_t)bc * Q * 3);
        h_taxa.resize((size_t)bc * Q * 4);
    }
    int64_t staged_p0 = -1;  // the pattern chunk whose states S.sb holds
    for (int64_t b0 = 0; b0 < nb_all && !h.rc; b0 += bc) {
        const int64_t nb = std::min<int64_t>(bc, nb_all - b0), nqt = nb * Q;
        PickArgs pa;
        pa.below = d_below;
        pa.clade = d_clade + b0 * 12;
        pa.binfo = d_binfo + b0 * 3;
        pa.n = n_taxa;
        pa.nw = B.nw;
        pa.Q = n_quartets;
        pa.total = nqt * 4;
        pa.seed = seed;
        pa.taxa = S.taxa.p;
        {
            Span sp(S, h.st, T_PICKS);
            hipLaunchKernelGGL(k_scf_picks, dim3((unsigned)((pa.total + kTB - 1) / kTB)), dim3(kTB),
                               0, h.st, pa);
        }
        h.hip("hipMemsetAsync", hipMemsetAsync(S.counts.p, 0, (size_t)nqt * 24, h.st));
        for (int64_t p0 = 0; p0 < n_pat && !h.rc; p0 += pc) {
            const int64_t n_cols = std::min<int64_t>(pc, n_pat - p0);
            const int64_t pitch = (n_cols + kPatTile - 1) / kPatTile * kPatTile;
            if (staged_p0 != p0) {
                sa.codes = d_codes;
                sa.n_pat = n_pat;
                sa.p0 = p0;
                sa.n_cols = n_cols;
                sa.pitch = pitch;
                sa.sb = S.sb.p;
                Span sp(S, h.st, T_STATES);
                hipLaunchKernelGGL(k_scf_states, dim3((unsigned)(pitch / kTB), (unsigned)n_taxa),
                                   dim3(kTB), 0, h.st, sa);
                staged_p0 = p0;
            }
            CountArgs ca;
            ca.sb = S.sb.p;
            ca.w = d_w;
            ca.taxa = S.taxa.p;
            ca.pitch = pitch;
            ca.p0 = p0;
            ca.n_cols = n_cols;
            ca.nqt = nqt;
            ca.n_taxa = n_taxa;
            ca.qb = qb;
            const int tile = kTB * ppl;
            ca.n_tiles = (int)((n_cols + tile - 1) / tile);
            ca.counts = S.counts.p;
            const int64_t n_qblocks = (nqt + qb - 1) / qb;
            // a workgroup walks several tiles where there are many: its global atomics come once
            const int64_t gy = std::max<int64_t>(
                1, std::min<int64_t>(std::min<int64_t>(ca.n_tiles, 65535), (8192 + n_qblocks - 1) / n_qblocks));
            const dim3 grid((unsigned)n_qblocks, (unsigned)gy);
            const size_t lds_bytes = acc_bytes(qb) + (lds ? (size_t)n_taxa * tile : 0);
            Span sp(S, h.st, T_COUNTS);
            if (!lds) launch_counts<8, false>(grid, lds_bytes, h.st, ca);
            else if (ppl == 8) launch_counts<8, true>(grid, lds_bytes, h.st, ca);
            else if (ppl == 4) launch_counts<4, true>(grid, lds_bytes, h.st, ca);
            else launch_counts<2, true>(grid, lds_bytes, h.st, ca);
        }
        h.hip(fn, hipGetLastError());
        h.to_host(h_counts.data(), S.counts.p, (size_t)nqt * 3);
        if (taxa_out) h.to_host(h_taxa.data(), S.taxa.p, (size_t)nqt * 4);
        if (!h.rc) h.hip(fn, hipStreamSynchronize(h.st));
        if (h.rc) break;
        add_spans(S);
        for (int64_t b = 0; b < nb; ++b) {
            const int64_t e = B.internal[b0 + b];
            std::copy(h_counts.begin() + b * Q * 3, h_counts.begin() + (b + 1) * Q * 3,
                      counts_out + e * Q * 3);
            if (taxa_out)
                std::copy(h_taxa.begin() + b * Q * 4, h_taxa.begin() + (b + 1) * Q * 4,
                          taxa_out + e * Q * 4);
        }
    }
    S.n_ev = 0;
    rc = h.finish(fn);
    if (!rc && S.prof) S.have_ms = true;
    return rc;
}

int pu_scf_profile(int device, int on) {
    if (device < 0 || device >= 64) return set_err(nullptr, PU_E_ARG, "device %d", device);
    std::lock_guard<std::mutex> lk(g_scf[device].mu);
    g_scf[device].prof = on != 0;
    g_scf[device].have_ms = false;
    return PU_OK;
}

int pu_scf_kernel_ms(int device, double *picks_ms, double *states_ms, double *counts_ms) {
    const char *fn = "pu_scf_kernel_ms";
    if (device < 0 || device >= 64 || !picks_ms || !states_ms || !counts_ms)
        return set_err(nullptr, PU_E_ARG, "%s: bad argument", fn);
    std::lock_guard<std::mutex> lk(g_scf[device].mu);
    if (!g_scf[device].have_ms) return set_err(nullptr, PU_E_STATE, "%s: nothing recorded", fn);
    *picks_ms = g_scf[device].ms[T_PICKS];
    *states_ms = g_scf[device].ms[T_STATES];
    *counts_ms = g_scf[device].ms[T_COUNTS];
    return PU_OK;
}

}  // extern "C"
