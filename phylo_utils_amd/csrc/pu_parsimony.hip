// pu_parsimony.hip -- Fitch parsimony on the device: the lengths of a batch of
// trees, the exact insertion lengths of query rows on every edge of a tree, and randomised
// stepwise-addition trees, and the exact lengths of all SPR neighbours of a tree
// with the search on them.  Stateless calls on the host layer of pu_service.h.  The reference
// project has no parsimony; the rules are DESIGN 4.22's and 4.26's, restated in
// tests/parsimony_reference.py and tests/parsimony_spr_reference.py.
//
// One lane owns one site pattern and walks the tree's op list, so a tree has no dependency across
// lanes; the tree (or replicate) and the pattern tile are the grid.  State sets are bit masks
// (uint8 for K <= 8, else uint32).  Every sum is an unsigned 64-bit integer: per wave a ballot and
// a popcount (unit weights) or a shuffle sum, per workgroup an LDS counter, then one 64-bit atomic
// add per edge and workgroup -- no result depends on the launch shape or on the chunking.
#include "pu_ctx.h"
#include "pu_service.h"
#include "pu_treeform.h"

namespace {
using namespace pu;

constexpr int kTB = 256;               // lanes of a workgroup = patterns of a tile
constexpr int kParsMaxTaxa = 4000;     // the per-edge LDS counters of a workgroup: 8 (2n - 3) bytes
constexpr int kMaxStates = 32;         // bits of the widest mask
constexpr size_t kWsCap = (size_t)256 << 20;  // node sets of one chunk
constexpr int kQT = 64;                // queries of one scoring workgroup

enum Mode {
    M_LEN = 0,   // post-order only: length and per-pattern changes
    M_EDGE = 1,  // and the pre-order pass: per-edge change counts
    M_STEP = 2,  // and the pre-order pass: per-edge misses of the row being inserted
    M_SETS = 3,  // and the pre-order pass: the edge sets, written out for the scoring kernel
    M_DIR = 4,   // and the pre-order pass: both directional sets of every edge, for k_spr_score
};

// Node ids: a tip is its alignment row (< n_taxa), an internal node is n_taxa + j.  Op i =
// (parent, left, right) has edges 2 i = (left, parent) and 2 i + 1 = (right, parent); the root
// edge is edge 2 n_ops.  Per launch every tree has n_ops ops; tree t of the launch is blockIdx.y.
struct FitchArgs {
    const uint8_t *codes;  // [n_taxa][n_pat]
    const void *masks;     // [n_codes] of M
    const uint64_t *w;     // [n_pat], or null: all 1
    int n_taxa, n_codes, n_ops;
    int64_t n_pat, p0, p1;  // the launch takes patterns [p0, p1)
    const int32_t *ops;     // [n_trees][ops_stride], n_ops rows of 3 each
    const int32_t *root;    // [n_trees][2]
    int64_t ops_stride;
    const int32_t *slot;    // [n_trees][2 n_ops + 1] counter of every edge, or null: its own index
    const int32_t *x;       // M_STEP: [n_trees] the row being inserted
    void *ws;               // [n_trees][1 or 2][n_ops][pc] downward, then upward sets of internal nodes
    int64_t pc;             // patterns per workspace row (>= p1 - p0)
    uint64_t *len;          // [n_trees]
    uint32_t *pp;           // [n_trees][n_pat] changes per pattern, or null
    uint64_t *acc;          // [n_trees][2 n_ops + 1] per-edge sums (M_EDGE, M_STEP)
    void *sets;             // M_SETS: [2 n_ops + 1][n_pat] edge sets of tree 0; M_DIR:
                            // [n_trees][2 (2 n_ops + 1)][pc], row slot[j] = D(child -> parent)
                            // of op-order edge j, row slot[j] ^ 1 the other direction
};

__device__ inline unsigned long long wave_sum(unsigned long long v) {
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// LDS of k_fitch, all dynamic (16-byte carve): [n_slots] counters, the length counter, the masks
__host__ __device__ inline size_t fitch_lds(int n_slots) {
    return ((size_t)(n_slots + 1) * 8 + 15) / 16 * 16 + kMaxCodes * 4;
}

template <class M, int MODE>
__global__ void __launch_bounds__(kTB) k_fitch(FitchArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int n_edges = 2 * a.n_ops + 1;
    const int n_slots = MODE == M_EDGE || MODE == M_STEP ? n_edges : 0;
    unsigned long long *s_acc = reinterpret_cast<unsigned long long *>(smem);
    unsigned long long *s_len = s_acc + n_slots;
    M *s_mask = reinterpret_cast<M *>(smem + ((size_t)(n_slots + 1) * 8 + 15) / 16 * 16);
    const int tid = (int)threadIdx.x, lane = tid & 63, t = (int)blockIdx.y;
    const int64_t p = a.p0 + (int64_t)blockIdx.x * kTB + tid;
    const bool live = p < a.p1;
    const int64_t lp = p - a.p0;
    const M full = (M) ~(M)0;
    if (tid < a.n_codes) s_mask[tid] = static_cast<const M *>(a.masks)[tid];
    for (int e = tid; e < n_slots; e += kTB) s_acc[e] = 0;
    if (tid == 0) *s_len = 0;
    __syncthreads();

    const int32_t *ops = a.ops + (int64_t)t * a.ops_stride;
    const int ra = a.root[2 * t], rb = a.root[2 * t + 1];
    const int n_arr = MODE == M_LEN ? 1 : 2;
    M *down = static_cast<M *>(a.ws) + (size_t)t * n_arr * a.n_ops * a.pc;
    M *up = down + (size_t)a.n_ops * a.pc;
    // a lane past the range holds the full set everywhere: it counts no change and no miss
    auto tip = [&](int v) -> M {
        return live ? s_mask[a.codes[(int64_t)v * a.n_pat + p]] : full;
    };
    auto get = [&](int v) -> M {
        if (v < a.n_taxa) return tip(v);
        return live ? down[(size_t)(v - a.n_taxa) * a.pc + lp] : full;
    };
    const unsigned long long wp = live ? (a.w ? a.w[p] : 1ull) : 0ull;

    uint32_t ch = 0;
    for (int i = 0; i < a.n_ops; ++i) {
        const int par = ops[3 * i], l = ops[3 * i + 1], r = ops[3 * i + 2];
        const M A = get(l), B = get(r);
        const M I = A & B;
        ch += I == 0;
        if (live) down[(size_t)(par - a.n_taxa) * a.pc + lp] = I ? I : (M)(A | B);
    }
    const M Ra = get(ra), Rb = get(rb);
    ch += (M)(Ra & Rb) == 0;
    if (a.pp && live) a.pp[(int64_t)t * a.n_pat + p] = ch;
    {
        const unsigned long long s = wave_sum(wp * ch);
        if (lane == 0 && s) atomicAdd(s_len, s);
    }

    if (MODE != M_LEN) {
        const int32_t *slot = a.slot ? a.slot + (int64_t)t * n_edges : nullptr;
        const M X = MODE == M_STEP ? tip(a.x[t]) : full;
        // the two directional sets of edge j are in registers: its set, change flag and miss flag
        auto emit = [&](int j, M D1, M D2) {
            const M I = D1 & D2;
            if (MODE == M_SETS) {
                if (live) static_cast<M *>(a.sets)[(int64_t)j * a.n_pat + p] = I ? I : (M)(D1 | D2);
                return;
            }
            if (MODE == M_DIR) {
                M *rows = static_cast<M *>(a.sets) + (size_t)t * 2 * n_edges * a.pc;
                if (live) {
                    rows[(size_t)slot[j] * a.pc + lp] = D1;
                    rows[(size_t)(slot[j] ^ 1) * a.pc + lp] = D2;
                }
                return;
            }
            const M E = I ? I : (M)(D1 | D2);
            const bool flag = MODE == M_EDGE ? I == 0 : (M)(X & E) == 0;
            const unsigned long long m = __ballot(flag);
            if (m) {  // wave-uniform
                const unsigned long long c = a.w ? wave_sum(flag ? wp : 0ull)
                                                 : (unsigned long long)__popcll(m);
                if (lane == 0 && c) atomicAdd(&s_acc[slot ? slot[j] : j], c);
            }
        };
        for (int i = a.n_ops - 1; i >= 0; --i) {
            const int par = ops[3 * i], l = ops[3 * i + 1], r = ops[3 * i + 2];
            const M U = par == ra ? Rb
                        : par == rb ? Ra
                                    : (live ? up[(size_t)(par - a.n_taxa) * a.pc + lp] : full);
            const M A = get(l), B = get(r);
            const M IL = B & U, IR = A & U;
            const M UL = IL ? IL : (M)(B | U), UR = IR ? IR : (M)(A | U);
            if (l >= a.n_taxa && live) up[(size_t)(l - a.n_taxa) * a.pc + lp] = UL;
            if (r >= a.n_taxa && live) up[(size_t)(r - a.n_taxa) * a.pc + lp] = UR;
            emit(2 * i, A, UL);
            emit(2 * i + 1, B, UR);
        }
        emit(2 * a.n_ops, Ra, Rb);
    }
    __syncthreads();
    if (tid == 0 && *s_len) atomicAdd(reinterpret_cast<unsigned long long *>(a.len) + t, *s_len);
    for (int e = tid; e < n_slots; e += kTB)
        if (s_acc[e])
            atomicAdd(reinterpret_cast<unsigned long long *>(a.acc) + (int64_t)t * n_edges + e,
                      s_acc[e]);
}

// misses of query q on edge e: sum over patterns of w [S_q & E(e) = 0].  grid (pattern tiles,
// edges, query tiles): a lane keeps its pattern's edge set and walks the tile's queries
struct ScoreArgs {
    const void *sets;       // [n_edges][n_pat]
    const uint8_t *qcodes;  // [n_query][n_pat]
    const void *masks;
    const uint64_t *w;
    int n_codes, n_query, n_edges;
    int64_t n_pat;
    uint64_t *out;  // [n_query][n_edges]
};

template <class M>
__global__ void __launch_bounds__(kTB) k_insert_score(ScoreArgs a) {
    __shared__ unsigned long long s_acc[kQT];
    __shared__ M s_mask[kMaxCodes];
    const int tid = (int)threadIdx.x, lane = tid & 63, e = (int)blockIdx.y;
    const int q0 = (int)blockIdx.z * kQT, nq = min(kQT, a.n_query - q0);
    const int64_t p = (int64_t)blockIdx.x * kTB + tid;
    const bool live = p < a.n_pat;
    if (tid < a.n_codes) s_mask[tid] = static_cast<const M *>(a.masks)[tid];
    if (tid < kQT) s_acc[tid] = 0;
    __syncthreads();
    const M E = live ? static_cast<const M *>(a.sets)[(int64_t)e * a.n_pat + p] : (M) ~(M)0;
    const unsigned long long wp = live ? (a.w ? a.w[p] : 1ull) : 0ull;
    for (int q = 0; q < nq; ++q) {
        const bool flag = live && (M)(s_mask[a.qcodes[(int64_t)(q0 + q) * a.n_pat + p]] & E) == 0;
        const unsigned long long m = __ballot(flag);
        if (m) {
            const unsigned long long c = a.w ? wave_sum(flag ? wp : 0ull)
                                             : (unsigned long long)__popcll(m);
            if (lane == 0 && c) atomicAdd(&s_acc[q], c);
        }
    }
    __syncthreads();
    if (tid < nq && s_acc[tid])
        atomicAdd(reinterpret_cast<unsigned long long *>(a.out) + (int64_t)(q0 + tid) * a.n_edges + e,
                  s_acc[tid]);
}

// ---- SPR ------------------------------------------------------------------------

// One step of the pre-order walk of the rest tree T' of a prune direction, built by the host
// (SprTree::dir_ops).  `sib` and `own` are rows of the directional sets [2 n_edges][pattern]:
//   OP_MERGED  E' = c(rows sib, own): the merged edge, counted into f = ea
//   OP_LOAD    stack[k] = row own: the set arriving at an end of the merged edge
//   OP_STEP    Y = c(row sib, stack[k - 1]) arrives at the child; E' = c(row own, Y), counted into f
//   OP_PUSH    OP_STEP, and stack[k] = Y: the walk goes on below the child
struct SprOp {
    int32_t k, sib, own, f;  // k: depth | kind << 28
};
enum { OP_STEP = 0, OP_PUSH = 1, OP_LOAD = 2, OP_MERGED = 3 };
constexpr int kKindShift = 28;

// A launch takes `rows` = (tree, direction of the chunk) pairs from row0 on, blockIdx.y each
struct SprArgs {
    const void *dirs;    // [n_trees][2 n_edges][pc]
    const uint64_t *w;   // [n_pat], or null
    int64_t p0, p1, pc;
    const SprOp *ops;
    const int64_t *off;  // [n_trees dc + 1]: row r has ops [off[r], off[r + 1])
    int n_edges, dc, d0; // dc directions per tree in the chunk, from direction d0
    int64_t row0;
    void *stack;         // [rows of the launch][depth][pc], or null: the stack is in LDS
    int depth;
    uint64_t *miss;      // [n_trees dc][n_edges]
};

// LDS of k_spr_score: the per-target counters, then (LDS tier) depth rows of kTB sets
__host__ __device__ inline size_t spr_lds(int n_edges, int depth, int msize) {
    return (size_t)n_edges * 8 + (size_t)depth * kTB * msize;
}

template <class M, bool LDS>
__global__ void __launch_bounds__(kTB) k_spr_score(SprArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int64_t row = a.row0 + blockIdx.y;
    const int64_t o0 = a.off[row], o1 = a.off[row + 1];
    if (o0 == o1) return;  // no valid direction: the whole workgroup leaves
    const int t = (int)(row / a.dc), dl = (int)(row % a.dc);
    unsigned long long *s_acc = reinterpret_cast<unsigned long long *>(smem);
    M *s_stack = reinterpret_cast<M *>(smem + (size_t)a.n_edges * 8);
    const SprOp *ops = a.ops + o0;
    const int n_ops = (int)(o1 - o0);
    for (int i = tid; i < n_ops; i += kTB)
        if ((ops[i].k >> kKindShift) != OP_LOAD) s_acc[ops[i].f] = 0;
    __syncthreads();

    const int64_t p = a.p0 + (int64_t)blockIdx.x * kTB + tid;
    const bool live = p < a.p1;
    const int64_t lp = p - a.p0;
    const M full = (M) ~(M)0;
    const M *dirs = static_cast<const M *>(a.dirs) + (size_t)t * 2 * a.n_edges * a.pc;
    M *g_stack = LDS ? nullptr
                     : static_cast<M *>(a.stack) + (size_t)blockIdx.y * a.depth * a.pc;
    // a lane past the range holds the full set everywhere and touches no memory
    auto D = [&](int r) -> M { return live ? dirs[(size_t)r * a.pc + lp] : full; };
    auto put = [&](int k, M v) {
        if (LDS) s_stack[k * kTB + tid] = v;
        else if (live) g_stack[(size_t)k * a.pc + lp] = v;
    };
    auto get = [&](int k) -> M {
        if (LDS) return s_stack[k * kTB + tid];
        return live ? g_stack[(size_t)k * a.pc + lp] : full;
    };
    const M Ds = D(a.d0 + dl);
    const unsigned long long wp = live ? (a.w ? a.w[p] : 1ull) : 0ull;

    for (int i = 0; i < n_ops; ++i) {
        const SprOp op = ops[i];
        const int kind = op.k >> kKindShift, k = op.k & ((1 << kKindShift) - 1);
        if (kind == OP_LOAD) {
            put(k, D(op.own));
            continue;
        }
        M Y;
        if (kind == OP_MERGED) Y = D(op.sib);
        else {
            const M S = D(op.sib), X = get(k - 1);
            const M I = S & X;
            Y = I ? I : (M)(S | X);
            if (kind == OP_PUSH) put(k, Y);
        }
        const M O = D(op.own);
        const M I = O & Y;
        const M E = I ? I : (M)(O | Y);
        const bool flag = live && (M)(Ds & E) == 0;
        const unsigned long long m = __ballot(flag);
        if (m) {  // wave-uniform
            const unsigned long long c = a.w ? wave_sum(flag ? wp : 0ull)
                                             : (unsigned long long)__popcll(m);
            if (lane == 0 && c) atomicAdd(&s_acc[op.f], c);
        }
    }
    __syncthreads();
    unsigned long long *out = reinterpret_cast<unsigned long long *>(a.miss) + row * a.n_edges;
    for (int i = tid; i < n_ops; i += kTB)
        if ((ops[i].k >> kKindShift) != OP_LOAD && s_acc[ops[i].f])
            atomicAdd(out + ops[i].f, s_acc[ops[i].f]);
}

// miss sums -> scores, in place: score[d][f] = L - miss(ea) + miss(f) on the targets, UINT64_MAX
// everywhere else.  grid (dc, trees); dynamic LDS: one flag byte per edge
struct SprFinishArgs {
    const SprOp *ops;
    const int64_t *off;
    int n_edges, dc;
    const uint64_t *len;  // [n_trees]
    uint64_t *miss;       // [n_trees dc][n_edges]
};

__global__ void __launch_bounds__(kTB) k_spr_finish(SprFinishArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = (int)threadIdx.x, t = (int)blockIdx.y;
    const int64_t row = (int64_t)t * a.dc + blockIdx.x;
    const int64_t o0 = a.off[row], o1 = a.off[row + 1];
    uint64_t *out = a.miss + row * a.n_edges;
    for (int f = tid; f < a.n_edges; f += kTB) smem[f] = 0;
    // the first op of a valid direction is the merged edge's
    const uint64_t base = o1 > o0 ? a.len[t] - out[a.ops[o0].f] : 0;
    __syncthreads();
    for (int64_t i = o0 + tid; i < o1; i += kTB) {
        const int kind = a.ops[i].k >> kKindShift;
        if (kind == OP_STEP || kind == OP_PUSH) smem[a.ops[i].f] = 1;
    }
    __syncthreads();
    for (int f = tid; f < a.n_edges; f += kTB) out[f] = smem[f] ? base + out[f] : ~(uint64_t)0;
}

// the smallest score of every tree's rows [dc][n_edges], ties to the lowest direction, then the
// lowest edge: best [n_trees][3] = (score, direction, edge).  grid (trees)
__global__ void __launch_bounds__(kTB) k_spr_argmin(const uint64_t *scores, int n_edges, int dc,
                                                    int d0, uint64_t *best) {
    __shared__ unsigned long long s_v[kTB / 64], s_i[kTB / 64];
    const int tid = (int)threadIdx.x, t = (int)blockIdx.x;
    const int64_t n = (int64_t)dc * n_edges;
    const uint64_t *s = scores + (int64_t)t * n;
    unsigned long long v = ~0ull, at = ~0ull;
    for (int64_t i = tid; i < n; i += kTB)  // ascending i: a later equal score does not replace
        if (s[i] < v) {
            v = s[i];
            at = (unsigned long long)i;
        }
    auto take = [&](unsigned long long ov, unsigned long long oi) {
        if (ov < v || (ov == v && oi < at)) {
            v = ov;
            at = oi;
        }
    };
    for (int o = 32; o; o >>= 1) {
        const unsigned long long ov = __shfl_xor(v, o), oi = __shfl_xor(at, o);
        take(ov, oi);
    }
    if ((tid & 63) == 0) {
        s_v[tid >> 6] = v;
        s_i[tid >> 6] = at;
    }
    __syncthreads();
    if (tid == 0) {
        for (int j = 1; j < kTB / 64; ++j) take(s_v[j], s_i[j]);
        best[3 * t] = v;
        best[3 * t + 1] = v == ~0ull ? 0 : (uint64_t)d0 + at / n_edges;
        best[3 * t + 2] = v == ~0ull ? 0 : at % n_edges;
    }
}

// ---- host side ---------------------------------------------------------------------------

struct ParsState : DevState {
    DevBuf<uint8_t> ws;
    DevBuf<uint8_t> stk;  // the arriving sets of k_spr_score where they do not fit in LDS
    bool prof = false;
    hipEvent_t ev[2] = {nullptr, nullptr};
    double ms = 0.0;
    bool have_ms = false;
};
ParsState g_pars[64];

// the alignment of a call: checked, and its masks and weights
struct Aln {
    int n_taxa, n_codes, K;
    int64_t n_pat;
    bool wide;  // uint32 masks
    std::vector<uint32_t> masks;
};

int check_aln(const char *fn, const uint8_t *codes, int n_taxa, int64_t n_pat, int n_codes, int K,
              const double *table, const int64_t *weights, Aln &A) {
    if (!codes || !table) return set_err(nullptr, PU_E_ARG, "%s: null buffer", fn);
    if (n_taxa < 3 || n_taxa > kParsMaxTaxa)
        return set_err(nullptr, PU_E_ARG, "%s: n_taxa = %d is outside [3, %d]", fn, n_taxa,
                       kParsMaxTaxa);
    if (n_pat < 1) return set_err(nullptr, PU_E_ARG, "%s: n_pat = %lld", fn, (long long)n_pat);
    if (K < 1 || K > kMaxStates)
        return set_err(nullptr, PU_E_ARG, "%s: n_states = %d is outside [1, %d]", fn, K,
                       kMaxStates);
    if (n_codes < 1 || n_codes > kMaxCodes)
        return set_err(nullptr, PU_E_ARG, "%s: n_codes = %d is outside [1, %d]", fn, n_codes,
                       kMaxCodes);
    A.n_taxa = n_taxa;
    A.n_codes = n_codes;
    A.K = K;
    A.n_pat = n_pat;
    A.wide = K > 8;
    A.masks.assign(n_codes, 0u);
    for (int c = 0; c < n_codes; ++c) {
        for (int k = 0; k < K; ++k)
            if (table[(size_t)c * K + k] > 0.0) A.masks[c] |= 1u << k;
        if (!A.masks[c])
            return set_err(nullptr, PU_E_ARG, "%s: code %d allows no state (an all-zero table row)",
                           fn, c);
    }
    if (int rc = check_codes(fn, codes, n_taxa, n_pat, n_codes)) return rc;
    if (weights) {
        // every sum is at most 2 n_taxa sum(w): kept below 2^63
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

template <int MODE>
void launch_fitch(bool wide, dim3 grid, size_t lds, hipStream_t st, const FitchArgs &a) {
    if (wide) hipLaunchKernelGGL((k_fitch<uint32_t, MODE>), grid, dim3(kTB), lds, st, a);
    else hipLaunchKernelGGL((k_fitch<uint8_t, MODE>), grid, dim3(kTB), lds, st, a);
}

void launch_fitch(int mode, bool wide, dim3 grid, size_t lds, hipStream_t st, const FitchArgs &a) {
    switch (mode) {
    case M_LEN: launch_fitch<M_LEN>(wide, grid, lds, st, a); break;
    case M_EDGE: launch_fitch<M_EDGE>(wide, grid, lds, st, a); break;
    case M_STEP: launch_fitch<M_STEP>(wide, grid, lds, st, a); break;
    case M_DIR: launch_fitch<M_DIR>(wide, grid, lds, st, a); break;
    default: launch_fitch<M_SETS>(wide, grid, lds, st, a); break;
    }
}

// the alignment on the device
struct DevAln {
    const uint8_t *codes = nullptr;
    const void *masks = nullptr;
    const uint64_t *w = nullptr;
    int msize = 1;
};

DevAln upload_aln(HostCall &h, const Aln &A, const uint8_t *codes, const int64_t *weights,
                  std::vector<uint8_t> &m8) {
    DevAln d;
    d.codes = h.to_device(codes, (size_t)A.n_taxa * A.n_pat);
    d.msize = A.wide ? 4 : 1;
    if (A.wide) d.masks = h.to_device(A.masks.data(), A.masks.size());
    else {
        m8.assign(A.masks.begin(), A.masks.end());
        d.masks = h.to_device(m8.data(), m8.size());
    }
    // non-negative int64 weights are the kernel's uint64 as they stand
    d.w = reinterpret_cast<const uint64_t *>(h.to_device(weights, weights ? (size_t)A.n_pat : 0));
    return d;
}

// How a call's trees and patterns are cut so that the node sets of one launch stay within kWsCap:
// pc patterns per launch (a multiple of kTB unless it is all of them) and tc trees per launch
struct Cut {
    int64_t pc, tc;
};
Cut cut_work(int n_arr, int n_ops, int msize, int64_t n_pat, int64_t n_trees) {
    const size_t per_pat = (size_t)n_arr * n_ops * msize;
    // PU_PARS_WS=bytes lowers the cap, so that a small shape is cut into pattern chunks too
    const size_t cap = (size_t)env_cap("PU_PARS_WS", (int64_t)kWsCap);
    int64_t pc = n_pat;
    if (per_pat * (size_t)pc > cap)
        pc = std::max<int64_t>(kTB, (int64_t)(cap / per_pat) / kTB * kTB);
    int64_t tc = std::max<int64_t>(1, (int64_t)(cap / (per_pat * (size_t)pc)));
    tc = env_cap("PU_PARS_CHUNK", std::min<int64_t>(std::min(tc, n_trees), 65535));  // grid.y
    return {pc, tc};
}

// event timing of a call's kernels: the launches between begin and end, summed into S.ms
struct Timed {
    ParsState &S;
    hipStream_t st;
    explicit Timed(ParsState &s, hipStream_t stream) : S(s), st(stream) {
        if (S.prof) {
            S.ms = 0.0;
            S.have_ms = true;
            for (hipEvent_t &e : S.ev)
                if (!e) (void)hipEventCreate(&e);
        }
    }
    void begin() {
        if (S.prof) (void)hipEventRecord(S.ev[0], st);
    }
    // after a wait for the stream
    void end_record() {
        if (S.prof) (void)hipEventRecord(S.ev[1], st);
    }
    void add() {
        float ms = 0.f;
        if (S.prof && hipEventSynchronize(S.ev[1]) == hipSuccess &&
            hipEventElapsedTime(&ms, S.ev[0], S.ev[1]) == hipSuccess)
            S.ms += ms;
    }
};

// ---- stepwise addition: the host's tree of one replicate ------------------------------------

// The growing tree rooted on edge 0, which always holds tip o[0]: `top` is the other end of edge
// 0, every other node v hangs below parent[v] by edge eid[v]
struct StepTree {
    int n = 0, top = -1, k = 0;  // k tips in the tree
    std::vector<int32_t> edges;  // [2n-3][2], the result
    std::vector<int> parent, eid, child;  // child [node][2]
    std::vector<int> edge_child;          // edge id -> its lower end
    std::vector<int> stack;

    void init(int n_taxa, const int32_t *o) {
        n = n_taxa;
        const int n_nodes = 2 * n - 2;
        edges.assign((size_t)(2 * n - 3) * 2, -1);
        parent.assign(n_nodes, -1);
        eid.assign(n_nodes, -1);
        child.assign((size_t)n_nodes * 2, -1);
        edge_child.assign(2 * n - 3, -1);
        for (int j = 0; j < 3; ++j) {
            edges[2 * j] = o[j];
            edges[2 * j + 1] = n;
        }
        top = n;
        parent[n] = o[0];
        eid[n] = 0;
        edge_child[0] = n;
        for (int j = 1; j < 3; ++j) {
            child[2 * n + j - 1] = o[j];
            parent[o[j]] = n;
            eid[o[j]] = j;
            edge_child[j] = o[j];
        }
        k = 3;
    }
    // tip x joins edge e: step k of DESIGN 4.22
    void insert(int x, int e) {
        const int m = n + k - 2, e1 = 2 * k - 3, e2 = 2 * k - 2;
        const int a = edges[2 * e], b = edges[2 * e + 1];
        const int v = edge_child[e], p = parent[v];  // p is the other end of e
        edges[2 * e + 1] = m;
        edges[2 * e1] = m;
        edges[2 * e1 + 1] = b;
        edges[2 * e2] = x;
        edges[2 * e2 + 1] = m;
        // m takes v's place below p
        parent[m] = p;
        if (v == top) top = m;
        else child[2 * p + (child[2 * p] == v ? 0 : 1)] = m;
        child[2 * m] = v;
        child[2 * m + 1] = x;
        parent[v] = m;
        parent[x] = m;
        eid[x] = e2;
        edge_child[e2] = x;
        if (v == b) {  // a is on the root's side: (a, m) is m's edge, (m, b) is v's
            eid[m] = e;
            eid[v] = e1;
        } else {       // b is on the root's side: (a, m) stays v's edge, (m, b) is m's
            eid[m] = e1;
            eid[v] = e;
        }
        edge_child[eid[m]] = m;
        edge_child[eid[v]] = v;
        (void)a;
        ++k;
    }
    // the k - 2 ops in post-order, the root edge and every op-order edge's id
    void emit(int32_t *ops, int32_t *root, int32_t *slot) {
        int n_out = 0;
        stack.clear();
        stack.push_back(top);
        // iterative post-order: a node is written after both subtrees
        std::vector<int> &s = stack;
        while (!s.empty()) {
            const int v = s.back();
            if (v >= 0) {
                s.back() = ~v;
                for (int j = 1; j >= 0; --j) {
                    const int c = child[2 * v + j];
                    if (c >= n) s.push_back(c);
                }
            } else {
                s.pop_back();
                const int u = ~v, l = child[2 * u], r = child[2 * u + 1];
                ops[3 * n_out] = u;
                ops[3 * n_out + 1] = l;
                ops[3 * n_out + 2] = r;
                slot[2 * n_out] = eid[l];
                slot[2 * n_out + 1] = eid[r];
                ++n_out;
            }
        }
        root[0] = parent[top];
        root[1] = top;
        slot[2 * n_out] = 0;
    }
};

// ---- SPR: the host's view of one tree -------------------------------------------

// The edge list of a tree (pu_treeform.h) with the walks and the move of the SPR calls.
struct SprTree : EdgeTree {
    // The other two edges of u than e, by edge id: ea < eb with far ends a, b
    void others(int u, int e, int &ea, int &a, int &eb, int &b) const {
        int x[2], g[2], c = 0;
        for (int j = 0; j < 3; ++j)
            if (adj[(size_t)u * 6 + 2 * j + 1] != e) {
                x[c] = adj[(size_t)u * 6 + 2 * j];
                g[c] = adj[(size_t)u * 6 + 2 * j + 1];
                ++c;
            }
        const int lo = g[0] < g[1] ? 0 : 1;
        ea = g[lo];
        a = x[lo];
        eb = g[1 - lo];
        b = x[1 - lo];
    }

    // the walk of the rest tree of direction d, appended to out; its stack depth is returned
    // (0: d is not valid, nothing appended)
    int dir_ops(int d, int radius, std::vector<SprOp> &out) {
        const int e = d >> 1, side = d & 1;
        const int u = edges[2 * e + 1 - side];
        if (u < n) return 0;
        int ea, a, eb, b;
        others(u, e, ea, a, eb, b);
        out.push_back({OP_MERGED << kKindShift, row(a, ea), row(b, eb), ea});
        int depth = 1;
        std::vector<int32_t> &todo = work;  // (child, parent, edge, sibling's row, depth k)
        todo.clear();
        auto below = [&](int v, int came, int k) {
            int x[2], g[2], c = 0;
            for (int j = 0; j < 3; ++j)
                if (adj[(size_t)v * 6 + 2 * j] != came) {
                    x[c] = adj[(size_t)v * 6 + 2 * j];
                    g[c] = adj[(size_t)v * 6 + 2 * j + 1];
                    ++c;
                }
            for (int j = 1; j >= 0; --j)
                todo.insert(todo.end(), {x[j], v, g[j], row(x[1 - j], g[1 - j]), k});
        };
        for (int end = 0; end < 2; ++end) {
            const int v = end ? b : a;
            if (v < n) continue;
            // entering a from b the set arriving is D(b -> u), and the other way round
            out.push_back({OP_LOAD << kKindShift, -1, end ? row(a, ea) : row(b, eb), -1});
            below(v, u, 1);
            while (!todo.empty()) {
                const size_t q = todo.size() - 5;
                const int c = todo[q], v2 = todo[q + 1], g = todo[q + 2], sib = todo[q + 3],
                          k = todo[q + 4];
                todo.resize(q);
                const bool push = c >= n && (radius == 0 || k < radius);
                out.push_back({k | (push ? OP_PUSH : OP_STEP) << kKindShift, sib, row(c, g), g});
                if (push) {
                    depth = std::max(depth, k + 1);
                    below(c, v2, k + 1);
                }
            }
        }
        return depth;
    }

    // the move (d, f) on a writable copy of the edge list
    static void apply(const SprTree &T, int32_t *ed, int d, int f) {
        const int e = d >> 1, side = d & 1, u = ed[2 * e + 1 - side];
        int ea, a, eb, b;
        T.others(u, e, ea, a, eb, b);
        const int x = ed[2 * f], y = ed[2 * f + 1];
        ed[2 * ea] = a;
        ed[2 * ea + 1] = b;
        ed[2 * f] = x;
        ed[2 * f + 1] = u;
        ed[2 * eb] = u;
        ed[2 * eb + 1] = y;
    }
};

// One scoring pass over a set of trees: all its launches, chunked over trees, then directions,
// then patterns.  After each (tree chunk, direction chunk) the scores are copied out, or their
// argmin is merged into best.
struct SprPass {
    HostCall &h;
    ParsState &S;
    const Aln &A;
    const DevAln &d;
    int radius;
    Timed &tm;

    // the cuts and the buffers of the call, set once by prepare(): a search's rounds share them
    int n = 0, n_ops = 0, E = 0, n_dir = 0, dc = 0;
    int64_t pc = 0, tc = 0, o_ops = 0, o_root = 0, o_slot = 0, n_int = 0;
    size_t cap = 0, lds_cap = 0, dirs_at = 0;
    std::vector<int32_t> hint;
    std::vector<SprOp> hops;
    std::vector<int64_t> hoff;
    std::vector<uint64_t> hbest;
    std::vector<SprTree> st;
    int32_t *d_int = nullptr;
    SprOp *d_ops = nullptr;
    int64_t *d_off = nullptr;
    uint64_t *d_miss = nullptr, *d_len = nullptr, *d_best = nullptr;

    SprPass(HostCall &h_, ParsState &S_, const Aln &A_, const DevAln &d_, int radius_, Timed &tm_)
        : h(h_), S(S_), A(A_), d(d_), radius(radius_), tm(tm_) {}

    // Once per call, for at most T trees per run(): how the work is cut, and every device buffer
    // of a chunk.  Later runs of fewer trees use the same chunk size and buffers.
    int prepare(int64_t T, bool want_best) {
        n = A.n_taxa;
        n_ops = n - 2;
        E = 2 * n - 3;
        n_dir = 2 * E;
        cap = (size_t)env_cap("PU_PARS_WS", (int64_t)kWsCap);
        // scores and op lists of a chunk: per tree and direction E counters and at most E ops
        const size_t per_dir = (size_t)E * (8 + sizeof(SprOp));
        dc = (int)std::min<size_t>(n_dir, std::max<size_t>(1, cap / per_dir));
        // node sets and directional sets of a chunk
        const size_t per_pat = (size_t)(2 * n_ops + n_dir) * d.msize;
        pc = A.n_pat;
        if (per_pat * (size_t)pc > cap)
            pc = std::max<int64_t>(kTB, (int64_t)(cap / per_pat) / kTB * kTB);
        tc = std::max<int64_t>(1, (int64_t)std::min(cap / (per_pat * (size_t)pc),
                                                    cap / (per_dir * (size_t)dc)));
        tc = env_cap("PU_PARS_CHUNK", std::min<int64_t>(std::min(tc, T), 65535));
        // PU_PARS_LDS=bytes lowers what the arriving sets may take of a workgroup's LDS
        lds_cap = (size_t)env_cap("PU_PARS_LDS", 65536 - 512);
        o_ops = 0;
        o_root = tc * n_ops * 3;
        o_slot = o_root + 2 * tc;
        n_int = o_slot + tc * E;
        hint.assign((size_t)n_int, 0);
        hbest.assign((size_t)tc * 3, 0);
        st.resize((size_t)tc);
        d_int = h.alloc<int32_t>((size_t)n_int);
        d_ops = h.alloc<SprOp>((size_t)tc * dc * E);
        d_off = h.alloc<int64_t>((size_t)tc * dc + 1);
        d_miss = h.alloc<uint64_t>((size_t)tc * dc * E);
        d_len = h.alloc<uint64_t>((size_t)tc);
        d_best = want_best ? h.alloc<uint64_t>((size_t)tc * 3) : nullptr;
        dirs_at = (size_t)tc * 2 * n_ops * pc * d.msize;
        if (!h.rc) h.rc = S.ws.reserve(dirs_at + (size_t)tc * n_dir * pc * d.msize);
        return h.rc;
    }

    // trees: host edge lists, at most as many as prepare() was told.  len_out [T]; scores_out
    // [T][2E][E] or null; best_out [T][3] or null (needs want_best).  With `apply_to` (the same
    // trees, writable), every tree whose best score is below its length takes that move in place:
    // the search's step.
    int run(const char *fn, const std::vector<const int32_t *> &trees, uint64_t *len_out,
            uint64_t *scores_out, uint64_t *best_out, int32_t *const *apply_to = nullptr) {
        const int64_t n_pat = A.n_pat, T = (int64_t)trees.size();
        if (best_out)
            for (int64_t t = 0; t < T; ++t) best_out[3 * t] = ~(uint64_t)0;

        for (int64_t t0 = 0; t0 < T && !h.rc; t0 += tc) {
            const int64_t nt = std::min<int64_t>(tc, T - t0);
            for (int64_t t = 0; t < nt; ++t) {
                if (int rc = st[t].build(fn, t0 + t, n, trees[t0 + t])) return h.rc = rc;
                st[t].schedule(&hint[o_ops + t * n_ops * 3], &hint[o_root + 2 * t],
                               &hint[o_slot + t * E]);
            }
            h.hip("hipMemcpyAsync", hipMemcpyAsync(d_int, hint.data(), (size_t)n_int * 4,
                                                   hipMemcpyHostToDevice, h.st));
            for (int d0 = 0; d0 < n_dir && !h.rc; d0 += dc) {
                const int dn = std::min(dc, n_dir - d0);
                hops.clear();
                hoff.assign(1, 0);
                int depth = 1;
                for (int64_t t = 0; t < nt; ++t)
                    for (int j = 0; j < dn; ++j) {
                        depth = std::max(depth, st[t].dir_ops(d0 + j, radius, hops));
                        hoff.push_back((int64_t)hops.size());
                    }
                const int64_t rows = nt * dn;
                if (!hops.empty())
                    h.hip("hipMemcpyAsync",
                          hipMemcpyAsync(d_ops, hops.data(), hops.size() * sizeof(SprOp),
                                         hipMemcpyHostToDevice, h.st));
                h.hip("hipMemcpyAsync", hipMemcpyAsync(d_off, hoff.data(), hoff.size() * 8,
                                                       hipMemcpyHostToDevice, h.st));
                h.hip("hipMemsetAsync", hipMemsetAsync(d_len, 0, (size_t)nt * 8, h.st));
                h.hip("hipMemsetAsync", hipMemsetAsync(d_miss, 0, (size_t)rows * E * 8, h.st));
                // the arriving sets: in LDS where the deepest walk of the chunk fits beside the
                // counters, else in the workspace, as many rows per launch as the cap holds
                const bool in_lds = spr_lds(E, depth, d.msize) <= lds_cap;
                int64_t rl = std::min<int64_t>(rows, 65535);
                if (!in_lds) {
                    const size_t per_row = (size_t)depth * pc * d.msize;
                    rl = std::min<int64_t>(rl, std::max<int64_t>(1, (int64_t)(cap / per_row)));
                    if (!h.rc) h.rc = S.stk.reserve((size_t)rl * per_row);
                }
                if (h.rc) break;
                tm.begin();
                for (int64_t p0 = 0; p0 < n_pat; p0 += pc) {
                    FitchArgs a{};
                    a.codes = d.codes;
                    a.masks = d.masks;
                    a.w = d.w;
                    a.n_taxa = n;
                    a.n_codes = A.n_codes;
                    a.n_ops = n_ops;
                    a.n_pat = n_pat;
                    a.p0 = p0;
                    a.p1 = std::min<int64_t>(n_pat, p0 + pc);
                    a.ops = d_int + o_ops;
                    a.ops_stride = (int64_t)n_ops * 3;
                    a.root = d_int + o_root;
                    a.slot = d_int + o_slot;
                    a.ws = S.ws.p;
                    a.pc = pc;
                    a.len = d_len;
                    a.sets = S.ws.p + dirs_at;
                    const unsigned tiles = (unsigned)((a.p1 - a.p0 + kTB - 1) / kTB);
                    launch_fitch(M_DIR, A.wide, dim3(tiles, (unsigned)nt), fitch_lds(0), h.st, a);
                    SprArgs s{};
                    s.dirs = S.ws.p + dirs_at;
                    s.w = d.w;
                    s.p0 = a.p0;
                    s.p1 = a.p1;
                    s.pc = pc;
                    s.ops = d_ops;
                    s.off = d_off;
                    s.n_edges = E;
                    s.dc = dn;
                    s.d0 = d0;
                    s.stack = in_lds ? nullptr : S.stk.p;
                    s.depth = depth;
                    s.miss = d_miss;
                    for (int64_t r0 = 0; r0 < rows; r0 += rl) {
                        s.row0 = r0;
                        const dim3 grid(tiles, (unsigned)std::min<int64_t>(rl, rows - r0));
                        const size_t lds = spr_lds(E, in_lds ? depth : 0, d.msize);
                        if (A.wide) {
                            if (in_lds) hipLaunchKernelGGL((k_spr_score<uint32_t, true>), grid,
                                                           dim3(kTB), lds, h.st, s);
                            else hipLaunchKernelGGL((k_spr_score<uint32_t, false>), grid,
                                                    dim3(kTB), lds, h.st, s);
                        } else {
                            if (in_lds) hipLaunchKernelGGL((k_spr_score<uint8_t, true>), grid,
                                                           dim3(kTB), lds, h.st, s);
                            else hipLaunchKernelGGL((k_spr_score<uint8_t, false>), grid,
                                                    dim3(kTB), lds, h.st, s);
                        }
                    }
                }
                const SprFinishArgs f{d_ops, d_off, E, dn, d_len, d_miss};
                hipLaunchKernelGGL(k_spr_finish, dim3((unsigned)dn, (unsigned)nt), dim3(kTB),
                                   (size_t)E, h.st, f);
                if (best_out)
                    hipLaunchKernelGGL(k_spr_argmin, dim3((unsigned)nt), dim3(kTB), 0, h.st,
                                       d_miss, E, dn, d0, d_best);
                h.hip(fn, hipGetLastError());
                tm.end_record();
                if (scores_out)
                    for (int64_t t = 0; t < nt; ++t)
                        h.to_host(scores_out + ((t0 + t) * n_dir + d0) * E,
                                  d_miss + (size_t)t * dn * E, (size_t)dn * E);
                if (best_out) h.to_host(hbest.data(), d_best, (size_t)nt * 3);
                if (d0 + dn >= n_dir) h.to_host(len_out + t0, d_len, (size_t)nt);
                if (h.hip(fn, hipStreamSynchronize(h.st))) break;
                tm.add();
                if (best_out)  // chunks come in ascending direction: only a smaller score replaces
                    for (int64_t t = 0; t < nt; ++t)
                        if (hbest[3 * t] < best_out[3 * (t0 + t)])
                            std::copy(&hbest[3 * t], &hbest[3 * t] + 3, best_out + 3 * (t0 + t));
            }
            // the chunk's adjacencies are still those of the trees just scored
            if (apply_to && best_out && !h.rc)
                for (int64_t t = 0; t < nt; ++t) {
                    const uint64_t *b = best_out + 3 * (t0 + t);
                    if (b[0] < len_out[t0 + t])
                        SprTree::apply(st[t], apply_to[t0 + t], (int)b[1], (int)b[2]);
                }
        }
        return h.rc;
    }
};

// the checks both SPR calls share, before any device is touched
int check_spr(const char *fn, int n_taxa, int n_trees, const int32_t *edges, int radius,
              int max_rounds) {
    if (n_trees < 1) return set_err(nullptr, PU_E_ARG, "%s: n_trees = %d", fn, n_trees);
    if (radius < 0) return set_err(nullptr, PU_E_ARG, "%s: radius = %d", fn, radius);
    if (max_rounds < 0) return set_err(nullptr, PU_E_ARG, "%s: max_rounds = %d", fn, max_rounds);
    SprTree T;
    const int64_t stride = (int64_t)(2 * n_taxa - 3) * 2;
    for (int64_t t = 0; t < n_trees; ++t)
        if (int rc = T.build(fn, t, n_taxa, edges + t * stride)) return rc;
    return PU_OK;
}

}  // namespace

extern "C" {

int pu_fitch_lengths(int device, int n_taxa, int64_t n_pat, int n_codes, int n_states,
                     const uint8_t *codes, const double *code_table, const int64_t *weights,
                     int n_trees, const int32_t *ops, const int32_t *root_edges,
                     uint64_t *lengths_out, uint32_t *pattern_changes_out,
                     uint64_t *edge_changes_out) {
    const char *fn = "pu_fitch_lengths";
    Aln A;
    int rc;
    if ((rc = check_aln(fn, codes, n_taxa, n_pat, n_codes, n_states, code_table, weights, A)))
        return rc;
    if (!ops || !root_edges || !lengths_out)
        return set_err(nullptr, PU_E_ARG, "%s: null buffer", fn);
    if (n_trees < 1) return set_err(nullptr, PU_E_ARG, "%s: n_trees = %d", fn, n_trees);
    const int n_ops = n_taxa - 2, n_edges = 2 * n_taxa - 3;
    std::vector<char> state;
    for (int64_t t = 0; t < n_trees; ++t)
        if ((rc = check_ops(fn, t, n_taxa, ops + t * n_ops * 3, root_edges + 2 * t, state)))
            return rc;
    if ((rc = check_device(device))) return rc;
    DeviceGuard g(device);
    HostCall h(device);
    if (h.rc) return h.rc;
    ParsState &S = g_pars[device];
    StateScope scope(S, h.st);
    if (scope.rc) return scope.rc;
    std::vector<uint8_t> m8;
    const DevAln d = upload_aln(h, A, codes, weights, m8);
    const int32_t *d_ops = h.to_device(ops, (size_t)n_trees * n_ops * 3);
    const int32_t *d_root = h.to_device(root_edges, (size_t)n_trees * 2);
    uint64_t *d_len = h.alloc<uint64_t>((size_t)n_trees);
    uint32_t *d_pp = pattern_changes_out ? h.alloc<uint32_t>((size_t)n_trees * n_pat) : nullptr;
    uint64_t *d_acc = edge_changes_out ? h.alloc<uint64_t>((size_t)n_trees * n_edges) : nullptr;
    const int mode = edge_changes_out ? M_EDGE : M_LEN;
    const int n_arr = mode == M_LEN ? 1 : 2;
    const Cut c = cut_work(n_arr, n_ops, d.msize, n_pat, n_trees);
    if (!h.rc) h.rc = S.ws.reserve((size_t)c.tc * n_arr * n_ops * c.pc * d.msize);
    Timed tm(S, h.st);
    if (!h.rc) {
        h.hip("hipMemsetAsync", hipMemsetAsync(d_len, 0, (size_t)n_trees * 8, h.st));
        if (d_acc)
            h.hip("hipMemsetAsync", hipMemsetAsync(d_acc, 0, (size_t)n_trees * n_edges * 8, h.st));
    }
    if (!h.rc) {
        tm.begin();
        for (int64_t t0 = 0; t0 < n_trees; t0 += c.tc) {
            const int64_t nt = std::min<int64_t>(c.tc, n_trees - t0);
            for (int64_t p0 = 0; p0 < n_pat; p0 += c.pc) {
                FitchArgs a{};
                a.codes = d.codes;
                a.masks = d.masks;
                a.w = d.w;
                a.n_taxa = n_taxa;
                a.n_codes = n_codes;
                a.n_ops = n_ops;
                a.n_pat = n_pat;
                a.p0 = p0;
                a.p1 = std::min<int64_t>(n_pat, p0 + c.pc);
                a.ops = d_ops + t0 * n_ops * 3;
                a.ops_stride = (int64_t)n_ops * 3;
                a.root = d_root + 2 * t0;
                a.ws = S.ws.p;
                a.pc = c.pc;
                a.len = d_len + t0;
                a.pp = d_pp ? d_pp + t0 * n_pat : nullptr;
                a.acc = d_acc ? d_acc + t0 * n_edges : nullptr;
                const dim3 grid((unsigned)((a.p1 - a.p0 + kTB - 1) / kTB), (unsigned)nt);
                launch_fitch(mode, A.wide, grid, fitch_lds(mode == M_LEN ? 0 : n_edges), h.st, a);
            }
        }
        h.hip(fn, hipGetLastError());
        tm.end_record();
    }
    h.to_host(lengths_out, d_len, (size_t)n_trees);
    if (d_pp) h.to_host(pattern_changes_out, d_pp, (size_t)n_trees * n_pat);
    if (d_acc) h.to_host(edge_changes_out, d_acc, (size_t)n_trees * n_edges);
    rc = h.finish(fn);
    if (!rc) tm.add();
    return rc;
}

int pu_fitch_insert_lengths(int device, int n_taxa, int64_t n_pat, int n_codes, int n_states,
                            const uint8_t *codes, const double *code_table,
                            const int64_t *weights, const int32_t *ops, const int32_t *root_edge,
                            int n_query, const uint8_t *query_codes, uint64_t *lengths_out) {
    const char *fn = "pu_fitch_insert_lengths";
    Aln A;
    int rc;
    if ((rc = check_aln(fn, codes, n_taxa, n_pat, n_codes, n_states, code_table, weights, A)))
        return rc;
    if (!ops || !root_edge || !lengths_out || !query_codes)
        return set_err(nullptr, PU_E_ARG, "%s: null buffer", fn);
    if (n_query < 1 || n_query > 65535 * kQT)
        return set_err(nullptr, PU_E_ARG, "%s: n_query = %d", fn, n_query);
    if ((rc = check_codes(fn, query_codes, n_query, n_pat, n_codes))) return rc;
    const int n_ops = n_taxa - 2, n_edges = 2 * n_taxa - 3;
    std::vector<char> state;
    if ((rc = check_ops(fn, 0, n_taxa, ops, root_edge, state))) return rc;
    if ((rc = check_device(device))) return rc;
    DeviceGuard g(device);
    HostCall h(device);
    if (h.rc) return h.rc;
    ParsState &S = g_pars[device];
    StateScope scope(S, h.st);
    if (scope.rc) return scope.rc;
    std::vector<uint8_t> m8;
    const DevAln d = upload_aln(h, A, codes, weights, m8);
    const int32_t *d_ops = h.to_device(ops, (size_t)n_ops * 3);
    const int32_t *d_root = h.to_device(root_edge, 2);
    const uint8_t *d_q = h.to_device(query_codes, (size_t)n_query * n_pat);
    uint64_t *d_len = h.alloc<uint64_t>(1);
    uint64_t *d_out = h.alloc<uint64_t>((size_t)n_query * n_edges);
    uint8_t *d_sets = h.alloc<uint8_t>((size_t)n_edges * n_pat * d.msize);
    const Cut c = cut_work(2, n_ops, d.msize, n_pat, 1);
    if (!h.rc) h.rc = S.ws.reserve((size_t)2 * n_ops * c.pc * d.msize);
    Timed tm(S, h.st);
    uint64_t len = 0;
    if (!h.rc) {
        h.hip("hipMemsetAsync", hipMemsetAsync(d_len, 0, 8, h.st));
        h.hip("hipMemsetAsync", hipMemsetAsync(d_out, 0, (size_t)n_query * n_edges * 8, h.st));
    }
    if (!h.rc) {
        tm.begin();
        for (int64_t p0 = 0; p0 < n_pat; p0 += c.pc) {
            FitchArgs a{};
            a.codes = d.codes;
            a.masks = d.masks;
            a.w = d.w;
            a.n_taxa = n_taxa;
            a.n_codes = n_codes;
            a.n_ops = n_ops;
            a.n_pat = n_pat;
            a.p0 = p0;
            a.p1 = std::min<int64_t>(n_pat, p0 + c.pc);
            a.ops = d_ops;
            a.ops_stride = (int64_t)n_ops * 3;
            a.root = d_root;
            a.ws = S.ws.p;
            a.pc = c.pc;
            a.len = d_len;
            a.sets = d_sets;
            const dim3 grid((unsigned)((a.p1 - a.p0 + kTB - 1) / kTB), 1);
            launch_fitch(M_SETS, A.wide, grid, fitch_lds(0), h.st, a);
        }
        ScoreArgs s{d_sets, d_q, d.masks, d.w, n_codes, n_query, n_edges, n_pat, d_out};
        const dim3 grid((unsigned)((n_pat + kTB - 1) / kTB), (unsigned)n_edges,
                        (unsigned)((n_query + kQT - 1) / kQT));
        if (A.wide) hipLaunchKernelGGL(k_insert_score<uint32_t>, grid, dim3(kTB), 0, h.st, s);
        else hipLaunchKernelGGL(k_insert_score<uint8_t>, grid, dim3(kTB), 0, h.st, s);
        h.hip(fn, hipGetLastError());
        tm.end_record();
    }
    h.to_host(&len, d_len, 1);
    h.to_host(lengths_out, d_out, (size_t)n_query * n_edges);
    rc = h.finish(fn);
    if (rc) return rc;
    tm.add();
    for (size_t i = 0; i < (size_t)n_query * n_edges; ++i) lengths_out[i] += len;
    return PU_OK;
}

int pu_parsimony_stepwise(int device, int n_taxa, int64_t n_pat, int n_codes, int n_states,
                          const uint8_t *codes, const double *code_table, const int64_t *weights,
                          int n_rep, const int32_t *orders, int32_t *edges_out,
                          uint64_t *step_lengths_out, uint64_t *lengths_out) {
    const char *fn = "pu_parsimony_stepwise";
    Aln A;
    int rc;
    if ((rc = check_aln(fn, codes, n_taxa, n_pat, n_codes, n_states, code_table, weights, A)))
        return rc;
    if (!orders || !edges_out || !step_lengths_out || !lengths_out)
        return set_err(nullptr, PU_E_ARG, "%s: null buffer", fn);
    if (n_rep < 1) return set_err(nullptr, PU_E_ARG, "%s: n_rep = %d", fn, n_rep);
    const int n = n_taxa, n_edges = 2 * n - 3;
    {
        std::vector<char> seen(n);
        for (int64_t r = 0; r < n_rep; ++r) {
            std::fill(seen.begin(), seen.end(), 0);
            for (int j = 0; j < n; ++j) {
                const int v = orders[r * n + j];
                if (v < 0 || v >= n || seen[v])
                    return set_err(nullptr, PU_E_ARG, "%s: order %lld is no permutation of the %d "
                                   "rows (entry %d = %d)", fn, (long long)r, n, j, v);
                seen[v] = 1;
            }
        }
    }
    if ((rc = check_device(device))) return rc;
    DeviceGuard g(device);
    HostCall h(device);
    if (h.rc) return h.rc;
    ParsState &S = g_pars[device];
    StateScope scope(S, h.st);
    if (scope.rc) return scope.rc;
    std::vector<uint8_t> m8;
    const DevAln d = upload_aln(h, A, codes, weights, m8);
    const int max_ops = n - 2;
    const Cut c = cut_work(2, max_ops, d.msize, n_pat, n_rep);
    const int64_t R = c.tc;  // replicates per chunk
    // the step's trees as one int32 block: per replicate ops [max_ops][3], root [2], slot [n_edges], x
    const int64_t o_ops = 0, o_root = R * max_ops * 3, o_slot = o_root + 2 * R,
                  o_x = o_slot + R * n_edges, n_int = o_x + R;
    std::vector<int32_t> hbuf((size_t)n_int);
    std::vector<uint64_t> hacc((size_t)R * (n_edges + 1));
    int32_t *d_int = h.alloc<int32_t>((size_t)n_int);
    uint64_t *d_acc = h.alloc<uint64_t>((size_t)R * (n_edges + 1));  // per-edge sums, then lengths
    if (!h.rc) h.rc = S.ws.reserve((size_t)R * 2 * max_ops * c.pc * d.msize);
    std::vector<StepTree> trees((size_t)R);
    Timed tm(S, h.st);
    for (int64_t r0 = 0; r0 < n_rep && !h.rc; r0 += R) {
        const int64_t nr = std::min<int64_t>(R, n_rep - r0);
        for (int64_t r = 0; r < nr; ++r) trees[r].init(n, orders + (r0 + r) * n);
        // pass k scores the tree of k tips: its length, and (k < n) the misses of o[k] on its
        // edges; the host then picks the edge and inserts
        for (int k = 3; k <= n && !h.rc; ++k) {
            const int n_ops = k - 2, ne = 2 * k - 3;
            const bool last = k == n;
            for (int64_t r = 0; r < nr; ++r) {
                trees[r].emit(&hbuf[o_ops + r * max_ops * 3], &hbuf[o_root + 2 * r],
                              &hbuf[o_slot + r * ne]);
                hbuf[o_x + r] = last ? 0 : orders[(r0 + r) * n + k];
            }
            h.hip("hipMemcpyAsync", hipMemcpyAsync(d_int, hbuf.data(), (size_t)n_int * 4,
                                                   hipMemcpyHostToDevice, h.st));
            h.hip("hipMemsetAsync", hipMemsetAsync(d_acc, 0, (size_t)R * (n_edges + 1) * 8, h.st));
            if (h.rc) break;
            tm.begin();
            for (int64_t p0 = 0; p0 < n_pat; p0 += c.pc) {
                FitchArgs a{};
                a.codes = d.codes;
                a.masks = d.masks;
                a.w = d.w;
                a.n_taxa = n;
                a.n_codes = n_codes;
                a.n_ops = n_ops;
                a.n_pat = n_pat;
                a.p0 = p0;
                a.p1 = std::min<int64_t>(n_pat, p0 + c.pc);
                a.ops = d_int + o_ops;
                a.ops_stride = (int64_t)max_ops * 3;
                a.root = d_int + o_root;
                a.slot = d_int + o_slot;
                a.x = d_int + o_x;
                a.ws = S.ws.p;
                a.pc = c.pc;
                a.acc = d_acc;
                a.len = d_acc + R * ne;
                const dim3 grid((unsigned)((a.p1 - a.p0 + kTB - 1) / kTB), (unsigned)nr);
                launch_fitch(last ? M_LEN : M_STEP, A.wide, grid, fitch_lds(last ? 0 : ne), h.st, a);
            }
            h.hip(fn, hipGetLastError());
            tm.end_record();
            h.to_host(hacc.data(), d_acc, (size_t)R * (ne + 1));
            if (h.hip(fn, hipStreamSynchronize(h.st))) break;
            tm.add();
            for (int64_t r = 0; r < nr; ++r) {
                const uint64_t len = hacc[R * ne + r];
                uint64_t *steps = step_lengths_out + (r0 + r) * (n - 2);
                if (k == 3) steps[0] = len;
                if (last) {
                    lengths_out[r0 + r] = len;
                    continue;
                }
                const uint64_t *miss = &hacc[r * ne];
                int best = 0;
                for (int e = 1; e < ne; ++e)
                    if (miss[e] < miss[best]) best = e;  // ties: the lowest edge id
                steps[k - 2] = len + miss[best];
                trees[r].insert(orders[(r0 + r) * n + k], best);
            }
        }
        if (!h.rc)
            for (int64_t r = 0; r < nr; ++r)
                std::copy(trees[r].edges.begin(), trees[r].edges.end(),
                          edges_out + (r0 + r) * n_edges * 2);
    }
    return h.finish(fn);
}

int pu_fitch_spr_scores(int device, int n_taxa, int64_t n_pat, int n_codes, int n_states,
                        const uint8_t *codes, const double *code_table, const int64_t *weights,
                        int n_trees, const int32_t *edges, int radius, uint64_t *lengths_out,
                        uint64_t *scores_out) {
    const char *fn = "pu_fitch_spr_scores";
    Aln A;
    int rc;
    if ((rc = check_aln(fn, codes, n_taxa, n_pat, n_codes, n_states, code_table, weights, A)))
        return rc;
    if (!edges || !lengths_out || !scores_out)
        return set_err(nullptr, PU_E_ARG, "%s: null buffer", fn);
    if ((rc = check_spr(fn, n_taxa, n_trees, edges, radius, 0))) return rc;
    if ((rc = check_device(device))) return rc;
    DeviceGuard g(device);
    HostCall h(device);
    if (h.rc) return h.rc;
    ParsState &S = g_pars[device];
    StateScope scope(S, h.st);
    if (scope.rc) return scope.rc;
    std::vector<uint8_t> m8;
    const DevAln d = upload_aln(h, A, codes, weights, m8);
    Timed tm(S, h.st);
    const int64_t stride = (int64_t)(2 * n_taxa - 3) * 2;
    std::vector<const int32_t *> trees;
    for (int64_t t = 0; t < n_trees; ++t) trees.push_back(edges + t * stride);
    SprPass pass(h, S, A, d, radius, tm);
    if (!h.rc && !pass.prepare(n_trees, false))
        pass.run(fn, trees, lengths_out, scores_out, nullptr);
    return h.finish(fn);
}

int pu_parsimony_spr(int device, int n_taxa, int64_t n_pat, int n_codes, int n_states,
                     const uint8_t *codes, const double *code_table, const int64_t *weights,
                     int n_trees, int32_t *edges_inout, int radius, int max_rounds,
                     uint64_t *lengths_out, int32_t *rounds_out, uint64_t *moves_out) {
    const char *fn = "pu_parsimony_spr";
    Aln A;
    int rc;
    if ((rc = check_aln(fn, codes, n_taxa, n_pat, n_codes, n_states, code_table, weights, A)))
        return rc;
    if (!edges_inout || !lengths_out || !rounds_out)
        return set_err(nullptr, PU_E_ARG, "%s: null buffer", fn);
    if ((rc = check_spr(fn, n_taxa, n_trees, edges_inout, radius, max_rounds))) return rc;
    if (moves_out && max_rounds == 0)
        return set_err(nullptr, PU_E_ARG, "%s: moves_out needs max_rounds > 0 (its rows)", fn);
    if ((rc = check_device(device))) return rc;
    DeviceGuard g(device);
    HostCall h(device);
    if (h.rc) return h.rc;
    ParsState &S = g_pars[device];
    StateScope scope(S, h.st);
    if (scope.rc) return scope.rc;
    std::vector<uint8_t> m8;
    const DevAln d = upload_aln(h, A, codes, weights, m8);
    Timed tm(S, h.st);
    const int64_t stride = (int64_t)(2 * n_taxa - 3) * 2;
    // the search works on a copy: an error leaves edges_inout as it was
    std::vector<int32_t> cur(edges_inout, edges_inout + (int64_t)n_trees * stride);
    std::vector<int> active((size_t)n_trees);
    for (int t = 0; t < n_trees; ++t) {
        active[t] = t;
        rounds_out[t] = 0;
    }
    if (moves_out) std::fill(moves_out, moves_out + (int64_t)n_trees * max_rounds * 3, 0);
    std::vector<const int32_t *> trees;
    std::vector<int32_t *> writable;
    std::vector<uint64_t> len, best;
    // the cuts and the device buffers of every round: sized once, for the first and largest set
    SprPass pass(h, S, A, d, radius, tm);
    if (!h.rc) pass.prepare(n_trees, true);
    while (!active.empty() && !h.rc) {
        trees.clear();
        writable.clear();
        for (int t : active) {
            trees.push_back(&cur[t * stride]);
            writable.push_back(&cur[t * stride]);
        }
        len.assign(active.size(), 0);
        best.assign(active.size() * 3, 0);
        // the pass applies each tree's improving move itself, on the adjacency it scored with
        if (pass.run(fn, trees, len.data(), nullptr, best.data(), writable.data())) break;
        std::vector<int> next;
        for (size_t i = 0; i < active.size(); ++i) {
            const int t = active[i];
            const uint64_t b = best[3 * i];
            lengths_out[t] = len[i];
            if (b == ~(uint64_t)0 || b >= len[i]) continue;  // no target, or no shorter neighbour
            const int dd = (int)best[3 * i + 1], f = (int)best[3 * i + 2];
            lengths_out[t] = b;
            if (moves_out) {
                uint64_t *m = moves_out + ((int64_t)t * max_rounds + rounds_out[t]) * 3;
                m[0] = (uint64_t)dd;
                m[1] = (uint64_t)f;
                m[2] = b;
            }
            if (++rounds_out[t] != max_rounds) next.push_back(t);
        }
        active.swap(next);
    }
    rc = h.finish(fn);
    if (rc) return rc;
    std::copy(cur.begin(), cur.end(), edges_inout);
    return PU_OK;
}

int pu_parsimony_profile(int device, int on) {
    if (device < 0 || device >= 64) return set_err(nullptr, PU_E_ARG, "device %d", device);
    std::lock_guard<std::mutex> lk(g_pars[device].mu);
    g_pars[device].prof = on != 0;
    g_pars[device].have_ms = false;
    return PU_OK;
}

int pu_parsimony_kernel_ms(int device, double *ms) {
    const char *fn = "pu_parsimony_kernel_ms";
    if (device < 0 || device >= 64 || !ms) return set_err(nullptr, PU_E_ARG, "%s: bad argument", fn);
    std::lock_guard<std::mutex> lk(g_pars[device].mu);
    if (!g_pars[device].have_ms) return set_err(nullptr, PU_E_STATE, "%s: nothing recorded", fn);
    *ms = g_pars[device].ms;
    return PU_OK;
}

}  // extern "C"
