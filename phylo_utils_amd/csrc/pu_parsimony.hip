// pu_parsimony.hip -- Fitch parsimony on the device: the lengths of a batch of
// trees, the exact insertion lengths of query rows on every edge of a tree, and randomised
// stepwise-addition trees.  Stateless calls on the host layer of pu_service.h.  The reference
// project has no parsimony; the rule is DESIGN 4.22's, restated in tests/parsimony_reference.py.
//
// One lane owns one site pattern and walks the tree's op list, so a tree has no dependency across
// lanes; the tree (or replicate) and the pattern tile are the grid.  State sets are bit masks
// (uint8 for K <= 8, else uint32).  Every sum is an unsigned 64-bit integer: per wave a ballot and
// a popcount (unit weights) or a shuffle sum, per workgroup an LDS counter, then one 64-bit atomic
// add per edge and workgroup -- no result depends on the launch shape or on the chunking.
#include "pu_ctx.h"
#include "pu_service.h"

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
    void *sets;             // M_SETS: [2 n_ops + 1][n_pat] edge sets of tree 0
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

// ---- host side ---------------------------------------------------------------------------

struct ParsState : DevState {
    DevBuf<uint8_t> ws;
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

// ops [n_ops][3] with root edge (ra, rb) is a post-order of a binary tree whose tips are exactly
// rows 0..n_taxa-1 and whose internal nodes are n_taxa..2 n_taxa-3
int check_ops(const char *fn, int64_t t, int n_taxa, const int32_t *ops, const int32_t *root,
              std::vector<char> &state) {
    const int n_nodes = 2 * n_taxa - 2;
    // 0 not made yet, 1 made (tips are made), 2 has a parent
    state.assign(n_nodes, 0);
    std::fill(state.begin(), state.begin() + n_taxa, 1);
    for (int i = 0; i < n_taxa - 2; ++i) {
        const int par = ops[3 * i], l = ops[3 * i + 1], r = ops[3 * i + 2];
        if (par < n_taxa || par >= n_nodes || state[par] != 0)
            return set_err(nullptr, PU_E_ARG, "%s: tree %lld op %d: parent %d is no new internal "
                           "node of [%d, %d)", fn, (long long)t, i, par, n_taxa, n_nodes);
        for (int c : {l, r}) {
            if (c < 0 || c >= n_nodes || state[c] != 1)
                return set_err(nullptr, PU_E_ARG, "%s: tree %lld op %d: child %d is not made yet "
                               "or has a parent already (not a post-order of a binary tree)", fn,
                               (long long)t, i, c);
            state[c] = 2;
        }
        state[par] = 1;
    }
    const int ra = root[0], rb = root[1];
    if (ra < 0 || rb < 0 || ra >= n_nodes || rb >= n_nodes || ra == rb || state[ra] != 1 ||
        state[rb] != 1)
        return set_err(nullptr, PU_E_ARG, "%s: tree %lld: root edge (%d, %d) does not join the two "
                       "nodes left without a parent", fn, (long long)t, ra, rb);
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
