// pu_simulate.hip -- alignments simulated down the context's tree on the GPU, and the C ABI
// of the simulator (pu_evolve_states, pu_simulate, pu_simulate_device).
//
// Reference behaviour (paths relative to the reference repository root):
//   evolve_states     src/simulation.pyx:63-87   child[s] ~ probs[parent[s], :, rate_class[s]]
//   weighted_choice   src/simulation.pyx:22-60   first j with cum_j > u * total
//   set_seed          src/simulation.pyx:13-19   libc srand: NOT reproduced (below)
//
// The reference draws from libc rand(), a sequential stream.  Here every draw has an address,
// (seed, global site g, draw index d), and its value is a pure function of that address
// (normative):
//     (x0, x1, x2, x3) = philox4x32_10(counter = (g lo, g hi, d, 0), key = (seed lo, seed hi))
//     u = ((x1 >> 5) * 2^26 + (x0 >> 6)) * 2^-53                       in [0, 1)
//     pick(w[0..n), u): cum_j = cum_{j-1} + w_j (plain fp64 adds in index order),
//                       r = u * cum_{n-1}, the first j with cum_j > r, else n - 1
//     d = 0 the site's rate category over the weights, d = 1 the state of root_a over the
//     frequencies, d = 2 + v the state of every other node v over row
//     P_v[category][state(parent(v))][.], P_v = P(len_v * rate)
// so a column does not depend on the launch grid, the chunking, the op order or on which
// other columns the call asked for.
//
//   k_sim_cumrows  one lane per row (node v, category, parent state): the K entries of P_v's
//                  row in the arithmetic every P builder here shares (pu_kernels.hip
//                  pmatrix_lane: evecs[i][k] * exp(evals[k] t) rounded once, then fma with
//                  ivecs[k][j] in k order), or the row of a host matrix (pu_set_model_p
//                  contexts: the provider's P), then its running sums.  Row root_a is zero.
//                  Lane 0 also cumulates the weights and the frequencies.
//   k_simulate     one lane per site.  The op index is wave-uniform (ops and node tables are
//                  read through scalar loads); ops run in reverse caller order, so a parent's
//                  state exists before its children draw.  A lane reads its row of the current
//                  edge's cumulative rows through L1 / L2 (an edge's rows are C K K 8 bytes:
//                  512 B for DNA, 12.8 KB for protein at C = 4, shared by every lane of the
//                  launch).  States of internal nodes go through a node-major uint8 buffer
//                  [n_nodes][chunk] (or the caller's nodes buffer): written once, read once
//                  per child, by the same lane, 64 consecutive bytes per wave.  Tip states go
//                  straight to the output rows.  No private array is indexed at run time.
//   k_evolve_states the single-branch seam: one lane per site, sums taken on the fly.
#include <hip/hip_runtime.h>

#include <stdlib.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "pu_ctx.h"
#include "pu_philox.h"
#include "pu_service.h"

// Built, tested and measured on gfx950 only (wave64, the launch shapes below).
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "pu_simulate.hip: gfx950 only, as the other kernel files of this library"
#endif

using namespace pu;

namespace pu {

struct SimState {
    int32_t *d_ops = nullptr;   // [n_ops][3] caller ops
    int32_t *d_info = nullptr;  // [n_nodes][2] {tip slot or -1, state kept in the node buffer}
    double *d_len = nullptr;    // [n_nodes] length of the edge above each node
    double *d_cum = nullptr;    // [n_nodes][C][K][K] cumulative rows, then [C] weights, [K] freqs
    double *d_pin = nullptr;    // host-matrix contexts: the provider's P [n_nodes][C][K][K]
    uint8_t *d_ws = nullptr;    // [n_nodes][chunk] node states of one chunk
    size_t ws_cap = 0;
    // host copies the uploads read (kept until the next change)
    std::vector<int32_t> h_ops, h_info;
    std::vector<double> h_len, h_pin;
};

}  // namespace pu

namespace {

constexpr int kSB = 256;
constexpr size_t kSimWsBytes = (size_t)256 << 20;  // the node-state workspace stays within this

struct SimArgs {
    int C, n_ops, root_a, root_b;
    uint64_t seed, first_site;  // global site of column 0 of this call
    int64_t off, n;             // this launch: columns [off, off + n)
    const int32_t *ops, *info;
    const double *cum, *cumw, *cumf;
    uint8_t *st;  // node states: node v, launch site s at st[v * st_ld + st_off + s]
    int64_t st_ld, st_off;
    uint8_t *tips;  // [n_tips][ld]
    int64_t ld;
    uint8_t *cats;  // [n_sites] or null
};

struct CumArgs {
    int C, n_nodes, root_a;
    const double *len, *rates, *evecs, *evals, *ivecs, *pin, *w, *pi;
    double *cum;
};

// the draw at address (seed, g, d): Philox4x32-10 with counter word 3 = 0 (pu_philox.h)
__device__ __forceinline__ double sim_u(uint64_t seed, uint64_t g, uint32_t d) {
    return philox_u(seed, g, d, 0u);
}

// pick over n cumulative sums in memory: the first j with cum_j > u * cum_{n-1}, else n - 1
// (descending scan: the last assignment is the smallest such j)
__device__ __forceinline__ int pick_cum(const double *__restrict__ cum, int n, double u) {
    const double r = __dmul_rn(u, cum[n - 1]);
    int idx = n - 1;
    for (int j = n - 2; j >= 0; --j)
        if (cum[j] > r) idx = j;
    return idx;
}
template <int K>
__device__ __forceinline__ int pick_row(const double *__restrict__ row, double u) {
    const double r = __dmul_rn(u, row[K - 1]);
    int idx = K - 1;
#pragma unroll
    for (int j = K - 2; j >= 0; --j)
        if (row[j] > r) idx = j;
    return idx;
}

template <int K>
__global__ void __launch_bounds__(kSB) k_sim_cumrows(CumArgs a) {
    const int e = (int)(blockIdx.x * kSB + threadIdx.x);  // row (v, c, i)
    if (e == 0) {
        double *cw = a.cum + (size_t)a.n_nodes * a.C * K * K, *cf = cw + a.C;
        double run = 0.0;
        for (int j = 0; j < a.C; ++j) cw[j] = run = j ? __dadd_rn(run, a.w[j]) : a.w[0];
        for (int j = 0; j < K; ++j) cf[j] = run = j ? __dadd_rn(run, a.pi[j]) : a.pi[0];
    }
    if (e >= a.n_nodes * a.C * K) return;
    const int m = e / K, i = e - m * K;
    const int v = m / a.C, c = m - v * a.C;
    double *out = a.cum + (size_t)e * K;
    if (v == a.root_a) {
#pragma unroll
        for (int j = 0; j < K; ++j) out[j] = 0.0;
        return;
    }
    double p[K];
    if (a.pin) {
#pragma unroll
        for (int j = 0; j < K; ++j) p[j] = a.pin[(size_t)e * K + j];
    } else {
        const double t = a.len[v] * a.rates[c];
        double ux[K];
#pragma unroll
        for (int k = 0; k < K; ++k) ux[k] = a.evecs[i * K + k] * exp(a.evals[k] * t);
#pragma unroll
        for (int j = 0; j < K; ++j) {
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < K; ++k) acc = fma(ux[k], a.ivecs[k * K + j], acc);
            p[j] = acc;
        }
    }
    double run = p[0];
    out[0] = run;
#pragma unroll
    for (int j = 1; j < K; ++j) {
        run = __dadd_rn(run, p[j]);
        out[j] = run;
    }
}

template <int K>
__global__ void __launch_bounds__(kSB) k_simulate(SimArgs a) {
    const int64_t s = (int64_t)blockIdx.x * kSB + threadIdx.x;
    if (s >= a.n) return;
    const int64_t col = a.off + s;
    const uint64_t g = a.first_site + (uint64_t)col;
    uint8_t *st = a.st + a.st_off + s;
    uint8_t *tip = a.tips + col;
    auto emit = [&](int v, int state) {
        const int slot = a.info[2 * v], keep = a.info[2 * v + 1];  // wave-uniform
        if (slot >= 0) tip[(int64_t)slot * a.ld] = (uint8_t)state;
        if (keep) st[(int64_t)v * a.st_ld] = (uint8_t)state;
    };
    auto draw = [&](int v, int parent_state, int cat) {
        const double *row = a.cum + (((size_t)v * a.C + cat) * K + parent_state) * K;
        return pick_row<K>(row, sim_u(a.seed, g, 2u + (uint32_t)v));
    };
    const int cat = pick_cum(a.cumw, a.C, sim_u(a.seed, g, 0u));
    if (a.cats) a.cats[col] = (uint8_t)cat;
    const int sa = pick_cum(a.cumf, K, sim_u(a.seed, g, 1u));
    emit(a.root_a, sa);
    emit(a.root_b, draw(a.root_b, sa, cat));
    for (int o = a.n_ops - 1; o >= 0; --o) {
        const int p = a.ops[3 * o], c1 = a.ops[3 * o + 1], c2 = a.ops[3 * o + 2];
        const int sp = st[(int64_t)p * a.st_ld];
        emit(c1, draw(c1, sp, cat));
        emit(c2, draw(c2, sp, cat));
    }
}

// src/simulation.pyx:63-87 over one branch; probs [C][K][K], any K and C up to 256
__global__ void __launch_bounds__(kSB)
    k_evolve_states(int K, int64_t n, uint64_t seed, uint64_t first_site, uint32_t d,
                    const double *__restrict__ probs, const uint8_t *__restrict__ parent,
                    const uint8_t *__restrict__ cls, uint8_t *__restrict__ child) {
    const int64_t s = (int64_t)blockIdx.x * kSB + threadIdx.x;
    if (s >= n) return;
    const double *row = probs + ((size_t)(cls ? cls[s] : 0) * K + parent[s]) * K;
    double total = row[0];
    for (int j = 1; j < K; ++j) total = __dadd_rn(total, row[j]);
    const double r = __dmul_rn(sim_u(seed, first_site + (uint64_t)s, d), total);
    double run = row[0];
    int idx = K - 1;
    for (int j = 0; j < K - 1; ++j) {
        if (run > r) {
            idx = j;
            break;
        }
        run = __dadd_rn(run, row[j + 1]);
    }
    child[s] = (uint8_t)idx;
}

int sim_state(pu_ctx *c) {
    if (c->sim) return PU_OK;
    SimState *s = new SimState;
    c->sim = s;
    const size_t nn = (size_t)c->n_nodes, kk = (size_t)c->C * c->K * c->K;
    int rc;
    if ((rc = dalloc(&c->err, &s->d_ops, 3 * nn)) || (rc = dalloc(&c->err, &s->d_info, 2 * nn)) ||
        (rc = dalloc(&c->err, &s->d_len, nn)) ||
        (rc = dalloc(&c->err, &s->d_cum, nn * kk + c->C + c->K))) {
        sim_free(c);
        return rc;
    }
    return PU_OK;
}

// sites per launch: the node-state workspace [n_nodes][chunk] within kSimWsBytes (whole waves),
// or PU_SIM_CHUNK (read at each call)
int64_t sim_chunk(const pu_ctx *c, int64_t n_sites) {
    int64_t chunk = std::max<int64_t>(64, (int64_t)(kSimWsBytes / (size_t)c->n_nodes) & ~(int64_t)63);
    if (const char *env = getenv("PU_SIM_CHUNK")) {
        const long long v = atoll(env);
        if (v > 0) chunk = v;
    }
    return std::min(chunk, n_sites);
}

// the tables and cumulative rows of the context's current schedule, lengths and model, queued
// on its stream
int sim_prepare(pu_ctx *c, bool keep_all) {
    if (c->K != 2 && c->K != 4 && c->K != 20)
        return set_err(&c->err, PU_E_ARG, "simulation: K = %d is not supported (2, 4, 20)", c->K);
    if (int rc = sim_state(c)) return rc;
    SimState *s = c->sim;
    const int nn = c->n_nodes;
    std::vector<int32_t> info(2 * (size_t)nn);
    for (int v = 0; v < nn; ++v) {
        info[2 * v] = c->tip_slot[v];
        info[2 * v + 1] = keep_all;
    }
    for (int o = 0; o < c->n_ops; ++o) info[2 * c->ops_in[3 * o] + 1] = 1;  // read by its children
    // the lengths pu_get_branch_lengths returns (up_len is ahead of the device's copy after
    // pu_optimise_edge / pu_minimise_edge; nothing of the context is touched here)
    std::vector<double> len(c->up_len.begin(), c->up_len.end());
    len[c->root_a] = 0.0;
    hipStream_t st = c->stream;
    // the tables are uploaded from the state's own host copies, and only when they changed: a
    // repeated call on the same tree queues kernels alone
    if (c->ops_in != s->h_ops || info != s->h_info || len != s->h_len) {
        HIPCHK(&c->err, hipStreamSynchronize(st));  // earlier copies have read the host copies
        s->h_ops = c->ops_in;
        s->h_info = info;
        s->h_len = len;
        if (c->n_ops)
            HIPCHK(&c->err, hipMemcpyAsync(s->d_ops, s->h_ops.data(), 3 * (size_t)c->n_ops * 4,
                                           hipMemcpyHostToDevice, st));
        HIPCHK(&c->err, hipMemcpyAsync(s->d_info, s->h_info.data(), s->h_info.size() * 4,
                                       hipMemcpyHostToDevice, st));
        HIPCHK(&c->err, hipMemcpyAsync(s->d_len, s->h_len.data(), s->h_len.size() * 8,
                                       hipMemcpyHostToDevice, st));
    }
    if (c->host_p) {  // the provider's P at every node's length (order 0)
        HIPCHK(&c->err, hipStreamSynchronize(st));
        s->h_pin.resize((size_t)nn * c->C * c->K * c->K);
        if (int rc = provide(c, 0, nn, len.data(), s->h_pin.data())) return rc;
        if (!s->d_pin)
            if (int rc = dalloc(&c->err, &s->d_pin, s->h_pin.size())) return rc;
        HIPCHK(&c->err, hipMemcpyAsync(s->d_pin, s->h_pin.data(), s->h_pin.size() * 8,
                                       hipMemcpyHostToDevice, st));
    }
    CumArgs a;
    a.C = c->C;
    a.n_nodes = nn;
    a.root_a = c->root_a;
    a.len = s->d_len;
    a.rates = c->d_rates;
    a.evecs = c->d_evecs;
    a.evals = c->d_evals;
    a.ivecs = c->d_ivecs;
    a.pin = c->host_p ? s->d_pin : nullptr;
    a.w = c->d_logw + c->C;
    a.pi = c->d_pi;
    a.cum = s->d_cum;
    const int grid = (int)(((size_t)nn * c->C * c->K + kSB - 1) / kSB);
    if (c->K == 2) hipLaunchKernelGGL(k_sim_cumrows<2>, dim3(grid), dim3(kSB), 0, st, a);
    else if (c->K == 4) hipLaunchKernelGGL(k_sim_cumrows<4>, dim3(grid), dim3(kSB), 0, st, a);
    else hipLaunchKernelGGL(k_sim_cumrows<20>, dim3(grid), dim3(kSB), 0, st, a);
    HIPCHK(&c->err, hipGetLastError());
    return PU_OK;
}

int sim_check(pu_ctx *c, int64_t first_site, int64_t n_sites, const uint8_t *tips, int64_t ld,
              const uint8_t *nodes, int64_t ld_nodes) {
    if (!c) return set_err(nullptr, PU_E_ARG, "null context");
    if (n_sites <= 0 || first_site < 0)
        return set_err(&c->err, PU_E_ARG, "simulation: n_sites = %lld, first_site = %lld",
                       (long long)n_sites, (long long)first_site);
    if (!tips) return set_err(&c->err, PU_E_ARG, "simulation: null tips output");
    if (ld < n_sites || (nodes && ld_nodes < n_sites))
        return set_err(&c->err, PU_E_ARG, "simulation: row stride below n_sites = %lld",
                       (long long)n_sites);
    if (!c->have_model) return set_err(&c->err, PU_E_STATE, "pu_set_model not called");
    if (!c->have_sched) return set_err(&c->err, PU_E_STATE, "pu_set_schedule not called");
    if (c->host_p && !c->pm_fn)
        return set_err(&c->err, PU_E_STATE, "this context runs on host transition matrices: "
                       "pu_set_pmatrix_provider first");
    return PU_OK;
}

}  // namespace

void pu::sim_free(pu_ctx *c) {
    SimState *s = c->sim;
    if (!s) return;
    dfree(s->d_ops);
    dfree(s->d_info);
    dfree(s->d_len);
    dfree(s->d_cum);
    dfree(s->d_pin);
    dfree(s->d_ws);
    delete s;
    c->sim = nullptr;
}

extern "C" {

int pu_simulate_device(pu_ctx *c, uint64_t seed, int64_t first_site, int64_t n_sites,
                       uint8_t *d_tips, int64_t ld, uint8_t *d_cats, uint8_t *d_nodes,
                       int64_t ld_nodes) {
    if (int rc = sim_check(c, first_site, n_sites, d_tips, ld, d_nodes, ld_nodes)) return rc;
    DeviceGuard g(c->device);
    if (int rc = sim_prepare(c, d_nodes != nullptr)) return rc;
    SimState *s = c->sim;
    const int64_t chunk = sim_chunk(c, n_sites);
    if (!d_nodes) {
        const size_t need = (size_t)c->n_nodes * (size_t)chunk;
        if (s->ws_cap < need) {
            dfree(s->d_ws);  // waits for the launches that used it
            s->ws_cap = 0;
            if (int rc = dalloc(&c->err, &s->d_ws, need)) return rc;
            s->ws_cap = need;
        }
    }
    SimArgs a;
    a.C = c->C;
    a.n_ops = c->n_ops;
    a.root_a = c->root_a;
    a.root_b = c->root_b;
    a.seed = seed;
    a.first_site = (uint64_t)first_site;
    a.ops = s->d_ops;
    a.info = s->d_info;
    a.cum = s->d_cum;
    a.cumw = s->d_cum + (size_t)c->n_nodes * c->C * c->K * c->K;
    a.cumf = a.cumw + c->C;
    a.st = d_nodes ? d_nodes : s->d_ws;
    a.st_ld = d_nodes ? ld_nodes : chunk;
    a.tips = d_tips;
    a.ld = ld;
    a.cats = d_cats;
    for (int64_t off = 0; off < n_sites; off += chunk) {
        a.off = off;
        a.n = std::min(chunk, n_sites - off);
        a.st_off = d_nodes ? off : 0;
        const dim3 grid((unsigned)((a.n + kSB - 1) / kSB));
        if (c->K == 2) hipLaunchKernelGGL(k_simulate<2>, grid, dim3(kSB), 0, c->stream, a);
        else if (c->K == 4) hipLaunchKernelGGL(k_simulate<4>, grid, dim3(kSB), 0, c->stream, a);
        else hipLaunchKernelGGL(k_simulate<20>, grid, dim3(kSB), 0, c->stream, a);
        HIPCHK(&c->err, hipGetLastError());
    }
    return PU_OK;
}

int pu_simulate(pu_ctx *c, uint64_t seed, int64_t first_site, int64_t n_sites, uint8_t *tips_out,
                uint8_t *cats_out, uint8_t *nodes_out, double *cum_out) {
    if (int rc = sim_check(c, first_site, n_sites, tips_out, n_sites, nullptr, 0)) return rc;
    DeviceGuard g(c->device);
    const size_t n = (size_t)n_sites, nt = (size_t)c->n_tips * n, nv = (size_t)c->n_nodes * n;
    HostCall h(c->stream, &c->err);
    uint8_t *d_t = h.alloc<uint8_t>(nt);
    uint8_t *d_c = cats_out ? h.alloc<uint8_t>(n) : nullptr;
    uint8_t *d_n = nodes_out ? h.alloc<uint8_t>(nv) : nullptr;
    // a declared tip that the schedule does not reach keeps state 0
    if (!h.rc) h.hip("hipMemsetAsync", hipMemsetAsync(d_t, 0, nt, h.st));
    if (!h.rc && d_n) h.hip("hipMemsetAsync", hipMemsetAsync(d_n, 0, nv, h.st));
    if (!h.rc)
        h.rc = pu_simulate_device(c, seed, first_site, n_sites, d_t, n_sites, d_c, d_n, n_sites);
    h.to_host(tips_out, d_t, nt);
    if (cats_out) h.to_host(cats_out, d_c, n);
    if (nodes_out) h.to_host(nodes_out, d_n, nv);
    if (!h.rc && cum_out)
        h.to_host(cum_out, c->sim->d_cum, (size_t)c->n_nodes * c->C * c->K * c->K);
    return h.finish("pu_simulate");
}

int pu_evolve_states(int device, int K, int C, int64_t n_sites, uint64_t seed,
                     int64_t first_site, uint32_t draw, const double *probs,
                     const uint8_t *parent_states, const uint8_t *rate_class,
                     uint8_t *child_states_out) {
    if (K < 1 || K > 256 || C < 1 || C > 256 || n_sites <= 0 || first_site < 0)
        return set_err(nullptr, PU_E_ARG, "pu_evolve_states: bad shape K=%d C=%d n_sites=%lld "
                       "first_site=%lld", K, C, (long long)n_sites, (long long)first_site);
    if (!probs || !parent_states || !child_states_out || (C > 1 && !rate_class))
        return set_err(nullptr, PU_E_ARG, "pu_evolve_states: null buffer");
    for (int64_t s = 0; s < n_sites; ++s)
        if (parent_states[s] >= K || (rate_class && rate_class[s] >= C))
            return set_err(nullptr, PU_E_ARG, "pu_evolve_states: site %lld: parent state %d / "
                           "rate class %d out of range", (long long)s, (int)parent_states[s],
                           rate_class ? (int)rate_class[s] : 0);
    int rc = check_device(device);
    if (rc) return rc;
    DeviceGuard g(device);
    std::lock_guard<std::mutex> lk(ws_mutex(device));
    const size_t nP = (size_t)C * K * K, n = (size_t)n_sites;
    double *w;
    hipStream_t st;
    if ((rc = ws_get(device, nP + 3 * ((n + 7) / 8), &w, &st))) return rc;
    uint8_t *dpar = reinterpret_cast<uint8_t *>(w + nP), *dcls = dpar + (n + 7) / 8 * 8,
            *dout = dcls + (n + 7) / 8 * 8;
    HIPCHK(nullptr, hipMemcpyAsync(w, probs, nP * 8, hipMemcpyHostToDevice, st));
    HIPCHK(nullptr, hipMemcpyAsync(dpar, parent_states, n, hipMemcpyHostToDevice, st));
    if (rate_class) HIPCHK(nullptr, hipMemcpyAsync(dcls, rate_class, n, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_evolve_states, dim3((unsigned)((n + kSB - 1) / kSB)), dim3(kSB), 0, st, K,
                       n_sites, seed, (uint64_t)first_site, draw, w, dpar,
                       rate_class ? dcls : nullptr, dout);
    HIPCHK(nullptr, hipGetLastError());
    HIPCHK(nullptr, hipMemcpyAsync(child_states_out, dout, n, hipMemcpyDeviceToHost, st));
    HIPCHK(nullptr, hipStreamSynchronize(st));
    return PU_OK;
}

}  // extern "C"
