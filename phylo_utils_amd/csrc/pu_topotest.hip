// pu_topotest.hip -- topology tests of candidate trees on the GPU (normative): the
// replicate counts behind RELL bootstrap proportions, the KH and SH tests, expected likelihood
// weights and the multiscale bootstrap of the AU test, stateless like the pu_boot_* calls, and
// the C ABI of it (pu_topology_tests, pu_topotest_profile, pu_topotest_kernel_ms).
//
// The reference has no topology test; the rule is this project's own.  L [T][S] holds the
// unweighted per-pattern lnL of T trees, w the integer pattern weights with N = sum w.  Block 0
// draws n_0 = N columns per replicate, block k >= 1 n_k = floor(r_k N + 0.5); replicate i of
// block k is global replicate first_rep + k R + i of pu_boot_weights_scaled's rule.  With
// B[r][t] = pu_rell_sums(W[r], L[t]), l_t = B(w, L[t]) and c_t[r] = B[r][t] - l_t (a tree whose
// l_t is not finite is excluded: c_t = -inf, it never wins, its counts are 0):
//     best[k][t] = #{r in block k : t = argmax_u B[r][u] over the included trees, lowest t}
//     kh[t]      = #{r in block 0 : c_u*[r] - c_t[r] >= l_u* - l_t}, u* = argmax_{u != t} l_u
//     sh[t]      = #{r in block 0 : max_u c_u[r] - c_t[r] >= max_u l_u - l_t}
// Every compared value is one fp64 subtraction of sums whose order is fixed (pu_rell.hip), and the
// counts are integers: nothing depends on the grid, the ranges or the order of the adds.  The
// file is compiled with contraction off.
//
//   k_topo_counts   one thread per replicate row, 256 rows per workgroup, all of one block.  The
//                   rows of B are [rows][ldo], so a thread walking its own row would read ldo
//                   doubles apart from its neighbours: the workgroup instead stages 256 rows x
//                   16 trees at a time through LDS -- 16 lanes read 128 contiguous bytes of a
//                   row, the tile is [256][17] doubles, whose odd stride keeps the row-per-lane
//                   reads off each other's banks -- once for the argmax, max_u c_u and the c of
//                   the two best trees by l, and in block 0 once more for the flags of every
//                   tree.  A wave votes on a tree's flag (all its lanes look at the same tree)
//                   and one lane adds the vote to the workgroup's LDS counters [3][T]; these
//                   are flushed with global integer atomics.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdlib.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "pu_ctx.h"
#include "pu_service.h"

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "pu_topotest.hip: gfx950 only, as the other kernel files of this library"
#endif

using namespace pu;

namespace {

constexpr int kMaxT = 1024;   // trees of a call: the LDS counters
constexpr int kRows = 256;    // replicate rows per workgroup, one per thread
constexpr int kTC = 16;       // trees per staged chunk
constexpr int kTs = kTC + 1;  // LDS row stride of the tile (doubles): odd
constexpr int64_t kMaxN = 0x7fffffff;
constexpr size_t kRangeBytes = (size_t)256 << 20;  // W, and B, of one range of rows

struct TopoArgs {
    const double *B;    // [n_rows][ldo]: this launch's rows, all of one block
    int64_t ldo;
    const double *lnl;  // [T]
    int n_rows, T;
    int b1, b2;         // the best and the second best tree by l (-inf for a non-finite l)
    int tests;          // block 0: kh and sh too
    uint32_t *counts;   // [3][T] of this block: best, kh, sh
};

__device__ __forceinline__ void stage(const TopoArgs &a, int64_t r0, int t0, double *tile) {
    const int tid = (int)threadIdx.x, col = tid % kTC;
    for (int row = tid / kTC; row < kRows; row += kRows / kTC) {
        const bool in = r0 + row < a.n_rows && t0 + col < a.T;
        tile[row * kTs + col] = in ? a.B[(r0 + row) * a.ldo + t0 + col] : 0.0;
    }
}

__global__ void __launch_bounds__(kRows) k_topo_counts(TopoArgs a) {
    __shared__ double tile[kRows * kTs];
    __shared__ uint32_t cnt[3 * kMaxT];
    const int tid = (int)threadIdx.x, lane = tid & 63, T = a.T;
    const int64_t r0 = (int64_t)blockIdx.x * kRows;
    const bool live = r0 + tid < a.n_rows;
    for (int i = tid; i < 3 * T; i += kRows) cnt[i] = 0u;
    const double *mine = tile + tid * kTs;
    int best = -1;
    double best_b = -INFINITY, c_max = -INFINITY, c_b1 = -INFINITY, c_b2 = -INFINITY;
    for (int t0 = 0; t0 < T; t0 += kTC) {
        __syncthreads();  // the previous chunk has been consumed (and cnt zeroed)
        stage(a, r0, t0, tile);
        __syncthreads();
        for (int j = 0; j < min(kTC, T - t0); ++j) {
            const int t = t0 + j;
            const double l = a.lnl[t];
            if (!isfinite(l)) continue;  // excluded: the same for every lane
            const double b = mine[j], c = b - l;
            if (best < 0 || b > best_b) {
                best = t;
                best_b = b;
            }
            c_max = fmax(c_max, c);
            c_b1 = t == a.b1 ? c : c_b1;
            c_b2 = t == a.b2 ? c : c_b2;
        }
    }
    if (live && best >= 0) atomicAdd(&cnt[best], 1u);
    if (a.tests) {
        const double l1 = a.lnl[a.b1], l2 = a.lnl[a.b2];
        const double l_b1 = isfinite(l1) ? l1 : -INFINITY, l_b2 = isfinite(l2) ? l2 : -INFINITY;
        for (int t0 = 0; t0 < T; t0 += kTC) {
            __syncthreads();
            stage(a, r0, t0, tile);
            __syncthreads();
            for (int j = 0; j < min(kTC, T - t0); ++j) {
                const int t = t0 + j;
                const double l = a.lnl[t];
                if (!isfinite(l)) continue;
                const double c = mine[j] - l;
                const double c_u = t == a.b1 ? c_b2 : c_b1, l_u = t == a.b1 ? l_b2 : l_b1;
                const bool kh = live && c_u - c >= l_u - l;
                const bool sh = live && c_max - c >= l_b1 - l;
                const int n_kh = __popcll(__ballot(kh)), n_sh = __popcll(__ballot(sh));
                if (lane == 0) {
                    if (n_kh) atomicAdd(&cnt[T + t], (uint32_t)n_kh);
                    if (n_sh) atomicAdd(&cnt[2 * T + t], (uint32_t)n_sh);
                }
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < (a.tests ? 3 : 1) * T; i += kRows)
        if (cnt[i]) atomicAdd(a.counts + i, cnt[i]);
}

// ---- host side ----------------------------------------------------------------------------

// events of a profiled call: 4 per range (start, after the weights, the sums, the counts)
struct TopoProfile {
    std::mutex mu;
    bool on = false;
    std::vector<hipEvent_t> ev;
    int n_ev = 0;
    int reserve(int64_t n_ranges) {
        n_ev = 0;
        while (on && (int64_t)ev.size() < 4 * n_ranges) {
            hipEvent_t e;
            HIPCHK(nullptr, hipEventCreate(&e));
            ev.push_back(e);
        }
        return PU_OK;
    }
    int mark(int phase, hipStream_t st) {
        if (!on) return PU_OK;
        HIPCHK(nullptr, hipEventRecord(ev[n_ev + phase], st));
        if (phase == 3) n_ev += 4;
        return PU_OK;
    }
};
TopoProfile g_prof[64];

}  // namespace

extern "C" {

int pu_topology_tests(int device, int T, int64_t S, const double *L, const double *site_weights,
                      uint64_t seed, int64_t first_rep, int R, int K, const double *scales,
                      uint32_t *counts_out, double *lnl_out, int64_t *n_draw_out,
                      double *rell_out) {
    const char *fn = "pu_topology_tests";
    if (!L || !site_weights || !counts_out || !lnl_out || !n_draw_out)
        return set_err(nullptr, PU_E_ARG, "%s: null buffer (L, site_weights, counts_out, lnl_out "
                       "or n_draw_out)", fn);
    if (T < 2 || T > kMaxT)
        return set_err(nullptr, PU_E_ARG, "%s: T = %d is outside [2, %d]", fn, T, kMaxT);
    if (S < 1) return set_err(nullptr, PU_E_ARG, "%s: S = %lld", fn, (long long)S);
    if (R < 1) return set_err(nullptr, PU_E_ARG, "%s: R = %d", fn, R);
    if (K < 0) return set_err(nullptr, PU_E_ARG, "%s: K = %d", fn, K);
    if (K > 0 && !scales) return set_err(nullptr, PU_E_ARG, "%s: null buffer (scales)", fn);
    int64_t N = 0;
    for (int64_t s = 0; s < S; ++s) {
        const double x = site_weights[s];
        if (!(x >= 0.0) || !(x <= (double)kMaxN) || x != floor(x))
            return set_err(nullptr, PU_E_ARG, "%s: site_weights[%lld] = %g is not an integer in "
                           "[0, 2^31 - 1]", fn, (long long)s, x);
        N = std::min<int64_t>(N + (int64_t)x, (int64_t)1 << 32);
    }
    if (N < 1 || N > kMaxN)
        return set_err(nullptr, PU_E_ARG, "%s: site_weights sum to %s, outside [1, 2^31 - 1]", fn,
                       N < 1 ? "0" : "more than 2^31 - 1");
    std::vector<int64_t> n_draw((size_t)K + 1, N);
    for (int k = 1; k <= K; ++k) {
        const double r = scales[k - 1];
        if (!std::isfinite(r) || !(r > 0.0))
            return set_err(nullptr, PU_E_ARG, "%s: scales[%d] = %g", fn, k - 1, r);
        const double n = floor(r * (double)N + 0.5);  // two roundings: contraction is off
        if (!(n >= 1.0) || !(n <= (double)kMaxN))
            return set_err(nullptr, PU_E_ARG, "%s: scales[%d] = %g draws %.0f columns, outside "
                           "[1, 2^31 - 1]", fn, k - 1, r, n);
        n_draw[k] = (int64_t)n;
    }
    const int64_t rows = ((int64_t)K + 1) * R;
    if (first_rep < 0 || first_rep + rows > ((int64_t)1 << 32))
        return set_err(nullptr, PU_E_ARG, "%s: first_rep = %lld: replicates %lld .. %lld are "
                       "outside [0, 2^32)", fn, (long long)first_rep, (long long)first_rep,
                       (long long)(first_rep + rows - 1));
    int rc;
    if ((rc = check_device(device))) return rc;
    DeviceGuard g(device);
    TopoProfile &P = g_prof[device];
    std::lock_guard<std::mutex> plk(P.mu);
    HostCall h(device);
    hipStream_t st = h.st;
    // the range: rows of W, and of B, within 256 MiB each
    const int64_t ld = (S + 63) & ~(int64_t)63;
    int64_t RC = std::max<int64_t>(1, (int64_t)std::min(kRangeBytes / (4 * (size_t)ld),
                                                         kRangeBytes / (8 * (size_t)T)));
    RC = env_cap("PU_TOPO_REP_CHUNK", std::min(RC, rows));
    std::vector<uint32_t> w32((size_t)S);
    for (int64_t s = 0; s < S; ++s) w32[s] = (uint32_t)site_weights[s];
    std::vector<int64_t> row_draw((size_t)rows);
    for (int64_t i = 0; i < rows; ++i) row_draw[i] = n_draw[i / R];
    const double *d_L = h.to_device(L, (size_t)T * S);
    const double *d_sw = h.to_device(site_weights, (size_t)S);
    const uint32_t *d_w32 = h.to_device(w32.data(), (size_t)S);
    const int64_t *d_draw = h.to_device(row_draw.data(), (size_t)rows);
    uint32_t *d_W = h.alloc<uint32_t>((size_t)RC * ld);
    double *d_B = h.alloc<double>((size_t)RC * T);
    double *d_lnl = h.alloc<double>((size_t)T);
    const size_t n_cnt = (size_t)(K + 1) * 3 * T;
    uint32_t *d_cnt = h.alloc<uint32_t>(n_cnt);
    // a buffer that does not fit: PU_E_NOMEM, the message naming its bytes (dalloc)
    if (h.rc) return h.finish(fn);
    if ((h.rc = P.reserve((rows + RC - 1) / RC))) return h.finish(fn);
    // l_t, and from it the two best trees: the only value the host reads back in mid-call
    h.rc = pu_rell_sums_device(device, st, T, S, d_L, S, 1, d_w32, ld, d_lnl, T);
    h.to_host(lnl_out, d_lnl, (size_t)T);
    h.hip(fn, hipMemsetAsync(d_cnt, 0, n_cnt * 4, st));
    if (h.rc) return h.finish(fn);
    h.hip(fn, hipStreamSynchronize(st));
    if (h.rc) return h.finish(fn);
    int b1 = -1, b2 = -1;
    auto key = [&](int t) { return std::isfinite(lnl_out[t]) ? lnl_out[t] : -INFINITY; };
    for (int t = 0; t < T; ++t)
        if (b1 < 0 || key(t) > key(b1)) b1 = t;
    for (int t = 0; t < T; ++t)
        if (t != b1 && (b2 < 0 || key(t) > key(b2))) b2 = t;
    const int64_t most = *std::max_element(n_draw.begin(), n_draw.end());  // sizes the grid
    for (int64_t q0 = 0; q0 < rows && !h.rc; q0 += RC) {
        const int64_t nr = std::min(RC, rows - q0);
        h.rc = P.mark(0, st);
        if (!h.rc)
            h.rc = pu_boot_weights_scaled_device(device, st, seed, first_rep + q0, (int)nr, S, d_sw,
                                                 most, d_draw + q0, d_W, ld);
        if (!h.rc) h.rc = P.mark(1, st);
        if (!h.rc) h.rc = pu_rell_sums_device(device, st, T, S, d_L, S, (int)nr, d_W, ld, d_B, T);
        if (!h.rc) h.rc = P.mark(2, st);
        // one launch per block the range touches: a workgroup's counters belong to one block
        for (int64_t q = q0; q < q0 + nr && !h.rc;) {
            const int64_t k = q / R, end = std::min(q0 + nr, (k + 1) * R);
            TopoArgs a;
            a.B = d_B + (q - q0) * T;
            a.ldo = T;
            a.lnl = d_lnl;
            a.n_rows = (int)(end - q);
            a.T = T;
            a.b1 = b1;
            a.b2 = b2;
            a.tests = k == 0;
            a.counts = d_cnt + (size_t)k * 3 * T;
            hipLaunchKernelGGL(k_topo_counts, dim3((unsigned)((a.n_rows + kRows - 1) / kRows)),
                               dim3(kRows), 0, st, a);
            h.hip(fn, hipGetLastError());
            q = end;
        }
        if (!h.rc) h.rc = P.mark(3, st);
        if (rell_out) h.to_host(rell_out + (size_t)q0 * T, d_B, (size_t)nr * T);
    }
    h.to_host(counts_out, d_cnt, n_cnt);
    if ((rc = h.finish(fn))) return rc;
    std::copy(n_draw.begin(), n_draw.end(), n_draw_out);
    return PU_OK;
}

int pu_topotest_profile(int device, int on) {
    if (device < 0 || device >= 64) return set_err(nullptr, PU_E_ARG, "device %d", device);
    std::lock_guard<std::mutex> lk(g_prof[device].mu);
    g_prof[device].on = on != 0;
    g_prof[device].n_ev = 0;
    return PU_OK;
}

int pu_topotest_kernel_ms(int device, double *weights_ms, double *rell_ms, double *counts_ms) {
    const char *fn = "pu_topotest_kernel_ms";
    if (device < 0 || device >= 64 || !weights_ms || !rell_ms || !counts_ms)
        return set_err(nullptr, PU_E_ARG, "%s: bad argument", fn);
    TopoProfile &P = g_prof[device];
    std::lock_guard<std::mutex> lk(P.mu);
    if (!P.n_ev) return set_err(nullptr, PU_E_STATE, "%s: nothing recorded", fn);
    DeviceGuard g(device);
    HIPCHK(nullptr, hipEventSynchronize(P.ev[P.n_ev - 1]));
    double ms[3] = {0.0, 0.0, 0.0};
    for (int i = 0; i < P.n_ev; i += 4)
        for (int k = 0; k < 3; ++k) {
            float x = 0.f;
            HIPCHK(nullptr, hipEventElapsedTime(&x, P.ev[i + k], P.ev[i + k + 1]));
            ms[k] += x;
        }
    *weights_ms = ms[0];
    *rell_ms = ms[1];
    *counts_ms = ms[2];
    return PU_OK;
}

}  // extern "C"
