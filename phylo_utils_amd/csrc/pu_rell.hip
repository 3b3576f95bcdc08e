// pu_rell.hip -- RELL sums (resampling of estimated log-likelihoods, Kishino et al. 1990) on
// the GPU, stateless like the pu_boot_* calls, and the C ABI of it (pu_rell_sums[_device]):
//     out[r][v] = B(W[r], L[v]) = sum_p W[r][p] L[v][p],   a pattern with W[r][p] == 0 adds
// nothing, whatever L[v][p] is (-inf and NaN included).  An (n_rep x S) . (S x n_vec) product
// in fp64 whose left factor is the uint32 weight matrix of pu_boot_weights.
//
// The sum order is a function of S alone (normative):
//   * the patterns are cut into segments of kSeg = 2048, segment g = [g kSeg, min(S, (g+1) kSeg));
//   * within a segment one thread adds the terms of its (r, v) serially in pattern order, each
//     as acc = fma((double)W[r][p], L[v][p], acc) from acc = +0;
//   * the segment sums are added serially in segment order, from segment 0's.
// So out[r][v] depends on (W[r], L[v], S) only: not on the other replicates or vectors of the
// call, on its position among them, on the chunking or on the leading dimensions.  No
// floating-point atomics.
//
//   k_rell          a VALU register-tile GEMM.  A workgroup of 256 threads owns 128 replicates x
//                   48 vectors x one segment; thread (ty, tx) owns replicates 8 ty .. 8 ty + 7 and
//                   vectors 3 tx .. 3 tx + 2, 24 fp64 accumulators.  It stages 32-pattern chunks
//                   of the tile's W rows (transposed, [pattern][replicate]) and L rows
//                   ([pattern][vector]) in LDS, so W is read once per 48 vectors (16 edges of the
//                   support pass), not once per vector.  A chunk all of whose staged L values are
//                   finite runs plain FMAs -- a zero weight then adds +-0 to an accumulator that is
//                   never -0, which leaves its bits alone --; a chunk that holds a -inf, +inf or
//                   NaN runs the same FMAs under a select on the weight.  Both give the same
//                   bits, so which one ran does not show in the result.
//   k_rell_combine  the segment sums of one (r, v) added in segment order (n_seg > 1).
//
// Why VALU and not the fp64 matrix cores: the zero-weight rule is a select per term, which an
// MFMA cannot apply (0 x -inf is NaN inside it), and on gfx950 the fp64 vector and matrix peaks
// are the same, so the register tile gives up no peak.  Memory: the segment sums of a launch,
// n_seg x n_rep x n_vec doubles, capped at 256 MiB by launching ranges of replicates.
#include <hip/hip_runtime.h>

#include <math.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "pu_ctx.h"
#include "pu_service.h"

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "pu_rell.hip: gfx950 only, as the other kernel files of this library"
#endif

using namespace pu;

namespace {

constexpr int kSeg = 2048;    // patterns per segment: part of the sum order, never change
constexpr int kCh = 32;       // patterns per staged chunk
constexpr int kTR = 128;      // replicates per workgroup
constexpr int kTV = 48;       // vectors per workgroup
constexpr int kRR = 8;        // replicates per thread
constexpr int kRV = 3;        // vectors per thread
constexpr int kWs = kTR + 4;  // LDS row stride of W (words): 16-byte aligned rows, banks spread
constexpr int kLs = kTV + 2;  // LDS row stride of L (doubles)
constexpr size_t kPartBytes = (size_t)256 << 20;

struct RellArgs {
    const double *L;    // [n_vec][ldl]
    const uint32_t *W;  // [n_rep][ldw]: this launch's replicates
    int64_t ldl, ldw, S;
    int n_vec, n_rep, n_seg;
    double *out;        // [n_rep][ldo]: this launch's rows (n_seg == 1)
    int64_t ldo;
    double *part;       // [n_seg][n_rep][n_vec] (n_seg > 1)
};

template <bool SELECT>
__device__ __forceinline__ void rell_chunk(const uint32_t *wl, const double *ll, int ty, int tx,
                                           double (&acc)[kRR][kRV]) {
#pragma unroll 4
    for (int p = 0; p < kCh; ++p) {
        const uint4 ua = *reinterpret_cast<const uint4 *>(wl + p * kWs + kRR * ty);
        const uint4 ub = *reinterpret_cast<const uint4 *>(wl + p * kWs + kRR * ty + 4);
        const uint32_t u[kRR] = {ua.x, ua.y, ua.z, ua.w, ub.x, ub.y, ub.z, ub.w};
        double lv[kRV];
#pragma unroll
        for (int j = 0; j < kRV; ++j) lv[j] = ll[p * kLs + kRV * tx + j];
#pragma unroll
        for (int i = 0; i < kRR; ++i) {
            const double du = (double)u[i];  // exact
#pragma unroll
            for (int j = 0; j < kRV; ++j) {
                const double t = fma(du, lv[j], acc[i][j]);
                acc[i][j] = (!SELECT || u[i] != 0u) ? t : acc[i][j];
            }
        }
    }
}

__global__ void __launch_bounds__(256) k_rell(RellArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t wl[kCh * kWs];
    __shared__ double ll[kCh * kLs];
    const int tid = (int)threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int g = (int)blockIdx.x, v0 = (int)blockIdx.y * kTV, r0 = (int)blockIdx.z * kTR;
    const int64_t s_lo = (int64_t)g * kSeg, s_hi = min(a.S, s_lo + kSeg);
    double acc[kRR][kRV];
#pragma unroll
    for (int i = 0; i < kRR; ++i)
#pragma unroll
        for (int j = 0; j < kRV; ++j) acc[i][j] = 0.0;
    for (int64_t s0 = s_lo; s0 < s_hi; s0 += kCh) {
        const int m = (int)min((int64_t)kCh, s_hi - s0);
        __syncthreads();  // the previous chunk has been consumed
        // outside the tile, the call or the segment: weight 0 against a finite 0
        for (int i = tid; i < kTR * kCh; i += 256) {
            const int r = i / kCh, p = i - r * kCh;
            wl[p * kWs + r] =
                (r0 + r < a.n_rep && p < m) ? a.W[(int64_t)(r0 + r) * a.ldw + s0 + p] : 0u;
        }
        int bad = 0;
        for (int i = tid; i < kTV * kCh; i += 256) {
            const int v = i / kCh, p = i - v * kCh;
            const double x =
                (v0 + v < a.n_vec && p < m) ? a.L[(int64_t)(v0 + v) * a.ldl + s0 + p] : 0.0;
            bad |= !isfinite(x);
            ll[p * kLs + v] = x;
        }
        bad = __syncthreads_or(bad);
        if (bad) rell_chunk<true>(wl, ll, ty, tx, acc);
        else rell_chunk<false>(wl, ll, ty, tx, acc);
    }
#pragma unroll
    for (int i = 0; i < kRR; ++i) {
        const int r = r0 + kRR * ty + i;
        if (r >= a.n_rep) continue;
#pragma unroll
        for (int j = 0; j < kRV; ++j) {
            const int v = v0 + kRV * tx + j;
            if (v >= a.n_vec) continue;
            if (a.n_seg == 1) a.out[(int64_t)r * a.ldo + v] = acc[i][j];
            else a.part[((size_t)g * a.n_rep + r) * a.n_vec + v] = acc[i][j];
        }
    }
}

__global__ void __launch_bounds__(256) k_rell_combine(RellArgs a) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)a.n_rep * a.n_vec) return;
    const int64_t r = e / a.n_vec, v = e - r * a.n_vec;
    const size_t slab = (size_t)a.n_rep * a.n_vec;
    double acc = a.part[e];
    for (int g = 1; g < a.n_seg; ++g) acc += a.part[(size_t)g * slab + e];
    a.out[r * a.ldo + v] = acc;
}

struct RellState : DevState {
    DevBuf<double> part;
};
RellState g_rell[64];

int check_rell(const char *fn, int n_vec, int64_t n_sites, const void *L, int n_rep, const void *W,
               const void *out) {
    if (!L || !W || !out) return set_err(nullptr, PU_E_ARG, "%s: null buffer", fn);
    if (n_vec < 1 || n_rep < 1 || n_sites < 1)
        return set_err(nullptr, PU_E_ARG, "%s: n_vec = %d, n_rep = %d, n_sites = %lld", fn, n_vec,
                       n_rep, (long long)n_sites);
    if ((n_sites + kSeg - 1) / kSeg > 0x7fffffff)
        return set_err(nullptr, PU_E_ARG, "%s: n_sites = %lld", fn, (long long)n_sites);
    return PU_OK;
}

int run_rell(int device, hipStream_t st, int n_vec, int64_t S, const double *d_L, int64_t ldl,
             int n_rep, const uint32_t *d_W, int64_t ldw, double *d_out, int64_t ldo) {
    RellState &B = g_rell[device];
    StateScope scope(B, st);
    int rc;
    if ((rc = scope.rc)) return rc;
    const int n_seg = (int)((S + kSeg - 1) / kSeg);
    const unsigned vt = (unsigned)((n_vec + kTV - 1) / kTV);
    if (vt > 65535u) return set_err(nullptr, PU_E_ARG, "pu_rell_sums: n_vec = %d", n_vec);
    // replicates per launch: whole tiles whose segment sums fit the workspace
    int64_t rc_n = n_rep;
    if (n_seg > 1) {
        const size_t per = (size_t)n_seg * n_vec * sizeof(double);
        rc_n = std::max<int64_t>(1, (int64_t)(kPartBytes / per));
        if (rc_n >= kTR) rc_n = rc_n / kTR * kTR;
        rc_n = std::min<int64_t>(rc_n, n_rep);
        if ((rc = B.part.reserve((size_t)n_seg * rc_n * n_vec))) return rc;
    }
    rc_n = std::min<int64_t>(rc_n, (int64_t)65535 * kTR);
    for (int64_t r0 = 0; r0 < n_rep; r0 += rc_n) {
        RellArgs a;
        a.L = d_L;
        a.W = d_W + r0 * ldw;
        a.ldl = ldl;
        a.ldw = ldw;
        a.S = S;
        a.n_vec = n_vec;
        a.n_rep = (int)std::min<int64_t>(rc_n, n_rep - r0);
        a.n_seg = n_seg;
        a.out = d_out + r0 * ldo;
        a.ldo = ldo;
        a.part = B.part.p;
        const dim3 grid((unsigned)n_seg, vt, (unsigned)((a.n_rep + kTR - 1) / kTR));
        hipLaunchKernelGGL(k_rell, grid, dim3(256), 0, st, a);
        HIPCHK(nullptr, hipGetLastError());
        if (n_seg > 1) {
            const int64_t ne = (int64_t)a.n_rep * n_vec;
            hipLaunchKernelGGL(k_rell_combine, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, st,
                               a);
            HIPCHK(nullptr, hipGetLastError());
        }
    }
    return PU_OK;
}

}  // namespace

extern "C" {

int pu_rell_sums_device(int device, void *stream, int n_vec, int64_t n_sites, const double *d_L,
                        int64_t ldl, int n_rep, const uint32_t *d_W, int64_t ldw, double *d_out,
                        int64_t ldo) {
    const char *fn = "pu_rell_sums_device";
    int rc;
    if ((rc = check_rell(fn, n_vec, n_sites, d_L, n_rep, d_W, d_out))) return rc;
    if (ldl < n_sites || ldw < n_sites || ldo < n_vec)
        return set_err(nullptr, PU_E_ARG, "%s: row strides %lld, %lld, %lld below n_sites = %lld, "
                       "n_sites, n_vec = %d", fn, (long long)ldl, (long long)ldw, (long long)ldo,
                       (long long)n_sites, n_vec);
    if ((rc = check_device(device))) return rc;
    DeviceGuard g(device);
    return run_rell(device, (hipStream_t)stream, n_vec, n_sites, d_L, ldl, n_rep, d_W, ldw, d_out,
                    ldo);
}

int pu_rell_sums(int device, int n_vec, int64_t n_sites, const double *L, int n_rep,
                 const uint32_t *W, double *out) {
    const char *fn = "pu_rell_sums";
    int rc;
    if ((rc = check_rell(fn, n_vec, n_sites, L, n_rep, W, out))) return rc;
    if ((rc = check_device(device))) return rc;
    DeviceGuard g(device);
    HostCall h(device);
    const double *d_L = h.to_device(L, (size_t)n_vec * n_sites);
    const uint32_t *d_W = h.to_device(W, (size_t)n_rep * n_sites);
    double *d_out = h.alloc<double>((size_t)n_rep * n_vec);
    if (!h.rc)
        h.rc = run_rell(device, h.st, n_vec, n_sites, d_L, n_sites, n_rep, d_W, n_sites, d_out,
                        n_vec);
    h.to_host(out, d_out, (size_t)n_rep * n_vec);
    return h.finish(fn);
}

}  // extern "C"
