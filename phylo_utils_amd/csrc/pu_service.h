// pu_service.h -- the host layer that the pair-distance, NJ, bootstrap and simulation calls share
// (pu_distance.hip, pu_nj.hip, pu_bootstrap.hip, pu_simulate.hip): growable device buffers, the
// per-device state protocol, the profiling events of a chunked call, the scope of a host-form
// call, and the argument rules and staged-row constants of the pair calls.  Included after
// pu_ctx.h.  Not part of the public ABI: nothing declared here is exported by the library.
#pragma once
#include <stdlib.h>

#include <algorithm>

#include "pu_ctx.h"

#pragma GCC visibility push(hidden)
namespace pu {

// ---- the staged-row layout of the count kernels (k_pair_counts, k_boot_pair_counts) -----------

constexpr int kMaxCodes = 32;  // 8 KB of fp64 bins per pair
constexpr int kCH = 128;       // sites per staged chunk
constexpr int kRow = kCH + 4;  // staged code row stride in bytes (33 words: odd)

// bins between neighbouring lanes: odd, so the lanes start on different banks
__host__ __device__ inline int bin_stride(int n_codes) { return (n_codes * n_codes) | 1; }

// v, or the positive integer in the environment variable where that is smaller (PU_DIST_CHUNK,
// PU_BOOT_REP_CHUNK; read at each call)
inline int64_t env_cap(const char *name, int64_t v) {
    if (const char *env = getenv(name)) {
        const long long cap = atoll(env);
        if (cap > 0) v = std::min<int64_t>(v, cap);
    }
    return v;
}

// ---- device buffers and the per-device state ------------------------------------------------

// a device buffer that is grown, never shrunk; growing waits for the launches that read it
template <class T>
struct DevBuf {
    T *p = nullptr;
    size_t cap = 0;
    int reserve(size_t n) {
        if (cap >= n) return PU_OK;
        dfree(p);
        cap = 0;
        if (int rc = dalloc(nullptr, &p, n)) return rc;
        cap = n;
        return PU_OK;
    }
};

// per-device buffers of a family of calls are guarded by mu; `done` marks the end of the last
// call's queued work, which the next call waits for before it touches them
struct DevState {
    std::mutex mu;
    hipEvent_t done = nullptr;
};

// a call's hold on a DevState: locks it, waits for the last call (rc: whether that worked), and
// marks the end of this call's queued work on every way out of it, an error return included:
// what was queued before the error still reads the state's buffers
struct StateScope {
    std::lock_guard<std::mutex> lk;
    DevState &s;
    hipStream_t st;
    int rc;
    StateScope(DevState &state, hipStream_t stream) : lk(state.mu), s(state), st(stream) {
        rc = begin();
    }
    ~StateScope() {
        if (s.done) (void)hipEventRecord(s.done, st);
    }
    StateScope(const StateScope &) = delete;

private:
    int begin() {
        if (s.done) HIPCHK(nullptr, hipEventSynchronize(s.done));
        else HIPCHK(nullptr, hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
        return PU_OK;
    }
};

// ---- profiling events of a chunked call: 3 per chunk (start, after the counts, after Newton) --

struct ChunkProfile {
    bool on = false;
    std::vector<hipEvent_t> ev;
    int n_ev = 0;
    // a new call of n_chunks chunks
    int reserve(int64_t n_chunks) {
        n_ev = 0;
        while (on && (int64_t)ev.size() < 3 * n_chunks) {
            hipEvent_t e;
            HIPCHK(nullptr, hipEventCreate(&e));
            ev.push_back(e);
        }
        return PU_OK;
    }
    // phase 0, 1, 2 of the current chunk; 2 closes it
    int mark(int phase, hipStream_t st) {
        if (!on) return PU_OK;
        HIPCHK(nullptr, hipEventRecord(ev[n_ev + phase], st));
        if (phase == 2) n_ev += 3;
        return PU_OK;
    }
};

// pu_*_profile / pu_*_kernel_ms of a state array whose elements hold a ChunkProfile `prof`
template <class S>
int profile_set(S (&states)[64], int device, int on) {
    if (device < 0 || device >= 64) return set_err(nullptr, PU_E_ARG, "device %d", device);
    std::lock_guard<std::mutex> lk(states[device].mu);
    states[device].prof.on = on != 0;
    states[device].prof.n_ev = 0;
    return PU_OK;
}

template <class S>
int profile_ms(const char *fn, S (&states)[64], int device, double *counts_ms,
               double *newton_ms) {
    if (device < 0 || device >= 64 || !counts_ms || !newton_ms)
        return set_err(nullptr, PU_E_ARG, "%s: bad argument", fn);
    std::lock_guard<std::mutex> lk(states[device].mu);
    const ChunkProfile &P = states[device].prof;
    if (!P.n_ev) return set_err(nullptr, PU_E_STATE, "%s: nothing recorded", fn);
    DeviceGuard g(device);
    HIPCHK(nullptr, hipEventSynchronize(P.ev[P.n_ev - 1]));
    double c = 0.0, w = 0.0;
    for (int i = 0; i < P.n_ev; i += 3) {
        float a = 0.f, b = 0.f;
        HIPCHK(nullptr, hipEventElapsedTime(&a, P.ev[i], P.ev[i + 1]));
        HIPCHK(nullptr, hipEventElapsedTime(&b, P.ev[i + 1], P.ev[i + 2]));
        c += a;
        w += b;
    }
    *counts_ms = c;
    *newton_ms = w;
    return PU_OK;
}

// ---- the scope of a host-form call ------------------------------------------------------------

// The stream, the device temporaries and the first error of a host-form call.  rc latches: once
// it is set, alloc / to_device / to_host do nothing, so a call is written straight down and
// ends in `return h.finish(fn)`, which waits for the stream before the destructor frees anything.
struct HostCall {
    std::unique_lock<std::mutex> lk;  // ws_mutex(device) of a stateless call
    hipStream_t st = nullptr;
    std::string *err = nullptr;
    int rc = PU_OK;
    bool queued = true;  // st is a stream that work may have been queued on
    std::vector<void *> tmp;

    // a stateless call: the device's scratch stream, under its mutex
    explicit HostCall(int device) : lk(ws_mutex(device)) {
        double *unused;
        rc = ws_get(device, 1, &unused, &st);
        queued = rc == PU_OK;
    }
    // a context's call: its stream and error slot
    HostCall(hipStream_t stream, std::string *e) : st(stream), err(e) {}
    HostCall(const HostCall &) = delete;
    ~HostCall() {
        for (void *p : tmp) (void)hipFree(p);
    }

    int hip(const char *what, hipError_t e) {
        if (!rc && e != hipSuccess)
            rc = set_err(err, PU_E_HIP, "%s: %s", what, hipGetErrorString(e));
        return rc;
    }
    template <class T>
    T *alloc(size_t n) {
        T *p = nullptr;
        if (!rc && !(rc = dalloc(err, &p, n)) && p) tmp.push_back(p);
        return p;
    }
    // a null source (an optional input) stays null
    template <class T>
    T *to_device(const T *src, size_t n) {
        T *p = src ? alloc<T>(n) : nullptr;
        if (!rc && p)
            hip("hipMemcpyAsync", hipMemcpyAsync(p, src, n * sizeof(T), hipMemcpyHostToDevice, st));
        return p;
    }
    template <class T>
    void to_host(T *dst, const T *src, size_t n) {
        if (!rc && n)
            hip("hipMemcpyAsync", hipMemcpyAsync(dst, src, n * sizeof(T), hipMemcpyDeviceToHost, st));
    }
    // the queued work reads the temporaries: wait for it whether or not the call failed
    int finish(const char *fn) {
        if (queued) {
            const hipError_t e = hipStreamSynchronize(st);
            hip(fn, e);
        }
        return rc;
    }
};

// ---- the argument rules of the pair calls ----------------------------------------------------

struct Shape {
    int n_taxa, n_codes;
    int64_t n_sites, n_pairs;
    const int32_t *pairs;  // [n_pairs][2] (host) or null: all i < j, row-major
    int n_rep;             // 1 for the pair calls
};

inline int check_pairs(const char *fn, int n_taxa, int64_t n_pairs, const int32_t *pairs) {
    const int64_t all = (int64_t)n_taxa * (n_taxa - 1) / 2;
    if (n_pairs < 1 || (!pairs && n_pairs != all))
        return set_err(nullptr, PU_E_ARG, "%s: n_pairs = %lld (without a pair list: all %lld)", fn,
                       (long long)n_pairs, (long long)all);
    if (pairs)
        for (int64_t p = 0; p < n_pairs; ++p) {
            const int i = pairs[2 * p], j = pairs[2 * p + 1];
            if (i < 0 || j < 0 || i >= n_taxa || j >= n_taxa || i == j)
                return set_err(nullptr, PU_E_ARG, "%s: pair %lld = (%d, %d) of %d taxa", fn,
                               (long long)p, i, j, n_taxa);
        }
    return PU_OK;
}

// null_buffer: one of the call's input buffers (codes, W) is missing
inline int check_shape(const char *fn, const Shape &s, bool null_buffer) {
    if (null_buffer) return set_err(nullptr, PU_E_ARG, "%s: null buffer", fn);
    if (s.n_rep < 1) return set_err(nullptr, PU_E_ARG, "%s: n_rep = %d", fn, s.n_rep);
    if (s.n_taxa < 2 || s.n_sites <= 0)
        return set_err(nullptr, PU_E_ARG, "%s: n_taxa = %d, n_sites = %lld", fn, s.n_taxa,
                       (long long)s.n_sites);
    if (s.n_codes < 1 || s.n_codes > kMaxCodes)
        return set_err(nullptr, PU_E_ARG, "%s: n_codes = %d is outside [1, %d]", fn, s.n_codes,
                       kMaxCodes);
    return check_pairs(fn, s.n_taxa, s.n_pairs, s.pairs);
}

inline int check_codes(const char *fn, const uint8_t *codes, int n_taxa, int64_t n_sites,
                       int n_codes) {
    for (int64_t i = 0; i < (int64_t)n_taxa * n_sites; ++i)
        if (codes[i] >= n_codes)
            return set_err(nullptr, PU_E_ARG, "%s: taxon %lld site %lld: code %d >= n_codes = %d",
                           fn, (long long)(i / n_sites), (long long)(i % n_sites), (int)codes[i],
                           n_codes);
    return PU_OK;
}

// the pair list of a call on the device: the given list, or all i < j
struct PairList {
    DevBuf<int32_t> d;
    std::vector<int32_t> h;
    int upload(hipStream_t st, int n_taxa, int64_t n_pairs, const int32_t *pairs) {
        h.resize(2 * (size_t)n_pairs);
        if (pairs) std::copy(pairs, pairs + 2 * n_pairs, h.begin());
        else {
            size_t k = 0;
            for (int i = 0; i < n_taxa; ++i)
                for (int j = i + 1; j < n_taxa; ++j) {
                    h[k++] = i;
                    h[k++] = j;
                }
        }
        if (int rc = d.reserve(h.size())) return rc;
        HIPCHK(nullptr, hipMemcpyAsync(d.p, h.data(), h.size() * 4, hipMemcpyHostToDevice, st));
        return PU_OK;
    }
};

// pu_nj.hip, for pu_bootstrap.hip too: the t column of out5 [n_mat][n (n - 1) / 2][5] (all pairs,
// row-major) as symmetric matrices [n_mat][n][ld], queued on st
int pair_matrix_all(hipStream_t st, int n_mat, int n, const double *d_out5, double *d_D,
                    int64_t ld);

}  // namespace pu
#pragma GCC visibility pop
