// pu_philox.h -- the one copy of the counter-based generator behind every draw of this library
// (pu_simulate.hip: DESIGN 4.10, counter word 3 = 0; pu_bootstrap.hip: DESIGN 4.14, counter
// word 3 = 1; pu_scf.hip: DESIGN 4.29, counter word 3 = 2; pu_lmap.hip: DESIGN 4.30, counter
// word 3 = 3).  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pu {

// Philox4x32-10 (Salmon et al., SC'11) on counter (g lo, g hi, c2, c3) under key (seed lo,
// seed hi); only x0 and x1 of the output are used:
//     u = ((x1 >> 5) * 2^26 + (x0 >> 6)) * 2^-53      in [0, 1)
__device__ __forceinline__ double philox_u(uint64_t seed, uint64_t g, uint32_t c2, uint32_t c3) {
    uint32_t c0 = (uint32_t)g, c1 = (uint32_t)(g >> 32);
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0;
        c1 = l1;
        c2 = h0 ^ c3 ^ k1;
        c3 = l0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    const uint64_t m = ((uint64_t)(c1 >> 5) << 26) | (uint64_t)(c0 >> 6);
    return (double)m * 0x1p-53;
}

}  // namespace pu
