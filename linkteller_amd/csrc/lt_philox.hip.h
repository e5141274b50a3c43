// Philox4x32-10 (Salmon et al., SC'11): counter (c0, c1, c2, c3), key (k0, k1).  Shared by the dropout masks of the trainers
// (lt_train.hip) and the per-cell noise streams of the edge-DP generators (lt_dp.hip); include/linkteller_hip.h states which
// counter and key words each of them uses.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

__device__ __forceinline__ uint4 lt_philox4x32_10(uint4 c, uint2 k) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r) { k.x += 0x9E3779B9u; k.y += 0xBB67AE85u; }
        const uint32_t lo0 = 0xD2511F53u * c.x, hi0 = __umulhi(0xD2511F53u, c.x);
        const uint32_t lo1 = 0xCD9E8D57u * c.z, hi1 = __umulhi(0xCD9E8D57u, c.z);
        c = make_uint4(hi1 ^ c.y ^ k.x, lo1, hi0 ^ c.w ^ k.y, lo0);
    }
    return c;
}
