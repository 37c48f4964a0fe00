// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC 2011): the counter-based generator behind
// the Gumbel noise of stochastic beam search (gumbel.hip).  A pure function of (counter, key): no state, so any thread can produce any
// draw, and a host program can reproduce every one of them (tests/philox_check.cpp, tests/gumbel_ref.py).  Plain C++ with no HIP header:
// a host compiler builds it alone.  drop_hash (common.hip.h) stays what dropout uses; this is what a sampler draws from.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CC_PHILOX_FN __host__ __device__ __forceinline__
#else
#define CC_PHILOX_FN inline
#endif

struct philox4 {
    uint32_t w[4];
};

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u;      // round multipliers
constexpr uint32_t PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;      // key increments (golden ratio, sqrt(3) - 1)

// ten rounds; the key is bumped between rounds (nine times)
CC_PHILOX_FN philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    for (int r = 0; r < 10; r++) {
        if (r) { k0 += PHILOX_W0; k1 += PHILOX_W1; }
        const uint64_t p0 = (uint64_t)PHILOX_M0 * c0, p1 = (uint64_t)PHILOX_M1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    }
    return philox4{{c0, c1, c2, c3}};
}

// word k of a result by selects: a run-time index into the array would put it in scratch memory on the device
CC_PHILOX_FN uint32_t philox_word(const philox4& p, uint32_t k) { return k == 0 ? p.w[0] : k == 1 ? p.w[1] : k == 2 ? p.w[2] : p.w[3]; }

// The four noise words of tokens 4 q .. 4 q + 3 of logits row `row` at decode step `step` under a 64-bit seed: token v reads word v & 3 of
// the call with q = v >> 2.  Four consecutive tokens share one call, which lines up with a 16-byte load of the row.
CC_PHILOX_FN philox4 gumbel_bits4(uint64_t seed, uint32_t step, uint32_t row, uint32_t q) {
    return philox4x32_10(q, row, step, 0u, (uint32_t)seed, (uint32_t)(seed >> 32));
}
