// minibatch_index.h — which dataset row stands behind minibatch position b: ONE definition for the library's kernels
// (dense_kernel.inc, bnn_kernel.inc, minibatch_gather_kernel of elbo_kernel.hip) and for the generated kernels, whose
// in-kernel training loop gathers its own rows (spec_main.h, SPEC_MINIBATCH).
#pragma once
#include "philox.h"

namespace bsvi {

// A keyed bijection of [0, DS) (4-round Feistel on the next power of four, cycle-walked) so that the B rows of a
// minibatch are distinct — sampling without replacement like np.random.choice(replace=False) in distributions.py:438.
// A function of (key, offset, b) alone: every rank, every workgroup and every engine draws the same rows.
__device__ __forceinline__ uint32_t minibatch_index_keyed(uint32_t DS, uint32_t seed_lo, uint32_t seed_hi, uint32_t offset_lo,
                                                          uint32_t offset_hi, uint32_t b) {
    uint32_t half_bits = 1;
    while ((1u << (2 * half_bits)) < DS) ++half_bits;
    const uint32_t mask = (1u << half_bits) - 1u;
    uint32_t x = b;
    for (int walk = 0; walk < 64; ++walk) {
        uint32_t lft = (x >> half_bits) & mask, rgt = x & mask;
        for (uint32_t round = 0; round < 4; ++round) {
            const u32x4 h = philox4x32(rgt, round, offset_lo, offset_hi, seed_lo ^ 0x5bd1e995u, seed_hi);
            const uint32_t t = lft ^ (h.x & mask);
            lft = rgt;
            rgt = t;
        }
        x = (lft << half_bits) | rgt;
        if (x < DS) return x;
    }
    return b % DS;
}

// The key of a minibatch source: the call's seed xor-ed with the constant of the source's key group (sources that share a
// RandomIndices variable share a group and with it the rows; group 0 is the dense path's key), 63 bits — as the host forms
// it for bsvi_minibatch_gather (engine.py, _refresh_minibatches).
__device__ __forceinline__ void minibatch_group_key(uint32_t seed_lo, uint32_t seed_hi, uint32_t group, uint32_t& key_lo, uint32_t& key_hi) {
    const unsigned long long c = 0x9E3779B97F4A7C15ull * (unsigned long long)group;
    key_lo = seed_lo ^ (uint32_t)c;
    key_hi = (seed_hi ^ (uint32_t)(c >> 32)) & 0x7FFFFFFFu;
}

}  // namespace bsvi
