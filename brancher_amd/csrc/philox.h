// philox.h — counter-based RNG for in-kernel reparameterisation noise (device code).
//
// The reference draws noise through torch's global generator once per node per iteration
// (torch normal.py:83-86 `_standard_normal`, reached from brancher/distributions.py:122).
// Here every draw is a pure function of (seed, global sample index, noise row, iteration,
// attempt), so a Monte-Carlo shard on any GPU sees the same stream it would see on one GPU
// and the kernel never reads noise from HBM.  Philox4x32 (Salmon et al., SC'11) with SEVEN rounds since round 6: the paper's Table 2
// lists Philox4x32-7 as the fewest rounds that pass BigCrush ("Crush-resistant"; 10 is its default for a safety margin).  The draw is
// the bound of the dense path's two launches (a drawing wave per SIMD at ~140 vector instructions per four normals), and
// three rounds are ~20 of them: config 4 103.8 -> 101.1 us per iteration (profiles/r6/philox_rounds.txt).  Parity is always on the
// noise a kernel REPORTS (the oracle replays it), so nothing else moves; seeds of earlier rounds give other streams.
//
// The posterior-predictive pass of the Bayesian neural networks (bnn_kernel.inc, bsvi_bnn_predict) draws from the likelihood on a
// stream of its own:  c0 = global sample index, c1 = row m of the caller's x, c2 / c3 = the 64-bit offset, key word k0 = seed low ^
// 0x2545f491 (another constant than the three of the minibatch / drawn-data streams, and not 0: no stream of the same seed has this
// key), k1 = seed high ^ call.  Categorical and Bernoulli read u01(word 0) of call 0; the Normal likelihood's output c takes normal
// c & 3 of the four box_muller_fast normals ((x, y) -> 0, 1; (z, w) -> 2, 3) of call c >> 2.  A Laplace or Cauchy likelihood's output c
// takes ONE word, word c & 3 (x, y, z, w) of the same call c >> 2, through laplace_noise / cauchy_noise (bsvi_device.h) — the Laplace
// draw is -sign(v) log1p(-|v|) of that uniform base noise v, the Cauchy draw the tangent itself.  The weights of that pass are the BNN
// path's ordinary draw (c1 = (row >> 2) | 0x40000000, the seed as it is).
//
// Latent prior scales of the Bayesian neural networks (bsvi_bnn_set_scale_latents): with quads = ceil(n_rows / 4), latent t takes
// normal t & 3 of the ordinary row-quad call whose quad index is quads + (t >> 2) — c1 = (quads + (t >> 2)) | 0x40000000, the same
// counters, key and box_muller_fast pairing as the rows, behind every quad a row uses.  A pure function of (seed, offset, global sample,
// t): the same over sample shards.  It is reported in row n_rows + t of noise_out and replayed from there when the caller hands noise in.
#pragma once
#if !defined(__HIPCC_RTC__)
#include <hip/hip_runtime.h>
#include <stdint.h>
#endif

namespace bsvi {

struct u32x4 { uint32_t x, y, z, w; };

constexpr int kPhiloxRounds = 7;

__device__ __forceinline__ u32x4 philox4x32(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < kPhiloxRounds; ++r) {
        // both halves of a product from ONE v_mad_u64_u32 (written as __umulhi + multiply the compiler emits a
        // quarter-rate v_mul_hi_u32 and a quarter-rate v_mul_lo_u32 per product: 40 instead of 20 per call)
        const uint64_t p0 = (uint64_t)M0 * c0, p1 = (uint64_t)M1 * c2;
        const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0;
        const uint32_t hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
        const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += W0; k1 += W1;
    }
    return {c0, c1, c2, c3};
}

// 24 random bits on (0, 1] — NOT the open interval: for x >> 8 == 2^24 - 1 the sum rounds to 2^24 in single precision and the
// result is exactly 1.0f (probability 2^-24 per word).  log(1) = 0 is fine for Box-Muller; a transform that cannot take 1 clamps
// its own result (bsvi_device.h: laplace_noise, cauchy_noise).  The Normal streams depend on this rounding bit for bit.
__device__ __forceinline__ float u01(uint32_t x) { return ((float)(x >> 8) + 0.5f) * (1.0f / 16777216.0f); }

__device__ __forceinline__ void box_muller(uint32_t a, uint32_t b, float& z0, float& z1) {
    const float r = sqrtf(-2.0f * logf(u01(a)));
    float s, c;
    sincosf(6.28318530717958647692f * u01(b), &s, &c);
    z0 = r * c;
    z1 = r * s;
}

}  // namespace bsvi
