// dense_local.inc — the local reparameterisation estimator of the dense-link path (Kingma, Salimans and Welling, 2015; included by
// elbo_kernel.hip behind dense_predict.inc; DESIGN.md 4.4.2).
//
// For a mean-field Normal posterior W[c][p] ~ N(mu, s) of a LINEAR link the logits of minibatch row b are themselves Normal,
//   m[b][c] = sum_p x[b][p] mu[c][p],   v[b][c] = sum_p x[b][p]^2 s[c][p]^2,   z_n[b][c] = m + sqrt(v) zeta[n][b][c],
// so the N weight draws, the N products X W_n^T and the N products back of the Pathwise launches are two products forward, two back, and
// N B C normals in place of N C P.  The prior and entropy terms are closed forms of the row parameters:
//   f = lik_weight (1 / N) sum_n sum_b log p(y_b | z_n[b]) + sum_r [ prior_weight (-log s0 - log sqrt(2 pi) - ((mu - mu0)^2 + s^2) / (2 s0^2))
//                                                                     + entropy_weight (log sqrt(2 pi e) + log s) ],      loss = -f
//
//   dense_head        the dense path's own launch, without noise workgroups: rowp (mu, s, mu0, s0), the minibatch of (seed, offset) as
//                     Pathwise gathers it (Xb [B_pad][P_pad], XbT [P_pad][B_pad], lab), `partial` cleared
//   dense_local_fwd   grid (ceil(B / 32), sample splits), 256 threads, two workgroups a CU.
//     products  m and v of the workgroup's 32 rows on v_mfma_f32_32x32x2_f32, two accumulators a wave.  A = x and, squared in registers,
//               x^2: the lane's fragment straight from XbT (rows k, 32 consecutive minibatch rows a half-wave: one 128-byte line) — the
//               four waves take the K chunks w, w + 4, ..., so no value of x is read by two waves and LDS would buy no reuse.  B = the
//               chunk of mu and of s^2, staged k-major by the wave itself (W[k][c], row stride 33: 32 consecutive p of one class in,
//               32 classes of one k out, no bank conflicts); classes >= C read as zero.  The waves' tiles are joined in wave order
//               through LDS; the tile keeps m and sd = sqrt(v).
//     samples   thread = (row tid & 31, sample lane tid >> 5): m[C], sd[C] of its row in registers, it walks the samples lane, lane + 8,
//               ... of the split.  Per sample the C normals — the caller's noise [N][B][C], or Philox call q = c >> 2 of (sample n, row b):
//               counter (n, (4 b + q) | 0x10000000, offset), the seed as the key, normal c & 3 of box_muller_fast's two pairs
//               (philox.h) — then z, the log-softmax or the sigmoid in registers, g = d lik / d z, and the sums of g, g zeta and lik.
//               The sample lanes are joined in lane order through LDS.
//     out       dM[split][b][32] = sum_n g,  dV[split][b][32] = sum_n g zeta / (2 sd) (0 where sd = 0: an all-zero row has z = m and
//               gives d s nothing), classes >= C and rows >= B zero;  likp[split][row tile] = the tile's likelihood, rows in order.
//     The products are recomputed by every sample split: they are N times cheaper than the per-sample products they replace.
//   dense_local_join  (more than one split) the splits of dM and dV added in split order, once — 25 column tiles each reading every split
//               themselves was a latency chain of 640 loads a thread at B = 512
//   dense_local_bwd   grid ceil(P / 32), 256 threads: d mu[c][p] = sum_b dM[b][c] x[b][p] and d(s^2)[c][p] = sum_b dV[b][c] x[b][p]^2 over
//               ALL minibatch rows on the same MFMA (A = dM / dV, 32 classes of a row: one line; B = Xb, 32 features of a row: one
//               line), the waves take the row chunks w, w + 4, ... and are joined in wave order: one workgroup owns its columns, no
//               partials in memory.  Epilogue = the row step: d s = 2 s d(s^2), the closed-form prior and entropy terms, the four
//               gradients into the uniform-table partials as dense_rows leaves them, the constant part of f per workgroup.
//   dense_local_tail  one workgroup: f from the likelihood and constant partials, the entries shared by all rows (stride 0), in fixed order
//   dense_param_kernel  the dense path's own, finalizing: loss, finite flag and d loss / d theta in the out block.
// No atomics, every sum in a fixed order: two calls on the same inputs leave the same bits, and a drawn call equals the call that is
// handed the noise it reported.

#include "dense_local_select.h"
namespace dloc = bsvi_dense_local;

constexpr uint32_t DL_TAG = 0x10000000u;

struct DenseLocal {
    const float* Xb; const float* XbT; const float* lab; const float* rowp;      // rowp: mu, s, mu0, s0 [4][R]
    const float* noise_in;      // [N][B][C] or null
    float* noise_out;           // [N][B][C] or null
    float* dM; float* dV;       // [splits][row_tiles 32][32]
    float* jM; float* jV;       // [row_tiles 32][32]
    float* likp;                // [splits][row_tiles]
    float* rowg; float* hpart; float* partial;
    uint32_t N, C, P, R, B, B_pad, P_pad, row_tiles, k_chunks, col_tiles, splits, samples_per_split, likelihood, n_uniform_grad;
    uint32_t base[4], stride[4];      // q loc, q scale, prior loc, prior scale in the uniform table
    float lik_weight, prior_weight, entropy_weight;
    uint32_t seed_lo, seed_hi, offset_lo, offset_hi;
};

template <int CT>
__global__ void __launch_bounds__(256, 2) dense_local_fwd(const DenseLocal T) {
    constexpr uint32_t TS = dloc::TS, CS = dloc::CS, KC = dloc::KC, LANES = dloc::LANES;
    __shared__ float buf[dloc::FWD_BUF];
    __shared__ float Mt[2][32 * TS];
    __shared__ float rowlik[LANES][32];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, lm = lane & 31u, lk = lane >> 5;
    const uint32_t tile = blockIdx.x, b0 = tile * 32u, split = blockIdx.y;

    // ---- products: m and v of the 32 rows, the wave's K chunks
    {
        float* const Wmu = buf + wave * 2u * KC * TS;
        float* const Ws2 = Wmu + KC * TS;
        xf_f32x16 am, av;
#pragma unroll
        for (int r = 0; r < 16; ++r) am[r] = av[r] = 0.0f;
        const float* const xt = T.XbT + (size_t)lk * T.B_pad + b0 + lm;      // + k B_pad: rows k < 32 k_chunks <= P_pad, columns < B_pad
        const uint32_t rounds = (T.k_chunks + 3u) / 4u;
        // the chunk of a round in registers: 16 values of x, and element j 64 + lane of mu and s — class 2 j + lk, feature lm
        float a[16], an[16], wm[8], wsd[8];
        auto fetch = [&](const uint32_t round) {
            const uint32_t chunk = round * 4u + wave, k0 = chunk * KC;
            const bool live = chunk < T.k_chunks;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const uint32_t c = 2u * j + lk, p = k0 + lm;
                const bool ok = live && c < T.C && p < T.P;
                wm[j] = ok ? T.rowp[c * T.P + p] : 0.0f;
                wsd[j] = ok ? T.rowp[T.R + c * T.P + p] : 0.0f;
            }
#pragma unroll
            for (int kk = 0; kk < 16; ++kk) an[kk] = live ? xt[(size_t)(k0 + 2u * kk) * T.B_pad] : 0.0f;
        };
        fetch(0);
        for (uint32_t round = 0; round < rounds; ++round) {
            const bool live = round * 4u + wave < T.k_chunks;
#pragma unroll
            for (int j = 0; j < 8; ++j) {      // (classes 2 j + lk <= 16 < TS: inside the row)
                Wmu[lm * TS + 2u * j + lk] = wm[j];
                Ws2[lm * TS + 2u * j + lk] = wsd[j] * wsd[j];
            }
#pragma unroll
            for (int kk = 0; kk < 16; ++kk) a[kk] = an[kk];
            __syncthreads();
            if (round + 1u < rounds) fetch(round + 1u);      // the next round's loads fly behind this round's products
            if (live) {
#pragma unroll
                for (int kk = 0; kk < 16; ++kk) {
                    const uint32_t at = (2u * kk + lk) * TS + lm;
                    const float bm = lm < T.C ? Wmu[at] : 0.0f, bs = lm < T.C ? Ws2[at] : 0.0f;
                    am = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kk], bm, am, 0, 0, 0);
                    av = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kk] * a[kk], bs, av, 0, 0, 0);
                }
            }
            __syncthreads();      // (the next round's staging overwrites the chunk)
        }
        // am[r] is m[row 8 (r >> 2) + 4 lk + (r & 3)][class lm]: the waves' tiles, joined in wave order
        float* const tm = buf + wave * 2u * 32u * TS;
        float* const tv = tm + 32u * TS;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const uint32_t row = 8u * (r >> 2) + 4u * lk + (r & 3);
            tm[row * TS + lm] = am[r];
            tv[row * TS + lm] = av[r];
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t e = tid + 256u * j, at = (e >> 5) * TS + (e & 31u);
            float m = 0.0f, v = 0.0f;
#pragma unroll
            for (uint32_t w = 0; w < 4u; ++w) { m += buf[w * 2u * 32u * TS + at]; v += buf[(w * 2u + 1u) * 32u * TS + at]; }
            Mt[0][at] = m;
            Mt[1][at] = sqrtf(v);
        }
        __syncthreads();
    }

    // ---- samples: thread = (row, sample lane)
    const uint32_t row = tid & 31u, sl = tid >> 5, b = b0 + row;
    float m[CT], sd[CT], G[CT], GZ[CT], L = 0.0f;
#pragma unroll
    for (int c = 0; c < CT; ++c) {
        m[c] = c < (int)T.C ? Mt[0][row * TS + c] : 0.0f;
        sd[c] = c < (int)T.C ? Mt[1][row * TS + c] : 0.0f;
        G[c] = GZ[c] = 0.0f;
    }
    const float label = T.lab[b];      // (b < 32 row_tiles <= B_pad)
    const uint32_t n0 = split * T.samples_per_split, n1 = min(T.N, n0 + T.samples_per_split);
    if (b < T.B) {
        for (uint32_t n = n0 + sl; n < n1; n += LANES) {
            float ze[CT];
            const size_t at = ((size_t)n * T.B + b) * T.C;
            if (T.noise_in) {
#pragma unroll
                for (int c = 0; c < CT; ++c) ze[c] = c < (int)T.C ? T.noise_in[at + c] : 0.0f;
            } else {
#pragma unroll
                for (int q = 0; q < (CT + 3) / 4; ++q) {
                    float e4[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                    if (4 * q < (int)T.C) {
                        const u32x4 x = philox4x32(n, (4u * b + q) | DL_TAG, T.offset_lo, T.offset_hi, T.seed_lo, T.seed_hi);
                        box_muller_fast(x.x, x.y, e4[0], e4[1]);
                        box_muller_fast(x.z, x.w, e4[2], e4[3]);
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (4 * q + i < CT) ze[4 * q + i] = 4 * q + i < (int)T.C ? e4[i] : 0.0f;
                }
            }
            if (T.noise_out) {
#pragma unroll
                for (int c = 0; c < CT; ++c)
                    if (c < (int)T.C) T.noise_out[at + c] = ze[c];
            }
            float z[CT];
#pragma unroll
            for (int c = 0; c < CT; ++c) z[c] = m[c] + sd[c] * ze[c];
            if (T.likelihood == BSVI_LIK_CATEGORICAL) {
                float mx = z[0];
#pragma unroll
                for (int c = 1; c < CT; ++c) if (c < (int)T.C) mx = fmaxf(mx, z[c]);
                float e[CT], se = 0.0f, zl = 0.0f;
#pragma unroll
                for (int c = 0; c < CT; ++c) {
                    e[c] = c < (int)T.C ? __expf(z[c] - mx) : 0.0f;
                    se += e[c];
                    zl = label == (float)c ? z[c] : zl;
                }
                // (se >= 1: the maximum contributes exp(0) — log and reciprocal are one instruction each, as in dense_forward)
                L += zl - (mx + __builtin_amdgcn_logf(se) * 0.6931471805599453f);
                const float inv = __builtin_amdgcn_rcpf(se);
#pragma unroll
                for (int c = 0; c < CT; ++c) {
                    const float g = c < (int)T.C ? (label == (float)c ? 1.0f : 0.0f) - inv * e[c] : 0.0f;
                    G[c] += g;
                    GZ[c] += g * ze[c];
                }
            } else {      // Bernoulli / Binomial(1): -binary_cross_entropy_with_logits(l, k)
                const float l = z[0];
                L += label * l - (fmaxf(l, 0.0f) + log1pf(expf(-fabsf(l))));
                const float g = label - sigmoidf_(l);
                G[0] += g;
                GZ[0] += g * ze[0];
            }
        }
    }
    // ---- the sample lanes in lane order (every read of the waves' tiles lies behind the barrier above)
    {
        float* const sg = buf + sl * 2u * 32u * CS;
        float* const sgz = sg + 32u * CS;
#pragma unroll
        for (int c = 0; c < CT; ++c)
            if (c < (int)T.C) { sg[row * CS + c] = G[c]; sgz[row * CS + c] = GZ[c]; }
        rowlik[sl][row] = L;
    }
    __syncthreads();
    const size_t out0 = ((size_t)split * T.row_tiles + tile) * 32u * 32u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t e = tid + 256u * j, r = e >> 5, c = e & 31u;
        float g = 0.0f, gz = 0.0f, dv = 0.0f;
        if (c < T.C) {
#pragma unroll
            for (uint32_t l = 0; l < LANES; ++l) { g += buf[l * 2u * 32u * CS + r * CS + c]; gz += buf[(l * 2u + 1u) * 32u * CS + r * CS + c]; }
            const float s = Mt[1][r * TS + c];
            dv = s > 0.0f ? gz * (0.5f / s) : 0.0f;
        }
        T.dM[out0 + e] = g;
        T.dV[out0 + e] = dv;
    }
    if (tid < 32u) {
        float t = 0.0f;
#pragma unroll
        for (uint32_t l = 0; l < LANES; ++l) t += rowlik[l][tid];
        rowlik[0][tid] = t;      // (the thread's own column)
    }
    __syncthreads();
    if (tid == 0u) {
        float t = 0.0f;
        for (uint32_t r = 0; r < 32u; ++r) t += rowlik[0][r];
        T.likp[(size_t)split * T.row_tiles + tile] = t;
    }
}

// the splits of a cell of dM and dV in split order
__global__ void __launch_bounds__(256) dense_local_join(const DenseLocal T) {
    const size_t cells = (size_t)T.row_tiles * 32u * 32u, i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= cells) return;
    float a = 0.0f, v = 0.0f;
    if ((i & 31u) < T.C) {
        for (uint32_t s0 = 0; s0 < T.splits; s0 += 8u) {      // eight loads of each array in flight, added in split order
            float m8[8], v8[8];
#pragma unroll
            for (uint32_t u = 0; u < 8u; ++u) {
                const bool ok = s0 + u < T.splits;
                const size_t at = (size_t)(ok ? s0 + u : 0u) * cells + i;
                const float x = T.dM[at], y = T.dV[at];
                m8[u] = ok ? x : 0.0f;
                v8[u] = ok ? y : 0.0f;
            }
#pragma unroll
            for (uint32_t u = 0; u < 8u; ++u) { a += m8[u]; v += v8[u]; }
        }
    }
    T.jM[i] = a;
    T.jV[i] = v;
}

// gM / gV: the joined [row_tiles 32][32] sums (the one split's own arrays when there is one)
__global__ void __launch_bounds__(256) dense_local_bwd(const DenseLocal T, const float* gM, const float* gV) {
    constexpr uint32_t TS = dloc::TS;
    __shared__ float part[4u * 2u * 32u * TS];
    __shared__ float red[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, lm = lane & 31u, lk = lane >> 5;
    const uint32_t p0 = blockIdx.x * dloc::COLS;      // (p0 + 31 < P_pad: a multiple of 64)
    xf_f32x16 amu, as2;
#pragma unroll
    for (int r = 0; r < 16; ++r) amu[r] = as2[r] = 0.0f;
    for (uint32_t chunk = wave; chunk < T.row_tiles; chunk += 4u) {
        float x[16], dm[16], dv[16];
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) {
            const uint32_t b = chunk * 32u + 2u * kk + lk;      // (< 32 row_tiles <= B_pad; rows >= B of Xb, gM, gV are zero)
            x[kk] = T.Xb[(size_t)b * T.P_pad + p0 + lm];
            dm[kk] = gM[(size_t)b * 32u + lm];
            dv[kk] = gV[(size_t)b * 32u + lm];
        }
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) {
            amu = __builtin_amdgcn_mfma_f32_32x32x2f32(dm[kk], x[kk], amu, 0, 0, 0);
            as2 = __builtin_amdgcn_mfma_f32_32x32x2f32(dv[kk], x[kk] * x[kk], as2, 0, 0, 0);
        }
    }
    // amu[r] is d mu[class 8 (r >> 2) + 4 lk + (r & 3)][feature p0 + lm]
    {
        float* const t0 = part + wave * 2u * 32u * TS;
        float* const t1 = t0 + 32u * TS;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const uint32_t c = 8u * (r >> 2) + 4u * lk + (r & 3);
            t0[c * TS + lm] = amu[r];
            t1[c * TS + lm] = as2[r];
        }
    }
    __syncthreads();
    // ---- the row step: thread -> (class, feature) cells, lanes along the features
    const float scale = T.lik_weight / (float)T.N;
    float hconst = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t e = tid + 256u * j, c = e >> 5, p = p0 + (e & 31u), at = c * TS + (e & 31u);
        if (c >= T.C || p >= T.P) continue;
        float dmu = 0.0f, ds2 = 0.0f;
#pragma unroll
        for (uint32_t w = 0; w < 4u; ++w) { dmu += part[w * 2u * 32u * TS + at]; ds2 += part[(w * 2u + 1u) * 32u * TS + at]; }
        const uint32_t r = c * T.P + p;
        const float mu = T.rowp[r], s = T.rowp[T.R + r], mu0 = T.rowp[2u * T.R + r], s0 = T.rowp[3u * T.R + r];
        const float delta = mu - mu0, is2 = 1.0f / (s0 * s0), sq = delta * delta + s * s;
        const float grad[4] = {scale * dmu - T.prior_weight * delta * is2,
                               2.0f * s * (scale * ds2) - T.prior_weight * s * is2 + T.entropy_weight / s,
                               T.prior_weight * delta * is2,
                               T.prior_weight * (sq * is2 / s0 - 1.0f / s0)};
        // only this thread touches the entries of its row; two of the four may be ONE entry (the reference's name-collision rule makes the
        // prior's roots the posterior's): their gradients are added in registers, in the order dense_rows adds them, and stored once —
        // four dependent read-modify-writes of global memory per cell were 20 us of this kernel
        uint32_t k[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) k[q] = T.stride[q] ? T.base[q] + r * T.stride[q] : 0xFFFFFFFFu;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (!T.stride[q]) {
                if (T.base[q] < T.n_uniform_grad) T.rowg[(size_t)q * T.R + r] = grad[q];
                continue;
            }
            if (k[q] >= T.n_uniform_grad) continue;
            bool first = true;
            float g = grad[q];
#pragma unroll
            for (int q2 = 0; q2 < 4; ++q2) {
                if (q2 < q && k[q2] == k[q]) first = false;
                if (q2 > q && k[q2] == k[q]) g += grad[q2];
            }
            if (first) T.partial[2u + k[q]] = g;
        }
        hconst += T.prior_weight * (-logf(s0) - kLogSqrt2Pi - 0.5f * sq * is2) + T.entropy_weight * (kHalfLog2PiE + logf(s));
    }
    const float h = block_sum(hconst, red, tid, 4);
    if (tid == 0u) T.hpart[blockIdx.x] = h;
}

// one workgroup: f, the non-finite flag and the uniform entries shared by all rows
__global__ void __launch_bounds__(256) dense_local_tail(const DenseLocal T) {
    __shared__ float red[4];
    const uint32_t tid = threadIdx.x;
    float h = 0.0f, l = 0.0f;
    for (uint32_t i = tid; i < T.col_tiles; i += 256u) h += T.hpart[i];
    for (uint32_t i = tid; i < T.splits * T.row_tiles; i += 256u) l += T.likp[i];
    const float htot = block_sum(h, red, tid, 4), ltot = block_sum(l, red, tid, 4);
    const float f = T.lik_weight * ltot / (float)T.N + htot;
    if (tid == 0u) {
        T.partial[0] = f;
        T.partial[1] = isfinite(f) ? 0.0f : 1.0f;
    }
    for (int q = 0; q < 4; ++q) {
        if (T.stride[q] || T.base[q] >= T.n_uniform_grad) continue;      // uniform: no divergence around the barriers
        float g = 0.0f;
        for (uint32_t r = tid; r < T.R; r += 256u) g += T.rowg[(size_t)q * T.R + r];
        const float tot = block_sum(g, red, tid, 4);
        if (tid == 0u) T.partial[2u + T.base[q]] += tot;
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------
static int dense_local_check(const bsvi_dense* p, const uint64_t n_samples) {
    if (!p) return fail(BSVI_ERR_INVALID, "bsvi_dense_local: null handle");
    if (p->d.entropy_weight == 0.0f)
        return fail(BSVI_ERR_INVALID, "bsvi_dense_local: the handle is a point estimate: there is nothing to reparameterise (use Pathwise or MAP)");
    if (p->d.estimator != BSVI_EST_PATHWISE)
        return fail(BSVI_ERR_INVALID, "bsvi_dense_local: the handle must be created with BSVI_EST_PATHWISE");
    if (p->d.n_classes > dloc::MAX_CLASSES)
        return fail(BSVI_ERR_INVALID, "bsvi_dense_local: " + std::to_string(p->d.n_classes) + " classes, served are 1 .. 16 (a row's logits stay in registers)");
    if (n_samples < 1 || n_samples > dloc::MAX_SAMPLES)
        return fail(BSVI_ERR_INVALID, "bsvi_dense_local: n_samples is " + std::to_string(n_samples) + ", served are 1 .. 65536");
    if (p->d.batch_size > dloc::MAX_BATCH)
        return fail(BSVI_ERR_INVALID, "bsvi_dense_local: a minibatch of " + std::to_string(p->d.batch_size) + " rows, served are up to 2^24 (the draw's counter)");
    return BSVI_OK;
}

static dloc::Plan dense_local_plan(const bsvi_dense* p, const uint32_t N) {
    const char* const e = getenv("BSVI_LOCAL_SPLITS");      // the plan's one knob: the number of sample splits (tests, timing)
    const int forced = e ? atoi(e) : 0;
    return dloc::local_plan(p->d.n_classes, p->d.n_features, p->d.batch_size, N, p->m.n_cu, p->d.n_uniform_grad, forced > 0 ? (uint32_t)forced : 0u);
}

extern "C" size_t bsvi_dense_local_workspace_bytes(const bsvi_dense* p, uint32_t n_samples) {
    if (dense_local_check(p, n_samples)) return 0;
    return dense_local_plan(p, n_samples).total;
}

extern "C" int bsvi_dense_local_fwd_bwd(const bsvi_dense* p, const bsvi_dense_local_args* a) {
    if (!a) return fail(BSVI_ERR_INVALID, "bsvi_dense_local_fwd_bwd: null argument");
    BSVI_CHECK_STRUCT(a, bsvi_dense_local_args);
    const int rc = dense_local_check(p, a->n_samples);
    if (rc) return rc;
    if (!a->params_dev || !a->out_dev || !a->workspace_dev) return fail(BSVI_ERR_INVALID, "bsvi_dense_local_fwd_bwd: null argument (params_dev, out_dev, workspace_dev)");
    if ((uintptr_t)a->workspace_dev & 255u) return fail(BSVI_ERR_INVALID, "bsvi_dense_local_fwd_bwd: workspace_dev is not 256-byte aligned");
    const uint32_t C = p->d.n_classes, P = p->d.n_features, R = C * P, N = a->n_samples;
    const dloc::Plan L = dense_local_plan(p, N);
    char* const ws = (char*)a->workspace_dev;
    // the dense path's head: row parameters and the gathered minibatch, f32 copies, no noise workgroups
    DParams D;
    memset(&D, 0, sizeof(D));
    D.uniform = p->uniform; D.consts = p->consts; D.params = a->params_dev; D.dataset = p->dataset; D.labels = p->labels;
    D.indices_in = a->indices_dev; D.indices_out = a->indices_out_dev;
    D.rowp = (float*)(ws + L.rowp); D.idx = (int32_t*)(ws + L.idx); D.Xb = (float*)(ws + L.Xb); D.XbT = (float*)(ws + L.XbT);
    D.lab = (float*)(ws + L.lab); D.partial = (float*)(ws + L.partial);
    D.C = C; D.P = P; D.P_pad = L.P_pad; D.DS = p->d.dataset_size; D.B = p->d.batch_size; D.B_pad = L.B_pad; D.R = R;
    D.likelihood = p->d.likelihood; D.n_uniform_grad = p->d.n_uniform_grad;
    D.q_loc_u = p->d.q_loc_u; D.q_scale_u = p->d.q_scale_u; D.prior_loc_u = p->d.prior_loc_u; D.prior_scale_u = p->d.prior_scale_u;
    D.q_loc_stride = p->d.q_loc_stride; D.q_scale_stride = p->d.q_scale_stride;
    D.prior_loc_stride = p->d.prior_loc_stride; D.prior_scale_stride = p->d.prior_scale_stride;
    D.seed_lo = (uint32_t)a->seed; D.seed_hi = (uint32_t)(a->seed >> 32);
    D.offset_lo = (uint32_t)a->offset; D.offset_hi = (uint32_t)(a->offset >> 32);
    const uint32_t n_tiles = (L.B_pad / 64u) * (L.P_pad / 64u), n_rowp = (R + 255u) / 256u;
    const hipStream_t s = (hipStream_t)a->stream;
    hipLaunchKernelGGL(dense_head, dim3(n_tiles + n_rowp), dim3(256), 0, s, D, 0u, n_tiles);
    DenseLocal T;
    memset(&T, 0, sizeof(T));
    T.Xb = D.Xb; T.XbT = D.XbT; T.lab = D.lab; T.rowp = D.rowp; T.noise_in = a->noise_dev; T.noise_out = a->noise_out_dev;
    T.dM = (float*)(ws + L.dM); T.dV = (float*)(ws + L.dV); T.jM = (float*)(ws + L.jM); T.jV = (float*)(ws + L.jV);
    T.likp = (float*)(ws + L.likp); T.rowg = (float*)(ws + L.rowg); T.hpart = (float*)(ws + L.hpart); T.partial = D.partial;
    T.N = N; T.C = C; T.P = P; T.R = R; T.B = p->d.batch_size; T.B_pad = L.B_pad; T.P_pad = L.P_pad;
    T.row_tiles = L.row_tiles; T.k_chunks = L.k_chunks; T.col_tiles = L.col_tiles; T.splits = L.splits; T.samples_per_split = L.samples_per_split;
    T.likelihood = p->d.likelihood; T.n_uniform_grad = p->d.n_uniform_grad;
    T.base[0] = D.q_loc_u; T.base[1] = D.q_scale_u; T.base[2] = D.prior_loc_u; T.base[3] = D.prior_scale_u;
    T.stride[0] = D.q_loc_stride; T.stride[1] = D.q_scale_stride; T.stride[2] = D.prior_loc_stride; T.stride[3] = D.prior_scale_stride;
    T.lik_weight = p->d.lik_weight; T.prior_weight = p->d.prior_weight; T.entropy_weight = p->d.entropy_weight;
    T.seed_lo = D.seed_lo; T.seed_hi = D.seed_hi; T.offset_lo = D.offset_lo; T.offset_hi = D.offset_hi;
    const dim3 grid(L.row_tiles, L.splits), block(256);
    switch (L.CT) {
    case 1: hipLaunchKernelGGL(dense_local_fwd<1>, grid, block, 0, s, T); break;
    case 4: hipLaunchKernelGGL(dense_local_fwd<4>, grid, block, 0, s, T); break;
    case 10: hipLaunchKernelGGL(dense_local_fwd<10>, grid, block, 0, s, T); break;
    default: hipLaunchKernelGGL(dense_local_fwd<16>, grid, block, 0, s, T);
    }
    const bool joined = L.splits > 1u;
    if (joined) hipLaunchKernelGGL(dense_local_join, dim3(L.row_tiles * 4u), block, 0, s, T);
    hipLaunchKernelGGL(dense_local_bwd, dim3(L.col_tiles), block, 0, s, T, joined ? T.jM : T.dM, joined ? T.jV : T.dV);
    hipLaunchKernelGGL(dense_local_tail, dim3(1), block, 0, s, T);
    // the dense path's parameter kernel, finalizing: f is already the mean over the samples (n_global = 1)
    RParams Rp;
    memset(&Rp, 0, sizeof(Rp));
    Rp.uniform = p->uniform; Rp.pu_ptr = p->pu_ptr; Rp.pu_idx = p->pu_idx; Rp.partials = D.partial; Rp.params = (float*)a->params_dev; Rp.out = a->out_dev;
    Rp.n_uniform_grad = p->d.n_uniform_grad; Rp.n_params = p->d.n_params; Rp.n_blocks = 1; Rp.n_global = 1; Rp.do_finalize = 1;
    Rp.loss_slot = a->loss_slot_dev; Rp.finite_slot = a->finite_slot_dev;
    const uint32_t n = p->d.n_params ? p->d.n_params : 1u;
    hipLaunchKernelGGL(dense_param_kernel, dim3((n + 255u) / 256u), block, 0, s, Rp);
    HIP_TRY(hipGetLastError());
    return BSVI_OK;
}
