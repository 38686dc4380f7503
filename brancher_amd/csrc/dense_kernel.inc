// dense_kernel.inc — the dense-link (matmul) path on the f32 matrix cores.  Included at the end
// of elbo_kernel.hip (one translation unit: it reuses reduce_kernel, wave_sum, Philox, the
// optimizer and the error helpers).
//
// Model shape (BASELINE config 4, examples/MNIST_logistic_regression.py:15-54):
//   q:  W[c][p] ~ Normal(mu[c][p], s[c][p])            mean-field, learnable through the uniform table
//   p:  W ~ Normal(mu0, s0)  (by the reference's name-collision rule mu0/s0 are usually q's own
//       roots, DESIGN.md §2),   k[b] ~ Categorical(logits = W x_b)  observed,  x a random minibatch
//   f[n] = sum_b log p(k_b | W_n x_b) + log p(W_n) + H[q]
//
// Data layout (all fp32, sample axis fastest, DESIGN.md §3):
//   eps  [R = C*P][n_pad]      standard normals; W[n][r] = mu[r] + s[r]*eps[r][n] is never stored
//   Xb   [B_pad][P_pad]        the gathered minibatch (zero padded), XbT [P_pad][B_pad] its transpose
//   dlog [C][n_pad][B_pad]     d f / d logits
// Kernels per iteration (6 launches, no atomics, every reduction in a fixed order):
//   dense_head       heterogeneous workgroups: eps (Philox or supplied) | row parameters from the uniform table |
//                    minibatch indices, labels and the gather of Xb / XbT in LDS-transposed 64x64 tiles
//                    (dense_prologue + dense_gather + dense_noise, in that order, when per-sample prior values
//                    are requested: the noise kernel then reads the row parameters)
//   dense_forward    MFMA GEMM, workgroup tile [16 samples x C classes] x [64 columns]; the A operand
//                    W = mu + s*eps is built while staging to LDS; log-softmax cross-entropy epilogue in
//                    registers -> lik, dlog
//   dense_backward   MFMA GEMM T_c[p][b] = sum_n eps[c,p,n] dlog[c,n,b], reduced against x -> d f/d s;
//                    the column sums of dlog (-> d f/d mu) and the row sums of eps, eps^2 ride along
//   dense_rows       per-row likelihood + prior + entropy gradients -> uniform-table adjoints
//   dense_epilogue   sum over samples of f, non-finite count, gradients of shared uniform entries
//   dense_param_kernel  chain rule to theta, finalize, optimizer step

#include "dense_select.h"
namespace dsel = bsvi_dense_select;      // the tile constants, the launch plan and the workspace layout

namespace bsvi {

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct DParams {
    const bsvi_uniform_entry* uniform;
    const float* consts;
    const float* params;
    const float* dataset;       // [DS][P]
    const float* labels;        // [DS]
    const float* noise_in;      // [R][n_local] or null
    const int32_t* indices_in;  // [B] or null
    float* noise_out;
    int32_t* indices_out;
    float* fvalue_out;
    // workspace
    float* rowp;        // [4][R]  mu, s, mu0, s0, then [R][2] {mu, s}
    int32_t* idx;       // [B_pad]
    float* Xb;          // [B_pad][P_pad]
    float* XbT;         // [P_pad][B_pad]
    float* lab;         // [B_pad]
    float* eps;         // [R][n_pad]
    float* pv_part;     // [row_chunks][n_pad]   per-sample prior value partial sums (per_sample launches only)
    float* qv_part;     // [row_chunks][n_pad]   per-sample -0.5 * sum_r eps^2: log q up to a constant (BlackBox only)
    float* s1;          // [ksplit][R]  sum_n eps        (written by dense_backward, column group 0)
    float* s2;          // [ksplit][R]  sum_n eps^2
    float* lik_part;    // [B_pad/64][n_pad]
    float* dlog;        // [C][n_pad][B_pad]
    float* ds_part;     // [ksplit * B_pad/64][R]   d f/d s  (likelihood part) per sample split and column group
    float* dmu_part;    // [ksplit * B_pad/64][R]   d f/d mu (likelihood part)
    float* rowg;        // [4][R]          row gradients of uniform entries shared by all rows (stride 0)
    float* hpart;       // [2][row blocks] per-block sums of dense_rows
    float* partial;     // [2 + n_uniform_grad]  block handed to reduce_kernel
    uint32_t C, P, P_pad, DS, B, B_pad, R;
    uint32_t n_local, n_global, n_pad, sample_base;
    uint32_t likelihood, n_uniform_grad;
    uint32_t q_loc_u, q_scale_u, prior_loc_u, prior_scale_u;
    uint32_t q_loc_stride, q_scale_stride, prior_loc_stride, prior_scale_stride;
    float lik_weight, prior_weight, entropy_weight;
    uint32_t seed_lo, seed_hi, offset_lo, offset_hi;
    uint32_t estimator;         // bsvi_estimator
    uint32_t per_sample;        // per-sample prior values are materialised: the caller wants f per sample, or BlackBox
    uint32_t row_chunk;         // rows per block of dense_noise
    uint32_t sums_folded;       // dense_sample_sums has added the row chunks of pv_part / qv_part into chunk 0
    uint32_t ksplit;            // sample-axis splits of dense_backward
    // the exact-data path (every dataset value is exactly a bf16 number: pixel counts, binarised images).  Both products of
    // the iteration then have ONE exact operand (the minibatch) and run on the bf16 matrix cores as three MFMAs on the
    // exact pieces hi + mid + lo of the other operand (bsvi_xgemm_nt, amort_kernel.hip):
    //   logitsT[b][(n, c)] = sum_p x[b][p] W[(n, c)][p]                      W = mu + s * eps, pieces written by dense_wsplit
    //   GT[p][(n, c)]      = sum_b x[b][p] dlog[(n, c)][b]                   dlog pieces written by dense_ce
    //   d f / d s[c][p] = sum_n eps[c][p][n] GT[p][(n, c)],  d f / d mu[c][p] = sum_n GT[p][(n, c)]      (dense_xreduce)
    // eps is never stored: dense_wsplit and dense_xreduce draw it from the same Philox counters.
    uint32_t xpath, Kp;         // Kp: features padded to the k step of the bf16 kernel
    uint16_t* Xb_bf;            // [B_pad][Kp]
    uint16_t* XbT_bf;           // [P][B_pad]
    uint16_t* Wp;               // [3][n_pad * C][Kp]
    float* logitsT;             // [B_pad][n_pad * C]
    uint16_t* dlogp;            // [3][n_pad * C][B_pad]
    float* GT;                  // [P][n_pad * C]
    uint32_t lik_parts;         // row chunks of lik_part that dense_epilogue adds per sample
    uint32_t xfused;            // the two fused launches (dense_xfused.inc): dlogp is class-major, [3][(c, n)][B_pad]
    unsigned long long* stamps; // profiling only (bsvi_debug_set_stamps): cycle counters of two workgroups of dense_xbwd
    // caller-weighted gradients (bsvi_dense_args::f_weight_dev / q_weight_dev, the second pass of a user-defined gradient
    // estimator):  sum_n a_n grad f_n + b_n grad log q_n.  The likelihood's d f / d logits carry a_n from the kernel that writes
    // them; the closed-form prior / entropy terms of dense_rows take A = sum a_n and the weighted row sums of eps, eps^2
    // (dense_weighted_sums); grad log q_n = -1 / s_r for every sample (dense_epilogue), so b enters as B = sum b_n.
    const float* f_weight;      // [n_local] or null (a_n = 1)
    const float* q_weight;      // [n_local] or null (BlackBox: b_n = f_n)
    float* logq_out;            // per-sample log q [n_local] or null (BlackBox plans)
    float* wsum;                // [2]  A, B
    float* ws1;                 // [R]  sum_n a_n eps
    float* ws2;                 // [R]  sum_n a_n eps^2
};

__device__ __forceinline__ uint16_t dense_bf16_bits(float x) { const __bf16 b = (__bf16)x; return __builtin_bit_cast(uint16_t, b); }
__device__ __forceinline__ float dense_bf16_value(uint16_t b) { return __uint_as_float((uint32_t)b << 16); }
// the three bf16 pieces of an f32: hi = rne(w), mid = rne(w - hi), lo = rne(w - hi - mid); hi + mid + lo == w exactly
__device__ __forceinline__ void dense_split3(float w, uint16_t& hi, uint16_t& mid, uint16_t& lo) {
    hi = dense_bf16_bits(w);
    const float r1 = w - dense_bf16_value(hi);
    mid = dense_bf16_bits(r1);
    lo = dense_bf16_bits(r1 - dense_bf16_value(mid));
}
// the normals of rows 4g .. 4g+3 of sample n: the one definition of the dense path's noise (dense_noise / dense_head draw the same)
__device__ __forceinline__ void dense_eps4(const DParams& D, uint32_t n, uint32_t g, float e[4]) {
    const u32x4 x = philox4x32(D.sample_base + n, g | 0x40000000u, D.offset_lo, D.offset_hi, D.seed_lo, D.seed_hi);
    box_muller_fast(x.x, x.y, e[0], e[1]);
    box_muller_fast(x.z, x.w, e[2], e[3]);
}

__device__ __forceinline__ float uniform_value(const DParams& D, uint32_t k) {
    const bsvi_uniform_entry e = D.uniform[k];
    const float x = e.is_param ? D.params[e.src] : D.consts[e.src];
    return e.a + e.b * utransform(e.transform, x);
}

// minibatch row b: supplied, or the keyed bijection of [0, DS) of minibatch_index.h (the one definition: the generated
// kernels' in-loop gather draws the same rows)
__device__ __forceinline__ uint32_t minibatch_index(const DParams& D, uint32_t b) {
    if (D.indices_in) return (uint32_t)D.indices_in[b];
    return minibatch_index_keyed(D.DS, D.seed_lo, D.seed_hi, D.offset_lo, D.offset_hi, b);
}

// LDS stores of staged fragments are built from the components (a HIP float4 object copied through a pointer cast can
// pin the whole fragment in scratch memory: amort_kernel.hip, DESIGN 4.6)
typedef float f32x4v __attribute__((ext_vector_type(4)));

__global__ void dense_prologue(const DParams D) {
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x, nth = gridDim.x * blockDim.x;
    for (uint32_t r = tid; r < D.R; r += nth) {
        const float loc = uniform_value(D, D.q_loc_u + r * D.q_loc_stride);
        const float scale = uniform_value(D, D.q_scale_u + r * D.q_scale_stride);
        D.rowp[r] = loc;
        D.rowp[D.R + r] = scale;
        D.rowp[4 * (size_t)D.R + 2 * r] = loc;          // interleaved copy: one 8-byte load in dense_forward
        D.rowp[4 * (size_t)D.R + 2 * r + 1] = scale;
        D.rowp[2 * D.R + r] = uniform_value(D, D.prior_loc_u + r * D.prior_loc_stride);
        D.rowp[3 * D.R + r] = uniform_value(D, D.prior_scale_u + r * D.prior_scale_stride);
    }
    for (uint32_t b = tid; b < D.B_pad; b += nth) {
        const int32_t i = b < D.B ? (int32_t)minibatch_index(D, b) : -1;
        D.idx[b] = i;
        D.lab[b] = i >= 0 ? D.labels[i] : 0.0f;
        if (D.indices_out && b < D.B) D.indices_out[b] = i;
    }
    for (uint32_t k = tid; k < 2 + D.n_uniform_grad; k += nth) D.partial[k] = 0.0f;
}

// gather the minibatch rows (EmpiricalDistribution._get_sample, distributions.py:446-457)
__global__ void dense_gather(const DParams D) {
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x, nth = gridDim.x * blockDim.x;
    for (uint32_t i = tid; i < D.B_pad * D.P_pad; i += nth) {
        const uint32_t b = i / D.P_pad, p = i - b * D.P_pad;
        const int32_t row = D.idx[b];
        const float v = (row >= 0 && p < D.P) ? D.dataset[(size_t)row * D.P + p] : 0.0f;
        D.Xb[i] = v;
        D.XbT[(size_t)p * D.B_pad + b] = v;
        if (D.xpath) {
            if (p < D.Kp) D.Xb_bf[(size_t)b * D.Kp + p] = dense_bf16_bits(v);
            if (p < D.P) D.XbT_bf[(size_t)p * D.B_pad + b] = dense_bf16_bits(v);
        }
    }
}

// eps.  Block = 256 samples x row_chunk rows; Philox counter = (sample, row/4): one call feeds 4 rows.
// The per-sample prior value is only materialised when the caller asked for per-sample f values;
// its sum over samples comes analytically from sum eps, sum eps^2 (dense_rows).
__global__ void __launch_bounds__(256) dense_noise(const DParams D) {
    const uint32_t n = blockIdx.x * 256 + threadIdx.x;
    const uint32_t r0 = blockIdx.y * D.row_chunk, r1 = min(r0 + D.row_chunk, D.R);
    const bool live = n < D.n_local;
    const bool want_pv = D.per_sample != 0, want_qv = D.estimator == BSVI_EST_BLACKBOX;
    float pv = 0.0f, qv = 0.0f;
    const float* mu = D.rowp;
    const float* s = D.rowp + D.R;
    const float* mu0 = D.rowp + 2 * D.R;
    const float* s0 = D.rowp + 3 * D.R;
    for (uint32_t r = r0; r < r1; r += 4) {
        float e[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (D.noise_in) {
            for (uint32_t j = 0; j < 4 && r + j < r1; ++j)
                if (live) e[j] = D.noise_in[(size_t)(r + j) * D.n_local + n];
        } else if (live) {
            const u32x4 x = philox4x32(D.sample_base + n, (r >> 2) | 0x40000000u, D.offset_lo, D.offset_hi, D.seed_lo, D.seed_hi);
            box_muller_fast(x.x, x.y, e[0], e[1]);
            box_muller_fast(x.z, x.w, e[2], e[3]);
        }
        for (uint32_t j = 0; j < 4 && r + j < r1; ++j) {
            const uint32_t rr = r + j;
            const float ej = e[j];
            if (n < D.n_pad) D.eps[(size_t)rr * D.n_pad + n] = ej;
            if (D.noise_out && live) D.noise_out[(size_t)rr * D.n_local + n] = ej;
            if (want_pv) {
                // log N(W | mu0, s0) with W = mu + s*eps, constants added in the epilogue
                const float u = (mu[rr] - mu0[rr] + s[rr] * ej) / s0[rr];
                pv += live ? -0.5f * u * u : 0.0f;
                if (want_qv) qv += live ? -0.5f * ej * ej : 0.0f;      // log N(W | mu, s) = -eps^2 / 2 - log s - const
            }
        }
    }
    if (want_pv && n < D.n_pad) D.pv_part[(size_t)blockIdx.y * D.n_pad + n] = pv;
    if (want_qv && n < D.n_pad) D.qv_part[(size_t)blockIdx.y * D.n_pad + n] = qv;
    // the 32 slack rows behind eps (read, never used, by the last feature chunk of dense_forward) stay finite
    if (blockIdx.y == 0 && n < D.n_pad)
        for (uint32_t rr = 0; rr < 32; ++rr) D.eps[(size_t)(D.R + rr) * D.n_pad + n] = 0.0f;
}

// The three heads of an iteration in ONE launch (they are independent when no per-sample prior value is asked
// for): eps generation, row parameters, and the minibatch gather.  Heterogeneous workgroups: the launch boundary
// between them (and the 15 us the short ones took while the chip idled) disappears, the VALU-bound noise blocks
// and the memory-bound gather tiles share the CUs.  (Cross-stream fork/join with events was tried first: the two
// waits cost what the overlap bought.)
//   blocks [0, n_noise)              eps rows (as dense_noise)
//   blocks [n_noise, +n_tiles)       gather of a 64-row x 64-feature tile, transposed through LDS so that Xb is
//                                    written along features and XbT along minibatch rows, both coalesced;
//                                    each tile derives the minibatch indices of its 64 rows itself
//   blocks [.., +n_rowp)             row parameters from the uniform table; the first also clears `partial`
__global__ void __launch_bounds__(256) dense_head(const DParams D, uint32_t n_noise, uint32_t n_tiles) {
    __shared__ float tile[64][65];
    __shared__ int32_t rows[64];
    const uint32_t tid = threadIdx.x;
    if (blockIdx.x < n_noise) {
        const uint32_t nbx = D.n_pad / 256 ? (D.n_pad + 255) / 256 : 1;
        const uint32_t bx = blockIdx.x % nbx, by = blockIdx.x / nbx;
        const uint32_t n = bx * 256 + tid;
        const uint32_t r0 = by * D.row_chunk, r1 = min(r0 + D.row_chunk, D.R);
        const bool live = n < D.n_local;
        for (uint32_t r = r0; r < r1; r += 4) {
            float e[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (D.noise_in) {
                for (uint32_t j = 0; j < 4 && r + j < r1; ++j)
                    if (live) e[j] = D.noise_in[(size_t)(r + j) * D.n_local + n];
            } else if (live) {
                const u32x4 x = philox4x32(D.sample_base + n, (r >> 2) | 0x40000000u, D.offset_lo, D.offset_hi, D.seed_lo, D.seed_hi);
                box_muller_fast(x.x, x.y, e[0], e[1]);
                box_muller_fast(x.z, x.w, e[2], e[3]);
            }
            for (uint32_t j = 0; j < 4 && r + j < r1; ++j) {
                if (n < D.n_pad) D.eps[(size_t)(r + j) * D.n_pad + n] = e[j];
                if (D.noise_out && live) D.noise_out[(size_t)(r + j) * D.n_local + n] = e[j];
            }
        }
        // the 32 slack rows behind eps (read, never used, by the last feature chunk of dense_forward) stay finite
        if (by == 0 && n < D.n_pad)
            for (uint32_t rr = 0; rr < 32; ++rr) D.eps[(size_t)(D.R + rr) * D.n_pad + n] = 0.0f;
        return;
    }
    const uint32_t g = blockIdx.x - n_noise;
    if (g < n_tiles) {
        const uint32_t ptiles = D.P_pad / 64, tb = g / ptiles, tp = g - tb * ptiles;
        const uint32_t b0 = tb * 64, p0 = tp * 64;
        if (tid < 64) {
            const uint32_t b = b0 + tid;
            const int32_t i = b < D.B ? (int32_t)minibatch_index(D, b) : -1;
            rows[tid] = i;
            if (tp == 0) {
                D.idx[b] = i;
                D.lab[b] = i >= 0 ? D.labels[i] : 0.0f;
                if (D.indices_out && b < D.B) D.indices_out[b] = i;
            }
        }
        __syncthreads();
        const uint32_t c = tid & 63u, q = tid >> 6;            // 4 rows of 64 columns per pass
        // (all 16 row loads of a thread in flight at once: taken one by one, each waited ~1 us for a random dataset row and
        //  the gather was a 12 us chain at config 4)
        float vals[16];
        const uint32_t p = p0 + c;
#pragma unroll
        for (uint32_t k = 0; k < 16; ++k) {
            const int32_t row = rows[q + 4 * k];
            vals[k] = (row >= 0 && p < D.P) ? D.dataset[(size_t)row * D.P + p] : 0.0f;
        }
#pragma unroll
        for (uint32_t k = 0; k < 16; ++k) {
            const uint32_t rr = q + 4 * k;
            const float v = vals[k];
            if (!D.xfused) D.Xb[(size_t)(b0 + rr) * D.P_pad + p] = v;       // (the fused exact-data launches read the bf16 copies only)
            if (D.xpath && p < D.Kp) {
                const uint32_t b = b0 + rr;
                // (fused form: fragment-major for dense_xfwd — element (b, k) of 32-row block b >> 5, k chunk k >> 4, lane ((k >> 3) & 1) * 32 + (b & 31))
                const size_t at = D.xfused ? ((((size_t)(b >> 5) * (D.Kp / 16u) + (p >> 4)) * 64u + ((p >> 3) & 1u) * 32u + (b & 31u)) * 8u + (p & 7u))
                                           : (size_t)b * D.Kp + p;
                D.Xb_bf[at] = dense_bf16_bits(v);
            }
            tile[rr][c] = v;
        }
        __syncthreads();
        for (uint32_t pp = q; pp < 64; pp += 4) {
            if (!D.xfused) D.XbT[(size_t)(p0 + pp) * D.B_pad + b0 + c] = tile[c][pp];
            if (D.xpath && p0 + pp < D.P) D.XbT_bf[(size_t)(p0 + pp) * D.B_pad + b0 + c] = dense_bf16_bits(tile[c][pp]);
        }
        return;
    }
    const uint32_t blk = g - n_tiles, r = blk * 256 + tid;
    if (r < D.R) {
        const float loc = uniform_value(D, D.q_loc_u + r * D.q_loc_stride);
        const float scale = uniform_value(D, D.q_scale_u + r * D.q_scale_stride);
        D.rowp[r] = loc;
        D.rowp[D.R + r] = scale;
        D.rowp[4 * (size_t)D.R + 2 * r] = loc;          // interleaved copy: one 8-byte load in dense_forward
        D.rowp[4 * (size_t)D.R + 2 * r + 1] = scale;
        D.rowp[2 * D.R + r] = uniform_value(D, D.prior_loc_u + r * D.prior_loc_stride);
        D.rowp[3 * D.R + r] = uniform_value(D, D.prior_scale_u + r * D.prior_scale_stride);
    }
    if (blk == 0) {
        for (uint32_t k = tid; k < 2 + D.n_uniform_grad; k += 256) D.partial[k] = 0.0f;
    }
}

// 16-lane row sum (a DPP row): every lane of the row gets the total
__device__ __forceinline__ float row16_sum(float v) {
    v += dpp_f<0xB1>(v);
    v += dpp_f<0x4E>(v);
    v += dpp_f<0x141>(v);
    v += dpp_f<0x140>(v);
    return v;
}

// Forward GEMM + likelihood.  Workgroup = 4 waves = ONE block of 16 samples x 64 minibatch columns
// (16 per wave, all classes): the A operand W = mu + s*eps of the 16 samples is identical for the four
// waves, so it is built once per 32-feature chunk while staging to LDS.  Tiles are small on purpose:
// 2 workgroups share a CU, so the staging / epilogue phases of one overlap the MFMA phase of the other.
// Chunk i+1 is prefetched into registers while the 8*CT MFMAs per wave of chunk i run.
// (Tried: 32 columns per wave, i.e. each A fragment reused twice and half the LDS reads per MFMA, one workgroup
//  per CU: 120 us against 104 us — the second resident workgroup is worth more than the LDS traffic.)
// MFMA v_mfma_f32_16x16x4_f32: A[i = l&15][k = l>>4], B[k = l>>4][j = l&15], D: col = l&15, row = (l>>4)*4 + reg.
// (CT = 16: the two eps buffers alone are 64 KB, one workgroup per CU — asking for two only earned a -Wpass-failed warning)
template <int CT>
__global__ void __launch_bounds__(256, CT <= 10 ? 2 : 1) dense_forward(const DParams D) {
    constexpr int XS = 80;                           // row stride of the x tile: = 16 (mod 32) keeps the
    constexpr int XSZ = 32 * XS, ESZ = CT * 32 * 16; // two 32-lane halves of a wave on disjoint banks
    __shared__ __attribute__((aligned(16))) float xs2[2 * XSZ];                   // double buffered: chunk i+1 is committed while chunk i
    __shared__ __attribute__((aligned(16))) float es2[2 * ESZ];                   // is still being read -> one barrier per chunk
    __shared__ float likred[4][16];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    // XCD-aware tile order: workgroup ids go round-robin over the 8 XCDs (id % 8), each with its own L2.
    // XCD x takes a contiguous run of sample blocks and all column blocks of it, so every 128-byte line
    // of eps is filled into exactly one L2 instead of one half per XCD.
    const uint32_t nblocks = D.n_pad / 16, id = blockIdx.x;
    uint32_t nblk, yblk;
    if ((nblocks & 7u) == 0) {
        const uint32_t per = nblocks >> 3, q = id >> 3;
        nblk = (id & 7u) * per + q % per;
        yblk = q / per;
    } else {
        nblk = id % nblocks;
        yblk = id / nblocks;
    }
    const uint32_t n0 = nblk * 16, bw0 = yblk * 64, b0 = bw0 + wave * 16;      // B_pad is a multiple of 64
    const uint32_t li = lane & 15u, lk = lane >> 4;
    f32x4 acc[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) acc[c] = 0.0f;
    // Staging is float4 wide: the address pipeline of a CU retires one 64-lane load instruction per ~16
    // cycles whatever its width, and with dword loads (70 per thread and chunk) it, not the matrix core,
    // set the pace.  Per chunk a thread now issues EP4 x (eps float4 + {loc, scale} float2) + 2 x float4.
    // float4 i4 = tid + 256 j of the eps tile is (class c = tid/128 + 2j, feature k = (tid/4)%32, samples 4*(tid%4)..+3).
    constexpr int EP4 = (CT * 128 + 255) / 256;
    static_assert(EP4 <= 8, "staging schedule below covers 8 eps float4 per thread");
    // The f32-input MFMA runs on the same FMA lanes as the vector ALU (it has the vector rate): VALU
    // instructions do not hide behind it, they add to it.  The staging below is therefore built to need
    // almost none: every address is (scalar base) + (per-thread byte offset fixed for the whole kernel)
    // -> `global_load v, voff, s[base]`, LDS addresses are (per-thread base) + immediate.
    const float2* ms = reinterpret_cast<const float2*>(D.rowp + 4 * (size_t)D.R);      // {loc, scale} per row
    // two register sets: chunk i+2 is being loaded into one while chunk i+1 is written to LDS from the other
    float4 er[2][EP4], xr[2][2];
    float2 mr[2][EP4];
    // float4 i4 = tid + 256 j of the eps tile: class c = tid/128 + 2j (wave-uniform), feature k = (tid/4)%32,
    // samples 4*(tid%4)..+3
    const uint32_t kt = (tid >> 2) & 31u;
    const uint32_t chalf = __builtin_amdgcn_readfirstlane(tid >> 7);
    const uint32_t e_voff = (kt * D.n_pad + n0 + 4u * (tid & 3u)) * 4u;      // bytes
    const uint32_t m_voff = kt * 8u;
    const uint32_t x_voff = ((tid >> 4) * D.B_pad + 4u * (tid & 15u)) * 4u;   // rows of the transposed minibatch
    // Rows past P of the last chunk read the next class's rows or the 32 zeroed slack rows behind eps
    // (finite either way) and get loc = scale = 0; classes past C re-read class C-1 the same way.
    auto fetch_e = [&](auto set, int j, uint32_t p) {
        constexpr int S = decltype(set)::value;
        if (j >= EP4) return;
        const uint32_t row = min(chalf + 2u * j, D.C - 1) * D.P + p;                      // scalar
        er[S][j] = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(D.eps + (size_t)row * D.n_pad) + e_voff);
        mr[S][j] = *reinterpret_cast<const float2*>(reinterpret_cast<const char*>(ms + row) + m_voff);
    };
    auto fetch_x = [&](auto set, uint32_t p) {
        constexpr int S = decltype(set)::value;
#pragma unroll
        for (int j = 0; j < 2; ++j)                                    // (k = tid/16 + 16j, columns 4*(tid%16)..+3)
            xr[S][j] = *reinterpret_cast<const float4*>(
                reinterpret_cast<const char*>(D.XbT + (size_t)(p + 16u * j) * D.B_pad + bw0) + x_voff);
    };
    auto commit_e = [&](auto set, int j, uint32_t p, float* ew) {
        constexpr int S = decltype(set)::value;
        if (j >= EP4) return;
        const bool ok = (chalf + 2u * j < D.C) && (p + kt < D.P);
        const float m = ok ? mr[S][j].x : 0.0f, sc = ok ? mr[S][j].y : 0.0f;
        float4 w;
        w.x = fmaf(sc, er[S][j].x, m);
        w.y = fmaf(sc, er[S][j].y, m);
        w.z = fmaf(sc, er[S][j].z, m);
        w.w = fmaf(sc, er[S][j].w, m);
        if (CT * 128 % 256 == 0 || tid + 256u * j < CT * 128u) *reinterpret_cast<f32x4v*>(ew + 4u * (tid + 256u * j)) = f32x4v{w.x, w.y, w.z, w.w};
    };
    auto commit_x = [&](auto set, float* xw) {
        constexpr int S = decltype(set)::value;
#pragma unroll
        for (int j = 0; j < 2; ++j)
            *reinterpret_cast<f32x4v*>(xw + ((tid >> 4) + 16u * j) * XS + 4u * (tid & 15u)) = f32x4v{xr[S][j].x, xr[S][j].y, xr[S][j].z, xr[S][j].w};
    };
    float a_n[CT], b_n;
    const float* xs_lane = xs2 + lk * XS + wave * 16 + li;       // + (cur*XSZ + 4*st*XS) immediates
    const float* es_lane = es2 + lk * 16 + li;                   // + (cur*ESZ + (c*32 + 4*st)*16) immediates
    const uint32_t p_end = (D.P + 31u) & ~31u, p_last = p_end - 32;
    using set0 = std::integral_constant<int, 0>;
    using set1 = std::integral_constant<int, 1>;
    // One chunk = 8 steps of CT MFMAs.  Per step: the LDS reads of step st+1, a slice of the staging of the
    // following chunks (global loads of chunk i+2 in steps 0-3 into register set `ld`; LDS writes of chunk
    // i+1 in steps 4-7 from the other set into the buffer last read before the previous barrier), then
    // the MFMAs.  Loads have a whole chunk (~1.5 us) to land.  Chunks past the end re-stage the last one
    // into an idle buffer, so there is no branch inside a chunk.
    auto chunk = [&](auto ld, auto st_set, auto curc, uint32_t p0) {
        constexpr int CUR = decltype(curc)::value;
        float* xw = xs2 + (CUR ^ 1) * XSZ;
        float* ew = es2 + (CUR ^ 1) * ESZ;
        const uint32_t p_ld = min(p0 + 64, p_last), p_st = min(p0 + 32, p_last);
        auto frags = [&](int st) {
            b_n = xs_lane[CUR * XSZ + 4 * st * XS];
#pragma unroll
            for (int c = 0; c < CT; ++c) a_n[c] = es_lane[CUR * ESZ + (c * 32 + 4 * st) * 16];
        };
        frags(0);
#pragma unroll
        for (int st = 0; st < 8; ++st) {
            float a_c[CT];
            const float bf = b_n;
#pragma unroll
            for (int c = 0; c < CT; ++c) a_c[c] = a_n[c];
            // keep the LDS reads of step st+1 ahead of the MFMAs of step st: left alone, the scheduler sinks
            // each read next to its use and every pair of MFMAs then waits out an LDS round trip
            __builtin_amdgcn_sched_barrier(0);
            if (st < 7) frags(st + 1);
            if (st < 4) { fetch_e(ld, 2 * st, p_ld); fetch_e(ld, 2 * st + 1, p_ld); }
            if (st == 3) fetch_x(ld, p_ld);
            if (st >= 4) { commit_e(st_set, 2 * (st - 4), p_st, ew); commit_e(st_set, 2 * (st - 4) + 1, p_st, ew); }
            if (st == 7) commit_x(st_set, xw);
            __builtin_amdgcn_sched_barrier(0);
            // classes past C (CT is the next compiled size) multiply zeros: no branch in the MFMA stream
#pragma unroll
            for (int c = 0; c < CT; ++c) acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_c[c], bf, acc[c], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();
    };
    // prologue: chunk 0 -> LDS buffer 0, chunk 1 -> register set 1
#pragma unroll
    for (int j = 0; j < EP4; ++j) fetch_e(set0{}, j, 0);
    fetch_x(set0{}, 0);
#pragma unroll
    for (int j = 0; j < EP4; ++j) fetch_e(set1{}, j, min(32u, p_last));
    fetch_x(set1{}, min(32u, p_last));
#pragma unroll
    for (int j = 0; j < EP4; ++j) commit_e(set0{}, j, 0, es2);
    commit_x(set0{}, xs2);
    __syncthreads();
    for (uint32_t p0 = 0; p0 < p_end; p0 += 64) {
        chunk(set0{}, set1{}, set0{}, p0);
        if (p0 + 32 < p_end) chunk(set1{}, set0{}, set1{}, p0 + 32);
    }
    // ---- epilogue: this lane holds activations[n = n0 + lk*4 + j][b = b0 + li][c] for all c
    float lik[4];
    const uint32_t b = b0 + li;
    const float label = D.lab[b];
    const bool bvalid = b < D.B;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t n = n0 + lk * 4 + j;
        const float w = (bvalid && n < D.n_local) ? D.lik_weight * (D.f_weight ? D.f_weight[n] : 1.0f) : 0.0f;
        if (D.likelihood == BSVI_LIK_CATEGORICAL) {
            // log-softmax cross entropy (Categorical logits, distributions.py:276-296): one exp per class
            float m = acc[0][j];
#pragma unroll
            for (int c = 1; c < CT; ++c) if (c < (int)D.C) m = fmaxf(m, acc[c][j]);
            float e[CT], se = 0.0f, zl = 0.0f;
#pragma unroll
            for (int c = 0; c < CT; ++c) {
                e[c] = (c < (int)D.C) ? __expf(acc[c][j] - m) : 0.0f;
                se += e[c];
                zl = (label == (float)c) ? acc[c][j] : zl;
            }
            // se >= 1 (the maximum contributes exp(0)): a normal float, so log and reciprocal are one instruction each
            lik[j] = w * (zl - (m + __builtin_amdgcn_logf(se) * 0.6931471805599453f));
            const float wr = w * __builtin_amdgcn_rcpf(se);
#pragma unroll
            for (int c = 0; c < CT; ++c)
                if (c < (int)D.C)
                    D.dlog[((size_t)c * D.n_pad + n) * D.B_pad + b] = ((label == (float)c) ? w : 0.0f) - wr * e[c];
        } else {   // Bernoulli / Binomial(1): -binary_cross_entropy_with_logits(l, k)
            const float l = acc[0][j];
            lik[j] = w * (label * l - (fmaxf(l, 0.0f) + log1pf(expf(-fabsf(l)))));
            D.dlog[((size_t)n) * D.B_pad + b] = w * (label - sigmoidf_(l));
        }
    }
    // sum over the 64 columns of the workgroup: 16 lanes of a row (DPP), then the four waves in fixed order
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float tot = row16_sum(lik[j]);
        if (li == 0) likred[wave][lk * 4 + j] = tot;
    }
    __syncthreads();
    if (tid < 16)
        D.lik_part[(size_t)yblk * D.n_pad + n0 + tid] = (likred[0][tid] + likred[1][tid]) + (likred[2][tid] + likred[3][tid]);
}

// Backward GEMM.  Workgroup = 4 waves = (class c, 64 features [16 per wave], 64 minibatch columns):
//   T[p][b] = sum_n eps[c,p,n] * dlog[c,n,b]      (K = samples)
//   d f / d s[c,p] (likelihood part) = sum_b x[b][p] * T[p][b]
// The B operand (a [16 samples x 64 columns] tile of dlog per step) is shared by the four waves
// through LDS; A is private: each lane reads float4 along n (K-contiguous), so MFMA step q of a
// 16-sample group uses k = 4*lk + q and the B fragment is read with the same permutation.  Both
// operands of step i+1 are in registers before the 16 MFMAs of step i issue.
// Riding along on data that is already in registers:
//   dbar[b] = sum_n dlog[c,n,b]  (column sums of the B tiles)  ->  d f/d mu[c,p] = sum_b x[b][p] dbar[b]
//   S1[c,p] = sum_n eps, S2[c,p] = sum_n eps^2  (row sums of A; column group 0 only)  for the prior terms
__global__ void __launch_bounds__(256) dense_backward(const DParams D) {
    constexpr int BS = 68;                           // = 4 (mod 8): rows 4*lk of the two lane halves
    constexpr int TSZ = 32 * BS;                     // fall on disjoint banks; tile = 32 samples x 64 columns
    __shared__ __attribute__((aligned(16))) float bs2[2 * TSZ];                   // double buffered: one barrier per 32-sample step
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    // grid = (class, sample split) units x 64-feature groups x 64-column groups.  The sample axis (the K
    // of this GEMM) is cut in `ksplit`; the pieces are added by dense_rows in fixed order.
    // XCD-aware order: workgroup ids go round-robin over the 8 XCDs (id % 8).  All workgroups of one
    // (class, split) unit run on ONE XCD, so its slice of eps (A) and of dlog (B) is pulled through the
    // fabric into exactly one L2: with column groups spread over the XCDs instead, PMC FETCH_SIZE showed
    // eps crossing the fabric 8 times (277 MB per launch against 53 MB of operands).
    const uint32_t pgroups = (D.P + 63) / 64, bgroups = D.B_pad / 64, inner = pgroups * bgroups;
    const uint32_t units = D.C * D.ksplit;
    uint32_t unit, rem;
    if ((units & 7u) == 0) {
        const uint32_t q = blockIdx.x >> 3;
        unit = (blockIdx.x & 7u) + 8u * (q / inner);
        rem = q % inner;
    } else {
        unit = blockIdx.x / inner;
        rem = blockIdx.x % inner;
    }
    const uint32_t c = unit / D.ksplit, ks = unit % D.ksplit, bg = rem % bgroups, cp = c * pgroups + rem / bgroups;
    const uint32_t part = ks * bgroups + bg;
    const uint32_t n_lo = ks * (D.n_pad / D.ksplit), n_hi = n_lo + D.n_pad / D.ksplit;
    const uint32_t p0 = (cp - c * pgroups) * 64 + wave * 16, b0 = bg * 64;
    const uint32_t li = lane & 15u, lk = lane >> 4;
    const uint32_t prow = min(p0 + li, D.P - 1);
    const float* arow = D.eps + (size_t)(c * D.P + prow) * D.n_pad + n_lo + 4 * lk;
    const uint32_t fr = tid >> 4, fc = (tid & 15u) * 4;      // this thread's float4s of the B tile: rows fr, fr+16
    const float* brow = D.dlog + ((size_t)c * D.n_pad + n_lo) * D.B_pad + b0 + (size_t)fr * D.B_pad + fc;
    const size_t brow16 = (size_t)16 * D.B_pad;
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = 0.0f;
    // n_pad / ksplit is a multiple of 32, so 32-sample steps tile a split exactly.  Two register sets:
    // the operands of step i+2 are requested while step i computes, so a load has two steps (~2 us) to land;
    // the B tile of step i+1 goes from its registers to the idle LDS buffer after the MFMAs of step i.
    const uint32_t n_len = n_hi - n_lo, n_last = n_len - 32;
    float4 Ar[2][2], Br[2][2];
    float4 dsum = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float s1 = 0.0f, s2 = 0.0f;
    using set0 = std::integral_constant<int, 0>;
    using set1 = std::integral_constant<int, 1>;
    auto load = [&](auto set, uint32_t nb) {
        constexpr int S = decltype(set)::value;
        Ar[S][0] = *reinterpret_cast<const float4*>(arow + nb);
        Ar[S][1] = *reinterpret_cast<const float4*>(arow + nb + 16);
        Br[S][0] = *reinterpret_cast<const float4*>(brow + (size_t)nb * D.B_pad);
        Br[S][1] = *reinterpret_cast<const float4*>(brow + (size_t)nb * D.B_pad + brow16);
    };
    auto stage = [&](auto set, float* bw, float keep) {
        constexpr int S = decltype(set)::value;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            *reinterpret_cast<f32x4v*>(&bw[(fr + 16 * h) * BS + fc]) = f32x4v{Br[S][h].x, Br[S][h].y, Br[S][h].z, Br[S][h].w};
            dsum.x += keep * Br[S][h].x; dsum.y += keep * Br[S][h].y; dsum.z += keep * Br[S][h].z; dsum.w += keep * Br[S][h].w;
        }
    };
    // (a wave past the last feature multiplies clamped rows and drops the result: no branch around the MFMAs,
    //  which would bounce the accumulators between register files every step)
    auto step = [&](auto set, auto other, uint32_t nb) {
        constexpr int S = decltype(set)::value;
        const float* bs = bs2 + S * TSZ;
        const float av[8] = {Ar[S][0].x, Ar[S][0].y, Ar[S][0].z, Ar[S][0].w, Ar[S][1].x, Ar[S][1].y, Ar[S][1].z, Ar[S][1].w};
        __builtin_amdgcn_sched_barrier(0);
        load(set, min(nb + 64, n_last));          // past the end: re-reads the last step, never used
        // (every column group accumulates the row sums, group 0 stores them: a branch here would split the step)
#pragma unroll
        for (int h = 0; h < 8; h += 4) {
            s1 += (av[h] + av[h + 1]) + (av[h + 2] + av[h + 3]);
            s2 += (av[h] * av[h] + av[h + 1] * av[h + 1]) + (av[h + 2] * av[h + 2] + av[h + 3] * av[h + 3]);
        }
        // 8 groups of 4 MFMAs (one A value against the 4 column tiles); the B fragments of group g+2 are
        // requested from LDS before the MFMAs of group g issue (sched_barrier pins that order: left alone,
        // the scheduler sinks each read next to its use and every MFMA pair waits out an LDS round trip)
        float bq[3][4];
        auto bfrag = [&](int g, float* out) {      // group g: tile row 16*(g/4) + 4*lk + (g%4)
            const uint32_t row = 16u * (g >> 2) + 4u * lk + (g & 3);
#pragma unroll
            for (int t = 0; t < 4; ++t) out[t] = bs[row * BS + 16 * t + li];
        };
        bfrag(0, bq[0]);
        bfrag(1, bq[1]);
#pragma unroll
        for (int g = 0; g < 8; ++g) {
            if (g + 2 < 8) bfrag(g + 2, bq[(g + 2) % 3]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int t = 0; t < 4; ++t)
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[g], bq[g % 3][t], acc[t], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
        // the other buffer was last read in the previous step, which every wave left through the barrier;
        // past the end the tile is a repeat and must not be counted in the column sums
        stage(other, bs2 + (S ^ 1) * TSZ, nb + 32 < n_len ? 1.0f : 0.0f);
        __syncthreads();
    };
    load(set0{}, 0);
    load(set1{}, min(32u, n_last));
    stage(set0{}, bs2, 1.0f);
    __syncthreads();
    for (uint32_t nb = 0; nb < n_len; nb += 64) {
        step(set0{}, set1{}, nb);
        if (nb + 32 < n_len) step(set1{}, set0{}, nb + 32);
    }
    __syncthreads();
    float* bs = bs2;
    // column sums of the 16-row tiles: thread (fr, fc) holds rows fr, fr+16, ... -> add the 16 fr
    __syncthreads();
    *reinterpret_cast<f32x4v*>(&bs[fr * BS + fc]) = f32x4v{dsum.x, dsum.y, dsum.z, dsum.w};
    __syncthreads();
    float db[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) db[t] += bs[rr * BS + 16 * t + li];
    }
    // T[p = p0 + lk*4 + j][b = b0 + 16 t + li]  against  x[b][p]
    float g[4] = {0.0f, 0.0f, 0.0f, 0.0f}, gm[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t p = p0 + lk * 4 + j;
            const float x = D.XbT[(size_t)p * D.B_pad + b0 + 16 * t + li];
            g[j] += x * acc[t][j];
            gm[j] += x * db[t];
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float tot = row16_sum(g[j]), totm = row16_sum(gm[j]);
        const uint32_t p = p0 + lk * 4 + j;
        if (li == 0 && p < D.P) {
            D.ds_part[(size_t)part * D.R + c * D.P + p] = tot;
            D.dmu_part[(size_t)part * D.R + c * D.P + p] = totm;
        }
    }
    if (bg == 0) {
        // lane (li, lk) summed samples 4*lk..4*lk+3 of every 16 for row p0+li: add the four lk
        s1 += __shfl_xor(s1, 16); s1 += __shfl_xor(s1, 32);
        s2 += __shfl_xor(s2, 16); s2 += __shfl_xor(s2, 32);
        if (lk == 0 && p0 + li < D.P) {
            D.s1[(size_t)ks * D.R + c * D.P + p0 + li] = s1;
            D.s2[(size_t)ks * D.R + c * D.P + p0 + li] = s2;
        }
    }
}

// fixed-order sum over a workgroup of up to 16 waves (every thread gets the total)
__device__ __forceinline__ float block_sum(float v, float* red, uint32_t tid, uint32_t n_waves) {
    const float w = wave_sum(v);
    __syncthreads();
    if ((tid & 63u) == 0) red[tid >> 6] = w;
    __syncthreads();
    float tot = 0.0f;
    for (uint32_t i = 0; i < n_waves; ++i) tot += red[i];
    return tot;
}

// One thread per weight row r = (class, feature): gradients of f with respect to the four uniform
// entries of the row (q loc, q scale, prior loc, prior scale) from the likelihood partials of
// dense_backward, the closed-form prior sums and the entropy.  A uniform entry of its own per row
// (stride != 0) is written here; entries shared by all rows go to rowg and are summed by the epilogue.
__device__ __forceinline__ void dense_rows_body(const DParams& D, float* red, float (*gsum)[4][64]) {
    const uint32_t tid = threadIdx.x;
    // fused exact-data path: 64 rows per workgroup; wave w adds the sample groups w, w + 4, ... of dense_xbwd's four partial
    // arrays (eight loads of each in flight) and the rows' threads (wave 0) join the four slices in order.  (One thread per
    // row walking all n_pad / 16 groups alone was a 26 us latency chain.)
    const bool sliced = D.xfused != 0;
    const uint32_t r = sliced ? blockIdx.x * 64 + (tid & 63u) : blockIdx.x * 256 + tid;
    if (sliced) {
        const uint32_t w = tid >> 6, lane = tid & 63u;
        float a[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (r < D.R) {
            const float* const src[4] = {D.ds_part, D.dmu_part, D.s1, D.s2};
            for (uint32_t g0 = w; g0 < D.ksplit; g0 += 32) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    float v[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const uint32_t g = g0 + 4u * u;
                        v[u] = g < D.ksplit ? src[q][(size_t)g * D.R + r] : 0.0f;
                    }
                    a[q] += ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
                }
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) gsum[q][w][lane] = a[q];
        __syncthreads();
    }
    const bool active = r < D.R && (!sliced || tid < 64);
    // (caller-weighted gradients: every closed-form sum over samples takes a_n — A for the count, dense_weighted_sums' row sums)
    const float N = D.f_weight ? D.wsum[0] : (float)D.n_local;
    float hconst = 0.0f, pvsum = 0.0f, qconst = 0.0f;
    if (active) {
        const float mu = D.rowp[r], s = D.rowp[D.R + r], mu0 = D.rowp[2 * D.R + r], s0 = D.rowp[3 * D.R + r];
        float S1 = 0.0f, S2 = 0.0f, ds_lik, dmu_lik;
        if (sliced) {
            ds_lik = (gsum[0][0][tid] + gsum[0][1][tid]) + (gsum[0][2][tid] + gsum[0][3][tid]);
            dmu_lik = (gsum[1][0][tid] + gsum[1][1][tid]) + (gsum[1][2][tid] + gsum[1][3][tid]);
            S1 = (gsum[2][0][tid] + gsum[2][1][tid]) + (gsum[2][2][tid] + gsum[2][3][tid]);
            S2 = (gsum[3][0][tid] + gsum[3][1][tid]) + (gsum[3][2][tid] + gsum[3][3][tid]);
        } else {
            for (uint32_t ks = 0; ks < D.ksplit; ++ks) { S1 += D.s1[(size_t)ks * D.R + r]; S2 += D.s2[(size_t)ks * D.R + r]; }
            // fixed-order sums of the (sample split, column group) partials, 4 loads of each array in flight
            float ds4[4] = {0.0f, 0.0f, 0.0f, 0.0f}, dm4[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            const uint32_t n_groups = D.xpath ? D.ksplit : D.ksplit * (D.B_pad / 64);     // (exact-data path: dense_xreduce's sample groups)
            for (uint32_t g2 = 0; g2 < n_groups; g2 += 4) {
#pragma unroll
                for (uint32_t u = 0; u < 4; ++u) {
                    const bool ok = g2 + u < n_groups;
                    const size_t at = (size_t)(ok ? g2 + u : 0) * D.R + r;
                    const float a = D.ds_part[at], b = D.dmu_part[at];
                    ds4[u] += ok ? a : 0.0f;
                    dm4[u] += ok ? b : 0.0f;
                }
            }
            ds_lik = (ds4[0] + ds4[1]) + (ds4[2] + ds4[3]);
            dmu_lik = (dm4[0] + dm4[1]) + (dm4[2] + dm4[3]);
        }
        if (D.f_weight) { S1 = D.ws1[r]; S2 = D.ws2[r]; }
        const float delta = mu - mu0, is2 = 1.0f / (s0 * s0);
        // prior: sum_n d log N(W | mu0, s0)
        const float sum_dw = -(N * delta + s * S1) * is2;                       // sum_n dlp/dW
        const float sum_dw_e = -(delta * S1 + s * S2) * is2;                    // sum_n dlp/dW * eps
        const float sum_sq = N * delta * delta + 2.0f * delta * s * S1 + s * s * S2;   // sum_n (W - mu0)^2
        const float grad[4] = {dmu_lik + D.prior_weight * sum_dw,
                               ds_lik + D.prior_weight * sum_dw_e + (D.entropy_weight != 0.0f ? D.entropy_weight * N / s : 0.0f),
                               -D.prior_weight * sum_dw,
                               D.prior_weight * (sum_sq * is2 / s0 - N / s0)};
        const uint32_t base[4] = {D.q_loc_u, D.q_scale_u, D.prior_loc_u, D.prior_scale_u};
        const uint32_t stride[4] = {D.q_loc_stride, D.q_scale_stride, D.prior_loc_stride, D.prior_scale_stride};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t k = base[q] + r * stride[q];
            if (k >= D.n_uniform_grad) continue;
            if (stride[q]) D.partial[2 + k] += grad[q];   // only this thread touches entry k (zeroed by the prologue)
            else D.rowg[(size_t)q * D.R + r] = grad[q];
        }
        // (entropy_weight = 0: a point estimate, whose scale is 0 — no 0 * log 0)
        hconst = D.prior_weight * (-logf(s0) - kLogSqrt2Pi)
               + (D.entropy_weight != 0.0f ? D.entropy_weight * (kHalfLog2PiE + logf(s)) : 0.0f);
        pvsum = -0.5f * D.prior_weight * sum_sq * is2;
        // BlackBox: the sample-independent part of log q(W) = sum_r log N(W_r | mu_r, s_r) (a point estimate has no q)
        if (D.estimator == BSVI_EST_BLACKBOX && D.entropy_weight != 0.0f) qconst = -logf(s) - kLogSqrt2Pi;
    }
    const float h = block_sum(hconst, red, tid, 4), pvs = block_sum(pvsum, red, tid, 4), qc = block_sum(qconst, red, tid, 4);
    if (tid == 0) {      // (hpart: three arrays of gridDim.x entries, read back by dense_epilogue with the same row-block count)
        D.hpart[blockIdx.x] = h;
        D.hpart[gridDim.x + blockIdx.x] = pvs;
        D.hpart[2 * gridDim.x + blockIdx.x] = qc;
    }
}

__global__ void __launch_bounds__(256) dense_rows(const DParams D) {
    __shared__ float red[4];
    __shared__ float gsum[4][4][64];
    dense_rows_body(D, red, gsum);
}

// Per-sample sums over the row chunks of pv_part / qv_part (per-sample prior value and -0.5 sum eps^2: the launches that need
// per-sample values, BlackBox above all).  64 samples per workgroup, its four waves take the chunks w, w + 4, ... (eight
// loads in flight each) and are joined in wave order; the totals replace chunk 0.  Left to dense_epilogue — ONE workgroup
// on ONE CU reading 2 x 123 x 1024 values — this was a 44 us serial tail of a 290 us iteration.
__global__ void __launch_bounds__(256) dense_sample_sums(const DParams D, uint32_t with_q) {
    __shared__ float part[2][4][64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, n = blockIdx.x * 64u + lane;
    const uint32_t row_chunks = (D.R + D.row_chunk - 1) / D.row_chunk;
    float pv[8], qv[8];
#pragma unroll
    for (uint32_t u = 0; u < 8; ++u) pv[u] = qv[u] = 0.0f;
    for (uint32_t ch = wave; ch < row_chunks; ch += 32u) {
#pragma unroll
        for (uint32_t u = 0; u < 8; ++u) {
            const uint32_t c = ch + 4u * u;
            const bool ok = c < row_chunks;
            const size_t at = (size_t)(ok ? c : 0u) * D.n_pad + n;
            const float a = D.pv_part[at], b = with_q ? D.qv_part[at] : 0.0f;
            pv[u] += ok ? a : 0.0f;
            qv[u] += ok ? b : 0.0f;
        }
    }
    part[0][wave][lane] = ((pv[0] + pv[1]) + (pv[2] + pv[3])) + ((pv[4] + pv[5]) + (pv[6] + pv[7]));
    part[1][wave][lane] = ((qv[0] + qv[1]) + (qv[2] + qv[3])) + ((qv[4] + qv[5]) + (qv[6] + qv[7]));
    __syncthreads();                                   // every chunk 0 value of this workgroup's samples has been read
    if (wave == 0) {
        D.pv_part[n] = (part[0][0][lane] + part[0][1][lane]) + (part[0][2][lane] + part[0][3][lane]);
        if (with_q) D.qv_part[n] = (part[1][0][lane] + part[1][1][lane]) + (part[1][2][lane] + part[1][3][lane]);
    }
}

// Caller-weighted gradients (DParams::f_weight): the row sums of a_n eps, a_n eps^2 that replace dense_backward's / dense_xbwd's
// plain ones in dense_rows, and A = sum a_n, B = sum b_n.  Workgroup = 64 row quads x 4 sample slices (slice k takes the samples
// k, k + 4, ...), joined in slice order; the noise is the caller's or drawn again from the counters of the forward kernels
// (dense_eps4).  Workgroup 0 also leaves A and B — fixed-order sums of at most a few thousand values.
__global__ void __launch_bounds__(256) dense_weighted_sums(const DParams D) {
    __shared__ float part[8][4][64];
    __shared__ float red[4];
    const uint32_t tid = threadIdx.x, ql = tid & 63u, slice = tid >> 6;
    const uint32_t quad = blockIdx.x * 64u + ql, r = quad * 4u;
    float acc[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (r < D.R) {
        for (uint32_t n = slice; n < D.n_local; n += 4u) {
            float e[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (D.noise_in) {
                for (uint32_t j = 0; j < 4u && r + j < D.R; ++j) e[j] = D.noise_in[(size_t)(r + j) * D.n_local + n];
            } else {
                dense_eps4(D, n, quad, e);
            }
            const float a = D.f_weight[n];
#pragma unroll
            for (int j = 0; j < 4; ++j) { acc[j] += a * e[j]; acc[4 + j] += a * e[j] * e[j]; }
        }
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) part[q][slice][ql] = acc[q];
    __syncthreads();
    if (tid < 64u && r < D.R) {
        for (uint32_t j = 0; j < 4u && r + j < D.R; ++j) {
            D.ws1[r + j] = (part[j][0][tid] + part[j][1][tid]) + (part[j][2][tid] + part[j][3][tid]);
            D.ws2[r + j] = (part[4 + j][0][tid] + part[4 + j][1][tid]) + (part[4 + j][2][tid] + part[4 + j][3][tid]);
        }
    }
    if (blockIdx.x == 0) {
        float a = 0.0f, b = 0.0f;
        for (uint32_t n = tid; n < D.n_local; n += 256u) { a += D.f_weight[n]; b += D.q_weight ? D.q_weight[n] : 0.0f; }
        const float A = block_sum(a, red, tid, 4), B = block_sum(b, red, tid, 4);
        if (tid == 0) { D.wsum[0] = A; D.wsum[1] = B; }
    }
}

// One workgroup: the sum over samples of f, the non-finite count and the gradients of the shared
// uniform entries, all in fixed order.  Handed to dense_param_kernel as ONE partial block.
template <uint32_t NT>
__device__ __forceinline__ void dense_epilogue_body(const DParams& D, float* red) {
    const uint32_t tid = threadIdx.x;
    const uint32_t row_blocks = D.xfused ? (D.R + 63) / 64 : (D.R + 255) / 256, row_chunks = D.sums_folded ? 1u : (D.R + D.row_chunk - 1) / D.row_chunk;
    float hc = 0.0f, pc = 0.0f, qc = 0.0f;
    for (uint32_t i = tid; i < row_blocks; i += NT) { hc += D.hpart[i]; pc += D.hpart[row_blocks + i]; qc += D.hpart[2 * row_blocks + i]; }
    const float htot = block_sum(hc, red, tid, NT / 64);    // sample-independent terms of f
    const float ptot = block_sum(pc, red, tid, NT / 64);    // sum over samples of the prior's sample-dependent term
    const float qtot = block_sum(qc, red, tid, NT / 64);    // sample-independent part of log q (BlackBox)
    const bool per_sample_prior = D.per_sample != 0;
    // BlackBox (gradient_estimators.py:29-36): value_n = log q(W_n) * stopgrad(f_n) + f_n.  The weights stay
    // reparameterised (variables.py:567 drops `differentiable=False`), so d log q(W_n(theta); theta) / d mu = 0 and
    // / d s_r = -1 / s_r for EVERY sample: the score term adds  -(sum_n f_n) / s_r  to the scale gradient of row r.
    const bool blackbox = D.estimator == BSVI_EST_BLACKBOX && D.entropy_weight != 0.0f;
    float fsum = 0.0f, bad = 0.0f, vsum = 0.0f;
    for (uint32_t n = tid; n < D.n_local; n += NT) {
        float f = htot;
        for (uint32_t g = 0; g < D.lik_parts; ++g) f += D.lik_part[(size_t)g * D.n_pad + n];
        float value = f;
        if (per_sample_prior) {
            float pv8[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, qv8[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
            for (uint32_t ch = 0; ch < row_chunks; ch += 8) {
#pragma unroll
                for (uint32_t u = 0; u < 8; ++u)
                    if (ch + u < row_chunks) {
                        pv8[u] += D.pv_part[(size_t)(ch + u) * D.n_pad + n];
                        if (blackbox) qv8[u] += D.qv_part[(size_t)(ch + u) * D.n_pad + n];
                    }
            }
            f += D.prior_weight * (((pv8[0] + pv8[1]) + (pv8[2] + pv8[3])) + ((pv8[4] + pv8[5]) + (pv8[6] + pv8[7])));
            if (D.fvalue_out) D.fvalue_out[n] = f;
            value = f;
            if (blackbox) {
                const float lq = qtot + (((qv8[0] + qv8[1]) + (qv8[2] + qv8[3])) + ((qv8[4] + qv8[5]) + (qv8[6] + qv8[7])));
                if (D.logq_out) D.logq_out[n] = lq;
                value = lq * f + f;
            }
        }
        fsum += f;
        vsum += value;
        bad += isfinite(value) ? 0.0f : 1.0f;
    }
    float fs = block_sum(fsum, red, tid, NT / 64);
    float vs = block_sum(vsum, red, tid, NT / 64);
    float bs = block_sum(bad, red, tid, NT / 64);
    if (!per_sample_prior) {
        fs += ptot;
        vs += ptot;
        if (!isfinite(ptot)) bs += 1.0f;
    }
    if (tid == 0) {
        D.partial[0] = vs;
        D.partial[1] = bs;
    }
    if (blackbox && D.q_scale_u < D.n_uniform_grad) {
        if (D.q_weight) fs = D.wsum[1];          // (a caller's weights of grad log q_n in place of f_n)
        float shared = 0.0f;
        for (uint32_t r = tid; r < D.R; r += NT) {
            const float g = -fs / D.rowp[D.R + r];
            if (D.q_scale_stride) D.partial[2 + D.q_scale_u + r * D.q_scale_stride] += g;     // (dense_rows wrote it: earlier launch)
            else shared += g;
        }
        if (!D.q_scale_stride) {
            const float tot = block_sum(shared, red, tid, NT / 64);
            if (tid == 0) D.partial[2 + D.q_scale_u] += tot;
        }
    }
    const uint32_t base[4] = {D.q_loc_u, D.q_scale_u, D.prior_loc_u, D.prior_scale_u};
    const uint32_t stride[4] = {D.q_loc_stride, D.q_scale_stride, D.prior_loc_stride, D.prior_scale_stride};
    for (int q = 0; q < 4; ++q) {
        if (stride[q] || base[q] >= D.n_uniform_grad) continue;     // uniform: no divergence around the barriers
        float g = 0.0f;
        for (uint32_t r = tid; r < D.R; r += NT) g += D.rowg[(size_t)q * D.R + r];
        const float tot = block_sum(g, red, tid, NT / 64);
        if (tid == 0) D.partial[2 + base[q]] += tot;
    }
}

__global__ void __launch_bounds__(1024) dense_epilogue(const DParams D) {
    __shared__ float red[16];
    dense_epilogue_body<1024>(D, red);
}

// theta-side of the chain rule, finalize and optimizer step for models with many parameters:
// one thread per parameter over as many workgroups as needed (the generic reduce_kernel is a
// single workgroup because it also sums workgroup partials; here there is exactly one block).
__device__ __forceinline__ void dense_param_body(const RParams& R, const uint32_t i, const float s, const float c) {
    const float loss = -s / (float)R.n_global;
    const float finite = isfinite(loss) ? 1.0f : 0.0f;
    if (i == 0) {
        R.out[0] = s;
        R.out[1] = c;
        if (R.do_finalize) {
            R.out[2] = loss;
            R.out[3] = finite;
            if (R.loss_slot) *R.loss_slot = loss;
            if (R.finite_slot) *R.finite_slot = finite;
        }
    }
    if (i >= R.n_params) return;
    const float scale = R.do_finalize ? -1.0f / (float)R.n_global : 1.0f;
    const float theta = R.params[i];
    float gsum = 0.0f;
    for (uint32_t j = R.pu_ptr[i]; j < R.pu_ptr[i + 1]; ++j) {
        const uint32_t k = R.pu_idx[j];
        const bsvi_uniform_entry e = R.uniform[k];
        gsum += R.partials[2 + k] * (e.b * utransform_grad(e.transform, theta));
    }
    const float grad = gsum * scale;
    R.out[BSVI_OUT_HEADER + i] = grad;
    if (R.do_step && finite != 0.0f && R.active_mask[i]) optimizer_update(R.cfg, R.params, R.state, R.n_params, i, grad);
}
__global__ void dense_param_kernel(const RParams R) { dense_param_body(R, blockIdx.x * blockDim.x + threadIdx.x, R.partials[0], R.partials[1]); }

// dense_epilogue folded into the parameter kernel (round 5; the fused exact-data path, Pathwise, closed-form prior, every row with its
// own uniform entries — BASELINE config 4): every workgroup adds the value of the estimator itself, in the same fixed order — 123
// row-block terms and one likelihood per sample, 5 KB out of L2 — instead of waiting for a one-workgroup launch to do it once
// (4.7 us of a 106 us iteration).  The sums are identical in every workgroup; workgroup 0 writes them to the partial block.
__global__ void __launch_bounds__(256) dense_param_fold_kernel(const RParams R, const DParams D, const uint32_t row_blocks) {
    __shared__ float red[4];
    __shared__ float tot[2];
    const uint32_t tid = threadIdx.x;
    float hc = 0.0f, pc = 0.0f;
    for (uint32_t i = tid; i < row_blocks; i += 256u) { hc += D.hpart[i]; pc += D.hpart[row_blocks + i]; }
    const float htot = block_sum(hc, red, tid, 4), ptot = block_sum(pc, red, tid, 4);
    float vsum = 0.0f, bad = 0.0f;
    for (uint32_t n = tid; n < D.n_local; n += 256u) {
        float f = htot;
        for (uint32_t g = 0; g < D.lik_parts; ++g) f += D.lik_part[(size_t)g * D.n_pad + n];
        vsum += f;
        bad += isfinite(f) ? 0.0f : 1.0f;
    }
    float vs = block_sum(vsum, red, tid, 4), bs = block_sum(bad, red, tid, 4);
    vs += ptot;
    if (!isfinite(ptot)) bs += 1.0f;
    if (tid == 0) {
        tot[0] = vs; tot[1] = bs;
        if (blockIdx.x == 0) { D.partial[0] = vs; D.partial[1] = bs; }
    }
    __syncthreads();
    dense_param_body(R, blockIdx.x * 256u + tid, tot[0], tot[1]);
}

}  // namespace bsvi

// ---- the exact-data path ----------------------------------------------------------------------------------------
// W = mu + s * eps of sample n as bf16 pieces, rows (n, c) with the features contiguous (the k axis of the product).  One
// workgroup per sample walks its C * Kp / 4 feature quads: ONE Philox call per quad (rows 4g .. 4g+3 are four consecutive
// features of one class: P is a multiple of 4 on this path), three 8-byte stores.  The per-sample prior value and
// -sum eps^2 / 2 (BlackBox, per-sample outputs) are sums over the same loop.
__global__ void __launch_bounds__(256) dense_wsplit(const DParams D) {
    __shared__ float red[4];
    const uint32_t n = blockIdx.x, tid = threadIdx.x;
    const uint32_t quads = D.Kp / 4, total = D.C * quads;
    const bool live = n < D.n_local;
    const bool want_pv = D.per_sample != 0, want_qv = D.estimator == BSVI_EST_BLACKBOX;
    const float2* ms = reinterpret_cast<const float2*>(D.rowp + 4 * (size_t)D.R);      // {loc, scale} per row
    const size_t plane = (size_t)D.n_pad * D.C * D.Kp;
    float pv = 0.0f, qv = 0.0f;
    for (uint32_t i = tid; i < total; i += 256) {
        const uint32_t c = i / quads, p = (i - c * quads) * 4;
        uint16_t hi[4] = {0, 0, 0, 0}, mid[4] = {0, 0, 0, 0}, lo[4] = {0, 0, 0, 0};
        if (p < D.P) {
            const uint32_t r = c * D.P + p;
            float e[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (live) {
                if (D.noise_in) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) e[j] = D.noise_in[(size_t)(r + j) * D.n_local + n];
                } else {
                    dense_eps4(D, n, r >> 2, e);
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float2 m = ms[r + j];
                const float w = m.x + m.y * e[j];
                dense_split3(w, hi[j], mid[j], lo[j]);
                if (D.noise_out && live && !D.xfused) D.noise_out[(size_t)(r + j) * D.n_local + n] = e[j];
                if (want_pv && live) {
                    const float u = (m.x - D.rowp[2 * D.R + r + j] + m.y * e[j]) / D.rowp[3 * D.R + r + j];
                    pv += -0.5f * u * u;
                    if (want_qv) qv += -0.5f * e[j] * e[j];
                }
            }
        }
        if (D.xfused) continue;             // (the fused launches draw W in LDS: only the per-sample sums are wanted here)
        const size_t at = ((size_t)n * D.C + c) * D.Kp + p;
        typedef uint16_t u16x4 __attribute__((ext_vector_type(4)));
        *reinterpret_cast<u16x4*>(D.Wp + at) = u16x4{hi[0], hi[1], hi[2], hi[3]};
        *reinterpret_cast<u16x4*>(D.Wp + plane + at) = u16x4{mid[0], mid[1], mid[2], mid[3]};
        *reinterpret_cast<u16x4*>(D.Wp + 2 * plane + at) = u16x4{lo[0], lo[1], lo[2], lo[3]};
    }
    if (want_pv) {
        const float ps = block_sum(pv, red, tid, 4), qs = block_sum(qv, red, tid, 4);
        if (tid == 0 && n < D.n_pad) {
            D.pv_part[n] = ps;                  // (one "row chunk": the epilogue reads it as the folded sum)
            if (want_qv) D.qv_part[n] = qs;
        }
    }
}

// likelihood and d f / d logits from logitsT[b][(n, c)]: workgroup = 64 minibatch columns x 8 samples.  The tile is read
// along (n, c) — contiguous — and turned in LDS; a wave then holds the 64 columns of ONE sample pair, so the sum over
// columns is a wave sum and the pieces of dlog leave along b, the k axis of the second product.
__global__ void __launch_bounds__(256) dense_ce(const DParams D) {
    constexpr int NS = 8;
    __shared__ float tile[64][NS * 16 + 1];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t bt = blockIdx.x % (D.B_pad / 64), nt = blockIdx.x / (D.B_pad / 64);
    const uint32_t b0 = bt * 64, n0 = nt * NS, width = NS * D.C, NC = D.n_pad * D.C;
    for (uint32_t i = tid; i < 64 * width; i += 256) {
        const uint32_t rb = i / width, k = i - rb * width;
        tile[rb][k] = D.logitsT[(size_t)(b0 + rb) * NC + (size_t)n0 * D.C + k];
    }
    __syncthreads();
    const uint32_t b = b0 + lane;
    const float w1 = b < D.B ? D.lik_weight : 0.0f;
    const float label = D.lab[b];
    const size_t plane = (size_t)NC * D.B_pad;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const uint32_t ns = wave * 2 + h, n = n0 + ns;
        const bool live = n < D.n_local;
        const float w = w1 * ((live && D.f_weight) ? D.f_weight[n] : 1.0f);
        float lik = 0.0f;
        if (D.likelihood == BSVI_LIK_CATEGORICAL) {
            float l[16], m = -INFINITY, zl = 0.0f;
#pragma unroll
            for (int c = 0; c < 16; ++c) {
                l[c] = c < (int)D.C ? tile[lane][ns * D.C + c] : -INFINITY;
                m = fmaxf(m, l[c]);
            }
            float se = 0.0f, e[16];
#pragma unroll
            for (int c = 0; c < 16; ++c) {
                e[c] = c < (int)D.C ? __expf(l[c] - m) : 0.0f;
                se += e[c];
                zl = (label == (float)c) ? l[c] : zl;
            }
            lik = w * (zl - (m + __builtin_amdgcn_logf(se) * 0.6931471805599453f));
            const float wr = w * __builtin_amdgcn_rcpf(se);
#pragma unroll
            for (int c = 0; c < 16; ++c)
                if (c < (int)D.C) {
                    const float g = live ? ((label == (float)c) ? w : 0.0f) - wr * e[c] : 0.0f;
                    uint16_t hi, mid, lo;
                    dense_split3(g, hi, mid, lo);
                    const size_t at = ((size_t)n * D.C + c) * D.B_pad + b;
                    D.dlogp[at] = hi; D.dlogp[plane + at] = mid; D.dlogp[2 * plane + at] = lo;
                }
        } else {   // Bernoulli / Binomial(1): -binary_cross_entropy_with_logits(l, k)
            const float l = tile[lane][ns];
            lik = w * (label * l - (fmaxf(l, 0.0f) + log1pf(expf(-fabsf(l)))));
            const float g = live ? w * (label - sigmoidf_(l)) : 0.0f;
            uint16_t hi, mid, lo;
            dense_split3(g, hi, mid, lo);
            const size_t at = (size_t)n * D.B_pad + b;
            D.dlogp[at] = hi; D.dlogp[plane + at] = mid; D.dlogp[2 * plane + at] = lo;
        }
        const float tot = wave_sum(live ? lik : 0.0f);
        if (lane == 0 && n < D.n_pad) D.lik_part[(size_t)bt * D.n_pad + n] = tot;
    }
}

// d f / d s, d f / d mu (likelihood parts) and the row sums of eps, eps^2 from GT[p][(n, c)]: one workgroup per feature
// quad; thread (sample lane, class) redraws the quad's normals of its samples (the counters dense_wsplit used), reads
// the four rows of GT along (n, c) and keeps sixteen sums; the sample lanes of a class are joined in lane order.
using dsel::kXGroups;       // sample groups of dense_xreduce (dense_rows adds them in order)
__global__ void __launch_bounds__(256) dense_xreduce(const DParams D) {
    __shared__ float red[16][256];
    const uint32_t tid = threadIdx.x, p = (blockIdx.x / kXGroups) * 4, grp = blockIdx.x % kXGroups;
    const uint32_t NL = 256 / D.C, c = tid % D.C, nl = tid / D.C, NC = D.n_pad * D.C;
    float acc[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.0f;
    if (nl < NL) {
        const uint32_t r = c * D.P + p;
        // (group g takes a contiguous range of samples: its threads then read GT along (n, c) without gaps)
        const uint32_t per = (D.n_local + kXGroups - 1) / kXGroups, n_end = min(D.n_local, (grp + 1) * per);
        for (uint32_t n = grp * per + nl; n < n_end; n += NL) {
            float e[4];
            if (D.noise_in) {
#pragma unroll
                for (int j = 0; j < 4; ++j) e[j] = D.noise_in[(size_t)(r + j) * D.n_local + n];
            } else {
                dense_eps4(D, n, r >> 2, e);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float g = D.GT[(size_t)(p + j) * NC + (size_t)n * D.C + c];
                acc[j] += e[j] * g;
                acc[4 + j] += g;
                acc[8 + j] += e[j];
                acc[12 + j] += e[j] * e[j];
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) red[q][tid] = acc[q];
    __syncthreads();
    if (tid < 16 * D.C) {
        const uint32_t q = tid / D.C, cc = tid % D.C;
        float s = 0.0f;
        for (uint32_t l = 0; l < NL; ++l) s += red[q][l * D.C + cc];
        const uint32_t j = q & 3u, r = cc * D.P + p + j;
        float* dst = q < 4 ? D.ds_part : (q < 8 ? D.dmu_part : (q < 12 ? D.s1 : D.s2));
        dst[(size_t)grp * D.R + r] = s;
    }
}

#include "dense_xfused.inc"

// ---- host side -------------------------------------------------------------------------------
// Which launches an iteration makes, their grids, LDS and derived arguments, and the workspace: dense_select.h.  Here: the environment
// (dense_read_switches), the device (bsvi_dense_create) and ONE loop over the plan's launches (dense_iterate).
struct bsvi_dense {
    bsvi_dense_desc d;
    void* dev_blob = nullptr;
    const bsvi_uniform_entry* uniform = nullptr;
    const float* consts = nullptr;
    const uint32_t* pu_ptr = nullptr;
    const uint32_t* pu_idx = nullptr;
    const float* dataset = nullptr;
    const float* labels = nullptr;
    dsel::Switches sw;       // the environment as bsvi_dense_create found it
    dsel::Model m;           // the shape, the estimator, and what the device granted
    dsel::ModelPlan mp;      // the path and its paddings
};

// the one place of the dense-link path that looks at the environment
static dsel::Switches dense_read_switches() {
    auto on = [](const char* knob) { const char* e = getenv(knob); return !(e && e[0] == '0'); };
    auto digit = [](const char* knob, int mask) { const char* e = getenv(knob); return e ? (e[0] - '0') & mask : 0; };
    auto number = [](const char* knob) { const char* e = getenv(knob); return e ? atoi(e) : 0; };
    dsel::Switches sw;
    sw.xgemm = on("BSVI_DENSE_XGEMM");
    sw.fused = on("BSVI_DENSE_FUSED");
    sw.fold = on("BSVI_DENSE_FOLD");
    sw.xf_ns = (uint32_t)number("BSVI_XF_NS");
    sw.xf_debug = digit("BSVI_XF_DEBUG", 7);
    sw.xb_debug = digit("BSVI_XB_DEBUG", 3);
    sw.xb_rb = number("BSVI_XB_RB");
    sw.xb_groups = (uint32_t)number("BSVI_XB_GROUPS");
    return sw;
}

// the templated families, by dsel::Kind minus the family's first: create raises their LDS attribute and dense_iterate launches through
// the same tables
typedef void (*dense_plain_fn)(const DParams);
typedef void (*dense_xfwd_fn)(const DParams, const uint32_t);
typedef void (*dense_xbwd_fn)(const DParams, const uint32_t, const uint32_t, const uint32_t, const uint32_t);
static const dense_plain_fn kDenseForward[] = {dense_forward<1>, dense_forward<4>, dense_forward<10>, dense_forward<16>};
static const dense_xfwd_fn kDenseXfwd[] = {dense_xfwd<0, 1>, dense_xfwd<0, 2>, dense_xfwd<1, 2>, dense_xfwd<2, 2>, dense_xfwd<3, 2>, dense_xfwd<4, 2>,
                                           dense_xfwd<5, 2>, dense_xfwd<6, 2>, dense_xfwd<0, 1, true>, dense_xfwd<0, 2, true>};
static const dense_xbwd_fn kDenseXbwd[] = {dense_xbwd<0, 2, 7>, dense_xbwd<0, 4, 7>, dense_xbwd<1, 4, 7>, dense_xbwd<2, 4, 7>, dense_xbwd<3, 4, 7>,
                                           dense_xbwd<0, 4, 9>, dense_xbwd<0, 2, 7, true>, dense_xbwd<0, 4, 7, true>, dense_xbwd<0, 4, 9, true>};
static_assert(sizeof(kDenseForward) / sizeof(kDenseForward[0]) == dsel::FORWARD_COUNT && sizeof(kDenseXfwd) / sizeof(kDenseXfwd[0]) == dsel::XFWD_COUNT &&
              sizeof(kDenseXbwd) / sizeof(kDenseXbwd[0]) == dsel::XBWD_COUNT, "one entry per kind of dense_select.h, in its order");
static bool dense_is_xfwd(int kind) { return kind >= dsel::XFWD_FIRST && kind < dsel::XFWD_FIRST + dsel::XFWD_COUNT; }

extern "C" int bsvi_dense_create(const bsvi_dense_desc* desc, bsvi_dense** out) {
    if (!desc || !out) return fail(BSVI_ERR_INVALID, "null argument");
    *out = nullptr;
    BSVI_CHECK_STRUCT(desc, bsvi_dense_desc);
    if (desc->abi_version != BSVI_ABI_VERSION) return fail(BSVI_ERR_INVALID, "ABI version mismatch");
    if (!desc->n_classes || !desc->n_features || !desc->batch_size || desc->batch_size > desc->dataset_size)
        return fail(BSVI_ERR_INVALID, "bad dense shape");
    if (desc->n_classes > 16) return fail(BSVI_ERR_UNSUPPORTED, "dense path supports at most 16 classes");
    if (desc->likelihood == BSVI_LIK_BERNOULLI && desc->n_classes != 1) return fail(BSVI_ERR_INVALID, "Bernoulli likelihood needs one output");
    if (desc->likelihood > BSVI_LIK_BERNOULLI) return fail(BSVI_ERR_UNSUPPORTED, "unknown likelihood");
    if (desc->estimator > BSVI_EST_BLACKBOX) return fail(BSVI_ERR_INVALID, "unknown estimator");
    const uint64_t R = (uint64_t)desc->n_classes * desc->n_features;
    const uint32_t bases[4] = {desc->q_loc_u, desc->q_scale_u, desc->prior_loc_u, desc->prior_scale_u};
    const uint32_t strides[4] = {desc->q_loc_stride, desc->q_scale_stride, desc->prior_loc_stride, desc->prior_scale_stride};
    for (int i = 0; i < 4; ++i)
        if (strides[i] > 1 || (uint64_t)bases[i] + strides[i] * (R - 1) >= desc->n_uniform) return fail(BSVI_ERR_INVALID, "row parameter range out of the uniform table");
    for (uint32_t k = 0; k < desc->n_uniform; ++k) {
        const bsvi_uniform_entry& e = desc->uniform[k];
        if (e.transform > BSVI_UT_SQUARE || (k < desc->n_uniform_grad) != (e.is_param != 0) ||
            e.src >= (e.is_param ? desc->n_params : desc->n_consts))
            return fail(BSVI_ERR_INVALID, "bad uniform table");
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(BSVI_ERR_NO_DEVICE, "no HIP device visible");
    bsvi_dense* p = new bsvi_dense();
    p->d = *desc;
    const size_t b_uni = align_up((size_t)desc->n_uniform * sizeof(bsvi_uniform_entry), 256);
    const size_t b_con = align_up((size_t)desc->n_consts * 4, 256);
    const size_t b_ptr = align_up(((size_t)desc->n_params + 1) * 4, 256);
    const size_t b_idx = align_up((size_t)desc->n_uniform_grad * 4, 256);
    const size_t b_dat = align_up((size_t)desc->dataset_size * desc->n_features * 4, 256);
    const size_t b_lab = align_up((size_t)desc->dataset_size * 4, 256);
    const size_t total = b_uni + b_con + b_ptr + b_idx + b_dat + b_lab + 256;
    std::vector<char> host(total, 0);
    size_t o = 0;
    const size_t o_uni = o; memcpy(&host[o], desc->uniform, (size_t)desc->n_uniform * sizeof(bsvi_uniform_entry)); o += b_uni;
    const size_t o_con = o; if (desc->n_consts) memcpy(&host[o], desc->consts, (size_t)desc->n_consts * 4); o += b_con;
    const size_t o_ptr = o; if (desc->n_params) memcpy(&host[o], desc->param_uniform_ptr, ((size_t)desc->n_params + 1) * 4); o += b_ptr;
    const size_t o_idx = o; if (desc->n_uniform_grad) memcpy(&host[o], desc->param_uniform_idx, (size_t)desc->n_uniform_grad * 4); o += b_idx;
    const size_t o_dat = o; memcpy(&host[o], desc->dataset, (size_t)desc->dataset_size * desc->n_features * 4); o += b_dat;
    const size_t o_lab = o; memcpy(&host[o], desc->labels, (size_t)desc->dataset_size * 4); o += b_lab;
    hipError_t e = hipMalloc(&p->dev_blob, total);
    if (e != hipSuccess) { delete p; return fail(BSVI_ERR_HIP, std::string("hipMalloc: ") + hipGetErrorString(e)); }
    e = hipMemcpy(p->dev_blob, host.data(), total, hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(p->dev_blob); delete p; return fail(BSVI_ERR_HIP, std::string("hipMemcpy: ") + hipGetErrorString(e)); }
    char* base = (char*)p->dev_blob;
    p->uniform = (const bsvi_uniform_entry*)(base + o_uni);
    p->consts = (const float*)(base + o_con);
    p->pu_ptr = (const uint32_t*)(base + o_ptr);
    p->pu_idx = (const uint32_t*)(base + o_idx);
    p->dataset = (const float*)(base + o_dat);
    p->labels = (const float*)(base + o_lab);
    p->sw = dense_read_switches();
    dsel::Model& m = p->m;
    m.C = desc->n_classes; m.P = desc->n_features; m.B = desc->batch_size; m.DS = desc->dataset_size;
    m.n_params = desc->n_params; m.n_uniform_grad = desc->n_uniform_grad;
    m.blackbox = desc->estimator == BSVI_EST_BLACKBOX; m.entropy_weight = desc->entropy_weight;
    for (int i = 0; i < 4; ++i) { m.base[i] = bases[i]; m.stride[i] = strides[i]; }
    if (dsel::wants_exact_scan(m, p->sw)) {      // the exact-data path: all dataset values exactly bf16
        const uint32_t* bits = reinterpret_cast<const uint32_t*>(desc->dataset);
        const size_t n_values = (size_t)desc->dataset_size * desc->n_features;
        m.exact_data = true;
        for (size_t i = 0; m.exact_data && i < n_values; ++i) m.exact_data = (bits[i] & 0xFFFFu) == 0u;
    }
    int dev = 0, n_cu = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n_cu > 0)
        m.n_cu = (uint32_t)n_cu;
    p->mp = dsel::model_plan(m, p->sw);
    // the device facts: a refused LDS grant sends the model to the six-launch sequence (regular kinds) or to seven-block tiles (nine-block
    // kinds); on a profiling kind it changes nothing
    for (uint32_t i = 0; i < p->mp.n_attr; ++i) {
        const dsel::Attr& at = p->mp.attr[i];
        const void* fn = dense_is_xfwd(at.kind) ? (const void*)kDenseXfwd[at.kind - dsel::XFWD_FIRST] : (const void*)kDenseXbwd[at.kind - dsel::XBWD_FIRST];
        if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)at.lds) == hipSuccess) continue;
        (void)hipGetLastError();
        if (at.cls == dsel::ATTR_REGULAR) m.fused_ok = false;
        if (at.cls == dsel::ATTR_NINE) m.xb9_ok = false;
    }
    p->d.uniform = nullptr; p->d.consts = nullptr; p->d.param_uniform_ptr = nullptr; p->d.param_uniform_idx = nullptr;
    p->d.dataset = nullptr; p->d.labels = nullptr;
    *out = p;
    return BSVI_OK;
}

extern "C" int bsvi_dense_exact_data(const bsvi_dense* p) { return (p && p->mp.path != dsel::F32) ? 1 : 0; }
extern "C" const char* bsvi_dense_kind_name(int kind) { return dsel::name(kind); }

extern "C" void bsvi_dense_destroy(bsvi_dense* p) {
    if (!p) return;
    if (p->dev_blob) (void)hipFree(p->dev_blob);
    delete p;
}

extern "C" size_t bsvi_dense_workspace_bytes(const bsvi_dense* p, uint32_t n_local) {
    if (!p || !n_local) return 0;
    dsel::Call c;
    c.n_local = n_local;      // (the layout follows the sample count alone)
    return dsel::layout(p->m, dsel::call_plan(p->m, p->sw, c)).total;
}

// what the selection needs of a call, behind the checks of the arguments that depend on the estimator
static int dense_call(const bsvi_dense* p, const bsvi_dense_args* a, dsel::Call& c) {
    if (!a->n_samples_local || !a->n_samples_global) return fail(BSVI_ERR_INVALID, "zero samples");
    if (a->q_weight_dev && p->d.estimator != BSVI_EST_BLACKBOX)
        return fail(BSVI_ERR_INVALID, "q_weight_dev needs a model lowered for the BlackBox estimator (its launches accumulate log q)");
    if (a->logq_out_dev && p->d.estimator != BSVI_EST_BLACKBOX)
        return fail(BSVI_ERR_INVALID, "logq_out_dev needs a model lowered for the BlackBox estimator (its launches accumulate log q)");
    if (p->d.estimator == BSVI_EST_BLACKBOX && !a->f_weight_dev != !a->q_weight_dev)
        return fail(BSVI_ERR_INVALID, "a BlackBox model takes f_weight_dev and q_weight_dev together (or neither)");
    c.n_local = a->n_samples_local;
    c.fvalue_out = a->fvalue_out_dev != nullptr; c.f_weight = a->f_weight_dev != nullptr; c.q_weight = a->q_weight_dev != nullptr;
    c.logq_out = a->logq_out_dev != nullptr; c.noise_in = a->noise_dev != nullptr;
    return BSVI_OK;
}

extern "C" int bsvi_dense_plan(const bsvi_dense* p, const bsvi_dense_args* a, int32_t* kinds, uint32_t capacity) {
    if (a) BSVI_CHECK_STRUCT(a, bsvi_dense_args);
    if (!p || !a || (!kinds && capacity)) return fail(BSVI_ERR_INVALID, "null argument");
    dsel::Call c;
    const int rc = dense_call(p, a, c);
    if (rc) return rc;
    const dsel::Plan plan = dsel::call_plan(p->m, p->sw, c);
    for (uint32_t i = 0; i < plan.n && i < capacity; ++i) kinds[i] = (int32_t)plan.launch[i].kind;
    return (int)plan.n;
}

static int dense_fill(const bsvi_dense* p, const bsvi_dense_args* a, DParams& D, dsel::Plan& plan) {
    if (a) BSVI_CHECK_STRUCT(a, bsvi_dense_args);
    if (!p || !a) return fail(BSVI_ERR_INVALID, "null argument");
    if (!a->params_dev || !a->out_dev || !a->workspace_dev) return fail(BSVI_ERR_INVALID, "null device pointer");
    dsel::Call c;
    const int rc = dense_call(p, a, c);
    if (rc) return rc;
    plan = dsel::call_plan(p->m, p->sw, c);
    const dsel::Layout L = dsel::layout(p->m, plan);
    char* ws = (char*)a->workspace_dev;
    memset(&D, 0, sizeof(D));
    D.uniform = p->uniform; D.consts = p->consts; D.params = a->params_dev; D.dataset = p->dataset; D.labels = p->labels;
    D.noise_in = a->noise_dev; D.indices_in = a->indices_dev; D.noise_out = a->noise_out_dev; D.indices_out = a->indices_out_dev;
    D.fvalue_out = a->fvalue_out_dev;
    D.f_weight = a->f_weight_dev; D.q_weight = a->q_weight_dev; D.logq_out = a->logq_out_dev;
    D.wsum = (float*)(ws + L.wsum); D.ws1 = (float*)(ws + L.ws1); D.ws2 = (float*)(ws + L.ws2);
    D.rowp = (float*)(ws + L.rowp); D.idx = (int32_t*)(ws + L.idx); D.Xb = (float*)(ws + L.Xb); D.XbT = (float*)(ws + L.XbT);
    D.lab = (float*)(ws + L.lab); D.eps = (float*)(ws + L.eps); D.pv_part = (float*)(ws + L.pv_part);
    D.qv_part = (float*)(ws + L.qv_part);
    D.estimator = p->d.estimator;
    D.per_sample = plan.per_sample;
    D.s1 = (float*)(ws + L.s1); D.s2 = (float*)(ws + L.s2); D.lik_part = (float*)(ws + L.lik_part);
    D.dlog = (float*)(ws + L.dlog); D.ds_part = (float*)(ws + L.ds_part); D.dmu_part = (float*)(ws + L.dmu_part);
    D.rowg = (float*)(ws + L.rowg); D.hpart = (float*)(ws + L.hpart); D.partial = (float*)(ws + L.partial);
    D.C = p->d.n_classes; D.P = p->d.n_features; D.P_pad = plan.P_pad; D.DS = p->d.dataset_size; D.B = p->d.batch_size;
    D.B_pad = plan.B_pad; D.R = plan.R;
    D.n_local = a->n_samples_local; D.n_global = a->n_samples_global; D.n_pad = plan.n_pad; D.sample_base = a->sample_base;
    D.likelihood = p->d.likelihood; D.n_uniform_grad = p->d.n_uniform_grad;
    D.q_loc_u = p->d.q_loc_u; D.q_scale_u = p->d.q_scale_u; D.prior_loc_u = p->d.prior_loc_u; D.prior_scale_u = p->d.prior_scale_u;
    D.q_loc_stride = p->d.q_loc_stride; D.q_scale_stride = p->d.q_scale_stride;
    D.prior_loc_stride = p->d.prior_loc_stride; D.prior_scale_stride = p->d.prior_scale_stride;
    D.lik_weight = p->d.lik_weight; D.prior_weight = p->d.prior_weight; D.entropy_weight = p->d.entropy_weight;
    D.seed_lo = (uint32_t)a->seed; D.seed_hi = (uint32_t)(a->seed >> 32);
    D.offset_lo = (uint32_t)a->offset; D.offset_hi = (uint32_t)(a->offset >> 32);
    D.row_chunk = dsel::kDenseRowChunk;
    D.xpath = plan.exact ? 1u : 0u; D.Kp = plan.Kp;
    if (plan.exact) {
        D.Xb_bf = (uint16_t*)(ws + L.Xb_bf); D.XbT_bf = (uint16_t*)(ws + L.XbT_bf); D.Wp = (uint16_t*)(ws + L.Wp);
        D.logitsT = (float*)(ws + L.logitsT); D.dlogp = (uint16_t*)(ws + L.dlogp); D.GT = (float*)(ws + L.GT);
    }
    D.ksplit = plan.ksplit; D.lik_parts = plan.lik_parts; D.xfused = plan.xfused ? 1u : 0u;
    D.stamps = g_debug_stamps;
    return BSVI_OK;
}

// One iteration: the plan of this call (dense_select.h), then its launches in order.  R arrives zeroed but for what an optimizer step
// adds to the parameter kernel's block.
static int dense_iterate(const bsvi_dense* p, const bsvi_dense_args* a, RParams& R) {
    DParams D;
    dsel::Plan plan;
    int rc = dense_fill(p, a, D, plan);
    if (rc) return rc;
    R.uniform = p->uniform; R.pu_ptr = p->pu_ptr; R.pu_idx = p->pu_idx;
    R.partials = D.partial; R.params = (float*)a->params_dev; R.out = a->out_dev;
    R.n_uniform_grad = p->d.n_uniform_grad; R.n_params = p->d.n_params; R.n_blocks = 1; R.n_global = D.n_global;
    DParams E = D;      // what dense_epilogue and dense_param_fold_kernel read: the per-sample sums may already be whole
    E.sums_folded = plan.sums_folded ? 1u : 0u;
    const hipStream_t s = (hipStream_t)a->stream;
    const int NC = (int)(D.n_pad * D.C);
    for (uint32_t i = 0; i < plan.n; ++i) {
        const dsel::Launch& l = plan.launch[i];
        const dim3 grid(l.grid_x, l.grid_y), block(l.block);
        dense_plain_fn plain = nullptr;      // the kernels that take the parameter block alone, without dynamic LDS
        switch (l.kind) {
        case dsel::WEIGHTED_SUMS: plain = dense_weighted_sums; break;
        case dsel::PROLOGUE: plain = dense_prologue; break;
        case dsel::GATHER: plain = dense_gather; break;
        case dsel::NOISE: plain = dense_noise; break;
        case dsel::FORWARD_1: case dsel::FORWARD_4: case dsel::FORWARD_10: case dsel::FORWARD_16: plain = kDenseForward[l.kind - dsel::FORWARD_FIRST]; break;
        case dsel::BACKWARD: plain = dense_backward; break;
        case dsel::WSPLIT: plain = dense_wsplit; break;
        case dsel::CE: plain = dense_ce; break;
        case dsel::XREDUCE: plain = dense_xreduce; break;
        case dsel::ROWS: case dsel::ROWS_SLICED: plain = dense_rows; break;
        case dsel::HEAD: hipLaunchKernelGGL(dense_head, grid, block, 0, s, D, l.arg[0], l.arg[1]); break;
        case dsel::XGEMM_LOGITS:
            rc = bsvi_xgemm_nt(D.Xb_bf, nullptr, D.Wp, (long)NC * D.Kp, D.logitsT, NC, (int)D.B_pad, NC, (int)D.Kp, s);
            if (rc) return rc;
            break;
        case dsel::XGEMM_GRAD:
            rc = bsvi_xgemm_nt(D.XbT_bf, nullptr, D.dlogp, (long)NC * D.B_pad, D.GT, NC, (int)D.P, NC, (int)D.B_pad, s);
            if (rc) return rc;
            break;
        case dsel::SAMPLE_SUMS: hipLaunchKernelGGL(dense_sample_sums, grid, block, 0, s, D, l.arg[0]); break;
        case dsel::EPILOGUE: hipLaunchKernelGGL(dense_epilogue, grid, block, 0, s, E); break;
        case dsel::PARAM: hipLaunchKernelGGL(dense_param_kernel, grid, block, 0, s, R); break;
        case dsel::PARAM_FOLD: hipLaunchKernelGGL(dense_param_fold_kernel, grid, block, 0, s, R, E, l.arg[0]); break;
        default:
            if (dense_is_xfwd(l.kind)) hipLaunchKernelGGL(kDenseXfwd[l.kind - dsel::XFWD_FIRST], grid, block, l.lds, s, D, l.arg[0]);
            else hipLaunchKernelGGL(kDenseXbwd[l.kind - dsel::XBWD_FIRST], grid, block, l.lds, s, D, l.arg[0], l.arg[1], l.arg[2], l.arg[3]);
        }
        if (plain) hipLaunchKernelGGL(plain, grid, block, 0, s, D);
    }
    HIP_TRY(hipGetLastError());
    return BSVI_OK;
}

extern "C" int bsvi_dense_fwd_bwd(const bsvi_dense* p, const bsvi_dense_args* a) {
    RParams R;
    memset(&R, 0, sizeof(R));
    return dense_iterate(p, a, R);
}

extern "C" int bsvi_dense_step(const bsvi_dense* p, const bsvi_dense_args* a, const bsvi_opt_cfg* cfg, float* params_dev,
                               float* state_dev, const uint8_t* active_mask_dev, float* loss_slot_dev, float* finite_slot_dev) {
    int rc = check_cfg(cfg);
    if (rc) return rc;
    if (!params_dev || !state_dev || !active_mask_dev) return fail(BSVI_ERR_INVALID, "null argument");
    if (a && a->n_samples_local != a->n_samples_global) return fail(BSVI_ERR_INVALID, "bsvi_dense_step is the single-GPU path");
    if (a && a->struct_size == sizeof(bsvi_dense_args) && (a->f_weight_dev || a->q_weight_dev))
        return fail(BSVI_ERR_INVALID, "caller-weighted gradients are an evaluation (bsvi_dense_fwd_bwd), not an optimizer step");
    bsvi_dense_args aa = *a;
    aa.params_dev = params_dev;
    RParams R;
    memset(&R, 0, sizeof(R));
    R.state = state_dev; R.active_mask = active_mask_dev; R.loss_slot = loss_slot_dev; R.finite_slot = finite_slot_dev;
    R.do_finalize = 1; R.do_step = 1; R.cfg = *cfg;
    return dense_iterate(p, &aa, R);
}

extern "C" int bsvi_dense_finalize(const bsvi_dense* p, float* out_dev, uint32_t n_global, void* stream) {
    if (!p || !out_dev || !n_global) return fail(BSVI_ERR_INVALID, "null argument");
    const uint32_t n = p->d.n_params ? p->d.n_params : 1;
    hipLaunchKernelGGL(finalize_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, out_dev, p->d.n_params, n_global);
    HIP_TRY(hipGetLastError());
    return BSVI_OK;
}
