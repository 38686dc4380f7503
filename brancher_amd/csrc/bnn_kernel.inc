// bnn_kernel.inc — Bayesian neural networks on the dense-link path (included by elbo_kernel.hip behind dense_kernel.inc).
//
// The reference's model family (tests/test_MNIST_bayesian_neural_network.py:20-60): a chain
//     logits = W_L act( ... act(W_1 x + b_1) ... ) + b_L
// in which EVERY weight matrix and every bias is a latent with a mean-field Normal posterior, the likelihood an observed
// Categorical (or Binomial(1)) over a random minibatch — or, for regression, an observed Normal whose loc is the chain and whose
// scale sigma is a constant of the model (BSVI_LIK_NORMAL, bsvi_bnn_create_normal): one real target per output and minibatch row,
// lab [B_pad][C], where the classifiers keep one label per row.  Per (row b, sample n):
//     lik = wgt sum_c (-1/2 u_c^2 - log sigma_c - 1/2 log 2 pi),  u_c = (y[b][c] - z_c) / sigma_c;   delta_c = wgt u_c / sigma_c
// at the three sites that hold a likelihood (bnn_upper, bnn_upper_gen, bnn_mid_gen); everything behind the deltas is unchanged.
// A learnable sigma (bsvi_bnn_create_normal_learnable: sigma_c = a + b g(theta), a parameter entry of the uniform table) takes
//     G_c = sum_n sum_b wgt (u_c^2 - 1) / sigma_c
// into the gradient of its entry: per (c, b, n) beside liknb at the two bnn_upper sites and summed over b by bnn_sig_rows (bnn_lik's
// order), per (c, n) out of the tile in bnn_mid_gen; then over n in double precision (bnn_epilogue) and into the entry (bnn_uniform_grads).
// All of it behind BParams::scale_learn / a generator switch: a constant sigma and the classifiers run what they ran.
// A scale head (bsvi_bnn_create_normal_heads: heteroscedastic regression) makes sigma a function of the input: the last layer has 2 C
// rows, z_c the loc and z_(C + c) the raw scale of output c, sigma_c = a + b g(z_(C + c)) with g softplus / exp / sigmoid, and the
// epilogue of every site seeds BOTH halves,
//     delta_c = wgt u_c / sigma_c,      delta_(C + c) = wgt (u_c^2 - 1) / sigma_c * b g'(z_(C + c))
// so that the reverse sweep, bnn_small, the second product and the row sums carry the gradient to the four head tensors as they carry
// any delta (no sigma table behind the targets, none of the scale_learn machinery).  BParams::C stays the number of TARGETS per row.
// The observed variable may be a Laplace or a Cauchy variable in the place of the Normal (bsvi_bnn_set_likelihood_family; BParams::family,
// a literal in the generated kernels): with psi the family's score, -|u| - log(2 sigma) and psi = sign(u), or -log(1 + u^2) - log(pi sigma)
// and psi = 2 u / (1 + u^2), and at every site  delta_c = wgt psi / sigma_c,  d f / d sigma_c = wgt (u psi - 1) / sigma_c  (the Normal:
// psi = u) — so a learnable sigma's sums and a scale head's second delta are what they were with u psi in the place of u^2, and
// bnn_mid_gen's sigma elements, which sum delta_c (y_c - z_c) = wgt u psi, need nothing.  One device function serves the three families (bnn_loc_scale_term).
// All latent scalars form ONE vector of R rows (weights1 first: H_1 x P
// rows r = h * P + p, then the other tensors); row r draws eps from the dense path's Philox counters (sample, r >> 2), so the
// noise of a model is one [R][N] matrix as on the dense path, and reads its four parameters (q loc, q scale, prior loc, prior
// scale) from the uniform table through a per-row index — any mixture of per-element arrays and shared scalars.
//
// An iteration (variables.py:843-870 for this graph):
//   bnn_head        row parameters; the minibatch (indices as on the dense path, gather of x)
//   bnn_draw        W = mu + s eps for every row and sample: weights1 as the B operand of the first product (three exact bf16
//                   pieces when the data is exactly bf16, else f32), the small tensors per sample; per-sample prior / log q sums
//   product 1       a1[b][(h, n)] = sum_p x[b][p] W1[n][h][p]              bf16 matrix cores on exact pieces | f32-input MFMA
//   bnn_upper       one thread per (sample, minibatch row): bias + activation, the upper layers (per-sample H_l x H_l-1 products),
//                   the likelihood (log-softmax cross-entropy | Bernoulli logits | Normal), the reverse sweep down to d f / d a1 (as
//                   the operand of the second product)
//   bnn_small / bnn_lik   per sample: gradients of the small tensors (sums over the minibatch), the sample's likelihood
//   product 2       GT[(h, n)][p] = sum_b d a1[(h, n)][b] x[b][p]
//   bnn_row_sums    per row: sum_n eps G, sum_n G, sum_n eps, sum_n eps^2 (fixed order)
//   bnn_row_sums (its last part) / bnn_epilogue / bnn_uniform_grads / dense_param_kernel      closed-form prior and entropy terms, the value, chain rule
// The two products carry the flops (2 x 2 N H_1 P B); everything else is elementwise or tiny and written for clarity.
//
// Point-estimated rows (bsvi_bnn_set_point_rows: the reference's RootVariable members of a posterior model, inference.MAP when every
// row is one): a byte per row; a point row has w = its q loc entry for every sample, no draw, no log q, no entropy and no score term, and
// its prior as any row of its kind.  The POINT instantiations of bnn_draw and bnn_row_sums read the byte (the normal of such a row is
// taken as 0: every formula of the row then holds as it stands, and bnn_row_terms / bnn_row_terms_sums leave out the terms in s); the
// Philox counters of the other rows do not move.  A model without a point row launches the instantiations it launched.
// The shared first layer (bnn_select.h, shared_first; BSVI_BNN_SHARED1=0 switches it off): with EVERY row of weights1 a point, all samples
// share weights1, and an iteration is
//   bnn_head_gather, bnn_draw    as above, without the N copies of weights1 (a chunk of weights1 rows takes its prior sum once)
//   bnn_first_shared             a1s[h][b] = sum_p x[b][p] W1[h][p], once (a wave per (b, h))
//   bnn_first_broadcast          a1s laid out as the a1 the middle kernel reads (its text and its launch are untouched)
//   the middle kernel            as above
//   bnn_da1_partial / _total     dbar[h][b] = sum_n d f / d a1[(h, n)][b], a fixed order in two steps, no atomics
//   bnn_second_shared            GT1[h][p] = sum_b dbar[h][b] x[b][p]: ONE second product, behind the sum over the samples
//   bnn_rows_shared              weights1's row terms from GT1;  bnn_row_sums takes the other rows (quad0)
// and the epilogue as above.  The workspace holds no copy of weights1 per sample and no per-sample GT then.
// The text of the two generated kernels, bnn_upper_gen and bnn_mid_gen, lives in bnn_source.h (host only: tests/test_bnn_source_cpu.py
// holds it to recorded digests without a GPU); this file fills its input (bnn_source_net) and compiles what it writes (bnn_gen_ready).

#include <atomic>

#include "bnn_select.h"
#include "bnn_source.h"

constexpr uint32_t BNN_MAX_LAYERS = 8;

struct BnnLayerDev { uint32_t rows, cols, w0, b0, act, act_off, delta_off, in_off; };

struct BParams {
    // tables
    const bsvi_uniform_entry* uniform; const float* consts; const float* params; const uint32_t* row_uniform;   // [4][R]
    const uint32_t* ur_ptr; const uint32_t* ur_item;          // uniform entry (with gradient) -> (role * R + row) items
    const float* dataset; const float* labels;
    BnnLayerDev layer[BNN_MAX_LAYERS];
    uint32_t n_layers, R, R1, Rs, P, C, H1, DS, B, B_pad, Kp, P_ld, n_local, n_pad, n_global, sample_base, NC;
    uint32_t n_uniform_grad, likelihood, estimator, exact, act_width;
    uint32_t LC, scale_u, scale_stride;       // targets per minibatch row (1 label; C for the Normal likelihood) and sigma's uniform entries
    uint32_t scale_learn;                     // sigma's entries are parameters: its gradient is accumulated (launch-uniform)
    // a scale head (bsvi_bnn_create_normal_heads; 0: none): the last layer has 2 C rows, the loc in row c and the raw scale in row C + c,
    // sigma_c = head_a + head_b g(raw) with g the BSVI_UT_* transform `heads`.  C, LC and the targets stay C per row: where a kernel
    // means "rows of the last layer" it reads layer[n_layers - 1].rows, never C
    uint32_t heads; float head_a, head_b;
    float lik_weight, prior_weight, entropy_weight;
    uint32_t seed_lo, seed_hi, offset_lo, offset_hi;
    const float* noise_in; float* noise_out; const int32_t* indices_in; int32_t* indices_out; float* fvalue_out; float* logq_out;
    // caller-weighted gradients (bsvi_bnn_args::f_weight_dev / q_weight_dev, the second pass of a user-defined gradient estimator,
    // engine.custom_estimator_loss): the launches leave sum_n a_n grad f_n + b_n grad log q_n.  a_n scales the likelihood's gradient
    // seeds (everything behind them is linear in the seeds), the closed-form prior terms take sum_n a_n eps_n, sum_n a_n eps_n^2 and
    // sum_n a_n, the entropy sum_n a_n, and the score term's sum_n f_n becomes sum_n b_n (d log q_n / d s_r = -1 / s_r for every sample)
    const float* f_weight;      // [n_local] or null (a_n = 1)
    const float* q_weight;      // [n_local] or null (BlackBox: b_n = f_n)
    // workspace
    float* rowp;            // [4][R]
    int32_t* idx;
    float* lab;             // [B_pad][LC]; Normal likelihood: then sigma [C] and -log sigma - 1/2 log 2 pi [C] (bnn_head_body)
    float* Xb; uint16_t* Xb_bf; uint16_t* XbT_bf;
    float* W1f; uint16_t* Wp; float* Wsm;
    float* a1T;             // [B_pad][NC]
    float* acts; float* deltas; float* liknb;
    float* da1T; uint16_t* dlogp;
    float* GT;              // exact: [P][NC]; f32: [NC][P_ld]
    float* gsm; float* lik; float* pv_part; float* qv_part; float* sums; float* rowg; double* hpart; float* partial; float* fs;
    uint32_t row_chunks;
    // a learnable sigma only (null otherwise): wgt (u^2 - 1) / sigma per (c, b, n) of the bnn_upper sites, its sum over b per (c, n),
    // and that over n
    float* sigt;            // [C][B_pad][n_pad]
    float* gsig;            // [C][n_pad]
    double* gsd;            // [C]
    // the prior of every row (bsvi_bnn_set_row_priors): BSVI_DIST_NORMAL | _LAPLACE | _CAUCHY, one byte per row, padded with Normal to
    // a whole quad.  Read by the MIXED instantiations of bnn_draw and bnn_row_sums alone: a model whose rows are all Normal never looks
    const uint8_t* row_kind;
    // the family of the loc-scale likelihood (bsvi_bnn_set_likelihood_family): BSVI_DIST_NORMAL | _LAPLACE | _CAUCHY, launch-uniform.
    // Behind every other member, so that no field the kernels of the models without it read has moved
    uint32_t family;
    // latent prior scales (bsvi_bnn_set_scale_latents; n_latents = 0: none, and nothing below is read): tau_t = exp(m_t + s_t eps) scales the
    // prior of the rows whose byte of row_latent is t (0xFF: none; padded with 0xFF to a whole quad), lat_uniform [4][T] the entries of
    // q loc, q scale, prior loc, prior scale, lat_count [T] the number of rows under each.  Per launch and (t, n), [T][n_pad]:
    // l, 1 / tau and eps (the latent blocks of bnn_head_gather), D = d f_n / d l and z = (l - m0) / s0 (bnn_latent_terms); lat_upart
    // [row_chunks][T][n_pad] the chunks' sums of u psi - 1 over the rows under t (bnn_draw), lat_f / lat_q [n_pad] the latents' per-sample
    // parts of f and log q, lat_b [n_pad] the score weights b_n (bnn_epilogue).  Behind every other member, as `family` is
    uint32_t n_latents;
    const uint8_t* row_latent; const uint32_t* lat_uniform; const uint32_t* lat_count;
    float* lat_l; float* lat_itau; float* lat_eps; float* lat_D; float* lat_z; float* lat_upart;
    double* lat_f; double* lat_q; double* lat_b;
    // point-estimated rows (bsvi_bnn_set_point_rows; null: none): a byte per row, padded with 0 to a whole quad.  A row whose byte is set is
    // not random in the posterior: w = its q loc entry for every sample, no draw, no log q and no entropy term.  Read by the POINT
    // instantiations of bnn_draw and bnn_row_sums alone.  Behind every other member, as `family` is
    const uint8_t* row_point;
    // the shared first layer (bnn_select.h, shared_first; 0: both products per sample): every row of weights1 is a point row, so
    // a1s [H1][B_pad] = W1 x is taken once (bnn_first_shared) and broadcast into a1T (bnn_first_broadcast), d f / d a1 is summed over the
    // samples in a fixed order — dpart [n_pad / 64][H1][B_pad] the sums of 64 samples (bnn_da1_partial), dbar [H1][B_pad] theirs
    // (bnn_da1_total) — and GT1 [H1][P] = dbar x (bnn_second_shared) goes into weights1's row terms directly (bnn_rows_shared); quad0: the
    // first row quad bnn_row_sums still takes (R1 / 4 then, else 0)
    uint32_t shared1, quad0;
    float* a1s; float* dpart; float* dbar; float* GT1;
    // the parameters of the layers' activations (bsvi_bnn_set_activation_params, or torch's defaults): read by bnn_upper and
    // bnn_predict_fwd for the kinds that have some.  Behind every other member, as `family` is
    float act_p[BNN_MAX_LAYERS][2];
};

// p: the layer's two parameters (BParams::act_p: leaky_relu's slope, elu's alpha, hardtanh's limits; the same expressions as
// bnn_source.h's act_text / act_grad_text / act_pair_text)
__device__ __forceinline__ float bnn_act(uint32_t act, float v, const float* p) {
    switch (act) {
    case BSVI_BNN_ACT_TANH: return tanhf(v);
    case BSVI_BNN_ACT_RELU: return fmaxf(v, 0.0f);
    case BSVI_BNN_ACT_SIGMOID: return sigmoidf_(v);
    case BSVI_BNN_ACT_SOFTPLUS: return v > 20.0f ? v : log1pf(expf(v));
    case BSVI_BNN_ACT_LEAKY_RELU: return v > 0.0f ? v : p[0] * v;
    case BSVI_BNN_ACT_ELU: return v > 0.0f ? v : p[0] * expm1f(v);
    case BSVI_BNN_ACT_SELU: return (float)BSVI_SELU_SCALE * (v > 0.0f ? v : (float)BSVI_SELU_ALPHA * expm1f(v));
    case BSVI_BNN_ACT_SOFTSIGN: return v / (1.0f + fabsf(v));
    case BSVI_BNN_ACT_HARDTANH: return fminf(fmaxf(v, p[0]), p[1]);
    case BSVI_BNN_ACT_SILU: return v * sigmoidf_(v);
    case BSVI_BNN_ACT_GELU: return v * (0.5f * (1.0f + erff(v * BSVI_INV_SQRT2)));
    default: return v;
    }
}
// derivative of the activation through its OUTPUT y (what the forward sweep stored)
__device__ __forceinline__ float bnn_act_grad(uint32_t act, float y, const float* p) {
    switch (act) {
    case BSVI_BNN_ACT_TANH: return 1.0f - y * y;
    case BSVI_BNN_ACT_RELU: return y > 0.0f ? 1.0f : 0.0f;
    case BSVI_BNN_ACT_SIGMOID: return y * (1.0f - y);
    case BSVI_BNN_ACT_SOFTPLUS: return y > 20.0f ? 1.0f : -expm1f(-y);
    case BSVI_BNN_ACT_LEAKY_RELU: return y > 0.0f ? 1.0f : p[0];
    case BSVI_BNN_ACT_ELU: return y > 0.0f ? 1.0f : y + p[0];
    case BSVI_BNN_ACT_SELU: return y > 0.0f ? (float)BSVI_SELU_SCALE : y + (float)(BSVI_SELU_SCALE * BSVI_SELU_ALPHA);
    case BSVI_BNN_ACT_SOFTSIGN: return (1.0f - fabsf(y)) * (1.0f - fabsf(y));
    case BSVI_BNN_ACT_HARDTANH: return y > p[0] && y < p[1] ? 1.0f : 0.0f;
    default: return 1.0f;      // NONE.  (SILU and GELU never come here: bnn_act_grad_from_input sends them to bnn_act_grad_input)
    }
}
// SILU and GELU are not monotone: their derivative through the PRE-activation v.  bnn_upper's forward sweep leaves it in the unit's delta
// slot, which nothing reads before the reverse sweep multiplies it in place
__device__ __forceinline__ bool bnn_act_grad_from_input(uint32_t act) { return act == BSVI_BNN_ACT_SILU || act == BSVI_BNN_ACT_GELU; }
__device__ __forceinline__ float bnn_act_grad_input(uint32_t act, float v) {
    if (act == BSVI_BNN_ACT_SILU) { const float sg = sigmoidf_(v); return sg * (1.0f + v * (1.0f - sg)); }
    if (act == BSVI_BNN_ACT_GELU) return 0.5f * (1.0f + erff(v * BSVI_INV_SQRT2)) + v * (BSVI_INV_SQRT_2PI * expf(-0.5f * v * v));
    return 1.0f;      // (no other kind: a kind added to bnn_act_grad_from_input gets its branch here)
}

// a scale head's sigma = a + b g(raw) and d sigma / d raw = b g'(raw): g softplus (as bnn_act writes it; torch's backward is 1 above the
// threshold), exp or sigmoid
__device__ __forceinline__ float bnn_head_sigma(const uint32_t t, const float a, const float b, const float raw, float& dsigma) {
    float g, dg;
    if (t == BSVI_UT_EXP) { g = expf(raw); dg = g; }
    else if (t == BSVI_UT_SIGMOID) { g = sigmoidf_(raw); dg = g * (1.0f - g); }
    else { g = raw > 20.0f ? raw : log1pf(expf(raw)); dg = raw > 20.0f ? 1.0f : sigmoidf_(raw); }
    dsigma = b * dg;
    return a + b * g;
}

// the loc-scale likelihoods in u = (y - z) / sigma: the value without its constant, plus the term k that stands beside it in the sum, and
// the score psi(u) = -d value / d u, so that every site seeds d f / d z = wgt psi / sigma and d f / d sigma = wgt (u psi - 1) / sigma
//     Normal  -u^2 / 2,  psi = u;      Laplace  -|u|,  psi = sign(u) with sign(0) = 0 (torch's abs backward);
//     Cauchy  -log(1 + u^2),  psi = 2 u / (1 + u^2)
// (the hardware logarithm, as bnn_prior_value: the sum 1 + u^2 rounds to 6e-8 absolute, what any term of O(1) of the sample's sum does)
// One launch-uniform branch per family with `+ k` inside it, each family's expression as it stood when each had a loop of its own.  The
// Normal's -0.5f * u * u + k was contracted to one FMA there; here the compiler sinks the `+ k` the three branches share behind them and
// leaves the product unfused (the per-sample f then differs in its last bit, tools/bnn_outputs_digest.py), so the FMA is spelled out.
__device__ __forceinline__ float bnn_loc_scale_term(const uint32_t family, const float u, const float k, float& psi) {
    if (family == BSVI_DIST_NORMAL) { psi = u; return fmaf(-0.5f * u, u, k); }
    if (family == BSVI_DIST_LAPLACE) { psi = u > 0.0f ? 1.0f : (u < 0.0f ? -1.0f : 0.0f); return -fabsf(u) + k; }
    const float q = 1.0f + u * u;
    psi = 2.0f * u / q;
    return -__logf(q) + k;
}
// ... and the constant of each beside -log sigma: -1/2 log 2 pi | -log 2 | -log pi
__device__ __forceinline__ float bnn_family_const(const uint32_t family) {
    return family == BSVI_DIST_NORMAL ? -0.91893853320467274178f : (family == BSVI_DIST_LAPLACE ? -0.69314718055994530942f : -1.14472988584940017414f);
}

__device__ __forceinline__ float bnn_uniform_value(const BParams& Q, uint32_t k) {
    const bsvi_uniform_entry e = Q.uniform[k];
    const float x = e.is_param ? Q.params[e.src] : Q.consts[e.src];
    return e.a + e.b * utransform(e.transform, x);
}

// the same value in double precision (the sample-independent terms of f: bnn_row_terms)
__device__ __forceinline__ double bnn_uniform_value_d(const BParams& Q, uint32_t k) {
    const bsvi_uniform_entry e = Q.uniform[k];
    const double x = (double)(e.is_param ? Q.params[e.src] : Q.consts[e.src]);
    double g = x;
    switch (e.transform) {
    case BSVI_UT_SOFTPLUS: g = x > 30.0 ? x : log1p(exp(x)); break;       // (torch.nn.functional.softplus, threshold 20: the same value in double precision)
    case BSVI_UT_SIGMOID: g = 1.0 / (1.0 + exp(-x)); break;
    case BSVI_UT_EXP: g = exp(x); break;
    case BSVI_UT_LOG: g = log(x); break;
    case BSVI_UT_TANH: g = tanh(x); break;
    case BSVI_UT_SQRT: g = sqrt(x); break;
    case BSVI_UT_SQUARE: g = x * x; break;
    default: break;
    }
    return (double)e.a + (double)e.b * g;
}

// the per-sample part of log p(w) of a row in u = (w - mu0) / s0, by select (the kinds differ across the lanes of bnn_draw); the
// sample-independent part is bnn_row_terms' / bnn_row_terms_sums'
// (log(1 + u^2) by the hardware logarithm: every lane evaluates all three, and log1pf's polynomial alone doubled the kernel's time at
//  784-20-10; the sum 1 + u^2 rounds to 6e-8 absolute, the size of the rounding of the Normal's -u^2 / 2 at u ~ 1)
__device__ __forceinline__ float bnn_prior_value(const uint32_t kind, const float u) {
    const float vn = -0.5f * u * u, vl = -fabsf(u), vc = -__logf(1.0f + u * u);
    return kind == BSVI_DIST_LAPLACE ? vl : (kind == BSVI_DIST_CAUCHY ? vc : vn);
}

// the four normals of quad g and sample n: the dense path's definition (dense_eps4)
__device__ __forceinline__ void bnn_philox_quad(const BParams& Q, uint32_t n, uint32_t g, float e[4]) {
    const u32x4 x = philox4x32(Q.sample_base + n, g | 0x40000000u, Q.offset_lo, Q.offset_hi, Q.seed_lo, Q.seed_hi);
    box_muller_fast(x.x, x.y, e[0], e[1]);
    box_muller_fast(x.z, x.w, e[2], e[3]);
}

// the normals of rows 4g .. 4g+3 of sample n: that quad, or the caller's
__device__ __forceinline__ void bnn_eps4(const BParams& Q, uint32_t n, uint32_t g, float e[4]) {
    if (Q.noise_in) {
#pragma unroll
        for (int j = 0; j < 4; ++j) e[j] = (4u * g + j < Q.R) ? Q.noise_in[(size_t)(4u * g + j) * Q.n_local + n] : 0.0f;
        return;
    }
    bnn_philox_quad(Q, n, g, e);
}

// the keyed bijection of the dense path (the fields minibatch_index reads): row of the dataset behind minibatch position i
__device__ __forceinline__ int32_t bnn_minibatch_row(const BParams& Q, uint32_t i) {
    if (i >= Q.B) return -1;
    DParams Dm;
    Dm.indices_in = Q.indices_in; Dm.DS = Q.DS;
    Dm.offset_lo = Q.offset_lo; Dm.offset_hi = Q.offset_hi; Dm.seed_lo = Q.seed_lo; Dm.seed_hi = Q.seed_hi;
    return (int32_t)minibatch_index(Dm, i);
}

// row parameters, minibatch indices + labels, and the cleared partial block.  threads: max(R, B_pad)
__device__ __forceinline__ void bnn_head_body(const BParams& Q, const uint32_t i, const uint32_t n_threads) {
    if (i < Q.R) {
#pragma unroll
        for (uint32_t q = 0; q < 4u; ++q) Q.rowp[(size_t)q * Q.R + i] = bnn_uniform_value(Q, Q.row_uniform[(size_t)q * Q.R + i]);
    }
    if (i < Q.B_pad) {
        const int32_t row = bnn_minibatch_row(Q, i);
        if (i < Q.B && Q.indices_out) Q.indices_out[i] = row;
        Q.idx[i] = row;
        for (uint32_t c = 0; c < Q.LC; ++c) Q.lab[(size_t)i * Q.LC + c] = row >= 0 ? Q.labels[(size_t)row * Q.LC + c] : 0.0f;
    }
    if (Q.likelihood == BSVI_LIK_NORMAL && !Q.heads && i < Q.C) {      // (R >= C: the last layer alone has C rows of weights)
        const float sigma = bnn_uniform_value(Q, Q.scale_u + i * Q.scale_stride);
        float* const sg = Q.lab + (size_t)Q.B_pad * Q.LC;
        sg[i] = sigma;
        sg[Q.C + i] = -logf(sigma) + bnn_family_const(Q.family);      // -log sigma - 1/2 log 2 pi | -log(2 sigma) | -log(pi sigma)
    }
    for (uint32_t k = i; k < 2u + Q.n_uniform_grad; k += n_threads) Q.partial[k] = 0.0f;
}

// x of the minibatch: f32 [B_pad][P_ld], or bf16 [B_pad][Kp] and its transpose [P][B_pad].  blocks: B_pad x ceil(Kp / 256)
// (the row is worked out here again rather than read from idx: the head's blocks run in the same launch)
__device__ __forceinline__ void bnn_gather_body(const BParams& Q, const uint32_t b, const uint32_t p) {
    const int32_t row = bnn_minibatch_row(Q, b);
    const float v = (row >= 0 && p < Q.P) ? Q.dataset[(size_t)row * Q.P + p] : 0.0f;
    if (Q.exact) {
        if (p < Q.Kp) Q.Xb_bf[(size_t)b * Q.Kp + p] = dense_bf16_bits(v);
        if (p < Q.P) Q.XbT_bf[(size_t)p * Q.B_pad + b] = dense_bf16_bits(v);
    } else if (p < Q.P_ld) {
        Q.Xb[(size_t)b * Q.P_ld + p] = v;
    }
}

// the normal of latent t and sample n: normal t & 3 of the row-quad call whose quad index is ceil(R / 4) + (t >> 2) — behind every quad of
// rows, the same counters, key and pairing as bnn_eps4 —, or row R + t of the caller's noise
__device__ __forceinline__ float bnn_latent_eps(const BParams& Q, const uint32_t n, const uint32_t t) {
    if (Q.noise_in) return Q.noise_in[(size_t)(Q.R + t) * Q.n_local + n];
    float e[4];
    bnn_philox_quad(Q, n, (Q.R + 3u) / 4u + (t >> 2), e);
    const uint32_t j = t & 3u;
    return j == 0u ? e[0] : (j == 1u ? e[1] : (j == 2u ? e[2] : e[3]));
}

// latent prior scales: l = m_t + s_t eps, 1 / tau and eps of every (latent, sample), once per launch and from the uniform table (the
// head's blocks fill rowp in the same launch).  threads: T x n_pad
__device__ __forceinline__ void bnn_latent_body(const BParams& Q, const uint32_t i) {
    if (i >= Q.n_latents * Q.n_pad) return;
    const uint32_t t = i / Q.n_pad, n = i - t * Q.n_pad;
    float l = 0.0f, e = 0.0f;
    if (n < Q.n_local) {
        e = bnn_latent_eps(Q, n, t);
        l = bnn_uniform_value(Q, Q.lat_uniform[t]) + bnn_uniform_value(Q, Q.lat_uniform[Q.n_latents + t]) * e;
        if (Q.noise_out) Q.noise_out[(size_t)(Q.R + t) * Q.n_local + n] = e;
    }
    Q.lat_l[i] = l; Q.lat_eps[i] = e; Q.lat_itau[i] = expf(-l);
}

// ONE launch for the two: the first B_pad x gy blocks gather, the rest are the head's (and behind those, the blocks of a model with
// latent prior scales: bnn_latent_body)
__global__ void __launch_bounds__(256) bnn_head_gather(const BParams Q, const uint32_t gy, const uint32_t head_blocks) {
    const uint32_t gather_blocks = Q.B_pad * gy;
    if (blockIdx.x < gather_blocks) bnn_gather_body(Q, blockIdx.x / gy, (blockIdx.x % gy) * 256u + threadIdx.x);
    else if (blockIdx.x < gather_blocks + head_blocks) bnn_head_body(Q, (blockIdx.x - gather_blocks) * 256u + threadIdx.x, head_blocks * 256u);
    else bnn_latent_body(Q, (blockIdx.x - gather_blocks - head_blocks) * 256u + threadIdx.x);
}

// W = mu + s eps.  One wave = (chunk of 64 row quads, sample), lanes along the rows: the pieces of weights1 leave as consecutive
// 8-byte stores along p, the small tensors as consecutive floats; the per-sample prior and log q sums of the chunk by a wave sum.
// grid: row_chunks x ceil(n_pad / 4), block 256 (round 6: four samples per workgroup instead of 64 k one-wave workgroups, and the row
// parameters of a quad by 16- / 8-byte loads where their arrays' offsets allow)
// MIXED: some row's prior is Laplace or Cauchy.  The lanes run along the rows, and a quad of the small tensors can straddle two
// tensors, so the kind is per row and the value is picked by select; MIXED = false is the kernel of the all-Normal models as it was.
// LATENT (with MIXED; bsvi_bnn_set_scale_latents): the prior scale of a row under latent t is b_r tau_(t, n), so u takes 1 / tau of the
// sample, and the wave holds u of every such row: it leaves sum_(r under t) (u psi - 1) of its chunk per latent present in the chunk (a wave
// sum per latent, lat_upart; zero for the others), which bnn_latent_terms adds in chunk order.  (u psi - 1, not u psi: the terms are
// centred, so the sum over 15 680 rows does not carry their count in its leading bits.)
// POINT (with MIXED; bsvi_bnn_set_point_rows): the normal of a point row is taken as 0 whatever was drawn or handed in, so w = mu exactly,
// the row adds nothing to the sample's log q sum and reports 0 in noise_out; its prior term is that of any row of its kind.  The Philox
// call of a quad is the one it was: the other rows of the quad keep their normals.
template <bool MIXED, bool LATENT = false, bool POINT = false>
__global__ void __launch_bounds__(256) bnn_draw(const BParams Q) {
    const uint32_t chunk = blockIdx.x, lane = threadIdx.x & 63u, n = blockIdx.y * 4u + (threadIdx.x >> 6), g = chunk * 64u + lane;
    if (n >= Q.n_pad) return;
    const bool live = n < Q.n_local;
    const uint32_t quads = (Q.R + 3u) / 4u;
    float pv = 0.0f, qv = 0.0f;
    if (POINT && !LATENT && Q.shared1 && !Q.noise_out && (chunk + 1u) * 256u <= Q.R1) {
        // the shared first layer: every row of this chunk is a point row of weights1, so its prior sum is the same for every sample —
        // one wave takes it and writes it to all of them (no copies of weights1 leave: the first product reads the q loc entries).
        // (Not with scale latents: every chunk then leaves its lat_upart, zeros for a chunk of point rows, behind the sample loop below.)
        if (blockIdx.y != 0u || threadIdx.x >= 64u) return;
        const uint32_t kinds = *reinterpret_cast<const uint32_t*>(Q.row_kind + 4u * (size_t)g);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const size_t r = 4u * (size_t)g + j;
            const float u = (Q.rowp[r] - Q.rowp[2 * (size_t)Q.R + r]) / Q.rowp[3 * (size_t)Q.R + r];
            pv += bnn_prior_value((kinds >> (8 * j)) & 0xFFu, u);
        }
        pv = wave_sum(pv);
        for (uint32_t m = lane; m < Q.n_pad; m += 64u) {
            Q.pv_part[(size_t)chunk * Q.n_pad + m] = m < Q.n_local ? pv : 0.0f;
            Q.qv_part[(size_t)chunk * Q.n_pad + m] = 0.0f;
        }
        return;
    }
    float up[4] = {0.0f, 0.0f, 0.0f, 0.0f};      // LATENT: u psi - 1 of the quad's rows, and their latents (a byte per row)
    uint32_t lats = 0xFFFFFFFFu;
    if (g < quads) {
        float e[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        const uint32_t points = POINT ? *reinterpret_cast<const uint32_t*>(Q.row_point + 4u * (size_t)g) : 0u;      // (a byte per row)
        if (live && !(POINT && points == 0x01010101u)) bnn_eps4(Q, n, g, e);      // (a quad of four point rows draws nothing)
        if (POINT) {
#pragma unroll
            for (int j = 0; j < 4; ++j) e[j] = ((points >> (8 * j)) & 0xFFu) ? 0.0f : e[j];
        }
        if (LATENT) lats = *reinterpret_cast<const uint32_t*>(Q.row_latent + 4u * (size_t)g);
        uint16_t hi[4] = {0, 0, 0, 0}, mid[4] = {0, 0, 0, 0}, lo[4] = {0, 0, 0, 0};
        float w4[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        // {q loc, q scale, prior loc, prior scale} of the quad's rows
        float rp[4][4];
        // (array a starts a * R floats into rowp: 16-byte loads where that is a multiple of four floats, 8-byte loads where of two)
        const bool whole = 4u * g + 3u < Q.R, base16 = ((uintptr_t)Q.rowp & 15u) == 0u;
        const uint32_t kinds = MIXED ? *reinterpret_cast<const uint32_t*>(Q.row_kind + 4u * (size_t)g) : 0u;      // (a byte per row)
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const size_t at = (size_t)a * Q.R + 4u * g;
            if (whole && base16 && (at & 3u) == 0u) {
                const xf_f32x4 v = *reinterpret_cast<const xf_f32x4*>(Q.rowp + at);
#pragma unroll
                for (int j = 0; j < 4; ++j) rp[a][j] = v[j];
            } else if (whole && base16 && (at & 1u) == 0u) {
                const float2 v0 = *reinterpret_cast<const float2*>(Q.rowp + at), v1 = *reinterpret_cast<const float2*>(Q.rowp + at + 2);
                rp[a][0] = v0.x; rp[a][1] = v0.y; rp[a][2] = v1.x; rp[a][3] = v1.y;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) rp[a][j] = (4u * g + j < Q.R) ? Q.rowp[at + j] : 1.0f;
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t r = 4u * g + j;
            if (r >= Q.R) continue;
            const float mu = rp[0][j], s = rp[1][j], mu0 = rp[2][j], s0 = rp[3][j];
            const float w = mu + s * e[j];
            w4[j] = live ? w : 0.0f;
            if (live) {
                float u = (w - mu0) / s0;
                if (LATENT) {
                    const uint32_t lt = (lats >> (8 * j)) & 0xFFu, kind = (kinds >> (8 * j)) & 0xFFu;
                    if (lt != 0xFFu) {
                        u *= Q.lat_itau[(size_t)lt * Q.n_pad + n];
                        const float au = fabsf(u), uu = u * u;
                        up[j] = (kind == BSVI_DIST_LAPLACE ? au : (kind == BSVI_DIST_CAUCHY ? 2.0f * uu / (1.0f + uu) : uu)) - 1.0f;
                    }
                }
                if (MIXED) pv += bnn_prior_value((kinds >> (8 * j)) & 0xFFu, u);
                else pv += -0.5f * u * u;
                qv += -0.5f * e[j] * e[j];
                if (Q.noise_out) Q.noise_out[(size_t)r * Q.n_local + n] = e[j];
            }
            if (r >= Q.R1) Q.Wsm[(size_t)n * Q.Rs + (r - Q.R1)] = w4[j];
            if (Q.exact) dense_split3(w4[j], hi[j], mid[j], lo[j]);
        }
        const uint32_t r0 = 4u * g;
        if (r0 < Q.R1 && !(POINT && Q.shared1)) {      // (P is a multiple of 4: a quad of weights1 stays in one row h)
            const uint32_t h = r0 / Q.P, p = r0 - h * Q.P;
            const size_t nc = (size_t)h * Q.n_pad + n;
            if (Q.exact) {
                const size_t plane = (size_t)Q.NC * Q.Kp;
                *reinterpret_cast<xf_u32x2*>(Q.Wp + nc * Q.Kp + p) = xf_pack4(hi);
                *reinterpret_cast<xf_u32x2*>(Q.Wp + plane + nc * Q.Kp + p) = xf_pack4(mid);
                *reinterpret_cast<xf_u32x2*>(Q.Wp + 2 * plane + nc * Q.Kp + p) = xf_pack4(lo);
                if (p + 4u == Q.P) {              // the lane with the row's last quad also clears its pad columns P .. Kp (Kp - P < 32)
                    for (uint32_t c = Q.P; c < Q.Kp; c += 4u) {
                        *reinterpret_cast<xf_u32x2*>(Q.Wp + nc * Q.Kp + c) = xf_u32x2{0u, 0u};
                        *reinterpret_cast<xf_u32x2*>(Q.Wp + plane + nc * Q.Kp + c) = xf_u32x2{0u, 0u};
                        *reinterpret_cast<xf_u32x2*>(Q.Wp + 2 * plane + nc * Q.Kp + c) = xf_u32x2{0u, 0u};
                    }
                }
            } else {
                *reinterpret_cast<xf_f32x4*>(Q.W1f + nc * Q.P_ld + p) = xf_f32x4{w4[0], w4[1], w4[2], w4[3]};
            }
        }
    }
    pv = wave_sum(pv); qv = wave_sum(qv);
    if (lane == 0) { Q.pv_part[(size_t)chunk * Q.n_pad + n] = pv; Q.qv_part[(size_t)chunk * Q.n_pad + n] = qv; }
    if (LATENT) {
        for (uint32_t t = 0; t < Q.n_latents; ++t) {
            float v = 0.0f;
            bool has = false;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool mine = ((lats >> (8 * j)) & 0xFFu) == t;
                v += mine ? up[j] : 0.0f;
                has = has || mine;
            }
            if (__ballot(has) != 0ull) v = wave_sum(v);      // (wave-uniform: a chunk without a row under t writes the zero)
            if (lane == 0) Q.lat_upart[((size_t)chunk * Q.n_latents + t) * Q.n_pad + n] = v;
        }
    }
}

// (the pad columns P .. Kp of the pieces are written by bnn_draw too — the lane that holds a row's last quad: no memset per call)

// activations / deltas of layer l live as [h][b][n] (n fastest: the lanes of a wave are consecutive samples)
#define BNN_AT(off, h, b, n) ((off) + ((size_t)(h) * Q.B_pad + (b)) * Q.n_pad + (n))

// One thread per (sample n, minibatch row b), lanes along n; a workgroup = 64 samples x 8 minibatch rows (a wave takes two).  When they
// fit (LDSW) the small tensors of the 64 samples are staged once per workgroup in LDS, transposed ([row][sample]), and every thread
// keeps the activations and deltas of its (n, b) in a column of LDS ([unit][thread]: consecutive threads, consecutive banks) — global
// memory then sees each of them once, on the way out for bnn_small.
// grid: ceil(n_pad / 64) x ceil(B_pad / 8), block 256
template <bool LDSW>
__global__ void __launch_bounds__(256) bnn_upper(const BParams Q) {
    float* const wl = g_lds;                                   // [Rs][65]
    float* const ya = g_lds + (size_t)Q.Rs * 65u + threadIdx.x;   // activations [unit][256] of this thread, then its deltas
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, n = blockIdx.x * 64u + lane;
    const uint32_t units = Q.act_width;
    float* const da = ya + (size_t)units * 256u;
    if (LDSW) {
        for (uint32_t i = threadIdx.x; i < 64u * Q.Rs; i += 256u) {
            const uint32_t sn = i / Q.Rs, r = i - sn * Q.Rs;       // consecutive threads: consecutive rows of one sample
            wl[r * 65u + sn] = Q.Wsm[(size_t)(blockIdx.x * 64u + sn) * Q.Rs + r];
        }
        __syncthreads();
    }
    const float* const wsm = Q.Wsm + (size_t)n * Q.Rs;
    auto W = [&](uint32_t r) { return LDSW ? wl[r * 65u + lane] : wsm[r]; };
    // unit u of layer l: activations at Y(l, u), deltas at D(l, u) — LDS columns, or the [h][b][n] arrays in memory
    const uint32_t nbu = Q.n_pad * Q.B_pad;
    const BnnLayerDev L1 = Q.layer[0], LL = Q.layer[Q.n_layers - 1];
    for (uint32_t bi = 0; bi < 2u; ++bi) {
        const uint32_t b = blockIdx.y * 8u + wave * 2u + bi;
        if (b >= Q.B_pad) continue;
        const bool live = n < Q.n_local && b < Q.B;
        auto Y = [&](const BnnLayerDev& L, uint32_t u) -> float& { return LDSW ? ya[(size_t)(L.act_off / nbu + u) * 256u] : Q.acts[BNN_AT(L.act_off, u, b, n)]; };
        auto Dl = [&](const BnnLayerDev& L, uint32_t u) -> float& { return LDSW ? da[(size_t)(L.act_off / nbu + u) * 256u] : Q.deltas[BNN_AT(L.delta_off, u, b, n)]; };
        // ---- forward
        for (uint32_t h = 0; h < L1.rows; ++h) {
            float v = Q.a1T[(size_t)b * Q.NC + (size_t)h * Q.n_pad + n];
            if (L1.b0 != 0xFFFFFFFFu) v += W(L1.b0 - Q.R1 + h);
            Y(L1, h) = bnn_act(L1.act, v, Q.act_p[0]);
            if (bnn_act_grad_from_input(L1.act)) Dl(L1, h) = bnn_act_grad_input(L1.act, v);
        }
        for (uint32_t l = 1; l < Q.n_layers; ++l) {
            const BnnLayerDev L = Q.layer[l], Lp = Q.layer[l - 1];
            for (uint32_t i = 0; i < L.rows; ++i) {
                float s = L.b0 != 0xFFFFFFFFu ? W(L.b0 - Q.R1 + i) : 0.0f;
                for (uint32_t j = 0; j < L.cols; ++j) s += W(L.w0 - Q.R1 + i * L.cols + j) * Y(Lp, j);
                Y(L, i) = bnn_act(L.act, s, Q.act_p[l]);
                if (bnn_act_grad_from_input(L.act)) Dl(L, i) = bnn_act_grad_input(L.act, s);
            }
        }
        // ---- likelihood and d f / d logits (distributions.py:294-311 / 561-592 through torch: log_softmax, BCE with logits)
        const float wgt = live ? Q.lik_weight * (Q.f_weight ? Q.f_weight[n] : 1.0f) : 0.0f, label = Q.lab[(size_t)b * Q.LC];
        float lik = 0.0f;
        if (Q.likelihood == BSVI_LIK_NORMAL) {
            // y_c ~ family(z_c, sigma_c) (distributions.py:137 through torch; bnn_loc_scale_term), the targets of row b in lab.  sigma a
            // constant or a parameter of the model: sigma and -log sigma + the family's constant per output behind the targets
            // (bnn_head_body).  A scale head, sigma_c = a + b g(z_(C + c)): the second half of the last layer is the raw scale, and its
            // delta carries d f / d sigma through the transform — the reverse sweep takes both halves down like any delta
            const float* const yb = Q.lab + (size_t)b * Q.LC;
            const float* const sg = Q.lab + (size_t)Q.B_pad * Q.LC;
            const uint32_t Ct = Q.heads ? LL.rows / 2u : LL.rows;
            const float kf = bnn_family_const(Q.family);
            float s = 0.0f;
            for (uint32_t c = 0; c < Ct; ++c) {
                float ds = 0.0f, psi;
                const float sigma = Q.heads ? bnn_head_sigma(Q.heads, Q.head_a, Q.head_b, Y(LL, Ct + c), ds) : sg[c], u = (yb[c] - Y(LL, c)) / sigma;
                if (Q.heads) s += bnn_loc_scale_term(Q.family, u, -logf(sigma), psi) + kf;
                else s += bnn_loc_scale_term(Q.family, u, sg[Ct + c], psi);
                Dl(LL, c) = wgt * psi / sigma;
                if (Q.heads) Dl(LL, Ct + c) = wgt * (u * psi - 1.0f) / sigma * ds;
                else if (Q.scale_learn) Q.sigt[((size_t)c * Q.B_pad + b) * Q.n_pad + n] = wgt * (u * psi - 1.0f) / sigma;
            }
            lik = wgt * s;
        } else if (Q.likelihood == BSVI_LIK_CATEGORICAL) {
            float m = -INFINITY;
            for (uint32_t c = 0; c < LL.rows; ++c) m = fmaxf(m, Y(LL, c));
            float se = 0.0f, zl = 0.0f;
            for (uint32_t c = 0; c < LL.rows; ++c) {
                const float z = Y(LL, c);
                se += expf(z - m);
                if (label == (float)c) zl = z;
            }
            const float lse = m + logf(se);
            lik = wgt * (zl - lse);
            for (uint32_t c = 0; c < LL.rows; ++c) Dl(LL, c) = wgt * ((label == (float)c ? 1.0f : 0.0f) - expf(Y(LL, c) - lse));
        } else {
            const float z = Y(LL, 0);
            lik = wgt * (label * z - (fmaxf(z, 0.0f) + log1pf(expf(-fabsf(z)))));
            Dl(LL, 0) = wgt * (label - sigmoidf_(z));
        }
        Q.liknb[(size_t)b * Q.n_pad + n] = lik;
        // ---- reverse sweep: delta_l = d f / d (pre-activation of layer l); the last layer's activation is the identity
        for (uint32_t l = Q.n_layers - 1; l >= 1; --l) {
            const BnnLayerDev L = Q.layer[l], Lp = Q.layer[l - 1];
            for (uint32_t j = 0; j < L.cols; ++j) {
                float s = 0.0f;
                for (uint32_t i = 0; i < L.rows; ++i) s += W(L.w0 - Q.R1 + i * L.cols + j) * Dl(L, i);
                Dl(Lp, j) = s * (bnn_act_grad_from_input(Lp.act) ? Dl(Lp, j) : bnn_act_grad(Lp.act, Y(Lp, j), Q.act_p[l - 1]));
            }
        }
        if (LDSW) {          // what bnn_small reads: every activation below the last layer, every delta
            for (uint32_t l = 0; l < Q.n_layers; ++l) {
                const BnnLayerDev L = Q.layer[l];
                for (uint32_t u = 0; u < L.rows; ++u) {
                    if (l + 1 < Q.n_layers) Q.acts[BNN_AT(L.act_off, u, b, n)] = Y(L, u);
                    Q.deltas[BNN_AT(L.delta_off, u, b, n)] = Dl(L, u);
                }
            }
        }
        // ---- d f / d a1 as the operand of the second product, [(h, n)][b]
        for (uint32_t h = 0; h < L1.rows; ++h) {
            const size_t at = ((size_t)h * Q.n_pad + n) * Q.B_pad + b;
            const float g = live ? Dl(L1, h) : 0.0f;
            if (Q.exact) {
                uint16_t hi, mid, lo;
                dense_split3(g, hi, mid, lo);
                const size_t plane = (size_t)Q.NC * Q.B_pad;
                Q.dlogp[at] = hi; Q.dlogp[plane + at] = mid; Q.dlogp[2 * plane + at] = lo;
            } else {
                Q.da1T[at] = g;
            }
        }
    }
}

// gradients of the small tensors of layer l, per sample: g[i][j] = sum_b delta_l[i][b] y_(l-1)[j][b], the bias as the column j = cols
// (y = 1); layer 0 has only that column (weights1 is the second product).  One thread = one sample x a 4 x 4 tile of (i, j) x a quarter
// of the minibatch rows (wave w takes rows w, w + 4, ...); the four slices are joined in wave order.
// grid: ceil(n_pad / 64) x i tiles x j tiles, block 256
__global__ void __launch_bounds__(256) bnn_small(const BParams Q, const uint32_t l) {
    __shared__ float part[3][16][64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, n = blockIdx.x * 64u + lane;
    const BnnLayerDev L = Q.layer[l];
    const uint32_t i0 = blockIdx.y * 4u, j_first = l ? 0u : L.cols, j0 = j_first + blockIdx.z * 4u;
    float acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[a][c] = 0.0f;
    for (uint32_t b = wave; b < Q.B; b += 4u) {
        float d[4], y[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) d[a] = i0 + a < L.rows ? Q.deltas[BNN_AT(L.delta_off, i0 + a, b, n)] : 0.0f;
#pragma unroll
        for (int c = 0; c < 4; ++c) y[c] = j0 + c < L.cols ? Q.acts[BNN_AT(L.in_off, j0 + c, b, n)] : (j0 + c == L.cols ? 1.0f : 0.0f);
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[a][c] += d[a] * y[c];
    }
    if (wave > 0) {
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int c = 0; c < 4; ++c) part[wave - 1][4 * a + c][lane] = acc[a][c];
    }
    __syncthreads();
    if (wave > 0) return;
    float* const g = Q.gsm + (size_t)n * Q.Rs;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const uint32_t i = i0 + a, j = j0 + c;
            if (i >= L.rows) continue;
            const float v = (acc[a][c] + part[0][4 * a + c][lane]) + (part[1][4 * a + c][lane] + part[2][4 * a + c][lane]);
            if (j < L.cols) g[L.w0 - Q.R1 + i * L.cols + j] = v;
            else if (j == L.cols && L.b0 != 0xFFFFFFFFu) g[L.b0 - Q.R1 + i] = v;
        }
}

// out[n] = sum over the minibatch rows b of t[b][n]: wave w adds the rows w, w + 4, ... (eight loads in flight), the four slices are
// joined in order.  block 256, lanes along the samples
__device__ __forceinline__ void bnn_rows_sum(const BParams& Q, const float* const t, float* const out) {
    __shared__ float part[4][64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, n = blockIdx.x * 64u + lane;
    float s = 0.0f;
    for (uint32_t b0 = wave; b0 < Q.B; b0 += 32u) {
        float v[8];
#pragma unroll
        for (uint32_t u = 0; u < 8u; ++u) v[u] = b0 + 4u * u < Q.B ? t[(size_t)(b0 + 4u * u) * Q.n_pad + n] : 0.0f;
        s += ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
    }
    part[wave][lane] = s;
    __syncthreads();
    if (wave == 0) out[n] = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
}

// the likelihood of a sample.  grid: ceil(n_pad / 64), block 256
__global__ void __launch_bounds__(256) bnn_lik(const BParams Q) { bnn_rows_sum(Q, Q.liknb, Q.lik); }

// a learnable sigma behind the bnn_upper sites: the sum over the minibatch rows of output c's terms, in bnn_lik's order.
// grid: ceil(n_pad / 64) x C, block 256
__global__ void __launch_bounds__(256) bnn_sig_rows(const BParams Q) {
    bnn_rows_sum(Q, Q.sigt + (size_t)blockIdx.y * Q.B_pad * Q.n_pad, Q.gsig + (size_t)blockIdx.y * Q.n_pad);
}

// one row: gradients with respect to its four uniform entries (the formulas of dense_rows_body) and its sample-independent terms of f
__device__ __forceinline__ void bnn_row_terms(const BParams& Q, const uint32_t r, const float ds_lik, const float dmu_lik, const float S1,
                                              const float S2, const float N, double& hconst, double& qconst, const bool point = false) {
    // (N: the number of samples, or sum_n a_n of caller-weighted gradients; S1, S2 weighted alike)
    const float mu = Q.rowp[r], s = Q.rowp[Q.R + r], mu0 = Q.rowp[2 * (size_t)Q.R + r], s0 = Q.rowp[3 * (size_t)Q.R + r];
    const float delta = mu - mu0, is2 = 1.0f / (s0 * s0);
    const float sum_dw = -(N * delta + s * S1) * is2;                       // sum_n d log p / d W
    const float sum_dw_e = -(delta * S1 + s * S2) * is2;                    // sum_n d log p / d W * eps
    const float sum_sq = N * delta * delta + 2.0f * delta * s * S1 + s * s * S2;   // sum_n (W - mu0)^2
    Q.rowg[r] = dmu_lik + Q.prior_weight * sum_dw;
    // (a point row: s = 0 and S1 = S2 = 0 — the closed form above holds as it stands; no entropy, no log s, no log q)
    Q.rowg[Q.R + r] = point ? 0.0f : ds_lik + Q.prior_weight * sum_dw_e + Q.entropy_weight * N / s;
    Q.rowg[2 * (size_t)Q.R + r] = -Q.prior_weight * sum_dw;
    Q.rowg[3 * (size_t)Q.R + r] = Q.prior_weight * (sum_sq * is2 / s0 - N / s0);
    // (in double precision from the parameters on: with one scale shared by all rows — every untrained model — the single-
    //  precision rounding of log s is the SAME for every row, a bias of R x 6e-8 in f that BlackBox multiplies by log q ~ 1e4;
    //  the sample-independent terms of f are R terms of O(1) whose sum cancels against the per-sample ones: kept in double
    //  precision from here to the per-sample f)
    const double sd = bnn_uniform_value_d(Q, Q.row_uniform[Q.R + r]), s0d = bnn_uniform_value_d(Q, Q.row_uniform[3 * (size_t)Q.R + r]);
    hconst = (double)Q.prior_weight * (-log(s0d) - 0.91893853320467274178) + (point ? 0.0 : (double)Q.entropy_weight * (1.41893853320467274178 + log(sd)));
    qconst = point ? 0.0 : -log(sd) - 0.91893853320467274178;
}

// ... of a row without that closed form in sum eps, sum eps^2: from the per-sample sums of bnn_row_sums<true>,
//     T0 = sum_n a_n t_n,  T1 = sum_n a_n eps_n t_n,      t = d log p / d w
// and T2 = sum_n a_n d log p / d s0 from the two: log p = g(u) - log s0 with u = (w - mu0) / s0 for every family, so
// d log p / d s0 = -u t - 1 / s0, and with w - mu0 = (mu - mu0) + s eps:   T2 = -((mu - mu0) T0 + s T1 + N) / s0
// (the same summands regrouped: no accumulators and no per-sample arithmetic of its own).
// Such rows are those whose prior is Laplace or Cauchy, and every row under a latent prior scale (bnn_row_sums<true, true>), the Normal
// ones too: the prior scale is then b_r tau_(t, n), so T0 and T1 carry 1 / (b_r tau) inside the sum, and the row's prior scale entry holds
// b_r — log p = g(u) - log b_r - l with u = (w - mu0) / (b_r tau), d log p / d b_r = -(w - mu0) t / b_r - 1 / b_r: T2's identity with b_r in
// the place of s0, and -log b_r in the constant where -log s0 stands; the per-sample -l is the latent's (bnn_latent_terms)
__device__ __forceinline__ void bnn_row_terms_sums(const BParams& Q, const uint32_t r, const uint32_t kind, const float ds_lik, const float dmu_lik,
                                                   const float T0, const float T1, const float N, double& hconst, double& qconst,
                                                   const bool point = false) {
    const float mu = Q.rowp[r], s = Q.rowp[Q.R + r], mu0 = Q.rowp[2 * (size_t)Q.R + r], s0 = Q.rowp[3 * (size_t)Q.R + r];
    const float T2 = -((mu - mu0) * T0 + s * T1 + N) / s0;
    Q.rowg[r] = dmu_lik + Q.prior_weight * T0;
    Q.rowg[Q.R + r] = point ? 0.0f : ds_lik + Q.prior_weight * T1 + Q.entropy_weight * N / s;
    Q.rowg[2 * (size_t)Q.R + r] = -Q.prior_weight * T0;
    Q.rowg[3 * (size_t)Q.R + r] = Q.prior_weight * T2;
    // (double precision, for bnn_row_terms' reason)  Laplace: -log(2 s0); Cauchy: -log(pi) - log(s0); Normal: -log(s0) - 1/2 log 2 pi
    const double sd = bnn_uniform_value_d(Q, Q.row_uniform[Q.R + r]), s0d = bnn_uniform_value_d(Q, Q.row_uniform[3 * (size_t)Q.R + r]);
    const double pconst = kind == BSVI_DIST_LAPLACE ? -log(2.0 * s0d) : (kind == BSVI_DIST_CAUCHY ? -1.14472988584940017414 - log(s0d) : -log(s0d) - 0.91893853320467274178);
    hconst = (double)Q.prior_weight * pconst + (point ? 0.0 : (double)Q.entropy_weight * (1.41893853320467274178 + log(sd)));
    qconst = point ? 0.0 : -log(sd) - 0.91893853320467274178;
}

// per row quad (one wave, lanes = samples): sum_n eps G, sum_n G, sum_n eps, sum_n eps^2, then the rows' gradients and constants.  grid: ceil(quads / 4), block 256: a wave per quad
// (round 6: four quads per workgroup, as bnn_draw)
// MIXED: eight more accumulators, T0 and T1 of bnn_row_terms_sums for each of the four rows, from w and u recomputed as bnn_draw
// computed them on the eps redrawn here anyway — no pass over memory of their own, the same wave_sum order; a Normal row of such a model
// keeps its closed form.  MIXED = false is the kernel of the all-Normal models as it was.
// LATENT (with MIXED; bsvi_bnn_set_scale_latents): a row under a latent has the prior scale b_r tau_(t, n), another one per sample, so all
// three kinds take T0 and T1 with 1 / (b_r tau) inside the sum (the Normal: t = -u / s0) — the same eight accumulators, one load of
// 1 / tau per sample where the quad's rows share a latent (every quad inside a tensor), else one per row; rows under no latent keep
// what MIXED gives them.
// POINT (with MIXED; bsvi_bnn_set_point_rows): the normal of a point row is 0 as in bnn_draw, so w = mu in the sums of its prior's kind, and
// its row terms carry no entropy, no log s and no log q (bnn_row_terms / bnn_row_terms_sums, point); its scale gradient item is 0.
template <bool MIXED, bool LATENT = false, bool POINT = false>
__global__ void __launch_bounds__(256) bnn_row_sums(const BParams Q) {
    const uint32_t quads = (Q.R + 3u) / 4u, g = (POINT ? Q.quad0 : 0u) + blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u, r0 = 4u * g;
    if (g >= quads) return;
    float acc[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) acc[k] = 0.0f;
    float asum = 0.0f;
    float tacc[8], rp[4][4], is0[4];
    uint32_t kinds = 0u, lats = 0xFFFFFFFFu, points = 0u;
    if (POINT) points = *reinterpret_cast<const uint32_t*>(Q.row_point + (size_t)r0);
    if (LATENT) lats = *reinterpret_cast<const uint32_t*>(Q.row_latent + (size_t)r0);
    const bool lat_shared = LATENT && lats == (lats & 0xFFu) * 0x01010101u, lat_any = LATENT && lats != 0xFFFFFFFFu;
    if (MIXED) {
#pragma unroll
        for (int k = 0; k < 8; ++k) tacc[k] = 0.0f;
        kinds = *reinterpret_cast<const uint32_t*>(Q.row_kind + (size_t)r0);
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int j = 0; j < 4; ++j) rp[a][j] = (r0 + j < Q.R) ? Q.rowp[(size_t)a * Q.R + r0 + j] : 1.0f;
#pragma unroll
        for (int j = 0; j < 4; ++j) is0[j] = 1.0f / rp[3][j];          // (once per row: the loop below multiplies)
    }
    for (uint32_t n = lane; n < Q.n_local; n += 64u) {
        float e[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (!(POINT && points == 0x01010101u)) bnn_eps4(Q, n, g, e);      // (a quad of four point rows draws nothing)
        if (POINT) {
#pragma unroll
            for (int j = 0; j < 4; ++j) e[j] = ((points >> (8 * j)) & 0xFFu) ? 0.0f : e[j];
        }
        const float aw = Q.f_weight ? Q.f_weight[n] : 1.0f;      // (G carries a_n already: the seeds were scaled)
        asum += aw;
        float it[4] = {1.0f, 1.0f, 1.0f, 1.0f};      // LATENT: 1 / tau of the sample for the quad's rows (1 for a row under no latent)
        if (LATENT && lat_any) {
            if (lat_shared) {
                it[0] = it[1] = it[2] = it[3] = Q.lat_itau[(size_t)(lats & 0xFFu) * Q.n_pad + n];
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint32_t lt = (lats >> (8 * j)) & 0xFFu;
                    if (lt != 0xFFu) it[j] = Q.lat_itau[(size_t)lt * Q.n_pad + n];
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t r = r0 + j;
            float G = 0.0f;
            if (r < Q.R1) {
                const uint32_t h = r / Q.P, p = r - h * Q.P;
                const size_t nc = (size_t)h * Q.n_pad + n;
                G = Q.exact ? Q.GT[(size_t)p * Q.NC + nc] : Q.GT[nc * Q.P_ld + p];
            } else if (r < Q.R) {
                G = Q.gsm[(size_t)n * Q.Rs + (r - Q.R1)];
            }
            acc[j] += e[j] * G; acc[4 + j] += G; acc[8 + j] += aw * e[j]; acc[12 + j] += aw * (e[j] * e[j]);
            if (MIXED) {
                const uint32_t kind = (kinds >> (8 * j)) & 0xFFu;
                const float isn = LATENT ? is0[j] * it[j] : is0[j];
                const float w = rp[0][j] + rp[1][j] * e[j], dw = w - rp[2][j], u = dw * isn;
                // Laplace: t = -sign(u) / s0 (sign(0) = 0, as torch's abs backward);  Cauchy: t = -2 u / ((1 + u^2) s0)
                // (LATENT: s0 the sample's b_r tau, and a Normal row under a latent t = -u / s0: its closed form does not hold)
                const float sg = dw > 0.0f ? 1.0f : (dw < 0.0f ? -1.0f : 0.0f);
                const float tn = (LATENT && ((lats >> (8 * j)) & 0xFFu) != 0xFFu) ? -u : 0.0f;
                const float t = (kind == BSVI_DIST_LAPLACE ? -sg : (kind == BSVI_DIST_CAUCHY ? -2.0f * u / (1.0f + u * u) : tn)) * isn;
                tacc[j] += aw * t; tacc[4 + j] += aw * (e[j] * t);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 16; ++k) acc[k] = wave_sum(acc[k]);
    if (MIXED) {
#pragma unroll
        for (int k = 0; k < 8; ++k) tacc[k] = wave_sum(tacc[k]);
    }
    const float Nw = Q.f_weight ? wave_sum(asum) : (float)Q.n_local;
    if (lane < 16u) {
        const uint32_t q = lane >> 2, j = lane & 3u;
        if (r0 + j < Q.R) {
            float v = 0.0f;
#pragma unroll
            for (int k = 0; k < 16; ++k) v = (lane == (uint32_t)k) ? acc[k] : v;
            Q.sums[(size_t)q * Q.R + r0 + j] = v;
        }
    }
    // ... and, lanes 0 .. 3 a row each, what bnn_rows did in a launch of its own: the gradients with respect to the row's four uniform
    // entries (the formulas of dense_rows_body) and the sample-independent terms of f, the quad's four added in row order
    double hconst = 0.0, qconst = 0.0;
    const uint32_t r = r0 + lane;
    if (lane < 4u && r < Q.R) {
        float ds_lik = 0.0f, dmu_lik = 0.0f, S1 = 0.0f, S2 = 0.0f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            ds_lik = (lane == (uint32_t)j) ? acc[j] : ds_lik; dmu_lik = (lane == (uint32_t)j) ? acc[4 + j] : dmu_lik;
            S1 = (lane == (uint32_t)j) ? acc[8 + j] : S1; S2 = (lane == (uint32_t)j) ? acc[12 + j] : S2;
        }
        uint32_t kind = BSVI_DIST_NORMAL;
        float T0 = 0.0f, T1 = 0.0f;
        if (MIXED) {
#pragma unroll
            for (int j = 0; j < 4; ++j) { T0 = (lane == (uint32_t)j) ? tacc[j] : T0; T1 = (lane == (uint32_t)j) ? tacc[4 + j] : T1; }
            kind = (kinds >> (8u * lane)) & 0xFFu;
        }
        const bool under_latent = LATENT && ((lats >> (8u * lane)) & 0xFFu) != 0xFFu;
        const bool point = POINT && ((points >> (8u * lane)) & 0xFFu) != 0u;
        if (under_latent || (MIXED && kind != BSVI_DIST_NORMAL)) bnn_row_terms_sums(Q, r, kind, ds_lik, dmu_lik, T0, T1, Nw, hconst, qconst, point);
        else bnn_row_terms(Q, r, ds_lik, dmu_lik, S1, S2, Nw, hconst, qconst, point);
    }
    double h4 = 0.0, q4 = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) { h4 += __shfl(hconst, j, 64); q4 += __shfl(qconst, j, 64); }
    if (lane == 0u) { Q.hpart[g] = h4; Q.hpart[quads + g] = q4; }
}

// ---- the shared first layer (BParams::shared1): weights1 is a point estimate, the same matrix for every sample ------------------------
// x of the minibatch at (b, p): the exact pieces' operand (bf16, exact) or the f32 one
__device__ __forceinline__ float bnn_xb(const BParams& Q, const uint32_t b, const uint32_t p) {
    return Q.exact ? __uint_as_float((uint32_t)Q.Xb_bf[(size_t)b * Q.Kp + p] << 16) : Q.Xb[(size_t)b * Q.P_ld + p];
}

// a1s[h][b] = sum_p x[b][p] W1[h][p], W1 the q loc entries of weights1 (rowp's first R1 floats).  f32 FMAs on exact operands, the wave's
// partial sums joined by wave_sum: the rule of data_path() (exact bf16 data times an f32 weight, accumulated in f32) without the pieces.
// One wave per (minibatch row, row of W1), lanes along p; consecutive waves share the minibatch row.  (With a wave per minibatch row and
// the rows of W1 one after another, the launch was 74 us at 784-20-10 and 512 rows: 512 waves, each a chain of H1 dependent sums.)
// grid: ceil(B_pad H1 / 4), block 256
__global__ void __launch_bounds__(256) bnn_first_shared(const BParams Q) {
    const uint32_t lane = threadIdx.x & 63u, w = blockIdx.x * 4u + (threadIdx.x >> 6), b = w / Q.H1, h = w - b * Q.H1;
    if (b >= Q.B_pad) return;
    float s = 0.0f;
    if (b < Q.B) {
#pragma unroll 4
        for (uint32_t p = lane; p < Q.P; p += 64u) s = fmaf(bnn_xb(Q, b, p), Q.rowp[(size_t)h * Q.P + p], s);
    }
    s = wave_sum(s);
    if (lane == 0u) Q.a1s[(size_t)h * Q.B_pad + b] = s;      // (pad rows of the minibatch: 0, as a row of zeros gives)
}

// a1s laid out as the a1 the middle kernels read: MID — bnn_mid_gen's [(h, n)][b], else [B_pad][(h, n)]; the pad samples 0, as the
// product of their zero weights is.  One thread per four consecutive values (16-byte stores): grid: ceil(B_pad NC / 1024), block 256
template <bool MID>
__global__ void __launch_bounds__(256) bnn_first_broadcast(const BParams Q) {
    const size_t i = ((size_t)blockIdx.x * 256u + threadIdx.x) * 4u;
    if (i >= (size_t)Q.B_pad * Q.NC) return;
    xf_f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
    if (MID) {                                   // (B_pad is a multiple of 32: four consecutive b of one (h, n))
        const uint32_t hn = (uint32_t)(i / Q.B_pad), b = (uint32_t)(i - (size_t)hn * Q.B_pad), h = hn / Q.n_pad, n = hn - h * Q.n_pad;
        if (n < Q.n_local) v = *reinterpret_cast<const xf_f32x4*>(Q.a1s + (size_t)h * Q.B_pad + b);
    } else {                                     // (n_pad is a multiple of 64: four consecutive n of one (b, h))
        const uint32_t b = (uint32_t)(i / Q.NC), hn = (uint32_t)(i - (size_t)b * Q.NC), h = hn / Q.n_pad, n = hn - h * Q.n_pad;
        const float a = Q.a1s[(size_t)h * Q.B_pad + b];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = n + j < Q.n_local ? a : 0.0f;
    }
    *reinterpret_cast<xf_f32x4*>(Q.a1T + i) = v;
}

// d f / d a1 summed over 64 samples: dpart[seg][h][b] = sum_(n in 64 seg .. 64 seg + 63, n < n_local) da1[(h, n)][b], from the operand of
// the second product as the middle kernel left it — three bf16 pieces whose sum is the f32 value exactly, or f32.  [(h, n)][b] has b
// fastest: a lane takes four consecutive b (8-byte loads of each piece | one 16-byte load), wave w the samples 16 w .. 16 w + 15 of the
// segment one after another with all their loads in flight, and the four waves are joined in order: a fixed order of additions, no
// atomics.  grid: ceil(B_pad / 256) x H1 x n_pad / 64, block 256
__global__ void __launch_bounds__(256) bnn_da1_partial(const BParams Q) {
    __shared__ float part[4][64][4];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, b = (blockIdx.x * 64u + lane) * 4u, h = blockIdx.y, seg = blockIdx.z;
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (b < Q.B_pad) {
        const size_t plane = (size_t)Q.NC * Q.B_pad;
#pragma unroll
        for (uint32_t k = 0; k < 16u; ++k) {
            const uint32_t n = seg * 64u + wave * 16u + k;
            if (n >= Q.n_local) continue;
            const size_t at = ((size_t)h * Q.n_pad + n) * Q.B_pad + b;
            if (Q.exact) {
                const xf_u32x2 hi = *reinterpret_cast<const xf_u32x2*>(Q.dlogp + at), mid = *reinterpret_cast<const xf_u32x2*>(Q.dlogp + plane + at),
                               lo = *reinterpret_cast<const xf_u32x2*>(Q.dlogp + 2 * plane + at);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint32_t sh = (j & 1) ? 0u : 16u, w = (uint32_t)j >> 1;      // (element j: the low half of word j / 2 first)
                    const float v = (__uint_as_float((hi[w] << sh) & 0xFFFF0000u) + __uint_as_float((mid[w] << sh) & 0xFFFF0000u))
                                    + __uint_as_float((lo[w] << sh) & 0xFFFF0000u);
                    acc[j] += v;
                }
            } else {
                const xf_f32x4 v = *reinterpret_cast<const xf_f32x4*>(Q.da1T + at);
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] += v[j];
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) part[wave][lane][j] = acc[j];
    __syncthreads();
    if (wave == 0u && b < Q.B_pad) {
        xf_f32x4 v;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (part[0][lane][j] + part[1][lane][j]) + (part[2][lane][j] + part[3][lane][j]);
        *reinterpret_cast<xf_f32x4*>(Q.dpart + ((size_t)seg * Q.H1 + h) * Q.B_pad + b) = v;
    }
}

// ... and the segments in order: dbar[h][b].  grid: ceil(H1 B_pad / 256), block 256
__global__ void __launch_bounds__(256) bnn_da1_total(const BParams Q) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x, n_hb = Q.H1 * Q.B_pad;
    if (i >= n_hb) return;
    float s = 0.0f;
    for (uint32_t seg = 0; seg < Q.n_pad / 64u; ++seg) s += Q.dpart[(size_t)seg * n_hb + i];
    Q.dbar[i] = s;
}

// GT1[h][p] = sum_b dbar[h][b] x[b][p]: sum_n of the per-sample second product, taken after the sum over the samples.  Lanes along p, the
// sixteen waves of a workgroup take a slice of the minibatch each and are joined in order.  grid: ceil(P / 64) x H1, block 1024
__global__ void __launch_bounds__(1024) bnn_second_shared(const BParams Q) {
    __shared__ float part[16][64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, p = blockIdx.x * 64u + lane, h = blockIdx.y;
    const uint32_t per = (Q.B + 15u) / 16u, b0 = wave * per, b1 = min(b0 + per, Q.B);
    float s = 0.0f;
    if (p < Q.P) {
#pragma unroll 8
        for (uint32_t b = b0; b < b1; ++b) s = fmaf(Q.dbar[(size_t)h * Q.B_pad + b], bnn_xb(Q, b, p), s);
    }
    part[wave][lane] = s;
    __syncthreads();
    if (wave == 0u && p < Q.P) {
        float t = 0.0f;
#pragma unroll
        for (int w = 0; w < 16; ++w) t += part[w][lane];
        Q.GT1[(size_t)h * Q.P + p] = t;
    }
}

// the row terms of weights1 from GT1: what bnn_row_sums leaves for a quad of point rows, without a loop over the samples — sum_n G is
// GT1, every sum with eps is 0, and the prior's per-sample t is the same for every sample (T0 = N t, T1 = 0).  One thread per row of
// weights1; the constants of a quad's four rows (P is a multiple of 4: four lanes of one wave) are added in row order.
// grid: ceil(R1 / 256), block 256
__global__ void __launch_bounds__(256) bnn_rows_shared(const BParams Q) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u, quads = (Q.R + 3u) / 4u;
    double hconst = 0.0, qconst = 0.0;
    if (r < Q.R1) {
        float Nw = (float)Q.n_local;
        if (Q.f_weight) {
            Nw = 0.0f;
            for (uint32_t n = 0; n < Q.n_local; ++n) Nw += Q.f_weight[n];
        }
        const uint32_t kind = Q.row_kind[r];
        const float G = Q.GT1[r];
        if (kind != BSVI_DIST_NORMAL) {
            const float is0 = 1.0f / Q.rowp[3 * (size_t)Q.R + r], dw = Q.rowp[r] - Q.rowp[2 * (size_t)Q.R + r], u = dw * is0;
            const float sg = dw > 0.0f ? 1.0f : (dw < 0.0f ? -1.0f : 0.0f);
            const float t = (kind == BSVI_DIST_LAPLACE ? -sg : -2.0f * u / (1.0f + u * u)) * is0;
            bnn_row_terms_sums(Q, r, kind, 0.0f, G, Nw * t, 0.0f, Nw, hconst, qconst, true);
        } else {
            bnn_row_terms(Q, r, 0.0f, G, 0.0f, 0.0f, Nw, hconst, qconst, true);
        }
        Q.sums[r] = 0.0f; Q.sums[(size_t)Q.R + r] = G; Q.sums[2 * (size_t)Q.R + r] = 0.0f; Q.sums[3 * (size_t)Q.R + r] = 0.0f;
    }
    double h4 = 0.0, q4 = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) { h4 += __shfl(hconst, (int)(lane & ~3u) + j, 64); q4 += __shfl(qconst, (int)(lane & ~3u) + j, 64); }
    if ((lane & 3u) == 0u && r < Q.R1) { Q.hpart[r / 4u] = h4; Q.hpart[quads + r / 4u] = q4; }
}

// latent prior scales, one thread per sample: the chunks' sums of u psi - 1 in chunk order, then per latent, with z = (l - m0) / s0,
//     D = d f_n / d l = prior_weight (sum_(r under t) (u psi - 1) - 1 - z / s0)
// and the latents' per-sample parts of f and log q (their constants are bnn_epilogue's, in double precision):
//     f_n += prior_weight sum_t (-(K_t + 1) l - 1/2 z^2),      log q_n += sum_t (-l - 1/2 eps^2)
// (K_t l in double precision: K_t is the number of rows of a tensor).  grid: ceil(n_pad / 256), block 256
__global__ void __launch_bounds__(256) bnn_latent_terms(const BParams Q) {
    const uint32_t n = blockIdx.x * 256u + threadIdx.x, T = Q.n_latents;
    if (n >= Q.n_pad) return;
    const bool live = n < Q.n_local;
    double fl = 0.0, ql = 0.0;
    for (uint32_t t = 0; t < T; ++t) {
        float U = 0.0f;
        const float* __restrict__ const up = Q.lat_upart + (size_t)t * Q.n_pad + n;
#pragma unroll 8
        for (uint32_t ch = 0; ch < Q.row_chunks; ++ch) U += up[(size_t)ch * T * Q.n_pad];
        const size_t at = (size_t)t * Q.n_pad + n;
        const float l = Q.lat_l[at], e = Q.lat_eps[at];
        const float m0 = bnn_uniform_value(Q, Q.lat_uniform[2u * T + t]), s0 = bnn_uniform_value(Q, Q.lat_uniform[3u * T + t]);
        const float z = (l - m0) / s0;
        Q.lat_D[at] = live ? Q.prior_weight * (U - 1.0f - z / s0) : 0.0f;
        Q.lat_z[at] = live ? z : 0.0f;
        fl += (double)Q.prior_weight * (-((double)Q.lat_count[t] + 1.0) * (double)l - 0.5 * (double)z * (double)z);
        ql += -(double)l - 0.5 * (double)e * (double)e;
    }
    Q.lat_f[n] = live ? fl : 0.0; Q.lat_q[n] = live ? ql : 0.0;
}

// one workgroup: per-sample f (and log q), the value of the estimator, its sum; all in a fixed order
__global__ void __launch_bounds__(1024) bnn_epilogue(const BParams Q, uint32_t row_blocks) {
    __shared__ double dred[16];
    const uint32_t tid = threadIdx.x;
    // fixed-order sum over the workgroup, in double precision (see bnn_row_terms): a butterfly inside each wave, then the sixteen waves in
    // order — two barriers (as a tree over 1 024 LDS cells with a barrier per level, the five sums of this launch were 16 us of it)
    auto total = [&](double v) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        __syncthreads();
        if ((tid & 63u) == 0u) dred[tid >> 6] = v;
        __syncthreads();
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < 16; ++w) t += dred[w];
        return t;
    };
    double hc = 0.0, qc = 0.0;
    for (uint32_t i = tid; i < row_blocks; i += 1024u) { hc += Q.hpart[i]; qc += Q.hpart[row_blocks + i]; }
    double htot = total(hc), qtot = total(qc);
    const bool blackbox = Q.estimator == BSVI_EST_BLACKBOX;
    // latent prior scales: the sample-independent terms of their log p, entropy (a LogNormal's, analytic) and log q, in latent order and in
    // double precision as the rows' (every thread the same sums)
    for (uint32_t t = 0; t < Q.n_latents; ++t) {
        const uint32_t T = Q.n_latents;
        const double md = bnn_uniform_value_d(Q, Q.lat_uniform[t]), sd = bnn_uniform_value_d(Q, Q.lat_uniform[T + t]);
        const double s0d = bnn_uniform_value_d(Q, Q.lat_uniform[3u * T + t]);
        htot += (double)Q.prior_weight * (-log(s0d) - 0.91893853320467274178) + (double)Q.entropy_weight * (md + 1.41893853320467274178 + log(sd));
        qtot += -log(sd) - 0.91893853320467274178;
    }
    double fsum = 0.0, vsum = 0.0, bad = 0.0;
    for (uint32_t n = tid; n < Q.n_local; n += 1024u) {
        if (Q.q_weight) fsum += (double)Q.q_weight[n];            // (caller weights of grad log q_n in place of f_n: bnn_uniform_grads reads their sum)
        double pv = 0.0, qv = 0.0;
        // (the chunks' partials in chunk order; unrolled so that eight chunks' loads are in flight: one at a time the 62 chunks of the
        //  784-20-10 network are 62 dependent round trips in this ONE workgroup)
        const float* __restrict__ const pvp = Q.pv_part + n;
        const float* __restrict__ const qvp = Q.qv_part + n;
#pragma unroll 8
        for (uint32_t ch = 0; ch < Q.row_chunks; ++ch) { pv += (double)pvp[(size_t)ch * Q.n_pad]; qv += (double)qvp[(size_t)ch * Q.n_pad]; }
        double f = htot + (double)Q.lik[n] + (double)Q.prior_weight * pv;
        if (Q.n_latents) { f += Q.lat_f[n]; qv += Q.lat_q[n]; Q.lat_b[n] = Q.q_weight ? (double)Q.q_weight[n] : f; }
        if (Q.fvalue_out) Q.fvalue_out[n] = (float)f;
        double value = f;
        if (blackbox) {
            const double lq = qtot + qv;
            if (Q.logq_out) Q.logq_out[n] = (float)lq;
            value = lq * f + f;
        }
        if (!Q.q_weight) fsum += f;
        vsum += value; bad += isfinite((float)value) ? 0.0 : 1.0;
    }
    const double fs = total(fsum), vs = total(vsum), bs = total(bad);
    if (tid == 0) { Q.partial[0] = (float)vs; Q.partial[1] = (float)bs; Q.fs[0] = (float)fs; }
    if (Q.scale_learn) {      // a learnable sigma: G_c = sum_n of the per-sample sums, in the same fixed order
        for (uint32_t c = 0; c < Q.C; ++c) {
            double g = 0.0;
            for (uint32_t n = tid; n < Q.n_local; n += 1024u) g += (double)Q.gsig[(size_t)c * Q.n_pad + n];
            const double gt = total(g);
            if (tid == 0) Q.gsd[c] = gt;
        }
    }
}

// latent prior scales: the four gradients of every latent, sums over n in a fixed order and double precision, into the items behind the
// rows' in rowg (bnn_uniform_grads adds them to their entries as it adds a row's):
//     m_t   sum a D + ew sum a  [- sum b]                            s_t   sum a D eps + ew sum a / s_t  [- sum b (eps + 1 / s_t)]
//     m0_t  pw sum a z / s0                                          s0_t  pw (sum a z^2 - sum a) / s0
// (a_n the caller's weights or 1; in brackets the BlackBox score term, b_n = f_n or the caller's as bnn_epilogue left them in lat_b, and
//  sum b in fs: d log q_n / d m_t = -1, d log q_n / d s_t = -eps - 1 / s_t).  grid: T, block 256: a workgroup per latent
__global__ void __launch_bounds__(256) bnn_latent_grads(const BParams Q) {
    __shared__ double dred[4];
    const uint32_t tid = threadIdx.x, t = blockIdx.x, T = Q.n_latents;
    auto total = [&](double v) {      // (bnn_epilogue's: a butterfly inside each wave, then the waves in order)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        __syncthreads();
        if ((tid & 63u) == 0u) dred[tid >> 6] = v;
        __syncthreads();
        return (dred[0] + dred[1]) + (dred[2] + dred[3]);
    };
    const bool blackbox = Q.estimator == BSVI_EST_BLACKBOX;
    double as = 0.0, d0 = 0.0, d1 = 0.0, z1 = 0.0, z2 = 0.0, be = 0.0;
    for (uint32_t n = tid; n < Q.n_local; n += 256u) {
        const size_t at = (size_t)t * Q.n_pad + n;
        const double a = Q.f_weight ? (double)Q.f_weight[n] : 1.0, D = (double)Q.lat_D[at], e = (double)Q.lat_eps[at], z = (double)Q.lat_z[at];
        as += a; d0 += a * D; d1 += a * D * e; z1 += a * z; z2 += a * z * z;
        if (blackbox) be += Q.lat_b[n] * e;
    }
    const double asum = total(as), D0 = total(d0), D1 = total(d1), Z1 = total(z1), Z2 = total(z2), BE = total(be);
    if (tid == 0) {
        const double sd = bnn_uniform_value_d(Q, Q.lat_uniform[T + t]), s0d = bnn_uniform_value_d(Q, Q.lat_uniform[3u * T + t]);
        const double ew = (double)Q.entropy_weight, pw = (double)Q.prior_weight, fs = blackbox ? (double)Q.fs[0] : 0.0;
        float* const g = Q.rowg + 4 * (size_t)Q.R;
        g[t] = (float)(D0 + ew * asum - fs);
        g[T + t] = (float)(D1 + ew * asum / sd - (blackbox ? BE + fs / sd : 0.0));
        g[2u * T + t] = (float)(pw * Z1 / s0d);
        g[3u * T + t] = (float)(pw * (Z2 - asum) / s0d);
    }
}

// one thread per uniform entry with a gradient: its rows' contributions in item order.  BlackBox (gradient_estimators.py:29-36
// with the weights kept reparameterised, variables.py:567): d log q_n / d s_r = -1 / s_r for every sample, so the score term
// adds -(sum_n f_n) / s_r to the scale gradient of row r.  grid: ceil(n_uniform_grad / 256)
__global__ void __launch_bounds__(256) bnn_uniform_grads(const BParams Q) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= Q.n_uniform_grad) return;
    const float fs = Q.fs[0];
    const bool blackbox = Q.estimator == BSVI_EST_BLACKBOX;
    float s = 0.0f;
    for (uint32_t it = Q.ur_ptr[k]; it < Q.ur_ptr[k + 1]; ++it) {
        const uint32_t item = Q.ur_item[it], role = item / Q.R, r = item - role * Q.R;
        s += Q.rowg[item];
        if (blackbox && role == 1u) s += -fs / Q.rowp[Q.R + r];
    }
    if (Q.scale_learn) {      // sigma's entries: output c adds G_c to entry scale_u + c * scale_stride (stride 0: the sum over c), to what
        double g = 0.0;       // the entry's rows gave above — one root may be a prior scale and sigma
        for (uint32_t c = 0; c < Q.C; ++c)
            if (Q.scale_u + c * Q.scale_stride == k) g += Q.gsd[c];
        s += (float)g;
    }
    Q.partial[2 + k] = s;
}

// ---- host side -------------------------------------------------------------------------------------------------------------
// a generated kernel of a handle; state: 0 not tried, 1 ready, -1 declined / failed (what stands behind it serves)
struct BnnGen { int state = 0; hipModule_t module = nullptr; hipFunction_t fn = nullptr; };

struct bsvi_bnn {
    bsvi_bnn_desc d;
    std::vector<bsvi_bnn_layer> layers;
    void* dev_blob = nullptr;
    const bsvi_uniform_entry* uniform = nullptr; const float* consts = nullptr;
    const uint32_t* pu_ptr = nullptr; const uint32_t* pu_idx = nullptr; const uint32_t* row_uniform = nullptr;
    const uint32_t* ur_ptr = nullptr; const uint32_t* ur_item = nullptr;
    const float* dataset = nullptr; const float* labels = nullptr;
    uint32_t R = 0, R1 = 0, Rs = 0, P = 0, C = 0, H1 = 0, B_pad = 0, Kp = 0, P_ld = 0;
    uint32_t LC = 1;             // targets per dataset row: one label, or C for the Normal likelihood
    uint32_t scale_u = 0, scale_stride = 0;      // Normal likelihood: sigma of output c is uniform entry scale_u + c * scale_stride
    bool scale_learn = false;    // ... parameter entries (bsvi_bnn_create_normal_learnable), else constants
    uint32_t heads = 0;          // a scale head (bsvi_bnn_create_normal_heads): its BSVI_UT_* transform; the last layer has 2 C rows
    float head_a = 0.0f, head_b = 1.0f;
    uint32_t family = BSVI_DIST_NORMAL;      // the loc-scale likelihood's family (bsvi_bnn_set_likelihood_family): Normal, Laplace or Cauchy
    uint8_t* row_kind = nullptr; // the prior of every row, in the blob (all Normal until bsvi_bnn_set_row_priors)
    bool mixed = false;          // some row is Laplace or Cauchy: the MIXED instantiations of bnn_draw / bnn_row_sums
    // latent prior scales (bsvi_bnn_set_scale_latents; 0: none): their tables and the entry -> item lists extended by their items, in a
    // blob of their own; the LATENT instantiations of bnn_draw / bnn_row_sums, bnn_latent_terms and the workspace behind everything else
    uint32_t n_latents = 0;
    void* lat_blob = nullptr;
    const uint8_t* row_latent = nullptr; const uint32_t* lat_uniform = nullptr; const uint32_t* lat_count = nullptr;
    std::vector<uint32_t> row_uniform_host;      // [4][R], kept for that call
    // point-estimated rows (bsvi_bnn_set_point_rows; null: none): a byte per row in a blob of its own; the POINT instantiations of
    // bnn_draw / bnn_row_sums
    uint8_t* row_point = nullptr;
    std::vector<uint8_t> row_point_host;
    // the shared first layer (bnn_select.h, shared_first): 0 not asked yet, 1 shared, -1 both products per sample.  Decided once, from
    // the point rows and BSVI_BNN_SHARED1 as they stand when the workspace is sized or the first launch is made (bnn_shared_first)
    mutable std::atomic<int> shared_state{0};
    // the parameters of the layers' activations: torch's defaults (bnn_create) until bsvi_bnn_set_activation_params
    float act_p[BNN_MAX_LAYERS][2] = {};
    mutable std::atomic<bool> launched{false};      // a launch was made: the priors stay as they are
    uint64_t act_floats = 0, delta_floats = 0;      // per (sample, minibatch row)
    uint32_t act_off[BNN_MAX_LAYERS] = {};
    bool exact = false;
    bool upper_lds = false;      // the small tensors of 64 samples fit LDS ([Rs][65] floats): bnn_upper<true>
    // the two kernels written for THIS network (round 5; their text: bnn_source.h), compiled with hiprtc at the first launch:
    // bnn_upper specialised, and the exact-data path's middle as one kernel (bnn_gen_ready)
    mutable std::mutex jit_mu;
    mutable BnnGen upper_gen, mid_gen;
    uint32_t n_cu = 256;
};

// what bnn_upper_gen reads of an iteration (bnn_source.h's upper_source declares the same struct)
struct BnnUpperArgs {
    const float* Wsm; const float* a1T; const float* lab; float* acts; float* deltas; float* liknb; float* da1T; uint16_t* dlogp;
    uint32_t n_local, n_pad, B, B_pad, NC, rows_per_wave, exact;
    float lik_weight;
    const float* f_weight;      // a_n per sample, or null
};
// ... of a network with a learnable sigma: the same fields, then where its terms go (the generated struct gains the same last member)
struct BnnUpperArgsSig { BnnUpperArgs a; float* sigt; };

// ... and of bnn_mid_gen (bnn_source.h's mid_source declares the same struct; a learnable sigma: its per-sample sums [C][n_pad])
struct BnnMidArgs {
    const float* Wsm; const float* a1; const float* lab; float* gsm; float* lik; uint16_t* dlogp;
    uint32_t n_local, n_pad, B, B_pad, NC;
    float lik_weight;
    const float* f_weight;      // a_n per sample, or null
};
struct BnnMidArgsSig { BnnMidArgs a; float* gsig; };

// the network as bnn_source.h reads it
static_assert(bsvi_bnn_source::MAX_LAYERS == BNN_MAX_LAYERS, "bnn_source.h holds as many layers as bnn_create admits");
static bsvi_bnn_source::Net bnn_source_net(const bsvi_bnn* p) {
    bsvi_bnn_source::Net N;
    N.n_layers = p->d.n_layers;
    for (uint32_t l = 0; l < N.n_layers; ++l) { N.layer[l] = p->layers[l]; N.act_off[l] = p->act_off[l]; }
    N.R1 = p->R1; N.Rs = p->Rs; N.act_floats = (uint32_t)p->act_floats; N.C = p->C; N.B_pad = p->B_pad;
    N.likelihood = p->d.likelihood; N.family = p->family; N.scale_learn = p->scale_learn; N.heads = p->heads;
    memcpy(&N.head_a_bits, &p->head_a, 4); memcpy(&N.head_b_bits, &p->head_b, 4);
    N.act_params_set = true;
    memcpy(N.act_p, p->act_p, sizeof N.act_p);
    const char* e = getenv("BSVI_BNN_CAUCHY_LOG");
    N.cauchy_log1p = e && !strcmp(e, "log1p");
    return N;
}

// does weights1 take the shared first layer?  (the switch is read where BSVI_BNN_MID is: at the first question, and kept)
static bool bnn_shared_first(const bsvi_bnn* p) {
    int st = p->shared_state.load();
    if (!st) {
        const char* e = getenv("BSVI_BNN_SHARED1");
        st = bsvi_bnn_select::shared_first(p->row_point ? p->row_point_host.data() : nullptr, p->R1, e && e[0] == '0') ? 1 : -1;
        p->shared_state.store(st);
    }
    return st > 0;
}

static size_t bnn_mid_lds_bytes(const bsvi_bnn* p) { return bsvi_bnn_select::mid_lds_bytes(p->Rs, p->act_floats, p->B_pad); }
// the middle kernel of this network under the given switches (bnn_select.h: sizes only — a failed compile is handled where it is tried)
static bsvi_bnn_select::BnnMiddle bnn_middle_for(const bsvi_bnn* p, bool mid_off, bool jit_off) {
    bsvi_bnn_select::Switches sw;
    sw.mid_off = mid_off; sw.jit_off = jit_off;
    return bsvi_bnn_select::middle(p->Rs, p->act_floats, p->B_pad, p->exact, sw);
}
// a generated kernel (mid: bnn_mid_gen, else bnn_upper_gen, asked once bnn_mid_gen does not serve), compiled on first use.  false: what
// stands behind it serves — the separate launches for bnn_mid_gen (BSVI_BNN_MID=0, data that is not exactly bf16, a tile beyond LDS),
// the static bnn_upper for bnn_upper_gen (BSVI_BNN_JIT=0, small tensors beyond the register file), and for either a failed compile
static bool bnn_gen_ready(const bsvi_bnn* p, const bool mid) {
    std::lock_guard<std::mutex> lock(p->jit_mu);
    BnnGen& g = mid ? p->mid_gen : p->upper_gen;
    if (g.state) return g.state > 0;
    g.state = -1;
    const char* e = getenv(mid ? "BSVI_BNN_MID" : "BSVI_BNN_JIT");
    const bool off = e && e[0] == '0';
    if (bnn_middle_for(p, mid ? off : true, mid ? false : off) != (mid ? bsvi_bnn_select::MID_GEN : bsvi_bnn_select::UPPER_GEN)) return false;
    const bsvi_bnn_source::Net net = bnn_source_net(p);
    const std::string src = mid ? bsvi_bnn_source::mid_source(net) : bsvi_bnn_source::upper_source(net);
    if (const char* dump = getenv("BSVI_BNN_SOURCE_DUMP")) {      // tools: the generated translation unit
        if (FILE* f = fopen((std::string(dump) + (mid ? ".mid" : "")).c_str(), "w")) { fputs(src.c_str(), f); fclose(f); }
    }
    std::vector<char> code;
    std::string log;
    if (bsvi_spec::obtain(src, code, log, nullptr)) {
        if (getenv("BSVI_DEBUG")) fprintf(stderr, "bsvi: the generated %s did not compile:\n%s\n", mid ? "bnn_mid" : "bnn_upper", log.c_str());
        return false;
    }
    const size_t lds = mid ? bnn_mid_lds_bytes(p) : bsvi_bnn_select::upper_gen_lds_bytes(p->Rs);
    hipError_t err = hipModuleLoadData(&g.module, code.data());
    if (err == hipSuccess) err = hipModuleGetFunction(&g.fn, g.module, mid ? "bnn_mid_gen" : "bnn_upper_gen");
    if (err == hipSuccess) err = hipFuncSetAttribute((const void*)g.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (err != hipSuccess) { (void)hipGetLastError(); g.fn = nullptr; return false; }
    g.state = 1;
    return true;
}


// the three entry points' common body; normal: bsvi_bnn_create_normal (the scale entries are its plain arguments: constants), learn:
// bsvi_bnn_create_normal_learnable (parameter entries)
// heads: bsvi_bnn_create_normal_heads (no scale entries: sigma is a transform of the last layer's second half)
struct BnnHeads { uint32_t transform; float a, b; };
static int bnn_create(const bsvi_bnn_desc* desc, const bool normal, const uint32_t scale_uniform, const uint32_t scale_stride, bsvi_bnn** out,
                      const bool learn = false, const BnnHeads* heads = nullptr) {
    if (!desc || !out) return fail(BSVI_ERR_INVALID, "null argument");
    *out = nullptr;
    BSVI_CHECK_STRUCT(desc, bsvi_bnn_desc);
    if (desc->abi_version != BSVI_ABI_VERSION) return fail(BSVI_ERR_INVALID, "ABI version mismatch");
    if (!desc->layers || !desc->n_layers || desc->n_layers > BNN_MAX_LAYERS) return fail(BSVI_ERR_INVALID, "1 .. 8 layers");
    if (!desc->n_features || !desc->batch_size || desc->batch_size > desc->dataset_size || !desc->n_rows) return fail(BSVI_ERR_INVALID, "bad shape");
    if (desc->n_features % 4) return fail(BSVI_ERR_UNSUPPORTED, "the number of features must be a multiple of 4 (the noise is drawn in quads of rows)");
    if (!normal && desc->likelihood == BSVI_LIK_NORMAL)
        return fail(BSVI_ERR_UNSUPPORTED, "the Normal likelihood needs its scale entries: create the model with bsvi_bnn_create_normal");
    if (normal && desc->likelihood != BSVI_LIK_NORMAL)
        return fail(BSVI_ERR_INVALID, heads ? "bsvi_bnn_create_normal_heads takes likelihood BSVI_LIK_NORMAL"
                                      : learn ? "bsvi_bnn_create_normal_learnable takes likelihood BSVI_LIK_NORMAL" : "bsvi_bnn_create_normal takes likelihood BSVI_LIK_NORMAL");
    if (desc->likelihood > BSVI_LIK_NORMAL) return fail(BSVI_ERR_UNSUPPORTED, "unknown likelihood");
    if (desc->estimator > BSVI_EST_BLACKBOX) return fail(BSVI_ERR_INVALID, "unknown estimator");
    for (uint32_t k = 0; k < desc->n_uniform; ++k) {
        const bsvi_uniform_entry& e = desc->uniform[k];
        if (e.transform > BSVI_UT_SQUARE || (k < desc->n_uniform_grad) != (e.is_param != 0) || e.src >= (e.is_param ? desc->n_params : desc->n_consts))
            return fail(BSVI_ERR_INVALID, "bad uniform table");
    }
    const uint32_t R = desc->n_rows;
    for (size_t i = 0; i < 4 * (size_t)R; ++i) if (desc->row_uniform[i] >= desc->n_uniform) return fail(BSVI_ERR_INVALID, "row parameter out of the uniform table");
    // the chain: layer 0 is [H1 x P] over the data and owns rows [0, H1 P); every other tensor lies behind it, inside [0, R)
    uint32_t width = desc->n_features;
    for (uint32_t l = 0; l < desc->n_layers; ++l) {
        const bsvi_bnn_layer& L = desc->layers[l];
        if (!L.rows || L.cols != width) return fail(BSVI_ERR_INVALID, "layer shapes do not chain");
        if (L.activation > BSVI_BNN_ACT_GELU) return fail(BSVI_ERR_UNSUPPORTED, "unknown activation");
        if ((uint64_t)L.weight_row0 + (uint64_t)L.rows * L.cols > R || (L.bias_row0 != 0xFFFFFFFFu && (uint64_t)L.bias_row0 + L.rows > R))
            return fail(BSVI_ERR_INVALID, "layer rows out of range");
        if (l == 0 && L.weight_row0 != 0) return fail(BSVI_ERR_INVALID, "the first layer's weights are rows [0, H1 P)");
        if (l > 0 && L.weight_row0 < desc->layers[0].rows * desc->n_features) return fail(BSVI_ERR_INVALID, "upper tensors lie behind weights1");
        if (L.bias_row0 != 0xFFFFFFFFu && L.bias_row0 < desc->layers[0].rows * desc->n_features) return fail(BSVI_ERR_INVALID, "biases lie behind weights1");
        width = L.rows;
    }
    if (desc->layers[desc->n_layers - 1].activation != BSVI_BNN_ACT_NONE) return fail(BSVI_ERR_INVALID, "the last layer yields the logits");
    if (desc->likelihood == BSVI_LIK_BERNOULLI && width != 1) return fail(BSVI_ERR_INVALID, "Bernoulli likelihood needs one output");
    if (heads) {
        if (heads->transform != BSVI_UT_SOFTPLUS && heads->transform != BSVI_UT_EXP && heads->transform != BSVI_UT_SIGMOID)
            return fail(BSVI_ERR_UNSUPPORTED, "bsvi_bnn_create_normal_heads: the transform of the scale head is softplus, exp or sigmoid");
        if (!std::isfinite(heads->a) || !std::isfinite(heads->b) || heads->a < 0.0f || !(heads->b > 0.0f))
            return fail(BSVI_ERR_INVALID, "bsvi_bnn_create_normal_heads: sigma = a + b g(raw) needs finite a >= 0 and b > 0");
        if (width % 2u)
            return fail(BSVI_ERR_INVALID, "bsvi_bnn_create_normal_heads: the last layer has an odd number of rows (C rows of the loc, then C of the raw scale)");
    } else if (normal) {
        // sigma of output c: entry scale_uniform + c * scale_stride, every one of them a constant of the model
        if (scale_stride > 1u) return fail(BSVI_ERR_INVALID, "scale_stride is 0 (one scale for every output) or 1 (one per output)");
        const uint64_t last = (uint64_t)scale_uniform + (uint64_t)scale_stride * (width - 1u);
        if (last >= desc->n_uniform) return fail(BSVI_ERR_INVALID, "scale entry out of the uniform table");
        if (!learn && scale_uniform < desc->n_uniform_grad)
            return fail(BSVI_ERR_UNSUPPORTED, "the scale of the Normal likelihood must be a constant of the model: a learnable scale is not implemented");
        if (learn) {
            // ... every one of them a parameter's, behind a transform that keeps sigma off zero whatever a step does to the parameter
            uint32_t n_param = 0;
            for (uint32_t c = 0; c < width; ++c) n_param += scale_uniform + c * scale_stride < desc->n_uniform_grad ? 1u : 0u;
            if (!n_param)
                return fail(BSVI_ERR_INVALID, "bsvi_bnn_create_normal_learnable: the scale entries are constants (a constant scale: bsvi_bnn_create_normal)");
            if (n_param != width) return fail(BSVI_ERR_INVALID, "bsvi_bnn_create_normal_learnable: the scale entries are a mix of constants and parameters");
            for (uint32_t c = 0; c < width; ++c) {
                const uint32_t t = desc->uniform[scale_uniform + c * scale_stride].transform;
                if (t != BSVI_UT_SOFTPLUS && t != BSVI_UT_EXP && t != BSVI_UT_SIGMOID)
                    return fail(BSVI_ERR_UNSUPPORTED, "bsvi_bnn_create_normal_learnable: the transform of a learnable scale is softplus, exp or sigmoid");
            }
        }
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(BSVI_ERR_NO_DEVICE, "no HIP device visible");
    bsvi_bnn* p = new bsvi_bnn();
    p->d = *desc;
    p->layers.assign(desc->layers, desc->layers + desc->n_layers);
    p->d.layers = nullptr;
    p->row_uniform_host.assign(desc->row_uniform, desc->row_uniform + 4 * (size_t)R);
    p->R = R; p->P = desc->n_features; p->C = width; p->H1 = desc->layers[0].rows;
    p->R1 = p->H1 * p->P; p->Rs = R - p->R1;
    p->Kp = (p->P + 31) / 32 * 32; p->P_ld = (p->P + 3) / 4 * 4;
    p->B_pad = (desc->batch_size + 31) / 32 * 32;
    if (normal) { p->LC = width; p->scale_u = scale_uniform; p->scale_stride = scale_stride; p->scale_learn = learn; }
    if (heads) { p->C = p->LC = width / 2u; p->heads = heads->transform; p->head_a = heads->a; p->head_b = heads->b; }
    for (uint32_t l = 0; l < desc->n_layers; ++l) { p->act_off[l] = (uint32_t)p->act_floats; p->act_floats += p->layers[l].rows; }
    for (uint32_t l = 0; l < desc->n_layers; ++l) bsvi_bnn_source::act_default(p->layers[l].activation, p->act_p[l]);
    p->delta_floats = p->act_floats;
    {   // exact data: both products on the bf16 matrix cores (three MFMAs on the exact pieces of the other operand); BSVI_DENSE_XGEMM=0: f32
        const char* xe = getenv("BSVI_DENSE_XGEMM");
        bool exact = !(xe && xe[0] == '0');
        const uint32_t* bits = reinterpret_cast<const uint32_t*>(desc->dataset);
        const size_t n_values = (size_t)desc->dataset_size * desc->n_features;
        for (size_t i = 0; exact && i < n_values; ++i) exact = (bits[i] & 0xFFFFu) == 0u;
        p->exact = exact;
    }
    // uniform entry -> rows that read it (role-major item = role * R + row), in row order: a fixed order of additions
    std::vector<uint32_t> ur_ptr(desc->n_uniform_grad + 1, 0u), ur_item;
    {
        std::vector<uint32_t> count(desc->n_uniform_grad, 0u);
        for (size_t i = 0; i < 4 * (size_t)R; ++i) if (desc->row_uniform[i] < desc->n_uniform_grad) ++count[desc->row_uniform[i]];
        for (uint32_t k = 0; k < desc->n_uniform_grad; ++k) ur_ptr[k + 1] = ur_ptr[k] + count[k];
        ur_item.resize(ur_ptr[desc->n_uniform_grad]);
        std::vector<uint32_t> at(ur_ptr.begin(), ur_ptr.end() - 1);
        for (size_t i = 0; i < 4 * (size_t)R; ++i) if (desc->row_uniform[i] < desc->n_uniform_grad) ur_item[at[desc->row_uniform[i]]++] = (uint32_t)i;
    }
    // (the rows' prior kinds, a byte each padded to a whole quad, behind everything else: all Normal until bsvi_bnn_set_row_priors)
    const std::vector<uint8_t> kinds(((size_t)R + 3) / 4 * 4, (uint8_t)BSVI_DIST_NORMAL);
    const size_t sizes[10] = {(size_t)desc->n_uniform * sizeof(bsvi_uniform_entry), (size_t)desc->n_consts * 4, ((size_t)desc->n_params + 1) * 4,
                             (size_t)desc->n_uniform_grad * 4, 4 * (size_t)R * 4, ur_ptr.size() * 4, ur_item.size() * 4,
                             (size_t)desc->dataset_size * desc->n_features * 4, (size_t)desc->dataset_size * p->LC * 4, kinds.size()};
    const void* srcs[10] = {desc->uniform, desc->consts, desc->param_uniform_ptr, desc->param_uniform_idx, desc->row_uniform, ur_ptr.data(),
                           ur_item.data(), desc->dataset, desc->labels, kinds.data()};
    size_t offs[10], total = 0;
    for (int i = 0; i < 10; ++i) { offs[i] = total; total += align_up(sizes[i], 256); }
    std::vector<char> host(total + 256, 0);
    for (int i = 0; i < 10; ++i) if (sizes[i] && srcs[i]) memcpy(&host[offs[i]], srcs[i], sizes[i]);
    hipError_t e = hipMalloc(&p->dev_blob, host.size());
    if (e == hipSuccess) e = hipMemcpy(p->dev_blob, host.data(), host.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) { if (p->dev_blob) (void)hipFree(p->dev_blob); delete p; return fail(BSVI_ERR_HIP, std::string("bsvi_bnn_create: ") + hipGetErrorString(e)); }
    char* base = (char*)p->dev_blob;
    p->uniform = (const bsvi_uniform_entry*)(base + offs[0]); p->consts = (const float*)(base + offs[1]);
    p->pu_ptr = (const uint32_t*)(base + offs[2]); p->pu_idx = (const uint32_t*)(base + offs[3]);
    p->row_uniform = (const uint32_t*)(base + offs[4]); p->ur_ptr = (const uint32_t*)(base + offs[5]); p->ur_item = (const uint32_t*)(base + offs[6]);
    p->dataset = (const float*)(base + offs[7]); p->labels = (const float*)(base + offs[8]); p->row_kind = (uint8_t*)(base + offs[9]);
    {
        const size_t wl_bytes = bsvi_bnn_select::upper_lds_bytes(p->Rs, p->act_floats);
        int dev = 0, n_cu = 0;
        if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n_cu > 0) p->n_cu = (uint32_t)n_cu;
        p->upper_lds = bnn_middle_for(p, true, true) == bsvi_bnn_select::UPPER_LDS &&
                       hipFuncSetAttribute((const void*)bnn_upper<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)wl_bytes) == hipSuccess;
        if (!p->upper_lds) (void)hipGetLastError();
    }
    p->d.uniform = nullptr; p->d.consts = nullptr; p->d.param_uniform_ptr = nullptr; p->d.param_uniform_idx = nullptr;
    p->d.row_uniform = nullptr; p->d.dataset = nullptr; p->d.labels = nullptr;
    *out = p;
    return BSVI_OK;
}

extern "C" int bsvi_bnn_create(const bsvi_bnn_desc* desc, bsvi_bnn** out) { return bnn_create(desc, false, 0u, 0u, out); }

extern "C" int bsvi_bnn_create_normal(const bsvi_bnn_desc* desc, uint32_t scale_uniform, uint32_t scale_stride, bsvi_bnn** out) {
    return bnn_create(desc, true, scale_uniform, scale_stride, out);
}

extern "C" int bsvi_bnn_create_normal_learnable(const bsvi_bnn_desc* desc, uint32_t scale_uniform, uint32_t scale_stride, bsvi_bnn** out) {
    return bnn_create(desc, true, scale_uniform, scale_stride, out, true);
}

extern "C" int bsvi_bnn_create_normal_heads(const bsvi_bnn_desc* desc, uint32_t transform, float a, float b, bsvi_bnn** out) {
    const BnnHeads heads{transform, a, b};
    return bnn_create(desc, true, 0u, 0u, out, false, &heads);
}

// the prior of every row: Normal (what every row is without this call), Laplace or Cauchy.  Before the first launch only — the
// launches choose their instantiations of bnn_draw / bnn_row_sums from what stands here
extern "C" int bsvi_bnn_set_row_priors(bsvi_bnn* p, const uint8_t* kinds, uint32_t n_rows) {
    if (!p || !kinds) return fail(BSVI_ERR_INVALID, "bsvi_bnn_set_row_priors: null argument");
    if (n_rows != p->R) return fail(BSVI_ERR_INVALID, "bsvi_bnn_set_row_priors: n_rows is not the model's number of rows");
    if (p->launched.load()) return fail(BSVI_ERR_INVALID, "bsvi_bnn_set_row_priors: the model was launched already (set the priors before the first launch)");
    bool mixed = false;
    for (uint32_t r = 0; r < n_rows; ++r) {
        if (kinds[r] != BSVI_DIST_NORMAL && kinds[r] != BSVI_DIST_LAPLACE && kinds[r] != BSVI_DIST_CAUCHY)
            return fail(BSVI_ERR_UNSUPPORTED, "bsvi_bnn_set_row_priors: the prior of a row is Normal, Laplace or Cauchy");
        mixed = mixed || kinds[r] != BSVI_DIST_NORMAL;
    }
    HIP_TRY(hipMemcpy(p->row_kind, kinds, n_rows, hipMemcpyHostToDevice));      // (the pad bytes of the last quad stay Normal)
    p->mixed = mixed;
    return BSVI_OK;
}

// the family of the loc-scale likelihood: Normal (what every regression handle is without this call), Laplace or Cauchy.  Before the
// first launch only — the generated kernels carry the family as a literal and are compiled at the first launch
extern "C" int bsvi_bnn_set_likelihood_family(bsvi_bnn* p, uint32_t kind) {
    if (!p) return fail(BSVI_ERR_INVALID, "bsvi_bnn_set_likelihood_family: null handle");
    if (p->d.likelihood != BSVI_LIK_NORMAL)
        return fail(BSVI_ERR_INVALID, "bsvi_bnn_set_likelihood_family: the handle is a classifier's (the family is that of a model made by bsvi_bnn_create_normal*)");
    if (kind != BSVI_DIST_NORMAL && kind != BSVI_DIST_LAPLACE && kind != BSVI_DIST_CAUCHY)
        return fail(BSVI_ERR_UNSUPPORTED, "bsvi_bnn_set_likelihood_family: the likelihood is Normal, Laplace or Cauchy");
    if (p->launched.load() || p->upper_gen.state || p->mid_gen.state)
        return fail(BSVI_ERR_INVALID, "bsvi_bnn_set_likelihood_family: the model was launched already (set the family before the first launch)");
    p->family = kind;
    return BSVI_OK;
}

// latent prior scales (include/bsvi.h).  Before the first launch only: the launches choose their instantiations and their workspace
// from what stands here.  The entry -> item lists are built again with the latents' items 4 R + q T + t behind the rows' of every entry
// (a fixed order of additions), and bnn_epilogue leaves the latents' gradients at those items of rowg.
constexpr uint32_t BNN_MAX_LATENTS = 18;
extern "C" int bsvi_bnn_set_scale_latents(bsvi_bnn* p, uint32_t n_latents, const uint8_t* row_latent, uint32_t n_rows, const uint32_t* latent_uniform) {
    if (!p || !row_latent || !latent_uniform) return fail(BSVI_ERR_INVALID, "bsvi_bnn_set_scale_latents: null argument");
    if (n_rows != p->R) return fail(BSVI_ERR_INVALID, "bsvi_bnn_set_scale_latents: n_rows is not the model's number of rows");
    if (!n_latents || n_latents > BNN_MAX_LATENTS) return fail(BSVI_ERR_INVALID, "bsvi_bnn_set_scale_latents: 1 .. 18 latents");
    if (p->launched.load()) return fail(BSVI_ERR_INVALID, "bsvi_bnn_set_scale_latents: the model was launched already (set the latents before the first launch)");
    const uint32_t T = n_latents, R = p->R, NG = p->d.n_uniform_grad;
    for (uint32_t i = 0; i < 4u * T; ++i)
        if (latent_uniform[i] >= p->d.n_uniform) return fail(BSVI_ERR_INVALID, "bsvi_bnn_set_scale_latents: latent parameter out of the uniform table");
    std::vector<uint32_t> count(T, 0u);
    for (uint32_t r = 0; r < R; ++r) {
        if (row_latent[r] == 0xFFu) continue;
        if (row_latent[r] >= T) return fail(BSVI_ERR_INVALID, "bsvi_bnn_set_scale_latents: a row names a latent past n_latents");
        ++count[row_latent[r]];
    }
    const std::vector<uint32_t>& ru = p->row_uniform_host;
    std::vector<uint32_t> ur_ptr(NG + 1, 0u), ur_item, n_items(NG, 0u);
    for (size_t i = 0; i < 4 * (size_t)R; ++i) if (ru[i] < NG) ++n_items[ru[i]];
    for (uint32_t i = 0; i < 4u * T; ++i) if (latent_uniform[i] < NG) ++n_items[latent_uniform[i]];
    for (uint32_t k = 0; k < NG; ++k) ur_ptr[k + 1] = ur_ptr[k] + n_items[k];
    ur_item.resize(ur_ptr[NG]);
    std::vector<uint32_t> at(ur_ptr.begin(), ur_ptr.end() - 1);
    for (size_t i = 0; i < 4 * (size_t)R; ++i) if (ru[i] < NG) ur_item[at[ru[i]]++] = (uint32_t)i;
    for (uint32_t i = 0; i < 4u * T; ++i) if (latent_uniform[i] < NG) ur_item[at[latent_uniform[i]]++] = 4u * R + i;
    std::vector<uint8_t> bytes(((size_t)R + 3) / 4 * 4, (uint8_t)0xFFu);
    memcpy(bytes.data(), row_latent, R);
    const size_t sizes[5] = {ur_ptr.size() * 4, ur_item.size() * 4, bytes.size(), 4 * (size_t)T * 4, (size_t)T * 4};
    const void* srcs[5] = {ur_ptr.data(), ur_item.data(), bytes.data(), latent_uniform, count.data()};
    size_t offs[5], total = 0;
    for (int i = 0; i < 5; ++i) { offs[i] = total; total += align_up(sizes[i], 256); }
    std::vector<char> host(total + 256, 0);
    for (int i = 0; i < 5; ++i) if (sizes[i]) memcpy(&host[offs[i]], srcs[i], sizes[i]);
    void* blob = nullptr;
    hipError_t e = hipMalloc(&blob, host.size());
    if (e == hipSuccess) e = hipMemcpy(blob, host.data(), host.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) { if (blob) (void)hipFree(blob); return fail(BSVI_ERR_HIP, std::string("bsvi_bnn_set_scale_latents: ") + hipGetErrorString(e)); }
    if (p->lat_blob) (void)hipFree(p->lat_blob);
    p->lat_blob = blob;
    char* base = (char*)blob;
    p->ur_ptr = (const uint32_t*)(base + offs[0]); p->ur_item = (const uint32_t*)(base + offs[1]);
    p->row_latent = (const uint8_t*)(base + offs[2]); p->lat_uniform = (const uint32_t*)(base + offs[3]); p->lat_count = (const uint32_t*)(base + offs[4]);
    p->n_latents = T;
    return BSVI_OK;
}

// point-estimated rows (include/bsvi.h).  Before the first launch only: the launches choose their instantiations of bnn_draw /
// bnn_row_sums from what stands here.  A call whose bytes are all 0 leaves the handle as it was made: the kernels of a model without points
extern "C" int bsvi_bnn_set_point_rows(bsvi_bnn* p, const uint8_t* row_point, uint32_t n_rows) {
    if (!p || !row_point) return fail(BSVI_ERR_INVALID, "bsvi_bnn_set_point_rows: null argument");
    if (n_rows != p->R) return fail(BSVI_ERR_INVALID, "bsvi_bnn_set_point_rows: n_rows is not the model's number of rows");
    if (p->launched.load()) return fail(BSVI_ERR_INVALID, "bsvi_bnn_set_point_rows: the model was launched already (set the point rows before the first launch)");
    bool any = false;
    for (uint32_t r = 0; r < n_rows; ++r) {
        if (row_point[r] > 1u) return fail(BSVI_ERR_INVALID, "bsvi_bnn_set_point_rows: a byte is 0 (a random row) or 1 (a point row)");
        // (the q scale of a point row is never read as a scale: an entry with a gradient there would take the score term's -f / s)
        if (row_point[r] && p->row_uniform_host[(size_t)p->R + r] < p->d.n_uniform_grad)
            return fail(BSVI_ERR_INVALID, "bsvi_bnn_set_point_rows: the q scale entry of a point row must be a constant");
        any = any || row_point[r] != 0u;
    }
    if (p->row_point) { (void)hipFree(p->row_point); p->row_point = nullptr; }
    p->row_point_host.clear();
    p->shared_state.store(0);
    if (!any) return BSVI_OK;
    std::vector<uint8_t> bytes(((size_t)n_rows + 3) / 4 * 4, (uint8_t)0u);      // (the pad bytes of the last quad: no point)
    memcpy(bytes.data(), row_point, n_rows);
    void* blob = nullptr;
    hipError_t e = hipMalloc(&blob, bytes.size());
    if (e == hipSuccess) e = hipMemcpy(blob, bytes.data(), bytes.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) { if (blob) (void)hipFree(blob); return fail(BSVI_ERR_HIP, std::string("bsvi_bnn_set_point_rows: ") + hipGetErrorString(e)); }
    p->row_point = (uint8_t*)blob;
    p->row_point_host.assign(row_point, row_point + n_rows);
    return BSVI_OK;
}

// the parameters of the layers' activations (include/bsvi.h).  Before the first launch only: the generated kernels carry them as literals
// and are compiled at the first launch (or by bsvi_bnn_middle).  The pair of a layer whose kind has no parameter is not read and not kept
extern "C" int bsvi_bnn_set_activation_params(bsvi_bnn* p, const float* params, uint32_t n_layers) {
    if (!p || !params) return fail(BSVI_ERR_INVALID, "bsvi_bnn_set_activation_params: null argument");
    if (n_layers != p->d.n_layers) return fail(BSVI_ERR_INVALID, "bsvi_bnn_set_activation_params: n_layers is not the model's number of layers");
    if (p->launched.load() || p->upper_gen.state || p->mid_gen.state)
        return fail(BSVI_ERR_INVALID, "bsvi_bnn_set_activation_params: the model was launched already (set the parameters before the first launch)");
    for (uint32_t l = 0; l < n_layers; ++l) {
        const uint32_t a = p->layers[l].activation;
        const float p0 = params[2 * l], p1 = params[2 * l + 1];
        if (!std::isfinite(p0) || !std::isfinite(p1)) return fail(BSVI_ERR_INVALID, "bsvi_bnn_set_activation_params: a parameter is not finite");
        if (a == BSVI_BNN_ACT_LEAKY_RELU && !(p0 > 0.0f))
            return fail(BSVI_ERR_INVALID, "bsvi_bnn_set_activation_params: the negative_slope of a leaky_relu layer must be > 0");
        if (a == BSVI_BNN_ACT_ELU && !(p0 > 0.0f)) return fail(BSVI_ERR_INVALID, "bsvi_bnn_set_activation_params: the alpha of an elu layer must be > 0");
        if (a == BSVI_BNN_ACT_HARDTANH && !(p0 < p1))
            return fail(BSVI_ERR_INVALID, "bsvi_bnn_set_activation_params: the limits of a hardtanh layer need min_val < max_val");
    }
    for (uint32_t l = 0; l < n_layers; ++l) {
        const uint32_t a = p->layers[l].activation;
        if (a == BSVI_BNN_ACT_LEAKY_RELU || a == BSVI_BNN_ACT_ELU || a == BSVI_BNN_ACT_HARDTANH) p->act_p[l][0] = params[2 * l];
        if (a == BSVI_BNN_ACT_HARDTANH) p->act_p[l][1] = params[2 * l + 1];
    }
    return BSVI_OK;
}

extern "C" void bsvi_bnn_destroy(bsvi_bnn* p) {
    if (!p) return;
    if (p->dev_blob) (void)hipFree(p->dev_blob);
    if (p->lat_blob) (void)hipFree(p->lat_blob);
    if (p->row_point) (void)hipFree(p->row_point);
    if (p->upper_gen.module) (void)hipModuleUnload(p->upper_gen.module);
    if (p->mid_gen.module) (void)hipModuleUnload(p->mid_gen.module);
    delete p;
}

extern "C" int bsvi_bnn_exact_data(const bsvi_bnn* p) { return (p && p->exact) ? 1 : 0; }

// 1: the launches of this handle take the shared first layer (every row of weights1 a point row, BSVI_BNN_SHARED1 not 0); 0: both
// products per sample; -1 for a null handle
extern "C" int bsvi_bnn_shared_first(const bsvi_bnn* p) { return p ? (bnn_shared_first(p) ? 1 : 0) : -1; }

// the middle kernel the next launch runs (bnn_launch asks the same questions in the same order): the generated kernels are compiled here
// as a launch would compile them, and one that did not compile reports what serves in its place
extern "C" int bsvi_bnn_middle(const bsvi_bnn* p) {
    if (!p) return -1;
    if (bnn_gen_ready(p, true)) return bsvi_bnn_select::MID_GEN;
    if (bnn_gen_ready(p, false)) return bsvi_bnn_select::UPPER_GEN;
    return p->upper_lds ? bsvi_bnn_select::UPPER_LDS : bsvi_bnn_select::UPPER_MEM;
}

// the <MIXED, LATENT, POINT> instantiation a handle's launches take: point rows (Q.row_point; with or without latents), else latent prior scales (Q.n_latents; a predict call fills none: its draw
// takes no prior), else some row's prior Laplace or Cauchy, else the all-Normal kernels
static void bnn_launch_draw(const bsvi_bnn* p, const BParams& Q, const uint32_t row_chunks, hipStream_t s) {
    const dim3 grid(row_chunks, (Q.n_pad + 3u) / 4u);
    if (Q.row_point && Q.n_latents) hipLaunchKernelGGL((bnn_draw<true, true, true>), grid, dim3(256), 0, s, Q);
    else if (Q.row_point) hipLaunchKernelGGL((bnn_draw<true, false, true>), grid, dim3(256), 0, s, Q);
    else if (Q.n_latents) hipLaunchKernelGGL((bnn_draw<true, true>), grid, dim3(256), 0, s, Q);
    else if (p->mixed) hipLaunchKernelGGL(bnn_draw<true>, grid, dim3(256), 0, s, Q);
    else hipLaunchKernelGGL(bnn_draw<false>, grid, dim3(256), 0, s, Q);
}
static void bnn_launch_row_sums(const bsvi_bnn* p, const BParams& Q, hipStream_t s) {
    const uint32_t n_quads = (Q.R + 3) / 4 - Q.quad0;      // (the shared first layer: weights1's quads are bnn_rows_shared's)
    if (!n_quads) return;
    const dim3 grid((n_quads + 3) / 4);
    if (Q.row_point && Q.n_latents) hipLaunchKernelGGL((bnn_row_sums<true, true, true>), grid, dim3(256), 0, s, Q);
    else if (Q.row_point) hipLaunchKernelGGL((bnn_row_sums<true, false, true>), grid, dim3(256), 0, s, Q);
    else if (Q.n_latents) hipLaunchKernelGGL((bnn_row_sums<true, true>), grid, dim3(256), 0, s, Q);
    else if (p->mixed) hipLaunchKernelGGL(bnn_row_sums<true>, grid, dim3(256), 0, s, Q);
    else hipLaunchKernelGGL(bnn_row_sums<false>, grid, dim3(256), 0, s, Q);
}

struct BnnLayout {
    size_t rowp, idx, lab, Xb, Xb_bf, XbT_bf, W1f, Wp, Wsm, a1T, acts, deltas, liknb, da1T, dlogp, GT, gsm, lik, pv, qv, sums, rowg, hpart, partial, fs, total;
    size_t sigt, gsig, gsd;
    size_t lat_l, lat_itau, lat_eps, lat_D, lat_z, lat_upart, lat_f, lat_q, lat_b;
    size_t a1s, dpart, dbar, GT1;
    uint32_t n_pad, NC, row_chunks, row_blocks;
};
static BnnLayout bnn_layout(const bsvi_bnn* p, uint32_t n_local) {
    BnnLayout L{};
    L.n_pad = (n_local + 63) / 64 * 64;
    L.NC = p->H1 * L.n_pad;
    L.row_chunks = ((p->R + 3) / 4 + 63) / 64;
    L.row_blocks = (p->R + 3) / 4;                      // (one pair of partial constants per row quad: bnn_row_sums)
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += align_up(bytes, 256); return at; };
    const size_t nb = (size_t)L.n_pad * p->B_pad;
    L.rowp = take(4 * (size_t)p->R * 4); L.idx = take((size_t)p->B_pad * 4);
    // (targets [B_pad][LC]; the Normal likelihood keeps sigma and its log term, [2][C], behind them)
    L.lab = take(((size_t)p->B_pad * p->LC + (p->d.likelihood == BSVI_LIK_NORMAL ? 2u * (size_t)p->C : 0u)) * 4);
    L.Xb = take(p->exact ? 0 : (size_t)p->B_pad * p->P_ld * 4);
    L.Xb_bf = take(p->exact ? (size_t)p->B_pad * p->Kp * 2 : 0); L.XbT_bf = take(p->exact ? (size_t)p->P * p->B_pad * 2 : 0);
    // (the shared first layer keeps no per-sample copies of weights1 and no per-sample second product: its four small arrays stand
    //  behind everything else)
    const bool shared = bnn_shared_first(p);
    L.W1f = take(p->exact || shared ? 0 : (size_t)L.NC * p->P_ld * 4); L.Wp = take(p->exact && !shared ? 3 * (size_t)L.NC * p->Kp * 2 : 0);
    L.Wsm = take((size_t)L.n_pad * (p->Rs ? p->Rs : 1) * 4);
    L.a1T = take((size_t)p->B_pad * L.NC * 4);
    L.acts = take(nb * p->act_floats * 4); L.deltas = take(nb * p->delta_floats * 4); L.liknb = take(nb * 4);
    L.da1T = take(p->exact ? 0 : (size_t)L.NC * p->B_pad * 4); L.dlogp = take(p->exact ? 3 * (size_t)L.NC * p->B_pad * 2 : 0);
    L.GT = take(shared ? 0 : p->exact ? (size_t)p->P * L.NC * 4 : (size_t)L.NC * p->P_ld * 4);
    L.gsm = take((size_t)L.n_pad * (p->Rs ? p->Rs : 1) * 4); L.lik = take((size_t)L.n_pad * 4);
    L.pv = take((size_t)L.row_chunks * L.n_pad * 4); L.qv = take((size_t)L.row_chunks * L.n_pad * 4);
    L.sums = take(4 * (size_t)p->R * 4); L.rowg = take(4 * ((size_t)p->R + p->n_latents) * 4); L.hpart = take(2 * (size_t)L.row_blocks * 8);
    L.partial = take((2 + (size_t)p->d.n_uniform_grad) * 4); L.fs = take(256);
    // (a learnable sigma's three arrays behind everything else: nothing moves, and nothing is added, for the networks without one)
    if (p->scale_learn) { L.sigt = take(nb * p->C * 4); L.gsig = take((size_t)L.n_pad * p->C * 4); L.gsd = take((size_t)p->C * 8); }
    // (latent prior scales: behind everything else, for such handles only)
    if (p->n_latents) {
        const size_t tn = (size_t)p->n_latents * L.n_pad * 4;
        L.lat_l = take(tn); L.lat_itau = take(tn); L.lat_eps = take(tn); L.lat_D = take(tn); L.lat_z = take(tn);
        L.lat_upart = take((size_t)L.row_chunks * tn);
        L.lat_f = take((size_t)L.n_pad * 8); L.lat_q = take((size_t)L.n_pad * 8); L.lat_b = take((size_t)L.n_pad * 8);
    }
    if (shared) {
        const size_t hb = (size_t)p->H1 * p->B_pad * 4;
        L.a1s = take(hb); L.dpart = take((size_t)(L.n_pad / 64u) * hb); L.dbar = take(hb); L.GT1 = take((size_t)p->R1 * 4);
    }
    L.total = o + 256;
    return L;
}

extern "C" size_t bsvi_bnn_workspace_bytes(const bsvi_bnn* p, uint32_t n_samples_local) {
    return p && n_samples_local ? bnn_layout(p, n_samples_local).total : 0;
}

static int bnn_fill(const bsvi_bnn* p, const bsvi_bnn_args* a, BParams& Q, BnnLayout& L) {
    if (!a) return fail(BSVI_ERR_INVALID, "null argument");
    BSVI_CHECK_STRUCT(a, bsvi_bnn_args);
    if (!p) return fail(BSVI_ERR_INVALID, "null argument");
    if (!a->params_dev && p->d.n_params) return fail(BSVI_ERR_INVALID, "params_dev is null");
    if (!a->out_dev || !a->workspace_dev) return fail(BSVI_ERR_INVALID, "out_dev / workspace_dev is null");
    if (!a->n_samples_local || !a->n_samples_global) return fail(BSVI_ERR_INVALID, "zero samples");
    if ((uint64_t)p->H1 * ((a->n_samples_local + 63) / 64 * 64) * (uint64_t)std::max(p->Kp, p->B_pad) >= (1ull << 31))
        return fail(BSVI_ERR_UNSUPPORTED, "bsvi_bnn: number_samples x hidden units x features beyond the 32-bit index range of the product kernels");
    L = bnn_layout(p, a->n_samples_local);
    memset(&Q, 0, sizeof Q);
    char* ws = (char*)a->workspace_dev;
    Q.uniform = p->uniform; Q.consts = p->consts; Q.params = a->params_dev; Q.row_uniform = p->row_uniform;
    Q.ur_ptr = p->ur_ptr; Q.ur_item = p->ur_item; Q.dataset = p->dataset; Q.labels = p->labels;
    Q.n_layers = p->d.n_layers;
    for (uint32_t l = 0; l < Q.n_layers; ++l) {
        const bsvi_bnn_layer& S = p->layers[l];
        BnnLayerDev& D = Q.layer[l];
        D.rows = S.rows; D.cols = S.cols; D.w0 = S.weight_row0; D.b0 = S.bias_row0; D.act = S.activation;
        const size_t nb = (size_t)L.n_pad * p->B_pad;
        if (nb * p->act_floats >= (1ull << 32)) return fail(BSVI_ERR_UNSUPPORTED, "bsvi_bnn: activations beyond the 32-bit offset range");
        D.act_off = (uint32_t)(nb * p->act_off[l]); D.delta_off = D.act_off;
        D.in_off = l ? (uint32_t)(nb * p->act_off[l - 1]) : 0u;
    }
    memcpy(Q.act_p, p->act_p, sizeof Q.act_p);
    Q.R = p->R; Q.R1 = p->R1; Q.Rs = p->Rs ? p->Rs : 1; Q.P = p->P; Q.C = p->C; Q.H1 = p->H1; Q.DS = p->d.dataset_size; Q.B = p->d.batch_size;
    Q.B_pad = p->B_pad; Q.Kp = p->Kp; Q.P_ld = p->P_ld; Q.n_local = a->n_samples_local; Q.n_pad = L.n_pad; Q.n_global = a->n_samples_global;
    Q.sample_base = a->sample_base; Q.NC = L.NC; Q.n_uniform_grad = p->d.n_uniform_grad; Q.likelihood = p->d.likelihood;
    Q.estimator = p->d.estimator; Q.exact = p->exact ? 1u : 0u; Q.act_width = (uint32_t)p->act_floats;
    Q.LC = p->LC; Q.scale_u = p->scale_u; Q.scale_stride = p->scale_stride; Q.scale_learn = p->scale_learn ? 1u : 0u;
    Q.heads = p->heads; Q.head_a = p->head_a; Q.head_b = p->head_b; Q.family = p->family;
    Q.lik_weight = p->d.lik_weight; Q.prior_weight = p->d.prior_weight; Q.entropy_weight = p->d.entropy_weight;
    Q.seed_lo = (uint32_t)a->seed; Q.seed_hi = (uint32_t)(a->seed >> 32); Q.offset_lo = (uint32_t)a->offset; Q.offset_hi = (uint32_t)(a->offset >> 32);
    Q.noise_in = a->noise_dev; Q.noise_out = a->noise_out_dev; Q.indices_in = a->indices_dev; Q.indices_out = a->indices_out_dev;
    Q.fvalue_out = a->fvalue_out_dev; Q.logq_out = a->logq_out_dev;
    if (a->q_weight_dev && p->d.estimator != BSVI_EST_BLACKBOX)
        return fail(BSVI_ERR_INVALID, "q_weight_dev needs a model lowered for the BlackBox estimator (its launches accumulate log q)");
    if (p->d.estimator == BSVI_EST_BLACKBOX && !a->f_weight_dev != !a->q_weight_dev)
        return fail(BSVI_ERR_INVALID, "a BlackBox model takes f_weight_dev and q_weight_dev together (or neither)");
    Q.f_weight = a->f_weight_dev; Q.q_weight = a->q_weight_dev;
    Q.rowp = (float*)(ws + L.rowp); Q.idx = (int32_t*)(ws + L.idx); Q.lab = (float*)(ws + L.lab);
    Q.Xb = (float*)(ws + L.Xb); Q.Xb_bf = (uint16_t*)(ws + L.Xb_bf); Q.XbT_bf = (uint16_t*)(ws + L.XbT_bf);
    Q.W1f = (float*)(ws + L.W1f); Q.Wp = (uint16_t*)(ws + L.Wp); Q.Wsm = (float*)(ws + L.Wsm); Q.a1T = (float*)(ws + L.a1T);
    Q.acts = (float*)(ws + L.acts); Q.deltas = (float*)(ws + L.deltas); Q.liknb = (float*)(ws + L.liknb);
    Q.da1T = (float*)(ws + L.da1T); Q.dlogp = (uint16_t*)(ws + L.dlogp); Q.GT = (float*)(ws + L.GT);
    Q.gsm = (float*)(ws + L.gsm); Q.lik = (float*)(ws + L.lik); Q.pv_part = (float*)(ws + L.pv); Q.qv_part = (float*)(ws + L.qv);
    Q.sums = (float*)(ws + L.sums); Q.rowg = (float*)(ws + L.rowg); Q.hpart = (double*)(ws + L.hpart); Q.partial = (float*)(ws + L.partial);
    Q.fs = (float*)(ws + L.fs); Q.row_chunks = L.row_chunks;
    if (p->scale_learn) { Q.sigt = (float*)(ws + L.sigt); Q.gsig = (float*)(ws + L.gsig); Q.gsd = (double*)(ws + L.gsd); }
    Q.row_kind = p->row_kind; Q.row_point = p->row_point;
    if (bnn_shared_first(p)) {
        Q.shared1 = 1u; Q.quad0 = p->R1 / 4u;
        Q.a1s = (float*)(ws + L.a1s); Q.dpart = (float*)(ws + L.dpart); Q.dbar = (float*)(ws + L.dbar); Q.GT1 = (float*)(ws + L.GT1);
    }
    if (p->n_latents) {
        Q.n_latents = p->n_latents; Q.row_latent = p->row_latent; Q.lat_uniform = p->lat_uniform; Q.lat_count = p->lat_count;
        Q.lat_l = (float*)(ws + L.lat_l); Q.lat_itau = (float*)(ws + L.lat_itau); Q.lat_eps = (float*)(ws + L.lat_eps);
        Q.lat_D = (float*)(ws + L.lat_D); Q.lat_z = (float*)(ws + L.lat_z); Q.lat_upart = (float*)(ws + L.lat_upart);
        Q.lat_f = (double*)(ws + L.lat_f); Q.lat_q = (double*)(ws + L.lat_q); Q.lat_b = (double*)(ws + L.lat_b);
    }
    return BSVI_OK;
}

static int bnn_launch(const bsvi_bnn* p, const BParams& Q, const BnnLayout& L, hipStream_t s) {
    const uint32_t head_n = std::max(Q.R, Q.B_pad);
    const uint32_t head_blocks = (head_n + 255) / 256, gy = (std::max(Q.Kp, Q.P_ld) + 255) / 256;
    p->launched.store(true);
    const uint32_t lat_blocks = (Q.n_latents * Q.n_pad + 255u) / 256u;      // (none without latent prior scales)
    hipLaunchKernelGGL(bnn_head_gather, dim3(Q.B_pad * gy + head_blocks + lat_blocks), dim3(256), 0, s, Q, gy, head_blocks);
    bnn_launch_draw(p, Q, L.row_chunks, s);
    int rc;
    const bool mid = bnn_gen_ready(p, true);
    if (Q.shared1) {
        // weights1 is the same for every sample: the first product once, broadcast in the layout the middle kernel reads
        rc = BSVI_OK;
        hipLaunchKernelGGL(bnn_first_shared, dim3((Q.B_pad * Q.H1 + 3u) / 4u), dim3(256), 0, s, Q);
        const dim3 bgrid((uint32_t)(((size_t)Q.B_pad * Q.NC / 4u + 255u) / 256u));
        if (mid) hipLaunchKernelGGL(bnn_first_broadcast<true>, bgrid, dim3(256), 0, s, Q);
        else hipLaunchKernelGGL(bnn_first_broadcast<false>, bgrid, dim3(256), 0, s, Q);
    }
    else if (mid) rc = bsvi_xgemm_nt_t(Q.Xb_bf, nullptr, Q.Wp, (long)Q.NC * Q.Kp, Q.a1T, (int)Q.B_pad, (int)Q.B_pad, (int)Q.NC, (int)Q.Kp, s);      // a1 as [(h, n)][b]
    else if (Q.exact) rc = bsvi_xgemm_nt(Q.Xb_bf, nullptr, Q.Wp, (long)Q.NC * Q.Kp, Q.a1T, (int)Q.NC, (int)Q.B_pad, (int)Q.NC, (int)Q.Kp, s);
    else rc = bsvi_gemm_f32(0, Q.Xb, (int)Q.P_ld, Q.W1f, (int)Q.P_ld, Q.a1T, (int)Q.NC, (int)Q.B_pad, (int)Q.NC, (int)Q.P, s);
    if (rc) return rc;
    if (mid) {
        // one workgroup per sample: upper layers, likelihood, reverse sweep, pieces of d f / d a1, gradients of the small tensors
        const BnnMidArgsSig M{{Q.Wsm, Q.a1T, Q.lab, Q.gsm, Q.lik, Q.dlogp, Q.n_local, Q.n_pad, Q.B, Q.B_pad, Q.NC, Q.lik_weight, Q.f_weight}, Q.gsig};
        size_t size = p->scale_learn ? sizeof M : sizeof M.a;      // (the kernel of a constant sigma declares the first part alone)
        void* config[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, (void*)&M, HIP_LAUNCH_PARAM_BUFFER_SIZE, &size, HIP_LAUNCH_PARAM_END};
        HIP_TRY(hipModuleLaunchKernel(p->mid_gen.fn, Q.n_pad, 1, 1, 256, 1, 1, (unsigned)bnn_mid_lds_bytes(p), s, nullptr, config));
    } else {
        const dim3 ugrid(Q.n_pad / 64, (Q.B_pad + 7) / 8);
        const size_t wl_bytes = bsvi_bnn_select::upper_lds_bytes(p->Rs, p->act_floats);
        if (bnn_gen_ready(p, false)) {
            // (no LDS beyond the staging tile and registers only: several workgroups per CU — two rows per wave as above)
            BnnUpperArgsSig US{{Q.Wsm, Q.a1T, Q.lab, Q.acts, Q.deltas, Q.liknb, Q.da1T, Q.dlogp, Q.n_local, Q.n_pad, Q.B, Q.B_pad, Q.NC, 2u, Q.exact, Q.lik_weight, Q.f_weight}, Q.sigt};
            BnnUpperArgs& U = US.a;
            static const uint32_t rpw = [] { const char* e = getenv("BSVI_BNN_ROWS_PER_WAVE"); return e ? (uint32_t)atoi(e) : 0u; }();
            if (rpw) U.rows_per_wave = rpw;
            size_t size = p->scale_learn ? sizeof US : sizeof U;
            void* config[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &US, HIP_LAUNCH_PARAM_BUFFER_SIZE, &size, HIP_LAUNCH_PARAM_END};
            const uint32_t gy = (Q.B_pad + 4u * U.rows_per_wave - 1u) / (4u * U.rows_per_wave);
            HIP_TRY(hipModuleLaunchKernel(p->upper_gen.fn, Q.n_pad / 64, gy, 1, 256, 1, 1, (unsigned)bsvi_bnn_select::upper_gen_lds_bytes(p->Rs), s, nullptr, config));
        }
        else if (p->upper_lds) hipLaunchKernelGGL(bnn_upper<true>, ugrid, dim3(256), wl_bytes, s, Q);
        else hipLaunchKernelGGL(bnn_upper<false>, ugrid, dim3(256), 0, s, Q);
        for (uint32_t l = 0; l < Q.n_layers; ++l) {
            const BnnLayerDev& D = Q.layer[l];
            if (l == 0 && D.b0 == 0xFFFFFFFFu) continue;
            const uint32_t jn = l ? D.cols + 1u : 1u;
            hipLaunchKernelGGL(bnn_small, dim3(Q.n_pad / 64, (D.rows + 3) / 4, (jn + 3) / 4), dim3(256), 0, s, Q, l);
        }
        hipLaunchKernelGGL(bnn_lik, dim3(Q.n_pad / 64), dim3(256), 0, s, Q);
        if (Q.scale_learn) hipLaunchKernelGGL(bnn_sig_rows, dim3(Q.n_pad / 64, Q.C), dim3(256), 0, s, Q);
    }
    if (Q.shared1) {
        // the sum over the samples first (two steps, a fixed order), then ONE second product, and weights1's row terms from it
        hipLaunchKernelGGL(bnn_da1_partial, dim3((Q.B_pad + 255u) / 256u, Q.H1, Q.n_pad / 64u), dim3(256), 0, s, Q);
        hipLaunchKernelGGL(bnn_da1_total, dim3((Q.H1 * Q.B_pad + 255u) / 256u), dim3(256), 0, s, Q);
        hipLaunchKernelGGL(bnn_second_shared, dim3((Q.P + 63u) / 64u, Q.H1), dim3(1024), 0, s, Q);
        hipLaunchKernelGGL(bnn_rows_shared, dim3((Q.R1 + 255u) / 256u), dim3(256), 0, s, Q);
        rc = BSVI_OK;
    }
    else if (Q.exact) rc = bsvi_xgemm_nt(Q.XbT_bf, nullptr, Q.dlogp, (long)Q.NC * Q.B_pad, Q.GT, (int)Q.NC, (int)Q.P, (int)Q.NC, (int)Q.B_pad, s);
    else rc = bsvi_gemm_f32(1, Q.da1T, (int)Q.B_pad, Q.Xb, (int)Q.P_ld, Q.GT, (int)Q.P_ld, (int)Q.NC, (int)Q.P, (int)Q.B_pad, s);
    if (rc) return rc;
    bnn_launch_row_sums(p, Q, s);
    if (Q.n_latents) hipLaunchKernelGGL(bnn_latent_terms, dim3(Q.n_pad / 256u + (Q.n_pad % 256u ? 1u : 0u)), dim3(256), 0, s, Q);
    hipLaunchKernelGGL(bnn_epilogue, dim3(1), dim3(1024), 0, s, Q, L.row_blocks);
    if (Q.n_latents) hipLaunchKernelGGL(bnn_latent_grads, dim3(Q.n_latents), dim3(256), 0, s, Q);
    if (Q.n_uniform_grad) hipLaunchKernelGGL(bnn_uniform_grads, dim3((Q.n_uniform_grad + 255) / 256), dim3(256), 0, s, Q);
    HIP_TRY(hipGetLastError());
    return BSVI_OK;
}

static void bnn_rparams(const bsvi_bnn* p, const BParams& Q, float* params, float* out, RParams& R) {
    memset(&R, 0, sizeof(R));
    R.uniform = p->uniform; R.pu_ptr = p->pu_ptr; R.pu_idx = p->pu_idx;
    R.partials = Q.partial; R.params = params; R.out = out;
    R.n_uniform_grad = p->d.n_uniform_grad; R.n_params = p->d.n_params; R.n_blocks = 1; R.n_global = Q.n_global;
}

extern "C" int bsvi_bnn_fwd_bwd(const bsvi_bnn* p, const bsvi_bnn_args* a) {
    BParams Q; BnnLayout L;
    int rc = bnn_fill(p, a, Q, L);
    if (rc) return rc;
    rc = bnn_launch(p, Q, L, (hipStream_t)a->stream);
    if (rc) return rc;
    RParams R;
    bnn_rparams(p, Q, const_cast<float*>(a->params_dev), a->out_dev, R);
    const uint32_t n = p->d.n_params ? p->d.n_params : 1;
    hipLaunchKernelGGL(dense_param_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)a->stream, R);
    HIP_TRY(hipGetLastError());
    return BSVI_OK;
}

extern "C" int bsvi_bnn_finalize(const bsvi_bnn* p, float* out_dev, uint32_t n_global, void* stream) {
    if (!p || !out_dev || !n_global) return fail(BSVI_ERR_INVALID, "null argument");
    const uint32_t n = p->d.n_params ? p->d.n_params : 1;
    hipLaunchKernelGGL(finalize_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, out_dev, p->d.n_params, n_global);
    HIP_TRY(hipGetLastError());
    return BSVI_OK;
}

extern "C" int bsvi_bnn_step(const bsvi_bnn* p, const bsvi_bnn_args* a, const bsvi_opt_cfg* cfg, float* params_dev, float* state_dev,
                             const uint8_t* active_mask_dev, float* loss_slot_dev, float* finite_slot_dev) {
    int rc = check_cfg(cfg);
    if (rc) return rc;
    if (!params_dev || !state_dev || !active_mask_dev) return fail(BSVI_ERR_INVALID, "null argument");
    if (a && a->n_samples_local != a->n_samples_global) return fail(BSVI_ERR_INVALID, "bsvi_bnn_step is the single-GPU path");
    if (!a) return fail(BSVI_ERR_INVALID, "null argument");
    bsvi_bnn_args aa = *a;
    aa.params_dev = params_dev;
    BParams Q; BnnLayout L;
    rc = bnn_fill(p, &aa, Q, L);
    if (rc) return rc;
    rc = bnn_launch(p, Q, L, (hipStream_t)a->stream);
    if (rc) return rc;
    RParams R;
    bnn_rparams(p, Q, params_dev, a->out_dev, R);
    R.state = state_dev; R.active_mask = active_mask_dev; R.loss_slot = loss_slot_dev; R.finite_slot = finite_slot_dev;
    R.do_finalize = 1; R.do_step = 1; R.cfg = *cfg;
    const uint32_t n = p->d.n_params ? p->d.n_params : 1;
    hipLaunchKernelGGL(dense_param_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)a->stream, R);
    HIP_TRY(hipGetLastError());
    return BSVI_OK;
}

// ---- posterior predictive (bsvi_bnn_predict, include/bsvi.h) ----------------------------------------------------------------
// N weight sets from the current posterior (bnn_draw as it is: the same weights a training launch of (seed, offset, sample_base) sees;
// its per-sample prior / log q partials are written and never read), the chain forward on rows the CALLER hands in, in passes of
// rows_pass rows:
//   bnn_predict_exact   are all values of x exactly bf16?  (one flag, read back by the host once per call: it chooses the product)
//   bnn_predict_head    row parameters, sigma of the Normal likelihood
//   bnn_draw            once per call
//   per pass:  bnn_predict_gather   x_new rows as the first product's operand (bf16 [rows][Kp] | f32 [rows][P_ld]; pads zero)
//              product 1            bsvi_xgemm_nt | bsvi_gemm_f32, as bnn_launch makes them: a1 [rows][(h, n)]
//              bnn_predict_fwd      one thread per (sample, row): bias + activation, the upper layers (TWO activation buffers of the
//                                   widest layer, ping-pong), the head: z, p, and the likelihood's draw
//              bnn_predict_reduce   one thread per (row, output): mean over the samples (and var), sample order, double precision
// The likelihood's noise is a Philox stream of its own (philox.h): c0 = global sample, c1 = row m of x_new, c2 / c3 = the offset, the
// key word k0 xor-ed with BNN_KEY_PREDICT — no training stream of the same seed has that key.
//   Categorical   inverse CDF on the STORED f32 probabilities: partial sums in class order c = 0, 1, ... in single precision, the first
//                 class whose partial sum is >= u01(word 0), the last class if none is
//   Bernoulli     u01(word 0) < p
//   Normal        loc_c + sigma_c e: output c takes normal c & 3 of the four box_muller_fast normals ((x, y) -> 0, 1; (z, w) -> 2, 3) of
//                 the call whose key word k1 is xor-ed with c >> 2: one call serves four outputs, no counter is used twice
constexpr uint32_t BNN_KEY_PREDICT = 0x2545F491u;

struct BnnPredict {
    const float* x_new;          // [M][P]
    uint32_t M, m0, rows_pass;   // rows of the call, first row of this pass, rows of a pass (a multiple of 32)
    const float* a1;             // [rows_pass][NC]
    float* act;                  // global arm: [2 max_width][rows_pass][n_pad]
    uint32_t max_width;
    const float* sg;             // Normal: sigma [C]
    uint32_t* flag;
    float* z_out; float* draw_out;        // [n_local][M][C] or null
    float* p;                    // the pass's p: element (n, j, c) of the pass at p[n * p_stride + j * C + c]
    size_t p_stride;
    float* mean_out; float* var_out;      // [M][C] or null
    // a scale head only: sigma of the pass, element (n, j, c) at sig[n * sig_stride + j * C + c] (what the reduce reads; z_out holds a copy)
    float* sig; size_t sig_stride;
};

// grid: any, block 256.  flag must hold 1; a value with low mantissa bits clears it (every writer writes the same 0)
__global__ void __launch_bounds__(256) bnn_predict_exact(const float* __restrict__ x, const size_t n, uint32_t* flag) {
    bool bad = false;
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (size_t)gridDim.x * 256u)
        bad = bad || (__float_as_uint(x[i]) & 0xFFFFu) != 0u;
    if (bad) *flag = 0u;
}

// threads: max(R, C)
__global__ void __launch_bounds__(256) bnn_predict_head(const BParams Q, const BnnPredict V) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < Q.R) {
#pragma unroll
        for (uint32_t q = 0; q < 4u; ++q) Q.rowp[(size_t)q * Q.R + i] = bnn_uniform_value(Q, Q.row_uniform[(size_t)q * Q.R + i]);
    }
    if (Q.likelihood == BSVI_LIK_NORMAL && !Q.heads && i < Q.C) const_cast<float*>(V.sg)[i] = bnn_uniform_value(Q, Q.scale_u + i * Q.scale_stride);
}

// row m0 + j of x_new as row j of the pass's operand, as bnn_gather_body writes the minibatch's (no transpose: there is no second
// product).  Rows from M on and columns from P on are zero; nothing is read beyond x_new[M][P].  blocks: rows_pass x ceil(Kp / 256)
__global__ void __launch_bounds__(256) bnn_predict_gather(const BParams Q, const BnnPredict V, const uint32_t gy) {
    const uint32_t j = blockIdx.x / gy, p = (blockIdx.x % gy) * 256u + threadIdx.x, m = V.m0 + j;
    const float v = (m < V.M && p < Q.P) ? V.x_new[(size_t)m * Q.P + p] : 0.0f;
    if (Q.exact) {
        if (p < Q.Kp) Q.Xb_bf[(size_t)j * Q.Kp + p] = dense_bf16_bits(v);
    } else if (p < Q.P_ld) {
        Q.Xb[(size_t)j * Q.P_ld + p] = v;
    }
}

// One thread per (sample n, row j of the pass), lanes along n; a workgroup = 64 samples x 8 rows (a wave takes two), as bnn_upper.
// LDSW: the small tensors of the 64 samples staged once per workgroup, transposed ([row][sample]), and the thread's two activation
// buffers a column of LDS each ([unit][thread]); else both in global memory.  The arithmetic of the forward sweep is bnn_upper's, in
// its order.  Padded samples (n >= n_local) and padded rows (m >= M) compute on zeros and write nothing.
// grid: ceil(n_pad / 64) x ceil(rows_pass / 8), block 256
template <bool LDSW>
__global__ void __launch_bounds__(256) bnn_predict_fwd(const BParams Q, const BnnPredict V) {
    float* const wl = g_lds;                                      // [Rs][65]
    float* const ya = g_lds + (size_t)Q.Rs * 65u + threadIdx.x;   // buffer 0 [max_width][256] of this thread, then buffer 1
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, n = blockIdx.x * 64u + lane;
    if (LDSW) {
        for (uint32_t i = threadIdx.x; i < 64u * Q.Rs; i += 256u) {
            const uint32_t sn = i / Q.Rs, r = i - sn * Q.Rs;
            wl[r * 65u + sn] = Q.Wsm[(size_t)(blockIdx.x * 64u + sn) * Q.Rs + r];
        }
        __syncthreads();
    }
    const float* const wsm = Q.Wsm + (size_t)n * Q.Rs;
    auto W = [&](uint32_t r) { return LDSW ? wl[r * 65u + lane] : wsm[r]; };
    const BnnLayerDev L1 = Q.layer[0], LL = Q.layer[Q.n_layers - 1];
    const uint32_t C = Q.heads ? LL.rows / 2u : LL.rows;      // targets per row; a scale head's last layer has 2 C rows
    for (uint32_t bi = 0; bi < 2u; ++bi) {
        const uint32_t j = blockIdx.y * 8u + wave * 2u + bi;
        if (j >= V.rows_pass) continue;
        const uint32_t m = V.m0 + j;
        const bool live = n < Q.n_local && m < V.M;
        auto Y = [&](uint32_t buf, uint32_t u) -> float& {
            return LDSW ? ya[(size_t)(buf * V.max_width + u) * 256u]
                        : V.act[((size_t)(buf * V.max_width + u) * V.rows_pass + j) * Q.n_pad + n];
        };
        uint32_t cur = 0;
        for (uint32_t h = 0; h < L1.rows; ++h) {
            float v = V.a1[(size_t)j * Q.NC + (size_t)h * Q.n_pad + n];
            if (L1.b0 != 0xFFFFFFFFu) v += W(L1.b0 - Q.R1 + h);
            Y(cur, h) = bnn_act(L1.act, v, Q.act_p[0]);
        }
        for (uint32_t l = 1; l < Q.n_layers; ++l) {
            const BnnLayerDev L = Q.layer[l];
            for (uint32_t i = 0; i < L.rows; ++i) {
                float s = L.b0 != 0xFFFFFFFFu ? W(L.b0 - Q.R1 + i) : 0.0f;
                // (unrolled by four: eight reads in flight in front of four dependent FMAs, the additions in the same order)
#pragma unroll 4
                for (uint32_t k = 0; k < L.cols; ++k) s += W(L.w0 - Q.R1 + i * L.cols + k) * Y(cur, k);
                Y(cur ^ 1u, i) = bnn_act(L.act, s, Q.act_p[l]);
            }
            cur ^= 1u;
        }
        if (!live) continue;
        const size_t at = ((size_t)n * V.M + m) * C;
        float* const pp = V.p + (size_t)n * V.p_stride + (size_t)j * C;
        // (a scale head: z_out is [n][M][2 C], the loc and then sigma itself; sigma of the pass stays in V.sig for the draw and the reduce)
        float* const sp = Q.heads ? V.sig + (size_t)n * V.sig_stride + (size_t)j * C : nullptr;
        if (Q.heads) {
            for (uint32_t c = 0; c < C; ++c) {
                float ds;
                sp[c] = bnn_head_sigma(Q.heads, Q.head_a, Q.head_b, Y(cur, C + c), ds);
                if (V.z_out) { V.z_out[2u * at + c] = Y(cur, c); V.z_out[2u * at + C + c] = sp[c]; }
            }
        } else if (V.z_out) for (uint32_t c = 0; c < C; ++c) V.z_out[at + c] = Y(cur, c);
        u32x4 x = {0u, 0u, 0u, 0u};
        if (V.draw_out && Q.likelihood != BSVI_LIK_NORMAL)
            x = philox4x32(Q.sample_base + n, m, Q.offset_lo, Q.offset_hi, Q.seed_lo ^ BNN_KEY_PREDICT, Q.seed_hi);
        if (Q.likelihood == BSVI_LIK_NORMAL) {
            for (uint32_t c = 0; c < C; ++c) pp[c] = Y(cur, c);
            if (V.draw_out) {
                for (uint32_t c0 = 0; c0 < C; c0 += 4u) {
                    const u32x4 w = philox4x32(Q.sample_base + n, m, Q.offset_lo, Q.offset_hi, Q.seed_lo ^ BNN_KEY_PREDICT, Q.seed_hi ^ (c0 >> 2));
                    float e[4];
                    if (Q.family == BSVI_DIST_NORMAL) {
                        box_muller_fast(w.x, w.y, e[0], e[1]);
                        box_muller_fast(w.z, w.w, e[2], e[3]);
                    } else {
                        // Laplace | Cauchy: ONE word per output, word c & 3 of the call the Normal's output c reads (philox.h) — a word of
                        // its own for every output, so that no two outputs of a row share a draw.  The library's draws of the two
                        // families (dist_math.h, sample_from_noise_generic): Laplace -sign(v) log1p(-|v|) of the uniform base noise v
                        const uint32_t wd[4] = {w.x, w.y, w.z, w.w};
                        for (uint32_t k = 0; k < 4u; ++k) {
                            if (Q.family == BSVI_DIST_LAPLACE) {
                                const float v = laplace_noise(wd[k]);
                                e[k] = -(v > 0.0f ? 1.0f : (v < 0.0f ? -1.0f : 0.0f)) * log1pf(-fabsf(v));
                            } else {
                                e[k] = cauchy_noise(wd[k]);
                            }
                        }
                    }
                    for (uint32_t c = c0; c < C && c < c0 + 4u; ++c) V.draw_out[at + c] = Y(cur, c) + (Q.heads ? sp[c] : V.sg[c]) * e[c - c0];
                }
            }
        } else if (Q.likelihood == BSVI_LIK_CATEGORICAL) {
            // log-softmax as bnn_upper does it, then expf: the probabilities as they are stored
            float mx = -INFINITY;
            for (uint32_t c = 0; c < C; ++c) mx = fmaxf(mx, Y(cur, c));
            float se = 0.0f;
            for (uint32_t c = 0; c < C; ++c) se += expf(Y(cur, c) - mx);
            const float lse = mx + logf(se), u = u01(x.x);
            float cum = 0.0f;
            uint32_t pick = C - 1u;
            bool found = false;
            for (uint32_t c = 0; c < C; ++c) {
                const float pc = expf(Y(cur, c) - lse);
                pp[c] = pc;
                cum += pc;
                if (!found && cum >= u) { pick = c; found = true; }
            }
            if (V.draw_out) for (uint32_t c = 0; c < C; ++c) V.draw_out[at + c] = c == pick ? 1.0f : 0.0f;
        } else {
            const float pb = sigmoidf_(Y(cur, 0));
            pp[0] = pb;
            if (V.draw_out) V.draw_out[at] = u01(x.x) < pb ? 1.0f : 0.0f;
        }
    }
}

// mean over the samples of p (and, Normal: the population variance of the loc about that mean, plus sigma_c^2) for the rows of a pass:
// one thread per (row j, output c), the samples in order n = 0, 1, ... in double precision — no atomics, and nothing that depends on
// how the rows were cut into passes.  grid: ceil(rows * C / 256), block 256
__global__ void __launch_bounds__(256) bnn_predict_reduce(const BParams Q, const BnnPredict V, const uint32_t rows) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x, C = Q.C;
    if (i >= rows * C) return;
    const uint32_t c = i % C;
    const float* const src = V.p + i;
    double s = 0.0;
    for (uint32_t n = 0; n < Q.n_local; ++n) s += (double)src[(size_t)n * V.p_stride];
    const double mean = s / (double)Q.n_local;
    const size_t at = (size_t)V.m0 * C + i;
    if (V.mean_out) V.mean_out[at] = (float)mean;
    if (V.var_out && Q.heads) {
        // the law of total variance: + the mean over the samples of sigma^2 — a second sum in sample order, inside the loop of the first
        // (784-20-(1+1), 512 rows, 1 024 samples, us per call: a loop of its own for sigma 840, this 722, the constant-sigma network of
        // the same widths 565; the loads of eight samples issued in front of their additions 864 — profiles/r19/bnn_heads.txt)
        const float* const sg = V.sig + i;
        double q = 0.0, s2 = 0.0;
        for (uint32_t n = 0; n < Q.n_local; ++n) {
            const double d = (double)src[(size_t)n * V.p_stride] - mean, sn = (double)sg[(size_t)n * V.sig_stride];
            q += d * d; s2 += sn * sn;
        }
        // (a Laplace likelihood's variance is 2 sigma^2)
        if (Q.family == BSVI_DIST_LAPLACE) V.var_out[at] = (float)(q / (double)Q.n_local + 2.0 * s2 / (double)Q.n_local);
        else V.var_out[at] = (float)(q / (double)Q.n_local + s2 / (double)Q.n_local);
    } else if (V.var_out) {
        double q = 0.0;
        for (uint32_t n = 0; n < Q.n_local; ++n) { const double d = (double)src[(size_t)n * V.p_stride] - mean; q += d * d; }
        const double sigma = (double)V.sg[c];
        if (Q.family == BSVI_DIST_LAPLACE) V.var_out[at] = (float)(q / (double)Q.n_local + 2.0 * sigma * sigma);
        else V.var_out[at] = (float)(q / (double)Q.n_local + sigma * sigma);
    }
}

static uint32_t bnn_max_width(const bsvi_bnn* p) {
    uint32_t w = 0;
    for (const bsvi_bnn_layer& l : p->layers) w = std::max(w, l.rows);
    return w;
}

static bsvi_bnn_select::PredictLayout bnn_predict_layout(const bsvi_bnn* p, uint32_t n_local, uint32_t n_rows, uint32_t rows_per_pass) {
    // (a scale head: the p region is twice as large — p of a pass [n][rows][C] as ever, then sigma of the pass [n][rows][C])
    return bsvi_bnn_select::predict_layout(p->R, p->Rs, p->P, p->heads ? 2u * p->C : p->C, p->H1, bnn_max_width(p), n_local, n_rows, rows_per_pass);
}

extern "C" size_t bsvi_bnn_predict_args_size(void) { return sizeof(bsvi_bnn_predict_args); }

extern "C" size_t bsvi_bnn_predict_workspace_bytes(const bsvi_bnn* p, uint32_t n_samples_local, uint32_t n_rows, uint32_t rows_per_pass) {
    if (!p || !n_samples_local || !n_rows || rows_per_pass % 32u) return 0;
    return bnn_predict_layout(p, n_samples_local, n_rows, rows_per_pass).total;
}

extern "C" uint32_t bsvi_bnn_predict_rows_per_pass(const bsvi_bnn* p, uint32_t n_samples_local, uint32_t n_rows, uint32_t rows_per_pass) {
    if (!p || !n_samples_local || !n_rows || rows_per_pass % 32u) return 0;
    return bnn_predict_layout(p, n_samples_local, n_rows, rows_per_pass).rows_pass;
}

extern "C" int bsvi_bnn_predict_lds(const bsvi_bnn* p) {
    return p ? (bsvi_bnn_select::predict_lds(p->Rs, bnn_max_width(p)) ? 1 : 0) : -1;
}

static thread_local int bnn_predict_last_exact = -1;
extern "C" int bsvi_bnn_predict_last_exact(void) { return bnn_predict_last_exact; }

extern "C" int bsvi_bnn_predict(const bsvi_bnn* p, const bsvi_bnn_predict_args* a) {
    // every check in front of any device work
    if (!a) return fail(BSVI_ERR_INVALID, "bsvi_bnn_predict: null argument");
    BSVI_CHECK_STRUCT(a, bsvi_bnn_predict_args);
    if (!a->x_dev) return fail(BSVI_ERR_INVALID, "bsvi_bnn_predict: x_dev is null");
    if (!a->n_rows) return fail(BSVI_ERR_INVALID, "bsvi_bnn_predict: n_rows is 0");
    if (!a->n_samples_local) return fail(BSVI_ERR_INVALID, "bsvi_bnn_predict: zero samples");
    if (a->rows_per_pass % 32u) return fail(BSVI_ERR_INVALID, "bsvi_bnn_predict: rows_per_pass must be a multiple of 32 (0: the default)");
    if (!a->workspace_dev) return fail(BSVI_ERR_INVALID, "bsvi_bnn_predict: workspace_dev is null");
    if (!p) return fail(BSVI_ERR_INVALID, "bsvi_bnn_predict: null handle");
    if (!a->params_dev && p->d.n_params) return fail(BSVI_ERR_INVALID, "bsvi_bnn_predict: params_dev is null");
    if (a->var_out && p->d.likelihood != BSVI_LIK_NORMAL)
        return fail(BSVI_ERR_INVALID, "bsvi_bnn_predict: var_out is for the Normal likelihood (a classifier's variance is p (1 - p) of mean_out)");
    if (a->var_out && p->family == BSVI_DIST_CAUCHY) return fail(BSVI_ERR_UNSUPPORTED, "bsvi_bnn_predict: the Cauchy likelihood has no variance");
    const bsvi_bnn_select::PredictLayout L = bnn_predict_layout(p, a->n_samples_local, a->n_rows, a->rows_per_pass);
    if ((uint64_t)L.NC * (uint64_t)std::max(p->Kp, L.rows_pass) >= (1ull << 31))
        return fail(BSVI_ERR_UNSUPPORTED, "bsvi_bnn_predict: number_samples x hidden units x max(features, rows_per_pass) beyond the 32-bit index range of the product kernels");
    if ((uint64_t)a->n_samples_local * a->n_rows * p->C >= (1ull << 40))
        return fail(BSVI_ERR_UNSUPPORTED, "bsvi_bnn_predict: number_samples x rows x outputs too large");
    const uint32_t max_width = bnn_max_width(p);
    const bool lds = bsvi_bnn_select::predict_lds(p->Rs, max_width);
    hipStream_t s = (hipStream_t)a->stream;
    char* ws = (char*)a->workspace_dev;

    BParams Q;
    memset(&Q, 0, sizeof Q);
    Q.uniform = p->uniform; Q.consts = p->consts; Q.params = a->params_dev; Q.row_uniform = p->row_uniform;
    Q.n_layers = p->d.n_layers;
    for (uint32_t l = 0; l < Q.n_layers; ++l) {
        const bsvi_bnn_layer& S = p->layers[l];
        BnnLayerDev& D = Q.layer[l];
        D.rows = S.rows; D.cols = S.cols; D.w0 = S.weight_row0; D.b0 = S.bias_row0; D.act = S.activation;
    }
    memcpy(Q.act_p, p->act_p, sizeof Q.act_p);
    Q.R = p->R; Q.R1 = p->R1; Q.Rs = p->Rs ? p->Rs : 1; Q.P = p->P; Q.C = p->C; Q.H1 = p->H1;
    Q.Kp = p->Kp; Q.P_ld = p->P_ld; Q.n_local = a->n_samples_local; Q.n_pad = L.n_pad; Q.n_global = a->n_samples_local;
    Q.sample_base = a->sample_base; Q.NC = L.NC; Q.likelihood = p->d.likelihood;
    Q.LC = p->LC; Q.scale_u = p->scale_u; Q.scale_stride = p->scale_stride;
    Q.heads = p->heads; Q.head_a = p->head_a; Q.head_b = p->head_b; Q.family = p->family;
    Q.seed_lo = (uint32_t)a->seed; Q.seed_hi = (uint32_t)(a->seed >> 32); Q.offset_lo = (uint32_t)a->offset; Q.offset_hi = (uint32_t)(a->offset >> 32);
    Q.noise_in = a->noise_dev; Q.noise_out = a->noise_out;
    Q.rowp = (float*)(ws + L.rowp); Q.Wsm = (float*)(ws + L.Wsm);
    Q.W1f = (float*)(ws + L.W1); Q.Wp = (uint16_t*)(ws + L.W1);
    Q.pv_part = (float*)(ws + L.part); Q.qv_part = Q.pv_part + (size_t)L.row_chunks * L.n_pad;
    Q.Xb = (float*)(ws + L.X); Q.Xb_bf = (uint16_t*)(ws + L.X);
    Q.row_chunks = L.row_chunks;
    Q.row_kind = p->row_kind; Q.row_point = p->row_point;
    p->launched.store(true);

    BnnPredict V;
    memset(&V, 0, sizeof V);
    V.x_new = a->x_dev; V.M = a->n_rows; V.rows_pass = L.rows_pass; V.a1 = (const float*)(ws + L.a1); V.act = (float*)(ws + L.act);
    V.max_width = max_width; V.sg = (const float*)(ws + L.sg); V.flag = (uint32_t*)(ws + L.flag);
    V.z_out = a->z_out; V.draw_out = a->draw_out; V.mean_out = a->mean_out; V.var_out = a->var_out;

    // exact data?  decided for the rows handed in, on the device, read back once (BSVI_DENSE_XGEMM=0: the f32 kernels, as at create)
    bool exact = false;
    {
        const char* xe = getenv("BSVI_DENSE_XGEMM");
        if (!(xe && xe[0] == '0')) {
            const uint32_t one = 1u;
            uint32_t flag = 0u;
            const size_t n_values = (size_t)a->n_rows * p->P;
            HIP_TRY(hipMemcpyAsync(V.flag, &one, 4, hipMemcpyHostToDevice, s));
            hipLaunchKernelGGL(bnn_predict_exact, dim3((unsigned)std::min<size_t>((n_values + 255) / 256, 1024)), dim3(256), 0, s, a->x_dev, n_values, V.flag);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(&flag, V.flag, 4, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            exact = flag == 1u;
        }
    }
    Q.exact = exact ? 1u : 0u;
    bnn_predict_last_exact = exact ? 1 : 0;
    if (lds) {
        static std::mutex mu;
        static size_t asked = 0;
        const size_t bytes = bsvi_bnn_select::predict_lds_bytes(p->Rs, max_width);
        std::lock_guard<std::mutex> lock(mu);
        if (bytes > asked) {
            HIP_TRY(hipFuncSetAttribute((const void*)bnn_predict_fwd<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
            asked = bytes;
        }
    }
    const uint32_t head_n = std::max(Q.R, Q.C);
    hipLaunchKernelGGL(bnn_predict_head, dim3((head_n + 255) / 256), dim3(256), 0, s, Q, V);
    // (the prior partials of the draw are written and never read: the MIXED instantiation all the same, so that the two stay one kernel each)
    bnn_launch_draw(p, Q, L.row_chunks, s);
    HIP_TRY(hipGetLastError());
    const uint32_t gy = (std::max(Q.Kp, Q.P_ld) + 255) / 256;
    for (uint32_t m0 = 0; m0 < a->n_rows; m0 += L.rows_pass) {
        const uint32_t rows = std::min(L.rows_pass, a->n_rows - m0);
        V.m0 = m0;
        if (a->p_out) { V.p = a->p_out + (size_t)m0 * p->C; V.p_stride = (size_t)a->n_rows * p->C; }
        else { V.p = (float*)(ws + L.p); V.p_stride = (size_t)L.rows_pass * p->C; }
        if (p->heads) { V.sig_stride = (size_t)L.rows_pass * p->C; V.sig = (float*)(ws + L.p) + (size_t)a->n_samples_local * V.sig_stride; }
        hipLaunchKernelGGL(bnn_predict_gather, dim3(L.rows_pass * gy), dim3(256), 0, s, Q, V, gy);
        int rc;
        if (exact) rc = bsvi_xgemm_nt(Q.Xb_bf, nullptr, Q.Wp, (long)Q.NC * Q.Kp, const_cast<float*>(V.a1), (int)Q.NC, (int)L.rows_pass, (int)Q.NC, (int)Q.Kp, s);
        else rc = bsvi_gemm_f32(0, Q.Xb, (int)Q.P_ld, Q.W1f, (int)Q.P_ld, const_cast<float*>(V.a1), (int)Q.NC, (int)L.rows_pass, (int)Q.NC, (int)Q.P, s);
        if (rc) return rc;
        const dim3 grid(Q.n_pad / 64, (L.rows_pass + 7) / 8);
        if (lds) hipLaunchKernelGGL(bnn_predict_fwd<true>, grid, dim3(256), bsvi_bnn_select::predict_lds_bytes(p->Rs, max_width), s, Q, V);
        else hipLaunchKernelGGL(bnn_predict_fwd<false>, grid, dim3(256), 0, s, Q, V);
        if (a->mean_out || a->var_out)
            hipLaunchKernelGGL(bnn_predict_reduce, dim3((rows * p->C + 255) / 256), dim3(256), 0, s, Q, V, rows);
        HIP_TRY(hipGetLastError());
    }
    return BSVI_OK;
}
