// bnn_particles.inc — a particle ensemble through the kernels of bnn_kernel.inc (included by elbo_kernel.hip behind it).
//
// Stein variational gradient descent keeps N point estimates of one network (inference.SteinVariationalGradientDescent): N weight sets
// theta[n], and of each the loss -log p(theta_n, minibatch) and its gradient.  The kernels of a Bayesian neural network already carry a
// weight set per SAMPLE through both products, the middle kernel and the epilogue, and hold the gradient of every sample before anything
// is summed; so the particles ride the sample axis, n_local = N, and an evaluation of all of them is
//   bnn_head_gather      as every iteration: the rows' prior parameters, the minibatch (ONE minibatch, shared by the particles)
//   bnn_particles_in     in the place of bnn_draw: theta[n][r] out of the [N][ld] table into the operands of the first product and
//                        the small tensors; the particle's prior value; the rows' constants
//   product 1, the middle kernel, product 2      bnn_launch_products, untouched
//   bnn_epilogue         f_n per particle (no row sums in front of it: no gradient is summed over n)
//   bnn_particles_out    in the place of bnn_row_sums: grad[n][r] = -(G[n][r] + prior_weight d log p(theta[n][r]) / d theta) into a second
//                        [N][ld] table, loss[n] = -f_n
// The table's row order is the latent vector's (weights1 first, r = h P + p; then the other tensors), D = R columns of ld >= R; columns
// R .. ld are neither read nor written.  No atomics and a fixed order of every sum: two calls leave the same bits.

struct BnnParticles {
    const float* theta; float* grad; float* loss;
    const float* fval;              // [n_pad] f_n as bnn_epilogue leaves it (fvalue_out)
    uint64_t ld;
    uint32_t theta16, grad16;       // the table's rows start on 16 bytes (ld a multiple of 4, the base aligned): 16-byte loads / stores
};

// the prior parameters {loc, scale} of the rows of quad g (rowp's arrays 2 and 3), as bnn_draw reads them: 16-byte loads where the
// array's offset allows, 8-byte where it is even, else masked scalars (a row past R: scale 1)
__device__ __forceinline__ void bnn_prior_quad(const BParams& Q, const uint32_t g, float mu0[4], float s0[4]) {
    const bool whole = 4u * g + 3u < Q.R, base16 = ((uintptr_t)Q.rowp & 15u) == 0u;
#pragma unroll
    for (int a = 2; a < 4; ++a) {
        float* const out = a == 2 ? mu0 : s0;
        const size_t at = (size_t)a * Q.R + 4u * g;
        if (whole && base16 && (at & 3u) == 0u) {
            const xf_f32x4 v = *reinterpret_cast<const xf_f32x4*>(Q.rowp + at);
#pragma unroll
            for (int j = 0; j < 4; ++j) out[j] = v[j];
        } else if (whole && base16 && (at & 1u) == 0u) {
            const float2 v0 = *reinterpret_cast<const float2*>(Q.rowp + at), v1 = *reinterpret_cast<const float2*>(Q.rowp + at + 2);
            out[0] = v0.x; out[1] = v0.y; out[2] = v1.x; out[3] = v1.y;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) out[j] = (4u * g + j < Q.R) ? Q.rowp[at + j] : 1.0f;
        }
    }
}

// theta of rows 4g .. 4g + 3 of particle n (0 for a row past R)
__device__ __forceinline__ void bnn_theta_quad(const BParams& Q, const BnnParticles& T, const uint32_t n, const uint32_t g, float w[4]) {
    const float* const th = T.theta + (size_t)n * T.ld + 4u * (size_t)g;
    if (T.theta16 && 4u * g + 3u < Q.R) {
        const xf_f32x4 v = *reinterpret_cast<const xf_f32x4*>(th);
#pragma unroll
        for (int j = 0; j < 4; ++j) w[j] = v[j];
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) w[j] = (4u * g + j < Q.R) ? th[j] : 0.0f;
    }
}

// One wave = (chunk of 64 row quads, particle), lanes along the rows — bnn_draw's split, so that pv_part has bnn_draw's chunks and
// bnn_epilogue adds them as it does: the table is read as consecutive 16-byte quads along the lane index, the pieces of weights1 leave as
// consecutive 8-byte stores along p, the small tensors as consecutive floats; nothing goes through LDS.  No noise: w = theta, qv_part = 0.
// The waves of particle 0 also leave the sample-independent terms of f, one pair per quad where bnn_row_sums leaves them (hpart): a
// point row's, prior_weight times the constant of its prior's kind, in double precision and row order (bnn_row_terms_sums); log q none.
// grid: row_chunks x ceil(n_pad / 4), block 256
__global__ void __launch_bounds__(256) bnn_particles_in(const BParams Q, const BnnParticles T) {
    const uint32_t chunk = blockIdx.x, lane = threadIdx.x & 63u, n = blockIdx.y * 4u + (threadIdx.x >> 6), g = chunk * 64u + lane;
    if (n >= Q.n_pad) return;
    const bool live = n < Q.n_local;
    const uint32_t quads = (Q.R + 3u) / 4u;
    float pv = 0.0f;
    if (g < quads) {
        const uint32_t kinds = *reinterpret_cast<const uint32_t*>(Q.row_kind + 4u * (size_t)g);      // (a byte per row, padded to the quad)
        float w4[4] = {0.0f, 0.0f, 0.0f, 0.0f}, mu0[4], s0[4];
        uint16_t hi[4] = {0, 0, 0, 0}, mid[4] = {0, 0, 0, 0}, lo[4] = {0, 0, 0, 0};
        if (live) {
            bnn_theta_quad(Q, T, n, g, w4);
            bnn_prior_quad(Q, g, mu0, s0);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t r = 4u * g + j;
            if (r >= Q.R) continue;
            if (live) pv += bnn_prior_value((kinds >> (8 * j)) & 0xFFu, (w4[j] - mu0[j]) / s0[j]);
            if (r >= Q.R1) Q.Wsm[(size_t)n * Q.Rs + (r - Q.R1)] = w4[j];
            if (Q.exact) dense_split3(w4[j], hi[j], mid[j], lo[j]);
        }
        const uint32_t r0 = 4u * g;
        if (r0 < Q.R1) {                          // (P is a multiple of 4: a quad of weights1 stays in one row h)
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
        if (n == 0u) {
            double h4 = 0.0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t r = 4u * g + j, kind = (kinds >> (8 * j)) & 0xFFu;
                if (r >= Q.R) continue;
                const double s0d = bnn_uniform_value_d(Q, Q.row_uniform[3 * (size_t)Q.R + r]);
                h4 += (double)Q.prior_weight * (kind == BSVI_DIST_LAPLACE ? -log(2.0 * s0d) : (kind == BSVI_DIST_CAUCHY ? -1.14472988584940017414 - log(s0d)
                                                                                               : -log(s0d) - 0.91893853320467274178));
            }
            Q.hpart[g] = h4; Q.hpart[quads + g] = 0.0;
        }
    }
    pv = wave_sum(pv);
    if (lane == 0) { Q.pv_part[(size_t)chunk * Q.n_pad + n] = pv; Q.qv_part[(size_t)chunk * Q.n_pad + n] = 0.0f; }
}

// the gradient of a particle's loss with respect to one weight: G = d f / d w of the likelihood, t = d log p(w) / d w of the row's prior in
// u = (w - mu0) / s0 —  Normal -u / s0,  Laplace -sign(w - mu0) / s0 with sign(0) = 0 (torch's abs backward),  Cauchy -2 u / ((1 + u^2) s0),
// the per-sample t of bnn_row_sums<MIXED> — and the loss is -f
__device__ __forceinline__ float bnn_particle_grad(const BParams& Q, const uint32_t kind, const float w, const float mu0, const float s0, const float G) {
    const float is0 = 1.0f / s0, dw = w - mu0, u = dw * is0;
    const float sg = dw > 0.0f ? 1.0f : (dw < 0.0f ? -1.0f : 0.0f);
    const float t = (kind == BSVI_DIST_LAPLACE ? -sg : (kind == BSVI_DIST_CAUCHY ? -2.0f * u / (1.0f + u * u) : -u)) * is0;
    return -(G + Q.prior_weight * t);
}

// rows 4g .. 4g + 3 of particle n from their four G: theta and the prior parameters as bnn_particles_in read them, one 16-byte store
// (masked scalars where the table's rows are not aligned, or for the quad that holds row R)
__device__ __forceinline__ void bnn_particle_store(const BParams& Q, const BnnParticles& T, const uint32_t n, const uint32_t g, const float G[4]) {
    const uint32_t kinds = *reinterpret_cast<const uint32_t*>(Q.row_kind + 4u * (size_t)g);
    float w[4], mu0[4], s0[4], v[4];
    bnn_theta_quad(Q, T, n, g, w);
    bnn_prior_quad(Q, g, mu0, s0);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = bnn_particle_grad(Q, (kinds >> (8 * j)) & 0xFFu, w[j], mu0[j], s0[j], G[j]);
    float* const out = T.grad + (size_t)n * T.ld + 4u * (size_t)g;
    if (T.grad16 && 4u * g + 3u < Q.R) {
        *reinterpret_cast<xf_f32x4*>(out) = xf_f32x4{v[0], v[1], v[2], v[3]};
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) if (4u * g + j < Q.R) out[j] = v[j];
    }
}

constexpr uint32_t BNP_TILE = 64, BNP_STRIDE = BNP_TILE + 1;

// grid: tile_blocks + flat_blocks, block 256.
// The first tile_blocks workgroups (the exact path: GT[p][(h, n)], n fastest, against the table's p fastest) transpose weights1's
// gradients: a workgroup = (64 columns p, one hidden unit h, 64 particles) through tile[p][n], a row 65 floats.  In: lanes along n, wave w
// the columns 16 w .. 16 w + 15 — 256-byte reads, and a half-wave's 32 stores fall on 32 banks (65 p + n).  Out: a lane takes four
// consecutive p of one particle, lane = (a & 7) + 8 b + 32 (a >> 3) for the quad a of 16 and the particle b of 4: a half-wave holds the
// quads a0 .. a0 + 7 of four particles, whose four reads (k = 0 .. 3) fall on banks 4 a + b + k + const, 32 different ones, and each
// particle's row leaves as two runs of 128 bytes.  Four passes of 4 particles per wave.
// The other workgroups, a thread per (particle, row quad), lanes along the rows: the f32 path's GT[(h, n)][p] (quads from 0) and the
// small tensors' gsm[n][Rs] (both paths) are copies of four consecutive floats with the prior term added in registers; thread i < N also
// writes loss[i] = -f_i.
__global__ void __launch_bounds__(256) bnn_particles_out(const BParams Q, const BnnParticles T, const uint32_t tile_blocks, const uint32_t tiles_p) {
    __shared__ float tile[BNP_TILE * BNP_STRIDE];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (blockIdx.x < tile_blocks) {
        const uint32_t tp = blockIdx.x % tiles_p, hz = blockIdx.x / tiles_p, h = hz % Q.H1, n0 = (hz / Q.H1) * BNP_TILE, p0 = tp * BNP_TILE;
#pragma unroll 4
        for (uint32_t k = 0; k < 16u; ++k) {
            const uint32_t pl = wave * 16u + k;
            // (n0 + lane < n_pad always: n_pad is a multiple of 64; the pad particles' columns hold what the product left, never written out)
            if (p0 + pl < Q.P) tile[pl * BNP_STRIDE + lane] = Q.GT[(size_t)(p0 + pl) * Q.NC + (size_t)h * Q.n_pad + n0 + lane];
        }
        __syncthreads();
        const uint32_t a = (lane & 7u) + 8u * (lane >> 5), b = (lane >> 3) & 3u, p = p0 + 4u * a;
#pragma unroll
        for (uint32_t pass = 0; pass < 4u; ++pass) {
            const uint32_t nl = wave * 16u + pass * 4u + b, n = n0 + nl;
            if (n >= Q.n_local || p >= Q.P) continue;      // (P is a multiple of 4: a quad is whole or absent)
            float G[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) G[k] = tile[(4u * a + k) * BNP_STRIDE + nl];
            bnn_particle_store(Q, T, n, (h * Q.P + p) / 4u, G);
        }
        return;
    }
    const uint32_t quads = (Q.R + 3u) / 4u, q0 = Q.exact ? Q.R1 / 4u : 0u, nq = quads - q0;
    const size_t i = (size_t)(blockIdx.x - tile_blocks) * 256u + threadIdx.x;
    if (i < Q.n_local) T.loss[i] = -T.fval[i];
    if (i >= (size_t)Q.n_local * nq) return;
    const uint32_t n = (uint32_t)(i / nq), g = q0 + (uint32_t)(i - (size_t)n * nq), r0 = 4u * g;
    float G[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (r0 < Q.R1) {
        const uint32_t h = r0 / Q.P, p = r0 - h * Q.P;
        const xf_f32x4 v = *reinterpret_cast<const xf_f32x4*>(Q.GT + ((size_t)h * Q.n_pad + n) * Q.P_ld + p);      // (P_ld = P: a multiple of 4)
#pragma unroll
        for (int j = 0; j < 4; ++j) G[j] = v[j];
    } else {
        const size_t at = (size_t)n * Q.Rs + (r0 - Q.R1);
        if ((at & 3u) == 0u && r0 + 3u < Q.R) {
            const xf_f32x4 v = *reinterpret_cast<const xf_f32x4*>(Q.gsm + at);
#pragma unroll
            for (int j = 0; j < 4; ++j) G[j] = v[j];
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) if (r0 + j < Q.R) G[j] = Q.gsm[at + j];
        }
    }
    bnn_particle_store(Q, T, n, g, G);
}

// ---- host side -------------------------------------------------------------------------------------------------------------
constexpr uint32_t BNN_MIN_PARTICLES = 2, BNN_MAX_PARTICLES = 256;

// what a handle must be to carry particles; every refusal names the feature or the limit
static int bnn_particles_check(const bsvi_bnn* p, const uint32_t n_particles) {
    if (n_particles < BNN_MIN_PARTICLES || n_particles > BNN_MAX_PARTICLES)
        return fail(BSVI_ERR_INVALID, "bsvi_bnn_particles: n_particles is " + std::to_string(n_particles) + ", served are 2 .. 256 particles");
    if (!p) return fail(BSVI_ERR_INVALID, "bsvi_bnn_particles: null handle");
    bool all_point = p->row_point && p->row_point_host.size() == p->R;
    for (uint32_t r = 0; all_point && r < p->R; ++r) all_point = p->row_point_host[r] != 0u;
    if (!all_point)
        return fail(BSVI_ERR_UNSUPPORTED, "bsvi_bnn_particles: not every row is a point row (a particle is a point estimate of every tensor: bsvi_bnn_set_point_rows)");
    if (p->n_latents) return fail(BSVI_ERR_UNSUPPORTED, "bsvi_bnn_particles: scale latents are not served (bsvi_bnn_set_scale_latents)");
    if (p->scale_learn) return fail(BSVI_ERR_UNSUPPORTED, "bsvi_bnn_particles: a learnable sigma is not served (bsvi_bnn_create_normal_learnable)");
    if (p->heads) return fail(BSVI_ERR_UNSUPPORTED, "bsvi_bnn_particles: a scale head is not served (bsvi_bnn_create_normal_heads)");
    if (p->d.estimator != BSVI_EST_PATHWISE) return fail(BSVI_ERR_UNSUPPORTED, "bsvi_bnn_particles: the BlackBox estimator is not served (a particle has no log q)");
    // the particles differ in weights1: both products per particle.  A handle that has not chosen yet chooses here, for good; one whose
    // launches took the shared first layer already is refused
    int undecided = 0;
    if (!p->shared_state.compare_exchange_strong(undecided, -1) && undecided > 0)
        return fail(BSVI_ERR_UNSUPPORTED, "bsvi_bnn_particles: the handle took the shared-first-layer plan (bsvi_bnn_shared_first): particles need a handle of their own");
    return BSVI_OK;
}

// the workspace of bsvi_bnn_fwd_bwd at n_particles samples, then f_n [n_pad]
extern "C" size_t bsvi_bnn_particles_workspace_bytes(const bsvi_bnn* p, uint32_t n_particles) {
    if (bnn_particles_check(p, n_particles)) return 0;
    const BnnLayout L = bnn_layout(p, n_particles);
    return L.total + align_up((size_t)L.n_pad * 4, 256);
}

extern "C" int bsvi_bnn_particles_fwd_bwd(const bsvi_bnn* p, const bsvi_bnn_args* a, const float* theta_dev, float* grad_dev, float* loss_dev,
                                          uint32_t n_particles, uint64_t ld, void* stream) {
    int rc = bnn_particles_check(p, n_particles);
    if (rc) return rc;
    if (!a || !theta_dev || !grad_dev || !loss_dev) return fail(BSVI_ERR_INVALID, "bsvi_bnn_particles_fwd_bwd: null argument");
    if (ld < p->R) return fail(BSVI_ERR_INVALID, "bsvi_bnn_particles_fwd_bwd: ld is " + std::to_string(ld) + ", a particle has " + std::to_string(p->R) + " values");
    if ((uint64_t)n_particles * ld >= (1ull << 31)) return fail(BSVI_ERR_UNSUPPORTED, "bsvi_bnn_particles_fwd_bwd: n_particles x ld beyond 2^31");
    if (a->f_weight_dev || a->q_weight_dev)
        return fail(BSVI_ERR_UNSUPPORTED, "bsvi_bnn_particles_fwd_bwd: custom estimators are not served (f_weight_dev / q_weight_dev)");
    if (theta_dev == grad_dev) return fail(BSVI_ERR_INVALID, "bsvi_bnn_particles_fwd_bwd: grad_dev may not be theta_dev");
    bsvi_bnn_args aa = *a;      // the particles are the samples: no noise in or out, one rank
    aa.n_samples_local = aa.n_samples_global = n_particles; aa.sample_base = 0;
    aa.noise_dev = nullptr; aa.noise_out_dev = nullptr; aa.logq_out_dev = nullptr;
    BParams Q; BnnLayout L;
    rc = bnn_fill(p, &aa, Q, L);
    if (rc) return rc;
    BnnParticles T;
    T.theta = theta_dev; T.grad = grad_dev; T.loss = loss_dev; T.ld = ld;
    T.fval = (const float*)((char*)a->workspace_dev + L.total);
    T.theta16 = (ld % 4u == 0u && ((uintptr_t)theta_dev & 15u) == 0u) ? 1u : 0u;
    T.grad16 = (ld % 4u == 0u && ((uintptr_t)grad_dev & 15u) == 0u) ? 1u : 0u;
    Q.fvalue_out = const_cast<float*>(T.fval);
    const hipStream_t s = (hipStream_t)stream;
    bnn_launch_head(p, Q, s);
    hipLaunchKernelGGL(bnn_particles_in, dim3(L.row_chunks, (Q.n_pad + 3u) / 4u), dim3(256), 0, s, Q, T);
    rc = bnn_launch_products(p, Q, s);
    if (rc) return rc;
    hipLaunchKernelGGL(bnn_epilogue, dim3(1), dim3(1024), 0, s, Q, L.row_blocks);
    const uint32_t tiles_p = (Q.P + BNP_TILE - 1u) / BNP_TILE, tile_blocks = Q.exact ? tiles_p * Q.H1 * (Q.n_pad / BNP_TILE) : 0u;
    const uint32_t quads = (Q.R + 3u) / 4u, nq = quads - (Q.exact ? Q.R1 / 4u : 0u);
    const size_t flat = std::max((size_t)Q.n_local * nq, (size_t)Q.n_local);
    hipLaunchKernelGGL(bnn_particles_out, dim3(tile_blocks + (uint32_t)((flat + 255u) / 256u)), dim3(256), 0, s, Q, T, tile_blocks, tiles_p);
    HIP_TRY(hipGetLastError());
    return BSVI_OK;
}
