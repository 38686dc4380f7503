// dense_particles.inc — a particle ensemble of a dense-link model (logistic regression) in ONE fused kernel (included by
// elbo_kernel.hip behind bnn_particles.inc; DESIGN.md 4.8).
//
// Stein variational gradient descent keeps N point estimates theta[n] of the weight matrix [C][P] (rows r = c P + p) and needs of each
//   loss[n]    = -( lik_weight lik[n] + prior_weight sum_r log N(theta[n][r]; mu0[r], s0[r]) )
//   grad[n][r] = -( lik_weight sum_b dlog[n][c][b] x[b][p] - prior_weight (theta[n][r] - mu0[r]) / s0[r]^2 )
// with lik[n] = sum_b log softmax(logits[n][:, b])[k_b] (Categorical) or sum_b k_b l - softplus(l) (Bernoulli, C = 1) and
// logits[n][c][b] = sum_p theta[n][c P + p] x[b][p].  The dense path's own kernels build W = mu + s eps while staging and sum over the
// sample axis inside the backward kernel; with particles nothing may be summed over n, so this is a kernel of its own.  A particle's
// whole gradient fits on the chip: logits and d f / d logits never reach HBM.
//
//   dense_head           the dense path's own launch, without noise workgroups: rowp (the rows' prior loc and scale), the ONE minibatch
//                        shared by the particles (Xb [B_pad][P_pad], XbT [P_pad][B_pad], lab), B_pad a multiple of 128 here
//   dense_particles      grid (ceil(N / NS), splits), 256 threads.  A workgroup owns one 32-row MFMA block of (particle, class) rows,
//                        row = s C + c for the NS = floor(32 / C) whole particles s of the block (dead rows are zero), and walks its
//                        share of the minibatch in passes of 128 columns, one 32-column block per wave:
//     phase 1  logits on v_mfma_f32_32x32x2_f32 (f32 inputs: nothing asks the data to be bf16-exact).  A = theta, staged k-major
//              Th[k][row] (row stride 33: the half-wave that loads 32 consecutive p of one row stores to 32 banks, the half-wave that
//              reads 32 rows of one k reads 32 banks), two buffers, one barrier per chunk of 32 features; B = XbT straight from global
//              memory (each wave has columns of its own: LDS would buy no reuse), the next chunk's 16 values in registers behind the
//              products of this one.
//     phase 2  the accumulator goes to the tile T[column][row] (row stride 33) and a lane takes (column, particle) pairs — lanes along
//              the columns: bank = column + const — max, sum of exp and dlog = lik_weight (onehot - softmax) | lik_weight (k - sigmoid)
//              in place, zero for columns b >= B and particles n >= N.  The pair's log-likelihood is added to liksum[s][column], an
//              address of the lane's own: a fixed order.
//     phase 3  grad_tile[32][P] += dlog_tile[32][128] . Xb[pass columns][P] on the same MFMA: A = T[k = column][row], read as 32
//              consecutive words per half-wave (no conflicts), B = the minibatch rows from global memory, 128-byte lines per
//              half-wave.  The waves split P in 32-column blocks, wave w the blocks w, w + 4, ...: NB <= 8 blocks per wave (P <= 1024)
//              stay in accumulators over all passes.
//     epilogue one split: the prior term from the same theta values in registers, grad and loss stored once (dword stores along p: a
//              half-wave writes one 128-byte line, whatever ld and the base are), the particle's prior value by xor-shuffles and a fixed
//              order of the waves.  Several splits (few workgroups for the chip: the passes are dealt over grid.y): the raw gradient
//              block and the likelihood go to part[split][n][r] / likp[split][n], and
//   dense_particles_join a workgroup per particle adds them in split order, adds the prior and stores grad and loss.
// No atomics, every sum in a fixed order: two calls leave the same bits.  Columns R .. ld of grad are never written.

constexpr uint32_t DP_MIN_PARTICLES = 2, DP_MAX_PARTICLES = 256, DP_MAX_CLASSES = 32, DP_MAX_FEATURES = 1024;
constexpr uint32_t DP_COLS = 128, DP_TS = 33;      // columns of a pass; row stride of Th and T

struct DenseParticles {
    const float* theta; float* grad; float* loss;
    const float* Xb; const float* XbT; const float* lab; const float* rowp;
    float* part;            // [splits][N][R]  (splits > 1)
    float* likp;            // [splits][N]
    uint64_t ld;
    uint32_t N, C, P, R, B, B_pad, P_pad, NS;
    uint32_t splits, passes_per_split, n_pass, likelihood;
    float lik_weight, prior_weight;
};

// d log N(w; mu0, s0) / d w and its value
__device__ __forceinline__ float dp_prior(const float w, const float mu0, const float s0, float& value) {
    const float is0 = 1.0f / s0, u = (w - mu0) * is0;
    value = -0.5f * u * u - logf(s0) - 0.91893853320467274178f;
    return -u * is0;
}

template <int NB>
__global__ void __launch_bounds__(256) dense_particles(const DenseParticles T) {
    __shared__ float Th[2][32 * DP_TS];
    __shared__ float Tt[DP_COLS * DP_TS];
    __shared__ float liksum[32][DP_COLS];
    __shared__ float rowsum[4][32];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, lm = lane & 31u, lk = lane >> 5;
    const uint32_t n0 = blockIdx.x * T.NS, split = blockIdx.y, live_rows = T.NS * T.C;
    const uint32_t n_chunk = (T.P + 31u) / 32u, n_blk = n_chunk;
    for (uint32_t i = tid; i < 32u * DP_COLS; i += 256u) (&liksum[0][0])[i] = 0.0f;

    // staging of theta: thread = (feature tid & 31, rows (tid >> 5) + 8 j): a half-wave reads 128 consecutive bytes of one row
    const uint32_t sp = tid & 31u;
    const float* trow[4];
    bool tlive[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t row = (tid >> 5) + 8u * j, s = row / T.C, c = row - s * T.C;
        tlive[j] = row < live_rows && n0 + s < T.N;
        trow[j] = T.theta + (size_t)(tlive[j] ? n0 + s : 0u) * T.ld + (size_t)(tlive[j] ? c : 0u) * T.P;
    }
    float tr[4];
    auto fetch_theta = [&](uint32_t chunk) {
        const uint32_t p = chunk * 32u + sp;
#pragma unroll
        for (int j = 0; j < 4; ++j) tr[j] = (tlive[j] && p < T.P) ? trow[j][p] : 0.0f;
    };
    auto commit_theta = [&](uint32_t buf) {
#pragma unroll
        for (int j = 0; j < 4; ++j) Th[buf][sp * DP_TS + (tid >> 5) + 8u * j] = tr[j];
    };

    xf_f32x16 acc[NB];
#pragma unroll
    for (int q = 0; q < NB; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[q][r] = 0.0f;

    const uint32_t pass0 = split * T.passes_per_split, pass1 = min(pass0 + T.passes_per_split, T.n_pass);
    for (uint32_t pass = pass0; pass < pass1; ++pass) {
        const uint32_t col = wave * 32u + lm, b = pass * DP_COLS + col;      // (b < B_pad: a multiple of 128)
        // ---- phase 1: logits[row][b] of the wave's 32 columns
        xf_f32x16 lg;
#pragma unroll
        for (int r = 0; r < 16; ++r) lg[r] = 0.0f;
        const float* const xt = T.XbT + (size_t)lk * T.B_pad + b;            // + (32 chunk + 2 kk) B_pad  (rows < P_pad: zero past P)
        float bc[16], bn[16];
        fetch_theta(0);
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) bc[kk] = xt[(size_t)(2 * kk) * T.B_pad];
        commit_theta(0);
        __syncthreads();
        for (uint32_t chunk = 0; chunk < n_chunk; ++chunk) {
            const uint32_t next = min(chunk + 1u, n_chunk - 1u);             // past the end: the last chunk again, never used
            fetch_theta(next);
#pragma unroll
            for (int kk = 0; kk < 16; ++kk) bn[kk] = xt[(size_t)(32u * next + 2 * kk) * T.B_pad];
            const float* const th = Th[chunk & 1u] + lk * DP_TS + lm;
#pragma unroll
            for (int kk = 0; kk < 16; ++kk) lg = __builtin_amdgcn_mfma_f32_32x32x2f32(th[2 * kk * DP_TS], bc[kk], lg, 0, 0, 0);
            commit_theta((chunk + 1u) & 1u);      // (last read before the previous barrier)
#pragma unroll
            for (int kk = 0; kk < 16; ++kk) bc[kk] = bn[kk];
            __syncthreads();
        }
        // ---- phase 2: lg[r] is logits[row = 8 (r >> 2) + 4 lk + (r & 3)][column lm of the wave]  ->  T[column][row]
        // (every wave left phase 3 of the previous pass through the barriers of phase 1)
#pragma unroll
        for (int r = 0; r < 16; ++r) Tt[col * DP_TS + 8u * (r >> 2) + 4u * lk + (r & 3)] = lg[r];
        __syncthreads();
        const float label = T.lab[b];
        for (uint32_t s = lk; s < T.NS; s += 2u) {
            float* const t = Tt + col * DP_TS + s * T.C;
            const float w = (b < T.B && n0 + s < T.N) ? T.lik_weight : 0.0f;
            float lik;
            if (T.likelihood == BSVI_LIK_CATEGORICAL) {
                float m = t[0];
                for (uint32_t c = 1; c < T.C; ++c) m = fmaxf(m, t[c]);
                float se = 0.0f, zl = 0.0f;
                for (uint32_t c = 0; c < T.C; ++c) {
                    const float v = t[c], e = expf(v - m);
                    zl = (label == (float)c) ? v : zl;
                    se += e;
                    t[c] = e;
                }
                lik = zl - (m + logf(se));
                const float wr = w / se;
                for (uint32_t c = 0; c < T.C; ++c) t[c] = ((label == (float)c) ? w : 0.0f) - wr * t[c];
            } else {      // Bernoulli / Binomial(1)
                const float l = t[0];
                lik = label * l - (fmaxf(l, 0.0f) + log1pf(expf(-fabsf(l))));
                t[0] = w * (label - sigmoidf_(l));
            }
            liksum[s][col] += w != 0.0f ? lik : 0.0f;
        }
        __syncthreads();
        // ---- phase 3: grad_tile[row][p] += sum_col dlog[row][col] x[pass column col][p]
        const float* const xb = T.Xb + (size_t)(pass * DP_COLS + lk) * T.P_pad + wave * 32u + lm;      // + 2 kk P_pad + 128 q
        const float* const ta = Tt + lk * DP_TS + lm;
#pragma unroll 2
        for (uint32_t k4 = 0; k4 < DP_COLS / 2u; k4 += 4u) {
            float a[4], x[4][NB];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                a[u] = ta[2u * (k4 + u) * DP_TS];
#pragma unroll
                for (int q = 0; q < NB; ++q)
                    x[u][q] = (wave + 4u * q < n_blk) ? xb[(size_t)(2u * (k4 + u)) * T.P_pad + 128u * q] : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int q = 0; q < NB; ++q)
                    if (wave + 4u * q < n_blk) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], x[u][q], acc[q], 0, 0, 0);
        }
    }
    __syncthreads();      // (no pass at all cannot happen: every split has one)

    // ---- epilogue: acc[q][r] is the likelihood's gradient of row 8 (r >> 2) + 4 lk + (r & 3), feature 32 (wave + 4 q) + lm
    float rowpv[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        rowpv[r] = 0.0f;
        const uint32_t row = 8u * (r >> 2) + 4u * lk + (r & 3), s = row / T.C, c = row - s * T.C, n = n0 + s;
        if (row >= live_rows || n >= T.N) continue;
#pragma unroll
        for (int q = 0; q < NB; ++q) {
            const uint32_t p = 32u * (wave + 4u * q) + lm;
            if (p >= T.P) continue;
            const uint32_t rr = c * T.P + p;
            if (T.splits > 1u) {
                T.part[((size_t)split * T.N + n) * T.R + rr] = acc[q][r];
            } else {
                float value;
                const float dp = dp_prior(T.theta[(size_t)n * T.ld + rr], T.rowp[2u * (size_t)T.R + rr], T.rowp[3u * (size_t)T.R + rr], value);
                T.grad[(size_t)n * T.ld + rr] = -(acc[q][r] + T.prior_weight * dp);
                rowpv[r] += value;
            }
        }
    }
    if (T.splits == 1u) {
        // the rows' prior values: the 32 lanes of a half-wave (xor-shuffles), then the four waves and the particle's rows in order
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float v = rowpv[r];
#pragma unroll
            for (int d = 16; d >= 1; d >>= 1) v += __shfl_xor(v, d);
            if (lm == 0u) rowsum[wave][8u * (r >> 2) + 4u * lk + (r & 3)] = v;
        }
        __syncthreads();
    }
    if (tid < T.NS && n0 + tid < T.N) {
        float lik = 0.0f;
        for (uint32_t c = 0; c < DP_COLS; ++c) lik += liksum[tid][c];
        if (T.splits > 1u) {
            T.likp[(size_t)split * T.N + n0 + tid] = lik;
        } else {
            float pv = 0.0f;
            for (uint32_t c = 0; c < T.C; ++c) {
                const uint32_t row = tid * T.C + c;
                pv += (rowsum[0][row] + rowsum[1][row]) + (rowsum[2][row] + rowsum[3][row]);
            }
            T.loss[n0 + tid] = -(T.lik_weight * lik + T.prior_weight * pv);
        }
    }
}

// grid: N, block 256: particle n's partial gradients and likelihoods in split order, the prior term, grad and loss
__global__ void __launch_bounds__(256) dense_particles_join(const DenseParticles T) {
    __shared__ float red[4];
    const uint32_t n = blockIdx.x, tid = threadIdx.x;
    float pv = 0.0f;
    for (uint32_t r = tid; r < T.R; r += 256u) {
        float g = 0.0f;
        for (uint32_t s = 0; s < T.splits; ++s) g += T.part[((size_t)s * T.N + n) * T.R + r];
        float value;
        const float dp = dp_prior(T.theta[(size_t)n * T.ld + r], T.rowp[2u * (size_t)T.R + r], T.rowp[3u * (size_t)T.R + r], value);
        T.grad[(size_t)n * T.ld + r] = -(g + T.prior_weight * dp);
        pv += value;
    }
    pv = block_sum(pv, red, tid, 4);
    if (tid == 0u) {
        float lik = 0.0f;
        for (uint32_t s = 0; s < T.splits; ++s) lik += T.likp[(size_t)s * T.N + n];
        T.loss[n] = -(T.lik_weight * lik + T.prior_weight * pv);
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------
// the shape of a call: paddings, the split of the passes, and the workspace (byte offsets, each 256-byte aligned)
struct DenseParticlesPlan {
    uint32_t B_pad, P_pad, NS, groups, n_pass, splits, passes_per_split, NB;
    size_t rowp, idx, Xb, XbT, lab, partial, part, likp, total;
};

static int dense_particles_check(const bsvi_dense* p, const uint32_t n_particles) {
    if (n_particles < DP_MIN_PARTICLES || n_particles > DP_MAX_PARTICLES)
        return fail(BSVI_ERR_INVALID, "bsvi_dense_particles: n_particles is " + std::to_string(n_particles) + ", served are 2 .. 256 particles");
    if (!p) return fail(BSVI_ERR_INVALID, "bsvi_dense_particles: null handle");
    if (p->d.n_classes > DP_MAX_CLASSES)
        return fail(BSVI_ERR_INVALID, "bsvi_dense_particles: " + std::to_string(p->d.n_classes) + " classes, served are 1 .. 32 (a particle's rows share one 32-row block)");
    if (p->d.n_features > DP_MAX_FEATURES)
        return fail(BSVI_ERR_INVALID, "bsvi_dense_particles: " + std::to_string(p->d.n_features) + " features, served are 1 .. 1024 (the gradient of a block stays in accumulators)");
    return BSVI_OK;
}

static DenseParticlesPlan dense_particles_plan(const bsvi_dense* p, const uint32_t N) {
    DenseParticlesPlan L;
    const uint32_t C = p->d.n_classes, P = p->d.n_features, R = C * P;
    L.B_pad = (p->d.batch_size + DP_COLS - 1u) / DP_COLS * DP_COLS;
    L.P_pad = (P + 63u) / 64u * 64u;
    L.NS = 32u / C;
    L.groups = (N + L.NS - 1u) / L.NS;
    L.n_pass = L.B_pad / DP_COLS;
    // few workgroups for the chip: the passes go over a second grid axis, as many splits as leave no CU a second workgroup
    uint32_t want = p->m.n_cu / L.groups;
    want = want < 1u ? 1u : (want > L.n_pass ? L.n_pass : want);
    L.passes_per_split = (L.n_pass + want - 1u) / want;
    L.splits = (L.n_pass + L.passes_per_split - 1u) / L.passes_per_split;
    const uint32_t per_wave = ((P + 31u) / 32u + 3u) / 4u;
    L.NB = per_wave <= 1u ? 1u : per_wave <= 2u ? 2u : per_wave <= 4u ? 4u : 8u;
    size_t o = 0;
    auto take = [&](size_t floats) { const size_t at = o; o += align_up(floats * 4, 256); return at; };
    L.rowp = take(6 * (size_t)R + 64);
    L.idx = take(L.B_pad);
    L.Xb = take((size_t)L.B_pad * L.P_pad);
    L.XbT = take((size_t)L.P_pad * L.B_pad + 128);
    L.lab = take(L.B_pad);
    L.partial = take(2 + (size_t)p->d.n_uniform_grad);
    L.part = take(L.splits > 1u ? (size_t)L.splits * N * R : 1);
    L.likp = take((size_t)L.splits * N);
    L.total = o + 256;
    return L;
}

extern "C" size_t bsvi_dense_particles_workspace_bytes(const bsvi_dense* p, uint32_t n_particles) {
    if (dense_particles_check(p, n_particles)) return 0;
    return dense_particles_plan(p, n_particles).total;
}

extern "C" int bsvi_dense_particles_fwd_bwd(const bsvi_dense* p, const bsvi_dense_args* a, const float* theta_dev, float* grad_dev, float* loss_dev,
                                            uint32_t n_particles, uint64_t ld, void* workspace_dev) {
    const int rc = dense_particles_check(p, n_particles);
    if (rc) return rc;
    if (a) BSVI_CHECK_STRUCT(a, bsvi_dense_args);
    if (!a || !a->params_dev || !theta_dev || !grad_dev || !loss_dev || !workspace_dev)
        return fail(BSVI_ERR_INVALID, "bsvi_dense_particles_fwd_bwd: null argument");
    const uint32_t C = p->d.n_classes, P = p->d.n_features, R = C * P;
    if (ld < R) return fail(BSVI_ERR_INVALID, "bsvi_dense_particles_fwd_bwd: ld is " + std::to_string(ld) + ", a particle has " + std::to_string(R) + " values");
    if ((uint64_t)n_particles * ld >= (1ull << 31)) return fail(BSVI_ERR_INVALID, "bsvi_dense_particles_fwd_bwd: n_particles x ld beyond 2^31");
    if (theta_dev == grad_dev) return fail(BSVI_ERR_INVALID, "bsvi_dense_particles_fwd_bwd: grad_dev may not be theta_dev");
    const DenseParticlesPlan L = dense_particles_plan(p, n_particles);
    char* const ws = (char*)workspace_dev;
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
    DenseParticles T;
    memset(&T, 0, sizeof(T));
    T.theta = theta_dev; T.grad = grad_dev; T.loss = loss_dev; T.ld = ld;
    T.Xb = D.Xb; T.XbT = D.XbT; T.lab = D.lab; T.rowp = D.rowp;
    T.part = (float*)(ws + L.part); T.likp = (float*)(ws + L.likp);
    T.N = n_particles; T.C = C; T.P = P; T.R = R; T.B = p->d.batch_size; T.B_pad = L.B_pad; T.P_pad = L.P_pad; T.NS = L.NS;
    T.splits = L.splits; T.passes_per_split = L.passes_per_split; T.n_pass = L.n_pass; T.likelihood = p->d.likelihood;
    T.lik_weight = p->d.lik_weight; T.prior_weight = p->d.prior_weight;
    const dim3 grid(L.groups, L.splits), block(256);
    switch (L.NB) {
    case 1: hipLaunchKernelGGL(dense_particles<1>, grid, block, 0, s, T); break;
    case 2: hipLaunchKernelGGL(dense_particles<2>, grid, block, 0, s, T); break;
    case 4: hipLaunchKernelGGL(dense_particles<4>, grid, block, 0, s, T); break;
    default: hipLaunchKernelGGL(dense_particles<8>, grid, block, 0, s, T);
    }
    if (L.splits > 1u) hipLaunchKernelGGL(dense_particles_join, dim3(n_particles), block, 0, s, T);
    HIP_TRY(hipGetLastError());
    return BSVI_OK;
}
