// bnn_ensemble.inc — the predictive of a particle ensemble of a Bayesian neural network, forward only, one fused kernel (included by
// elbo_kernel.hip behind bnn_particles.inc; DESIGN.md 4.8).
//
// N point estimates theta[n] of one network in the [N][ld] table of bsvi_bnn_particles_fwd_bwd (the latent vector's row order: weights1
// first, r = h P + p, then the other tensors at their weight_row0 / bias_row0), read IN PLACE for any ld >= R and any alignment, and M
// rows x[m] the caller hands in, [M][P].  Per (particle n, row m): the whole chain, the head as bnn_predict_fwd defines it, and on
// request the likelihood's draw of that kernel's stream with the particle as the sample.  Nothing between x and the probabilities goes
// through device memory.
//   bnn_ensemble_fwd    grid (row tiles, splits), 256 threads.  A workgroup owns E.rows rows of x (128: 32 a wave; 64 or 32 for the
//                       widths whose two tiles of 128 rows do not fit LDS — the upper waves then only stage) and walks the particle
//                       groups y, y + splits, ...: E.group particles at once.  Every layer is ONE routine (be_layer): a product on
//                       v_mfma_f32_32x32x2_f32 whose K axis is streamed in chunks of 32 through two LDS buffers (one barrier a chunk, the
//                       next chunk's global loads in registers behind the products of this one), up to ENS_BLOCKS 32-column blocks in
//                       accumulators at once, then bias + activation into the layer's tile [particle][row][unit].
//                         first layer   A = the x chunk, staged from the caller's array; the columns are (particle, unit) pairs side by
//                                       side, col = g H1 + h, so one x chunk serves every particle of the group; B = the chunk of the
//                                       group's weights1 rows straight from the table
//                         upper layers  A = the particle's tile of the layer below (k past its width: zero), a block of columns
//                                       belongs to one particle; B = the chunk of that particle's weight rows from the table
//                       16-byte loads where the address of a quad allows, masked scalars where not; no feature past P, no column past
//                       R, no row past M and no particle past N is read.  The head: a thread per (particle, row) turns the logits into
//                       the stored probabilities (and the draw's class) in the other tile, then the workgroup stores probs, outputs and
//                       draws as runs along (m, c).
//   bnn_predict_reduce  as it is: one thread per (m, c), the particles in order n = 0, 1, ... in double precision — the mean, and the
//                       variance of a Normal / Laplace likelihood.
// No atomics; every (n, m) is computed by one workgroup in one order, whatever the grid: two calls leave the same bits.

constexpr uint32_t BE_ROWS = bsvi_bnn_select::ENS_ROWS, BE_CHUNK = bsvi_bnn_select::ENS_CHUNK, BE_TS = BE_CHUNK + 1u,
                   BE_BLOCKS = bsvi_bnn_select::ENS_BLOCKS;
static_assert(BE_ROWS == 128u && BE_CHUNK == 32u && BE_BLOCKS == 4u, "bnn_ensemble_fwd stages 128 rows x 32 values with 256 threads, four quads each");

struct BnnEnsemble {
    const float* theta; uint64_t ld;      // [N][ld]
    const float* x;                       // [M][P]
    uint32_t N, M, group, rows, n_groups;
    uint32_t stride[2], tile[2];          // EnsemblePlan's
    float* p;                             // [N][M][C]: the caller's, or the workspace's
    float* z_out; float* draw_out;        // [N][M][C] or null
    float* sg;                            // Normal: sigma [C] for the reduce (written by workgroup (0, 0))
};

// row[k .. k + 3] of a row of K values as zeros past K (a null row: zeros): one 16-byte load where the quad is whole and aligned
__device__ __forceinline__ void be_load4(const float* const row, const uint32_t k, const uint32_t K, float v[4]) {
    if (row && k + 3u < K && ((uintptr_t)(row + k) & 15u) == 0u) {
        const xf_f32x4 q = *reinterpret_cast<const xf_f32x4*>(row + k);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = q[j];
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (row && k + j < K) ? row[k + j] : 0.0f;
    }
}

// column lm of the 32-column block B of a layer of `width` units -> (particle g of the group, unit u); false: a dead column.
// PACKED (the first product): (particle, unit) pairs side by side, col = g width + u; else bpp blocks per particle.
template <bool PACKED>
__device__ __forceinline__ bool be_column(const uint32_t B, const uint32_t lm, const uint32_t width, const uint32_t bpp, const uint32_t g_live,
                                          uint32_t& g, uint32_t& u) {
    if (PACKED) { const uint32_t col = B * 32u + lm; g = col / width; u = col - g * width; }
    else { g = B / bpp; u = (B - g * bpp) * 32u + lm; }
    return g < g_live && u < width;
}

// Layer l of the particles n0 .. n0 + g_live of a group on the workgroup's rows m0 ..: out = act(A W^T + b) into the tile l & 1.
// FIRST: A is x, streamed; else the tile (l - 1) & 1.  Ends behind a barrier.
template <bool FIRST>
__device__ __forceinline__ void be_layer(const BParams& Q, const BnnEnsemble& E, const uint32_t l, const uint32_t m0, const uint32_t n0,
                                         const uint32_t g_live) {
    const BnnLayerDev L = Q.layer[l];
    const uint32_t K = L.cols, W = L.rows, bpp = (W + 31u) / 32u;
    float* const sA = g_lds;                                    // [2][128][33]
    float* const sB = g_lds + 2u * BE_ROWS * BE_TS;             // [2][128][33]: row = column of the pass
    const float* const tin = g_lds + E.tile[(l + 1u) & 1u];
    const uint32_t sin = E.stride[(l + 1u) & 1u], sout = E.stride[l & 1u];
    float* const tout = g_lds + E.tile[l & 1u];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, lm = lane & 31u, lk = lane >> 5;
    const uint32_t srow = threadIdx.x >> 3, sq = (threadIdx.x & 7u) * 4u;      // staging: row srow + 32 i, the quad at sq
    const uint32_t n_blocks = FIRST ? (g_live * W + 31u) / 32u : g_live * bpp, n_chunks = (K + BE_CHUNK - 1u) / BE_CHUNK;
    const bool mma = 32u * wave < E.rows;
    for (uint32_t B0 = 0; B0 < n_blocks; B0 += BE_BLOCKS) {
        const uint32_t nb = min(BE_BLOCKS, n_blocks - B0);
        const float* wrow[BE_BLOCKS];
        const float* xrow[BE_BLOCKS];
#pragma unroll
        for (uint32_t i = 0; i < BE_BLOCKS; ++i) {
            uint32_t g, u;
            const bool live = i < nb && be_column<FIRST>(B0 + i, srow, W, bpp, g_live, g, u);
            wrow[i] = live ? E.theta + (size_t)(n0 + g) * E.ld + L.w0 + (size_t)u * K : nullptr;
            const uint32_t row = srow + 32u * i;
            xrow[i] = (FIRST && row < E.rows && m0 + row < E.M) ? E.x + (size_t)(m0 + row) * K : nullptr;
        }
        float fa[BE_BLOCKS][4], fb[BE_BLOCKS][4];
        auto fetch = [&](const uint32_t c) {
#pragma unroll
            for (uint32_t i = 0; i < BE_BLOCKS; ++i) {
                be_load4(wrow[i], c * BE_CHUNK + sq, K, fb[i]);
                if (FIRST) be_load4(xrow[i], c * BE_CHUNK + sq, K, fa[i]);
            }
        };
        auto commit = [&](const uint32_t buf) {
#pragma unroll
            for (uint32_t i = 0; i < BE_BLOCKS; ++i)
#pragma unroll
                for (uint32_t j = 0; j < 4u; ++j) {
                    const uint32_t at = (buf * BE_ROWS + 32u * i + srow) * BE_TS + sq + j;
                    sB[at] = fb[i][j];
                    if (FIRST) sA[at] = fa[i][j];
                }
        };
        xf_f32x16 acc[BE_BLOCKS];
#pragma unroll
        for (uint32_t i = 0; i < BE_BLOCKS; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][r] = 0.0f;
        fetch(0u);
        commit(0u);
        __syncthreads();
        for (uint32_t c = 0; c < n_chunks; ++c) {
            const bool more = c + 1u < n_chunks;
            if (more) fetch(c + 1u);
            if (mma) {
                const float* const ap = sA + ((c & 1u) * BE_ROWS + 32u * wave + lm) * BE_TS + lk;
                const float* const bp = sB + ((c & 1u) * BE_ROWS + lm) * BE_TS + lk;
                // a chunk's 32 terms are summed in accumulators of their own and then added to the running sum: the rounding of a long
                // K axis stays that of a sum of K / 32 terms (one chain over 256 units left 1.3e-5 on a loc of 27, twice the yardstick)
                xf_f32x16 part[BE_BLOCKS];
#pragma unroll
                for (uint32_t i = 0; i < BE_BLOCKS; ++i)
#pragma unroll
                    for (int r = 0; r < 16; ++r) part[i][r] = 0.0f;
#pragma unroll
                for (uint32_t kk = 0; kk < BE_CHUNK / 2u; ++kk) {
                    float a = FIRST ? ap[2u * kk] : 0.0f;
#pragma unroll
                    for (uint32_t i = 0; i < BE_BLOCKS; ++i) {
                        if (i >= nb) continue;
                        if (!FIRST) {      // (a block's particle: its tile of the layer below; k past its width is a dead row)
                            const uint32_t k = c * BE_CHUNK + 2u * kk + lk, g = (B0 + i) / bpp;
                            a = k < K ? tin[(size_t)(g * E.rows + 32u * wave + lm) * sin + k] : 0.0f;
                        }
                        part[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bp[(32u * i) * BE_TS + 2u * kk], part[i], 0, 0, 0);
                    }
                }
#pragma unroll
                for (uint32_t i = 0; i < BE_BLOCKS; ++i)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[i][r] += part[i][r];
            }
            if (more) commit((c + 1u) & 1u);      // (last read before the previous barrier)
            __syncthreads();
        }
        // acc[i][r] is row 32 wave + 8 (r >> 2) + 4 lk + (r & 3), column lm of block B0 + i
        if (mma) {
#pragma unroll
            for (uint32_t i = 0; i < BE_BLOCKS; ++i) {
                uint32_t g, u;
                if (i >= nb || !be_column<FIRST>(B0 + i, lm, W, bpp, g_live, g, u)) continue;
                const float bias = L.b0 != 0xFFFFFFFFu ? E.theta[(size_t)(n0 + g) * E.ld + L.b0 + u] : 0.0f;
#pragma unroll
                for (uint32_t r = 0; r < 16u; ++r) {
                    const uint32_t row = 32u * wave + 8u * (r >> 2) + 4u * lk + (r & 3u);
                    tout[(size_t)(g * E.rows + row) * sout + u] = bnn_act(L.act, acc[i][r] + bias, Q.act_p[l]);
                }
            }
        }
    }
    __syncthreads();
}

// grid: (row tiles, splits), block 256, dynamic LDS EnsemblePlan::lds_bytes
__global__ void __launch_bounds__(256) bnn_ensemble_fwd(const BParams Q, const BnnEnsemble E) {
    const uint32_t m0 = blockIdx.x * E.rows, nl = Q.n_layers, C = Q.C;
    const uint32_t rows_live = min(E.rows, E.M - m0), per = rows_live * C;      // (m0 < M: the grid has ceil(M / rows) row tiles)
    if (Q.likelihood == BSVI_LIK_NORMAL && blockIdx.x == 0u && blockIdx.y == 0u)
        for (uint32_t c = threadIdx.x; c < C; c += 256u) E.sg[c] = bnn_uniform_value(Q, Q.scale_u + c * Q.scale_stride);
    const float* const zt = g_lds + E.tile[(nl - 1u) & 1u];
    float* const pt = g_lds + E.tile[nl & 1u];
    const uint32_t sz = E.stride[(nl - 1u) & 1u], sp = E.stride[nl & 1u];
    for (uint32_t grp = blockIdx.y; grp < E.n_groups; grp += gridDim.y) {
        const uint32_t n0 = grp * E.group, g_live = min(E.group, E.N - n0);
        be_layer<true>(Q, E, 0u, m0, n0, g_live);
        for (uint32_t l = 1; l < nl; ++l) be_layer<false>(Q, E, l, m0, n0, g_live);
        // the head, a thread per (particle, row): the stored probabilities pr[0 .. C), and in pr[C] the draw's class (Bernoulli: pr[1] the draw)
        for (uint32_t i = threadIdx.x; i < g_live * rows_live; i += 256u) {
            const uint32_t g = i / rows_live, row = i - g * rows_live;
            const float* const zr = zt + (size_t)(g * E.rows + row) * sz;
            float* const pr = pt + (size_t)(g * E.rows + row) * sp;
            if (Q.likelihood == BSVI_LIK_NORMAL) {
                for (uint32_t c = 0; c < C; ++c) pr[c] = zr[c];
                continue;
            }
            const float u = E.draw_out ? u01(bnn_predict_words(Q, n0 + g, m0 + row, 0u).x) : 0.0f;
            if (Q.likelihood == BSVI_LIK_CATEGORICAL) {
                // log-softmax, then expf: the probabilities as they are stored; the inverse CDF on them, in class order
                float mx = -INFINITY;
                for (uint32_t c = 0; c < C; ++c) mx = fmaxf(mx, zr[c]);
                float se = 0.0f;
                for (uint32_t c = 0; c < C; ++c) se += expf(zr[c] - mx);
                const float lse = mx + logf(se);
                float cum = 0.0f;
                uint32_t pick = C - 1u;
                bool found = false;
                for (uint32_t c = 0; c < C; ++c) {
                    const float pc = expf(zr[c] - lse);
                    pr[c] = pc;
                    cum += pc;
                    if (!found && cum >= u) { pick = c; found = true; }
                }
                pr[C] = __uint_as_float(pick);
            } else {
                const float pb = sigmoidf_(zr[0]);
                pr[0] = pb;
                pr[1] = u < pb ? 1.0f : 0.0f;
            }
        }
        __syncthreads();
        // the stores: per particle one run of rows_live x C floats along (m, c)
        for (uint32_t i = threadIdx.x; i < g_live * per; i += 256u) {
            const uint32_t g = i / per, rem = i - g * per, row = rem / C, c = rem - row * C, n = n0 + g, m = m0 + row;
            const float* const zr = zt + (size_t)(g * E.rows + row) * sz;
            const float* const pr = pt + (size_t)(g * E.rows + row) * sp;
            const size_t at = ((size_t)n * E.M + m) * C + c;
            E.p[at] = pr[c];
            if (E.z_out) E.z_out[at] = zr[c];
            if (E.draw_out) {
                if (Q.likelihood == BSVI_LIK_NORMAL) {
                    float e[4];
                    bnn_predict_noise4(Q, n, m, c & ~3u, e);
                    E.draw_out[at] = zr[c] + bnn_uniform_value(Q, Q.scale_u + c * Q.scale_stride) * e[c & 3u];
                } else if (Q.likelihood == BSVI_LIK_CATEGORICAL) {
                    E.draw_out[at] = c == __float_as_uint(pr[C]) ? 1.0f : 0.0f;
                } else {
                    E.draw_out[at] = pr[1];
                }
            }
        }
        __syncthreads();      // (the next group's first layer writes the tiles)
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------
static bsvi_bnn_select::EnsemblePlan bnn_ensemble_plan(const bsvi_bnn* p, const uint32_t n_particles, const uint32_t n_rows) {
    uint32_t widths[BNN_MAX_LAYERS] = {};
    const uint32_t nl = (uint32_t)std::min<size_t>(p->layers.size(), BNN_MAX_LAYERS);
    for (uint32_t l = 0; l < nl; ++l) widths[l] = p->layers[l].rows;
    return bsvi_bnn_select::ensemble_plan(widths, nl, n_particles, n_rows);
}

static int bnn_ensemble_refuse(const bsvi_bnn_select::EnsemblePlan& E) {
    return fail(BSVI_ERR_UNSUPPORTED, "bsvi_bnn_predict_particles: a layer of " + std::to_string(E.widest) + " units, served are layers of up to " +
                                          std::to_string(bsvi_bnn_select::ENS_MAX_WIDTH) + " (two activation tiles of 32 rows within " +
                                          std::to_string(bsvi_bnn_select::LDS_LIMIT / 1024u) + " KB of LDS)");
}

extern "C" size_t bsvi_bnn_predict_particles_args_size(void) { return sizeof(bsvi_bnn_predict_particles_args); }

extern "C" size_t bsvi_bnn_predict_particles_workspace_bytes(const bsvi_bnn* p, uint32_t n_particles, uint32_t n_rows) {
    if (!p) { fail(BSVI_ERR_INVALID, "bsvi_bnn_predict_particles: null handle"); return 0; }
    if (!n_rows) { fail(BSVI_ERR_INVALID, "bsvi_bnn_predict_particles: n_rows is 0"); return 0; }
    if (bnn_particles_check(p, n_particles)) return 0;
    const bsvi_bnn_select::EnsemblePlan E = bnn_ensemble_plan(p, n_particles, n_rows);
    if (!E.served) { bnn_ensemble_refuse(E); return 0; }
    return E.workspace_bytes;
}

extern "C" int bsvi_bnn_predict_particles(const bsvi_bnn* p, const bsvi_bnn_predict_particles_args* a) {
    // every check in front of any device work
    if (!a) return fail(BSVI_ERR_INVALID, "bsvi_bnn_predict_particles: null argument");
    BSVI_CHECK_STRUCT(a, bsvi_bnn_predict_particles_args);
    if (!p) return fail(BSVI_ERR_INVALID, "bsvi_bnn_predict_particles: null handle");
    if (!a->theta_dev) return fail(BSVI_ERR_INVALID, "bsvi_bnn_predict_particles: theta_dev is null");
    if (!a->x_dev) return fail(BSVI_ERR_INVALID, "bsvi_bnn_predict_particles: x_dev is null");
    if (!a->n_rows) return fail(BSVI_ERR_INVALID, "bsvi_bnn_predict_particles: n_rows is 0");
    if (!a->workspace_dev) return fail(BSVI_ERR_INVALID, "bsvi_bnn_predict_particles: workspace_dev is null");
    int rc = bnn_particles_check(p, a->n_particles);
    if (rc) return rc;
    if (a->ld < p->R)
        return fail(BSVI_ERR_INVALID, "bsvi_bnn_predict_particles: ld is " + std::to_string(a->ld) + ", a particle has " + std::to_string(p->R) + " values");
    if (!a->params_dev && p->d.n_params) return fail(BSVI_ERR_INVALID, "bsvi_bnn_predict_particles: params_dev is null");
    if (a->var_out && p->d.likelihood != BSVI_LIK_NORMAL)
        return fail(BSVI_ERR_INVALID, "bsvi_bnn_predict_particles: var_out is for the Normal likelihood (a classifier's variance is p (1 - p) of mean_out)");
    if (a->var_out && p->family == BSVI_DIST_CAUCHY) return fail(BSVI_ERR_UNSUPPORTED, "bsvi_bnn_predict_particles: the Cauchy likelihood has no variance");
    if ((uint64_t)a->n_rows * p->C >= (1ull << 31) || (uint64_t)a->n_particles * a->n_rows * p->C >= (1ull << 40))
        return fail(BSVI_ERR_UNSUPPORTED, "bsvi_bnn_predict_particles: n_particles x rows x outputs too large");
    const bsvi_bnn_select::EnsemblePlan P = bnn_ensemble_plan(p, a->n_particles, a->n_rows);
    if (!P.served) return bnn_ensemble_refuse(P);
    if (P.row_tiles > 0x7FFFFFFFu / 2u || P.splits > 65535u) return fail(BSVI_ERR_UNSUPPORTED, "bsvi_bnn_predict_particles: too many row tiles");
    const hipStream_t s = (hipStream_t)a->stream;
    char* const ws = (char*)a->workspace_dev;

    BParams Q;
    memset(&Q, 0, sizeof Q);
    Q.uniform = p->uniform; Q.consts = p->consts; Q.params = a->params_dev;
    Q.n_layers = p->d.n_layers;
    for (uint32_t l = 0; l < Q.n_layers; ++l) {
        const bsvi_bnn_layer& S = p->layers[l];
        BnnLayerDev& D = Q.layer[l];
        D.rows = S.rows; D.cols = S.cols; D.w0 = S.weight_row0; D.b0 = S.bias_row0; D.act = S.activation;
    }
    memcpy(Q.act_p, p->act_p, sizeof Q.act_p);
    Q.R = p->R; Q.R1 = p->R1; Q.P = p->P; Q.C = p->C; Q.H1 = p->H1;
    Q.n_local = Q.n_global = a->n_particles; Q.likelihood = p->d.likelihood; Q.family = p->family;
    Q.LC = p->LC; Q.scale_u = p->scale_u; Q.scale_stride = p->scale_stride;
    Q.seed_lo = (uint32_t)a->seed; Q.seed_hi = (uint32_t)(a->seed >> 32); Q.offset_lo = (uint32_t)a->offset; Q.offset_hi = (uint32_t)(a->offset >> 32);

    BnnEnsemble E;
    memset(&E, 0, sizeof E);
    E.theta = a->theta_dev; E.ld = a->ld; E.x = a->x_dev; E.N = a->n_particles; E.M = a->n_rows;
    E.group = P.group; E.rows = P.rows; E.n_groups = P.n_groups;
    for (int t = 0; t < 2; ++t) { E.stride[t] = P.stride[t]; E.tile[t] = P.tile[t]; }
    E.p = a->p_out ? a->p_out : (float*)(ws + P.probs);
    E.z_out = a->z_out; E.draw_out = a->draw_out; E.sg = (float*)(ws + P.sigma);
    {
        static std::mutex mu;
        static size_t asked = 0;
        std::lock_guard<std::mutex> lock(mu);
        if (P.lds_bytes > asked) {
            HIP_TRY(hipFuncSetAttribute((const void*)bnn_ensemble_fwd, hipFuncAttributeMaxDynamicSharedMemorySize, (int)P.lds_bytes));
            asked = P.lds_bytes;
        }
    }
    hipLaunchKernelGGL(bnn_ensemble_fwd, dim3(P.row_tiles, P.splits), dim3(256), P.lds_bytes, s, Q, E);
    if (a->mean_out || a->var_out) {
        BnnPredict V;
        memset(&V, 0, sizeof V);
        V.M = a->n_rows; V.p = E.p; V.p_stride = (size_t)a->n_rows * p->C; V.sg = E.sg;
        V.mean_out = a->mean_out; V.var_out = a->var_out;
        hipLaunchKernelGGL(bnn_predict_reduce, dim3((a->n_rows * p->C + 255u) / 256u), dim3(256), 0, s, Q, V, a->n_rows);
    }
    HIP_TRY(hipGetLastError());
    return BSVI_OK;
}
