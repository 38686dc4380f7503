// dense_predict.inc — the posterior predictive of a dense-link model (logistic regression) and of its particle ensembles, forward only
// (included by elbo_kernel.hip behind dense_particles.inc; DESIGN.md 4.8).
//
// For M rows x[m] the CALLER hands in and N weight sets W_n [C][P] (rows r = c P + p):
//   logits[n][m][c] = sum_p W_n[c P + p] x[m][p],   probs[n][m][:] = softmax(logits[n][m][:]) | sigmoid of the one logit (C = 1),
//   mean[m][c] = (1 / N) sum_n probs[n][m][c],   and on request one draw of the likelihood per (n, m): one-hot | 0 / 1.
// The weight sets come from one of three sources behind the same kernel body (the template argument):
//   DPR_PHILOX  W_n = mu + s eps_n, eps from dense_eps4 — the dense path's one noise definition, so a prediction at (seed, offset,
//               sample_base) sees exactly the weights a training launch at the same triple drew; a point estimate has s = 0
//   DPR_NOISE   the same with the caller's eps [R][N]
//   DPR_TABLE   W_n = theta[n] of an [N][ld] table in the layout of bsvi_dense_particles_fwd_bwd, read in place (any ld >= C P, any
//               alignment: scalar loads)
//
//   dense_predict_head  X [M][P] -> XT [P_pad][M_pad] through 64 x 64 LDS tiles (both sides coalesced; M_pad a multiple of 128, P_pad
//                       even, zero where m >= M or p >= P), and in the sampled modes mu and s of every row from the uniform table, as
//                       dense_prologue writes them.  No minibatch, no labels.
//   dense_predict       grid (M_pad / 128, splits), 256 threads.  A workgroup owns 128 rows of X, a 32-column MFMA block per wave, and
//                       walks its share of the weight sets in groups of NS = floor(32 / C) whole sets: one 32-row block of (set, class)
//                       rows, row = s C + c, dead rows zero.
//     phase 1  logits on v_mfma_f32_32x32x2_f32.  A = the group's W block, k-major in LDS, Wk[k][row] with row stride 33, two buffers,
//              one barrier per chunk of 32 features, BUILT while staging: thread (row tid >> 3, features 4 (tid & 7) .. + 3) reads the
//              table, or draws — its four features are one quad of rows r, one Philox call (two when C P + p is no multiple of 4: the
//              quads are those of r, as in training) — and forms mu + s eps in registers behind the products of the chunk before.
//              B = XT straight from global memory, the next chunk's 16 values in registers.  Nothing is accumulated per feature: P
//              has no upper limit; rows k >= P_pad are not read.
//     phase 2  accumulators -> tile T[column][row] (row stride 33); logits leave from there when asked for; a lane takes (column, set)
//              pairs, lanes along the columns: max, sum of exp, probabilities in place (sigmoid for C = 1), and the draw's class into
//              Kd[set][column].
//     sweep    of set s, probs[n][m0 .. m0 + 127][0 .. C) is ONE contiguous run of 128 C floats: thread t takes elements t, t + 256, ...
//              (at most 16), consecutive lanes write consecutive dwords whatever C is.  The same elements are the thread's cells of the
//              mean: it adds the group's sets to them in ascending set order, in registers.
//   mean       one split: divided by N and stored.  Few row tiles (the scripts' one-row call): the set groups are dealt over grid.y, as
//              many splits as leave no CU a second workgroup, the sums go to part[split][M][C] and
//   dense_predict_join  adds them in split order and divides by N.
// No atomics, every sum in a fixed order: two calls leave the same bits.  Rows m >= M and sets n >= N contribute nothing and are never
// stored.  The draw's uniform is u01(word m & 3) of Philox counter (sample_base + n, (m >> 2) | 0x20000000, offset, seed): a tag of its
// own next to the weights' 0x40000000 (philox.h).

constexpr uint32_t DPR_PHILOX = 0, DPR_NOISE = 1, DPR_TABLE = 2;
constexpr uint32_t DPR_COLS = 128, DPR_TS = 33, DPR_CELLS = 16, DPR_DRAW_TAG = 0x20000000u;

struct DensePredict {
    const float* theta;      // [N][ld]          (DPR_TABLE)
    const float* rowp;       // mu [R], s [R]    (sampled)
    const float* noise_in;   // [R][N]           (DPR_NOISE)
    float* noise_out;        // [R][N] or null
    const float* X;          // [M][P]
    float* XT;               // [P_pad][M_pad]
    float* probs; float* mean; float* logits; float* draws;      // each may be null
    float* part;             // [splits][M][C]
    uint64_t ld;
    uint32_t N, C, P, R, M, M_pad, P_pad, NS, n_groups, groups_per_split, splits, likelihood, sample_base;
    uint32_t seed_lo, seed_hi, offset_lo, offset_hi;
};

// blocks [0, n_tiles): a 64-row x 64-feature tile of X, transposed through LDS; behind them 256 rows of the row parameters each
__global__ void __launch_bounds__(256) dense_predict_head(const DParams D, const DensePredict T, const uint32_t n_tiles) {
    __shared__ float tile[64][65];
    const uint32_t tid = threadIdx.x;
    if (blockIdx.x < n_tiles) {
        const uint32_t ptiles = (T.P_pad + 63u) / 64u, tm = blockIdx.x / ptiles, tp = blockIdx.x - tm * ptiles;
        const uint32_t m0 = tm * 64u, p0 = tp * 64u, c = tid & 63u, q = tid >> 6;
#pragma unroll
        for (uint32_t k = 0; k < 16; ++k) {
            const uint32_t m = m0 + q + 4u * k, p = p0 + c;
            tile[q + 4u * k][c] = (m < T.M && p < T.P) ? T.X[(size_t)m * T.P + p] : 0.0f;
        }
        __syncthreads();
        for (uint32_t pp = q; pp < 64u; pp += 4u)
            if (p0 + pp < T.P_pad) T.XT[(size_t)(p0 + pp) * T.M_pad + m0 + c] = tile[c][pp];      // (m0 + c < M_pad: a multiple of 64)
        return;
    }
    const uint32_t r = (blockIdx.x - n_tiles) * 256u + tid;
    if (r < T.R) {
        D.rowp[r] = uniform_value(D, D.q_loc_u + r * D.q_loc_stride);
        D.rowp[T.R + r] = uniform_value(D, D.q_scale_u + r * D.q_scale_stride);
    }
}

// (one workgroup a CU: the unrolled sweeps take 244 .. 256 VGPRs and 16 .. 48 AGPRs, no scratch; __launch_bounds__(256, 2) fits the table
//  variant into 256 registers but spills 92 .. 100 bytes a lane in the two sampled ones — set aside, profiles/r29/dense_predict.txt)
template <uint32_t SRC>
__global__ void __launch_bounds__(256) dense_predict(const DensePredict T) {
    __shared__ float Wk[2][32 * DPR_TS];
    __shared__ float Tt[DPR_COLS * DPR_TS];
    __shared__ uint8_t Kd[32 * DPR_COLS];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, lm = lane & 31u, lk = lane >> 5;
    const uint32_t m0 = blockIdx.x * DPR_COLS, split = blockIdx.y, live_rows = T.NS * T.C;
    const uint32_t n_chunk = (T.P + 31u) / 32u;
    const uint32_t col = wave * 32u + lm, m = m0 + col;                      // (m < M_pad)
    const uint32_t run = min(T.M - m0, DPR_COLS) * T.C;                      // floats of a set's rows of this tile that exist
    DParams Dn;                                                              // (what dense_eps4 reads)
    Dn.sample_base = T.sample_base; Dn.offset_lo = T.offset_lo; Dn.offset_hi = T.offset_hi; Dn.seed_lo = T.seed_lo; Dn.seed_hi = T.seed_hi;

    // the thread's elements e = tid + 256 j of a set's run: where they sit in the tile (without the set's s C), and their sums over the sets
    uint32_t toff[DPR_CELLS];
    float macc[DPR_CELLS];
#pragma unroll
    for (int j = 0; j < (int)DPR_CELLS; ++j) {
        const uint32_t e = tid + 256u * j, ec = e / T.C;
        toff[j] = ec * DPR_TS + (e - ec * T.C);
        macc[j] = 0.0f;
    }

    // staging of W: thread = (block row tid >> 3, features 4 (tid & 7) .. + 3 of the chunk)
    const uint32_t srow = tid >> 3, sfq = tid & 7u, ss = srow / T.C, sc = srow - ss * T.C;
    float tr[4];
    auto fetch_w = [&](const uint32_t n0, const uint32_t chunk) {
        const uint32_t p0 = chunk * 32u + 4u * sfq, n = n0 + ss;
#pragma unroll
        for (int i = 0; i < 4; ++i) tr[i] = 0.0f;
        if (srow >= live_rows || n >= T.N || p0 >= T.P) return;
        const uint32_t r0 = sc * T.P + p0;
        if (SRC == DPR_TABLE) {
            const float* const th = T.theta + (size_t)n * T.ld + r0;
#pragma unroll
            for (int i = 0; i < 4; ++i) tr[i] = p0 + i < T.P ? th[i] : 0.0f;
            return;
        }
        float e[4];
        if (SRC == DPR_NOISE) {
#pragma unroll
            for (int i = 0; i < 4; ++i) e[i] = p0 + i < T.P ? T.noise_in[(size_t)(r0 + i) * T.N + n] : 0.0f;
        } else {
            // rows r0 .. r0 + 3 lie in quad r0 >> 2 and, when r0 is no multiple of 4, in the next
            const uint32_t sh = r0 & 3u;
            float ea[4], eb[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            dense_eps4(Dn, n, r0 >> 2, ea);
            if (sh != 0u) dense_eps4(Dn, n, (r0 >> 2) + 1u, eb);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint32_t at = sh + i;
                e[i] = at == 0u ? ea[0] : at == 1u ? ea[1] : at == 2u ? ea[2] : at == 3u ? ea[3] : at == 4u ? eb[0] : at == 5u ? eb[1] : eb[2];
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (p0 + i >= T.P) continue;
            if (T.noise_out && blockIdx.x == 0u) T.noise_out[(size_t)(r0 + i) * T.N + n] = e[i];
            tr[i] = T.rowp[r0 + i] + T.rowp[T.R + r0 + i] * e[i];
        }
    };
    auto commit_w = [&](const uint32_t buf) {
#pragma unroll
        for (int i = 0; i < 4; ++i) Wk[buf][(4u * sfq + i) * DPR_TS + srow] = tr[i];
    };

    const float* const xt = T.XT + (size_t)lk * T.M_pad + m;                 // + (32 chunk + 2 kk) M_pad: rows < P_pad exist
    float bc[16], bn[16];
    auto fetch_x = [&](const uint32_t chunk, float* const b) {
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) {
            const uint32_t k = 32u * chunk + 2u * kk;
            b[kk] = k + lk < T.P_pad ? xt[(size_t)k * T.M_pad] : 0.0f;
        }
    };

    const uint32_t g0 = split * T.groups_per_split, g1 = min(g0 + T.groups_per_split, T.n_groups);
    for (uint32_t g = g0; g < g1; ++g) {
        const uint32_t n0 = g * T.NS;
        // ---- phase 1: logits[row][m] of the wave's 32 columns
        xf_f32x16 lg;
#pragma unroll
        for (int r = 0; r < 16; ++r) lg[r] = 0.0f;
        fetch_w(n0, 0);
        fetch_x(0, bc);
        commit_w(0);
        __syncthreads();
        for (uint32_t chunk = 0; chunk < n_chunk; ++chunk) {
            const bool more = chunk + 1u < n_chunk;
            if (more) {
                fetch_w(n0, chunk + 1u);
                fetch_x(chunk + 1u, bn);
            }
            const float* const wk = Wk[chunk & 1u] + lk * DPR_TS + lm;
#pragma unroll
            for (int kk = 0; kk < 16; ++kk) lg = __builtin_amdgcn_mfma_f32_32x32x2f32(wk[2 * kk * DPR_TS], bc[kk], lg, 0, 0, 0);
            if (more) {
                commit_w((chunk + 1u) & 1u);      // (last read before the previous barrier)
#pragma unroll
                for (int kk = 0; kk < 16; ++kk) bc[kk] = bn[kk];
            }
            __syncthreads();
        }
        // ---- phase 2: lg[r] is logits[row = 8 (r >> 2) + 4 lk + (r & 3)][column lm of the wave]  ->  T[column][row]
        // (every wave left the sweep of the group before through the barriers of phase 1)
#pragma unroll
        for (int r = 0; r < 16; ++r) Tt[col * DPR_TS + 8u * (r >> 2) + 4u * lk + (r & 3)] = lg[r];
        __syncthreads();
        if (T.logits) {
            for (uint32_t s = 0; s < T.NS && n0 + s < T.N; ++s) {
                float* const out = T.logits + ((size_t)(n0 + s) * T.M + m0) * T.C;
#pragma unroll
                for (int j = 0; j < (int)DPR_CELLS; ++j) {
                    const uint32_t e = tid + 256u * j;
                    if (e < run) out[e] = Tt[toff[j] + s * T.C];
                }
            }
            __syncthreads();
        }
        for (uint32_t s = lk; s < T.NS; s += 2u) {
            if (n0 + s >= T.N || m >= T.M) continue;
            float* const t = Tt + col * DPR_TS + s * T.C;
            float u = 0.0f;
            if (T.draws) {
                const u32x4 x = philox4x32(T.sample_base + n0 + s, (m >> 2) | DPR_DRAW_TAG, T.offset_lo, T.offset_hi, T.seed_lo, T.seed_hi);
                const uint32_t w = m & 3u;
                u = u01(w == 0u ? x.x : w == 1u ? x.y : w == 2u ? x.z : x.w);
            }
            if (T.likelihood == BSVI_LIK_CATEGORICAL) {
                float mx = t[0];
                for (uint32_t c = 1; c < T.C; ++c) mx = fmaxf(mx, t[c]);
                float se = 0.0f;
                for (uint32_t c = 0; c < T.C; ++c) {
                    const float e = expf(t[c] - mx);
                    se += e;
                    t[c] = e;
                }
                const float inv = 1.0f / se;
                // the inverse CDF on the stored probabilities, in class order: the first class whose partial sum is >= u, else the last
                float cum = 0.0f;
                uint32_t k = T.C - 1u;
                for (uint32_t c = 0; c < T.C; ++c) {
                    const float pc = t[c] * inv;
                    t[c] = pc;
                    cum += pc;
                    if (cum >= u && k == T.C - 1u) k = c;
                }
                Kd[s * DPR_COLS + col] = (uint8_t)k;
            } else {      // Bernoulli / Binomial(1): the class of the one-hot rule below is 0 for a draw of 1
                const float pr = sigmoidf_(t[0]);
                t[0] = pr;
                Kd[s * DPR_COLS + col] = u < pr ? 0u : 1u;
            }
        }
        __syncthreads();
        // ---- sweep: a set's rows of this tile are one contiguous run; the thread's elements are its cells of the mean
        for (uint32_t s = 0; s < T.NS && n0 + s < T.N; ++s) {
            const size_t at = ((size_t)(n0 + s) * T.M + m0) * T.C;
#pragma unroll
            for (int j = 0; j < (int)DPR_CELLS; ++j) {
                const uint32_t e = tid + 256u * j;
                if (e >= run) continue;
                const float v = Tt[toff[j] + s * T.C];
                macc[j] += v;
                if (T.probs) T.probs[at + e] = v;
                if (T.draws) {
                    const uint32_t ec = toff[j] / DPR_TS, c = toff[j] - ec * DPR_TS;
                    T.draws[at + e] = Kd[s * DPR_COLS + ec] == c ? 1.0f : 0.0f;
                }
            }
        }
    }
    float* const out = T.splits > 1u ? T.part + ((size_t)split * T.M + m0) * T.C : (T.mean ? T.mean + (size_t)m0 * T.C : nullptr);
    if (!out) return;
    const float count = (float)T.N;
#pragma unroll
    for (int j = 0; j < (int)DPR_CELLS; ++j) {
        const uint32_t e = tid + 256u * j;
        if (e < run) out[e] = T.splits > 1u ? macc[j] : macc[j] / count;
    }
}

// the splits' sums of a cell in split order, divided by N
__global__ void __launch_bounds__(256) dense_predict_join(const DensePredict T) {
    const size_t cells = (size_t)T.M * T.C, i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= cells) return;
    float v = 0.0f;
    for (uint32_t s = 0; s < T.splits; ++s) v += T.part[(size_t)s * cells + i];
    T.mean[i] = v / (float)T.N;
}

// ---- host side -------------------------------------------------------------------------------------------------------------
struct DensePredictPlan {
    uint32_t M_pad, P_pad, NS, n_groups, row_tiles, groups_per_split, splits;
    size_t rowp, XT, part, total;      // byte offsets into the workspace, each 256-byte aligned
};

static int dense_predict_check(const bsvi_dense* p, const uint64_t n_sets, const uint64_t n_rows) {
    if (!p) return fail(BSVI_ERR_INVALID, "bsvi_dense_predict: null handle");
    if (n_sets < 1) return fail(BSVI_ERR_INVALID, "bsvi_dense_predict: n_sets is 0, a prediction needs at least one weight set");
    if (n_rows < 1) return fail(BSVI_ERR_INVALID, "bsvi_dense_predict: n_rows is 0, a prediction needs at least one row");
    if (p->d.n_classes > 32u)
        return fail(BSVI_ERR_UNSUPPORTED, "bsvi_dense_predict: " + std::to_string(p->d.n_classes) + " classes, served are 1 .. 32 (a set's rows share one 32-row block)");
    if (n_sets * n_rows * p->d.n_classes >= (1ull << 31))
        return fail(BSVI_ERR_INVALID, "bsvi_dense_predict: n_sets x n_rows x classes is " + std::to_string(n_sets * n_rows * p->d.n_classes) + ", served is less than 2^31");
    return BSVI_OK;
}

static DensePredictPlan dense_predict_plan(const bsvi_dense* p, const uint32_t N, const uint32_t M, const uint32_t sets_per_split) {
    DensePredictPlan L;
    const uint32_t C = p->d.n_classes, P = p->d.n_features;
    L.M_pad = (M + DPR_COLS - 1u) / DPR_COLS * DPR_COLS;
    L.P_pad = P + (P & 1u);
    L.NS = 32u / C;
    L.n_groups = (N + L.NS - 1u) / L.NS;
    L.row_tiles = L.M_pad / DPR_COLS;
    if (sets_per_split) {
        L.groups_per_split = (sets_per_split + L.NS - 1u) / L.NS;
    } else {      // few row tiles for the chip: the groups go over a second grid axis, as many splits as leave no CU a second workgroup
        uint32_t want = p->m.n_cu / L.row_tiles;
        want = want < 1u ? 1u : (want > L.n_groups ? L.n_groups : want);
        L.groups_per_split = (L.n_groups + want - 1u) / want;
    }
    if (L.groups_per_split > L.n_groups) L.groups_per_split = L.n_groups;
    L.splits = (L.n_groups + L.groups_per_split - 1u) / L.groups_per_split;
    size_t o = 0;
    auto take = [&](size_t floats) { const size_t at = o; o += align_up(floats * 4, 256); return at; };
    L.rowp = take(2 * (size_t)C * P);
    L.XT = take((size_t)L.P_pad * L.M_pad);
    L.part = take(L.splits > 1u ? (size_t)L.splits * M * C : 1);
    L.total = o + 256;
    return L;
}

extern "C" size_t bsvi_dense_predict_args_size(void) { return sizeof(bsvi_dense_predict_args); }

extern "C" size_t bsvi_dense_predict_workspace_bytes(const bsvi_dense* p, uint32_t n_sets, uint32_t n_rows, uint32_t sets_per_split) {
    if (dense_predict_check(p, n_sets, n_rows)) return 0;
    return dense_predict_plan(p, n_sets, n_rows, sets_per_split).total;
}

extern "C" int bsvi_dense_predict(const bsvi_dense* p, const bsvi_dense_predict_args* a) {
    if (!a) return fail(BSVI_ERR_INVALID, "bsvi_dense_predict: null argument");
    BSVI_CHECK_STRUCT(a, bsvi_dense_predict_args);
    const int rc = dense_predict_check(p, a->n_sets, a->n_rows);
    if (rc) return rc;
    const uint32_t C = p->d.n_classes, P = p->d.n_features, R = C * P, N = a->n_sets, M = a->n_rows;
    const bool table = a->theta_dev != nullptr;
    if (!a->x_dev || !a->workspace_dev || (!table && !a->params_dev))
        return fail(BSVI_ERR_INVALID, "bsvi_dense_predict: null argument (x_dev, workspace_dev, and params_dev of a sampled call)");
    if (table && a->noise_dev) return fail(BSVI_ERR_INVALID, "bsvi_dense_predict: a table call (theta_dev) takes no noise_dev: nothing is drawn");
    if (table && a->noise_out) return fail(BSVI_ERR_INVALID, "bsvi_dense_predict: a table call (theta_dev) has no noise_out: nothing is drawn");
    if (table && a->ld < R) return fail(BSVI_ERR_INVALID, "bsvi_dense_predict: ld is " + std::to_string(a->ld) + ", a weight set has " + std::to_string(R) + " values");
    if ((uint64_t)N * (table ? a->ld : (uint64_t)R) >= (1ull << 31)) return fail(BSVI_ERR_INVALID, "bsvi_dense_predict: n_sets x ld beyond 2^31");
    if (!table && C > 16u)
        return fail(BSVI_ERR_UNSUPPORTED, "bsvi_dense_predict: a sampled call on a handle of " + std::to_string(C) + " classes; the dense path samples at most 16 classes (17 .. 32 serve tables of particles)");
    const DensePredictPlan L = dense_predict_plan(p, N, M, a->sets_per_split);
    char* const ws = (char*)a->workspace_dev;
    DParams D;
    memset(&D, 0, sizeof(D));
    D.uniform = p->uniform; D.consts = p->consts; D.params = a->params_dev; D.rowp = (float*)(ws + L.rowp);
    D.q_loc_u = p->d.q_loc_u; D.q_scale_u = p->d.q_scale_u; D.q_loc_stride = p->d.q_loc_stride; D.q_scale_stride = p->d.q_scale_stride;
    DensePredict T;
    memset(&T, 0, sizeof(T));
    T.theta = a->theta_dev; T.ld = a->ld; T.rowp = D.rowp; T.noise_in = a->noise_dev; T.noise_out = a->noise_out;
    T.X = a->x_dev; T.XT = (float*)(ws + L.XT); T.part = (float*)(ws + L.part);
    T.probs = a->p_out; T.mean = a->mean_out; T.logits = a->z_out; T.draws = a->draw_out;
    T.N = N; T.C = C; T.P = P; T.R = R; T.M = M; T.M_pad = L.M_pad; T.P_pad = L.P_pad; T.NS = L.NS; T.n_groups = L.n_groups;
    T.groups_per_split = L.groups_per_split; T.splits = L.splits; T.likelihood = p->d.likelihood; T.sample_base = a->sample_base;
    T.seed_lo = (uint32_t)a->seed; T.seed_hi = (uint32_t)(a->seed >> 32);
    T.offset_lo = (uint32_t)a->offset; T.offset_hi = (uint32_t)(a->offset >> 32);
    const hipStream_t s = (hipStream_t)a->stream;
    const uint32_t n_tiles = (L.M_pad / 64u) * ((L.P_pad + 63u) / 64u), n_rowp = table ? 0u : (R + 255u) / 256u;
    hipLaunchKernelGGL(dense_predict_head, dim3(n_tiles + n_rowp), dim3(256), 0, s, D, T, n_tiles);
    const dim3 grid(L.row_tiles, L.splits), block(256);
    if (table) hipLaunchKernelGGL(dense_predict<DPR_TABLE>, grid, block, 0, s, T);
    else if (a->noise_dev) hipLaunchKernelGGL(dense_predict<DPR_NOISE>, grid, block, 0, s, T);
    else hipLaunchKernelGGL(dense_predict<DPR_PHILOX>, grid, block, 0, s, T);
    if (L.splits > 1u && T.mean) hipLaunchKernelGGL(dense_predict_join, dim3((uint32_t)(((size_t)M * C + 255u) / 256u)), block, 0, s, T);
    HIP_TRY(hipGetLastError());
    return BSVI_OK;
}
