// bnn_select.h — which kernel serves the middle of a Bayesian-neural-network iteration (upper layers, likelihood, reverse sweep), and the
// LDS each of them asks for: ONE pure function from the network's size to the kind.  Host only: no HIP, no getenv —
// bnn_kernel.inc fills the input (bnn_gen_ready, bnn_create); tests/c_abi/bnn_select_table.cpp walks the table without a GPU.
// A kernel that does not compile is not this header's business: the fallbacks stay where the compile is tried.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace bsvi_bnn_select {

// The values are public: bsvi_bnn_middle returns them.
enum BnnMiddle {
    MID_GEN = 0,            // bnn_mid_gen: generated, one workgroup per sample, lanes along the minibatch rows (exact-bf16 data only)
    UPPER_GEN = 1,          // bnn_upper_gen: generated, small tensors and activations in registers
    UPPER_LDS = 2,          // bnn_upper<true>: static, small tensors and activations in LDS
    UPPER_MEM = 3           // bnn_upper<false>: static, activations and deltas in global memory
};

constexpr size_t LDS_LIMIT = 150u * 1024u;          // what a workgroup may ask of a CU's 160 KiB
constexpr uint32_t MID_MAX_ACT = 96;                // units bnn_mid_gen keeps per thread (y and d: twice that many registers)
constexpr uint32_t GEN_MAX_FLOATS = 400;            // Rs + 2 act_floats floats per thread of bnn_upper_gen: the register file

struct Switches { bool mid_off = false, jit_off = false; };      // BSVI_BNN_MID=0, BSVI_BNN_JIT=0

// Rs: rows of the latent vector behind weights1 (every bias, every upper weight matrix; 0 is staged as 1); act_floats: the sum of all
// layer widths; B_pad: the minibatch rounded up to 32 rows
inline size_t rows(uint32_t Rs) { return Rs ? Rs : 1u; }
// bnn_mid_gen: the sample's small tensors [Rs4] | the tile [2 act_floats][B_pad + 4]
inline size_t mid_lds_bytes(uint32_t Rs, uint64_t act_floats, uint32_t B_pad) {
    return ((rows(Rs) + 3u) / 4u * 4u + 2u * (size_t)act_floats * ((size_t)B_pad + 4u)) * 4u;
}
// bnn_upper_gen: the staging tile [Rs][65] of the workgroup's 64 samples
inline size_t upper_gen_lds_bytes(uint32_t Rs) { return rows(Rs) * 65u * 4u; }
// bnn_upper<true>: that tile, then activations and deltas [2 act_floats][256]
inline size_t upper_lds_bytes(uint32_t Rs, uint64_t act_floats) { return (rows(Rs) * 65u + 2u * (size_t)act_floats * 256u) * 4u; }

inline BnnMiddle middle(uint32_t Rs, uint64_t act_floats, uint32_t B_pad, bool exact, Switches sw) {
    if (!sw.mid_off && exact && mid_lds_bytes(Rs, act_floats, B_pad) <= LDS_LIMIT && act_floats <= MID_MAX_ACT && B_pad % 4u == 0u) return MID_GEN;
    if (!sw.jit_off && (uint64_t)Rs + 2u * act_floats <= GEN_MAX_FLOATS && upper_gen_lds_bytes(Rs) <= LDS_LIMIT) return UPPER_GEN;
    return upper_lds_bytes(Rs, act_floats) <= LDS_LIMIT ? UPPER_LDS : UPPER_MEM;
}

// ---- the first layer of a network whose weights1 is a point estimate (bsvi_bnn_set_point_rows): every sample then sees the same
// weights1, so the first product is taken once and broadcast, and the second after the sum over the samples ("shared"); else both
// products run per sample as for any network.  row_point: the point byte of every row (null: no row is a point), of which the first
// R1 = H1 P are weights1's; shared_off: BSVI_BNN_SHARED1=0.  b1 and every other tensor may be anything.
inline bool shared_first(const uint8_t* row_point, uint32_t R1, bool shared_off) {
    if (shared_off || !row_point || !R1) return false;
    for (uint32_t r = 0; r < R1; ++r)
        if (!row_point[r]) return false;
    return true;
}

// ---- the posterior-predictive pass (bsvi_bnn_predict): forward only, so a thread keeps TWO activation buffers of the widest layer
// (ping-pong) instead of every layer's activations and deltas.  max_width: the widest layer's output (the largest layers[l].rows).
// bnn_predict_fwd<true>: the staging tile [Rs][65] of the workgroup's 64 samples, then the two buffers [2 max_width][256]
inline size_t predict_lds_bytes(uint32_t Rs, uint32_t max_width) { return (rows(Rs) * 65u + 2u * (size_t)max_width * 256u) * 4u; }
// true: bnn_predict_fwd<true> (small tensors and activations in LDS); false: bnn_predict_fwd<false> (both through global memory)
inline bool predict_lds(uint32_t Rs, uint32_t max_width) { return predict_lds_bytes(Rs, max_width) <= LDS_LIMIT; }

constexpr size_t PREDICT_A1_BYTES = 64u << 20;      // what the default rows_per_pass lets the first product's result take
// rows of a pass when the caller names none: a multiple of 32 that keeps a1 [rows][H1 n_pad] within PREDICT_A1_BYTES and the products'
// 32-bit index range, never more than the rows there are (rounded up to 32), never less than 32
inline uint32_t predict_rows_per_pass(uint32_t H1, uint32_t n_pad, uint32_t n_rows) {
    const uint64_t nc = (uint64_t)H1 * n_pad, all = ((uint64_t)n_rows + 31u) / 32u * 32u;
    uint64_t r = PREDICT_A1_BYTES / (nc * 4u) / 32u * 32u;
    const uint64_t idx = ((1ull << 31) - 1u) / nc / 32u * 32u;
    if (r > idx) r = idx;
    if (r > all) r = all;
    return (uint32_t)(r < 32u ? 32u : r);
}

struct PredictLayout {
    size_t rowp, sg, flag, Wsm, W1, part, X, a1, act, p, total;
    uint32_t n_pad, NC, row_chunks, rows_pass;
};
// the workspace of a predict call (every region 256-byte aligned): row parameters [4][R] | sigma [C] | the exact-data flag | the small
// tensors [n_pad][Rs] | weights1 as the product's operand (three bf16 pieces [3][NC][Kp] or f32 [NC][P_ld]: room for either, the rows
// handed in decide) | the draw's per-chunk partials (written, never read) | the rows of a pass (bf16 [rows][Kp] or f32 [rows][P_ld]) |
// a1 [rows][NC] | the activations of the global arm [2 max_width][rows][n_pad] | p of a pass [n][rows][C] when the caller keeps none
inline PredictLayout predict_layout(uint32_t R, uint32_t Rs, uint32_t P, uint32_t C, uint32_t H1, uint32_t max_width, uint32_t n_local,
                                    uint32_t n_rows, uint32_t rows_per_pass) {
    PredictLayout L{};
    L.n_pad = (n_local + 63u) / 64u * 64u;
    L.NC = H1 * L.n_pad;
    L.row_chunks = ((R + 3u) / 4u + 63u) / 64u;
    L.rows_pass = rows_per_pass ? rows_per_pass : predict_rows_per_pass(H1, L.n_pad, n_rows);
    const size_t Kp = ((size_t)P + 31u) / 32u * 32u, P_ld = ((size_t)P + 3u) / 4u * 4u, rp = L.rows_pass;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += (bytes + 255u) / 256u * 256u; return at; };
    auto larger = [](size_t a, size_t b) { return a > b ? a : b; };
    L.rowp = take(4u * (size_t)R * 4u); L.sg = take((size_t)C * 4u); L.flag = take(4u);
    L.Wsm = take((size_t)L.n_pad * rows(Rs) * 4u);
    L.W1 = take(larger(3u * (size_t)L.NC * Kp * 2u, (size_t)L.NC * P_ld * 4u));
    L.part = take(2u * (size_t)L.row_chunks * L.n_pad * 4u);
    L.X = take(larger(rp * Kp * 2u, rp * P_ld * 4u));
    L.a1 = take(rp * L.NC * 4u);
    L.act = take(predict_lds(Rs, max_width) ? 0u : 2u * (size_t)max_width * rp * L.n_pad * 4u);
    L.p = take((size_t)n_local * rp * C * 4u);
    L.total = o + 256u;
    return L;
}

// ---- the predictive of a particle ensemble (bsvi_bnn_predict_particles, bnn_ensemble.inc): every size its launch derives.
// A workgroup of 256 owns `rows` rows of x (128; 64 or 32 when two activation tiles of 128 rows do not fit) and walks groups of `group`
// particles.  LDS, in floats: the staged K chunks of A and B, two buffers each [2][128][ENS_CHUNK + 1] | tile 0 | tile 1, tile t
// [group][rows][stride_t] holding the outputs of the layers l with l % 2 == t (stride: the widest of them plus one slot, odd).
constexpr uint32_t ENS_ROWS = 128, ENS_CHUNK = 32, ENS_BLOCKS = 4, ENS_MAX_WIDTH = 320, ENS_WORKGROUPS = 512;
constexpr size_t ENS_STAGE_FLOATS = 2u * 2u * ENS_ROWS * (ENS_CHUNK + 1u);

struct EnsemblePlan {
    uint32_t served;                // 0: a layer is wider than ENS_MAX_WIDTH (`widest` names it)
    uint32_t widest;
    uint32_t group;                 // particles a workgroup carries at once
    uint32_t blocks;                // 32-column MFMA blocks held in accumulators at once (of the first product's columns group x H1)
    uint32_t rows;                  // rows of x per workgroup
    uint32_t stride[2], tile[2];    // the tiles' row strides and offsets, in floats
    size_t lds_bytes;
    uint32_t n_groups, row_tiles, splits;      // grid (row_tiles, splits): split y takes the groups y, y + splits, ...
    size_t sigma, probs, workspace_bytes;      // the workspace: sigma [C] | probs [N][M][C] (used when the caller keeps none)
};

// widths: the layers' output widths (hidden ..., C), n_layers of them
inline EnsemblePlan ensemble_plan(const uint32_t* widths, uint32_t n_layers, uint32_t n_particles, uint32_t n_rows) {
    EnsemblePlan E{};
    uint32_t w[2] = {0u, 0u};
    for (uint32_t l = 0; l < n_layers; ++l) {
        if (widths[l] > E.widest) E.widest = widths[l];
        if (widths[l] > w[l & 1u]) w[l & 1u] = widths[l];
    }
    const uint32_t C = n_layers ? widths[n_layers - 1u] : 0u, H1 = n_layers ? widths[0] : 0u;
    if (!n_layers || !H1 || !n_particles || !n_rows || E.widest > ENS_MAX_WIDTH) return E;
    // (the head leaves the probabilities and the draw's class beside the logits' tile: C + 1 slots of the other one)
    if (w[n_layers & 1u] < C + 1u) w[n_layers & 1u] = C + 1u;
    for (uint32_t t = 0; t < 2u; ++t) E.stride[t] = (w[t] + 1u) | 1u;
    const uint32_t cols = ENS_BLOCKS * 32u;
    uint32_t fit = H1 >= cols ? 1u : cols / H1;
    if (fit > n_particles) fit = n_particles;
    for (uint32_t rows = ENS_ROWS; rows >= 32u && !E.group; rows /= 2u)
        for (uint32_t g = fit; g >= 1u; --g)
            if ((ENS_STAGE_FLOATS + (size_t)g * rows * (E.stride[0] + E.stride[1])) * 4u <= LDS_LIMIT) { E.group = g; E.rows = rows; break; }
    if (!E.group) return E;      // (never for a width within ENS_MAX_WIDTH: one particle on 32 rows fits)
    E.served = 1u;
    const uint32_t first_blocks = (E.group * H1 + 31u) / 32u;
    E.blocks = first_blocks < ENS_BLOCKS ? first_blocks : ENS_BLOCKS;
    E.tile[0] = (uint32_t)ENS_STAGE_FLOATS;
    E.tile[1] = E.tile[0] + E.group * E.rows * E.stride[0];
    E.lds_bytes = ((size_t)E.tile[1] + (size_t)E.group * E.rows * E.stride[1]) * 4u;
    E.n_groups = (n_particles + E.group - 1u) / E.group;
    E.row_tiles = (n_rows + E.rows - 1u) / E.rows;
    // few row tiles (the one-row call): the groups are dealt over grid.y until the chip has ENS_WORKGROUPS workgroups
    E.splits = E.row_tiles >= ENS_WORKGROUPS ? 1u : (ENS_WORKGROUPS + E.row_tiles - 1u) / E.row_tiles;
    if (E.splits > E.n_groups) E.splits = E.n_groups;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += (bytes + 255u) / 256u * 256u; return at; };
    E.sigma = take((size_t)C * 4u);
    E.probs = take((size_t)n_particles * n_rows * C * 4u);
    E.workspace_bytes = o + 256u;
    return E;
}

inline const char* name(int kind) {
    switch (kind) {
    case MID_GEN: return "mid_gen";
    case UPPER_GEN: return "upper_gen";
    case UPPER_LDS: return "upper_lds";
    case UPPER_MEM: return "upper_mem";
    default: return "?";
    }
}

}  // namespace bsvi_bnn_select
