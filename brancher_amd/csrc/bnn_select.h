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
