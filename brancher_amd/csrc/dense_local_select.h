// dense_local_select.h — the shape of a call of the local reparameterisation estimator of the dense-link path (dense_local.inc,
// DESIGN.md 4.4.2): tiles, sample splits, LDS and the workspace, as ONE pure function of the sizes.  Host only: no HIP, no look at the
// environment (dense_local.inc reads the one knob, BSVI_LOCAL_SPLITS, and hands it in); tests/c_abi/dense_local_plan.cpp walks it
// without a GPU.  Nothing of dense_select.h's plan tables is involved: the call has a launch sequence of its own.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace bsvi_dense_local {

constexpr uint32_t ROWS = 32;            // minibatch rows of a dense_local_fwd workgroup: one MFMA block
constexpr uint32_t KC = 32;              // features of a K chunk
constexpr uint32_t COLS = 32;            // features of a dense_local_bwd workgroup: one MFMA block
constexpr uint32_t LANES = 8;            // sample lanes of a workgroup: 256 threads = 32 rows x 8 lanes
constexpr uint32_t TS = 33;              // row stride of the LDS tiles (32 + 1: no bank conflicts along either axis)
constexpr uint32_t MAX_CLASSES = 16, MAX_SAMPLES = 65536, MAX_BATCH = 1u << 24;
constexpr uint32_t LDS_LIMIT = 64u * 1024u;      // static LDS of a workgroup

// LDS of the two kernels in bytes (what their __shared__ arrays add up to)
//   fwd: ONE buffer used three times — the mu and s^2 chunks of the four waves [4][2][KC][TS], then the waves' tiles of m and v
//        [4][2][ROWS][TS], then the sample lanes' sums [LANES][2][ROWS][CS] — beside the joined tile m, sd [2][ROWS][TS] and the rows'
//        likelihoods [LANES][ROWS]
constexpr uint32_t CS = 17;              // class stride of the sample lanes' sums (MAX_CLASSES + 1)
constexpr uint32_t FWD_BUF = LANES * 2u * ROWS * CS;
static_assert(FWD_BUF >= 4u * 2u * KC * TS && FWD_BUF >= 4u * 2u * ROWS * TS, "the three uses of the buffer");
constexpr uint32_t fwd_lds_bytes() { return (FWD_BUF + 2u * ROWS * TS + LANES * ROWS) * 4u; }
//   bwd: the waves' tiles of d mu and d s^2 [4][2][32][TS] and the block sums' four words
constexpr uint32_t bwd_lds_bytes() { return (4u * 2u * 32u * TS + 4u) * 4u; }

struct Plan {
    uint32_t B_pad, P_pad;               // the head's paddings of Xb [B_pad][P_pad] / XbT [P_pad][B_pad]: multiples of 64
    uint32_t row_tiles, k_chunks;        // dense_local_fwd: grid.x, and the K chunks its four waves deal out
    uint32_t splits, samples_per_split;  // grid.y; split i takes the samples [i sps, min(N, (i + 1) sps)), sps a multiple of LANES
    uint32_t col_tiles;                  // dense_local_bwd: grid.x
    uint32_t CT;                         // the register tier of the sample loop: 1, 4, 10 or 16 classes
    // byte offsets into the workspace, each 256-byte aligned
    size_t rowp, idx, Xb, XbT, lab, partial, rowg, hpart, dM, dV, jM, jV, likp, total;
};

constexpr size_t align256(size_t x) { return (x + 255u) & ~(size_t)255u; }

// force_splits: 0, or the number of sample splits asked for (BSVI_LOCAL_SPLITS; clamped to what N gives)
inline Plan local_plan(uint32_t C, uint32_t P, uint32_t B, uint32_t N, uint32_t n_cu, uint32_t n_uniform_grad, uint32_t force_splits) {
    Plan L;
    const uint32_t R = C * P;
    L.B_pad = (B + 63u) / 64u * 64u;
    L.P_pad = (P + 63u) / 64u * 64u;
    L.row_tiles = (B + ROWS - 1u) / ROWS;
    L.k_chunks = (P + KC - 1u) / KC;
    L.col_tiles = (P + COLS - 1u) / COLS;
    L.CT = C <= 1u ? 1u : C <= 4u ? 4u : C <= 10u ? 10u : 16u;
    // the sample loop is what fills the chip: two workgroups a CU (their draws and exponentials overlap), every lane at least one sample
    const uint32_t max_splits = (N + LANES - 1u) / LANES;
    uint32_t want = force_splits ? force_splits : (2u * (n_cu ? n_cu : 1u) + L.row_tiles - 1u) / L.row_tiles;
    want = want < 1u ? 1u : (want > max_splits ? max_splits : want);
    L.samples_per_split = ((N + want - 1u) / want + LANES - 1u) / LANES * LANES;
    L.splits = (N + L.samples_per_split - 1u) / L.samples_per_split;
    size_t o = 0;
    auto take = [&](size_t floats) { const size_t at = o; o += align256(floats * 4u); return at; };
    const size_t tile_floats = (size_t)L.row_tiles * ROWS * 32u;      // [row][32 classes], classes >= C and rows >= B zero
    L.rowp = take(6u * (size_t)R + 64u);
    L.idx = take(L.B_pad);
    L.Xb = take((size_t)L.B_pad * L.P_pad);
    L.XbT = take((size_t)L.P_pad * L.B_pad + 128u);
    L.lab = take(L.B_pad);
    L.partial = take(2u + (size_t)n_uniform_grad);
    L.rowg = take(4u * (size_t)R);
    L.hpart = take(L.col_tiles);
    L.dM = take((size_t)L.splits * tile_floats);
    L.dV = take((size_t)L.splits * tile_floats);
    L.jM = take(tile_floats);
    L.jV = take(tile_floats);
    L.likp = take((size_t)L.splits * L.row_tiles);
    L.total = o + 256u;
    return L;
}

}  // namespace bsvi_dense_local
