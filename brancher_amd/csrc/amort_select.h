// amort_select.h — which kernel serves a product of the amortised path (amort_kernel.hip), with which grid, dynamic LDS and derived
// arguments; how a weight gradient is cut along its rows; and which product path a layer takes: pure functions of the shape, the
// operands' addresses and the switches.  Host only: no HIP, no look at the environment — amort_kernel.hip fills Switches from the
// environment and Facts from the launch arguments; tests/c_abi/amort_select_table.cpp walks the table without a GPU.
//
// Oddities kept as they were found (the launchers' behaviour is this header's specification):
//  - BSVI_X6_DEBUG 2, 3, 4, 5, 9 apply to the forward (NT) product only, 12 and 13 (= 10 + DBG) to the input-gradient (NN) one; every
//    other value is ignored.  A DBG form is taken AHEAD of the fused likelihood (`lik` is then false: the caller launches amort_lik)
//    and ahead of BSVI_X6_VAR; DBG 9 is the only one built on the hand-ordered main loop.
//  - BSVI_X6_VAR: only 1 selects the hand-ordered loop; every other value the compiler's order.  The LIK form is always hand-ordered.
//  - BSVI_X6_V=5, a misaligned operand, N not a multiple of 4, or either 2^31 byte guard sends a six-piece product to round 5's
//    register-staged kernel, which has no DBG, VAR or LIK form.
//  - BSVI_NARROW_GEN=1 switches off outer, rowdot and skinny_k4nt, but not skinny_k4.
//  - rowdot's LDS bound is K * SKINNY floats <= 64 KiB whatever N is (N = 2 stages a quarter of that).
//  - BSVI_SKINNY_ROWS is not clamped (0 divides by zero); BSVI_GEMM_PF takes exactly three characters, and only '2' means depth 2.
//  - the TN product's narrow side is A when M <= N, so M = N <= 8 reads A as the narrow operand.
//  - BSVI_XGEMM_TALL=1 asks for 256-row tiles, taken from 256 rows only.
//  - BSVI_X6_MODES unset is 3; the forward pass reads bit 0, the input gradient bit 1.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace bsvi_amort_select {

constexpr int BM = 128, BN = 128, BK = 16;      // the f32-input MFMA kernel's workgroup tile and k step
constexpr int XBK = 32;                         // the bf16 kernels' k per step: two MFMA k chunks of 16
constexpr int SKINNY = 8;                       // a side this narrow: the memory-bound kernels
constexpr int kX6MinRows = 256;                 // rows from which x6gemm_kernel's 128-row tiles fill the chip better than the f32 kernel's 64-row ones

enum { MODE_NT = 0, MODE_NN = 1, MODE_TN = 2 };

// The values are public: bsvi_debug_gemm_kind returns them.
enum Kind {
    NONE = 0,               // an empty product: nothing is launched
    OUTER4, OUTER8, SKINNY_TN,
    ROWDOT2, ROWDOT4, ROWDOT8, SKINNY_N,
    SKINNY_K4NT_1, SKINNY_K4NT_2, SKINNY_K4NT_3, SKINNY_K4NT_4, SKINNY_K4NT_5, SKINNY_K4NT_6, SKINNY_K4NT_7, SKINNY_K4NT_8,
    SKINNY_K4, SKINNY_K,
    GEMM_TN_64_PF1, GEMM_TN_64_PF2,
    GEMM_NT_64_PF1, GEMM_NT_64_PF2, GEMM_NT_128_PF1, GEMM_NT_128_PF2,
    GEMM_NN_64_PF1, GEMM_NN_64_PF2, GEMM_NN_128_PF1, GEMM_NN_128_PF2,
    X6_NT, X6_NT_VAR1, X6_NT_LIK, X6_NT_DBG2, X6_NT_DBG3, X6_NT_DBG4, X6_NT_DBG5, X6_NT_DBG9,
    X6_NN, X6_NN_VAR1, X6_NN_DBG2, X6_NN_DBG3,
    X6_R5_NT, X6_R5_NN,
    XGEMM_GLDS_128, XGEMM_GLDS_256, XGEMM_REG_128, XGEMM_REG_256,
    KIND_COUNT
};

inline const char* name(int kind) {
    static const char* const names[KIND_COUNT] = {
        "none", "outer<4>", "outer<8>", "skinny_tn", "rowdot<2>", "rowdot<4>", "rowdot<8>", "skinny_n",
        "skinny_k4nt<1>", "skinny_k4nt<2>", "skinny_k4nt<3>", "skinny_k4nt<4>", "skinny_k4nt<5>", "skinny_k4nt<6>", "skinny_k4nt<7>", "skinny_k4nt<8>",
        "skinny_k4", "skinny_k", "gemm<tn,64,1>", "gemm<tn,64,2>",
        "gemm<nt,64,1>", "gemm<nt,64,2>", "gemm<nt,128,1>", "gemm<nt,128,2>", "gemm<nn,64,1>", "gemm<nn,64,2>", "gemm<nn,128,1>", "gemm<nn,128,2>",
        "x6<nt>", "x6<nt,var1>", "x6<nt,lik>", "x6<nt,dbg2>", "x6<nt,dbg3>", "x6<nt,dbg4>", "x6<nt,dbg5>", "x6<nt,dbg9>",
        "x6<nn>", "x6<nn,var1>", "x6<nn,dbg2>", "x6<nn,dbg3>", "x6_r5<nt>", "x6_r5<nn>",
        "xgemm_glds<128>", "xgemm_glds<256>", "xgemm<128>", "xgemm<256>"};
    return kind >= 0 && kind < KIND_COUNT ? names[kind] : "?";
}

// every knob the selection reads, at its default
struct Switches {
    bool second_generation = true;      // BSVI_NARROW_GEN != 1
    int skinny_rows = 16;               // BSVI_SKINNY_ROWS
    int half_below = 1536;              // BSVI_GEMM_HALF_BELOW
    int pf[3] = {2, 2, 2};              // BSVI_GEMM_PF=<nt><nn><tn>: global-load steps in flight, per mode
    bool x6_v6 = true;                  // BSVI_X6_V != 5
    int x6_var = 1;                     // BSVI_X6_VAR
    int x6_debug = 0;                   // BSVI_X6_DEBUG
    bool xgemm_tall = false;            // BSVI_XGEMM_TALL == 1
    bool xgemm_glds = true;             // BSVI_XGEMM_GLDS != 0
    int x6tn_slots = 512;               // BSVI_X6TN_SLOTS
    int x6_modes = 3;                   // BSVI_X6_MODES: bit 0 forward, bit 1 input gradient
    int x6_nn_only = -1;                // BSVI_X6_NN_ONLY: 10 * net + layer, or < 0 for all
    bool x6_tn = true;                  // BSVI_X6_TN != 0
    bool x6_tn_data = true;             // BSVI_X6_TN_DATA != 0
    bool fuse_lik = true;               // BSVI_AMORT_FUSE_LIK != 0
};

// what a launcher knows about its product; addresses only for their alignment, 0 = the operand is absent.  b is the f32 operand B, or
// the bf16 pieces of a six-piece product (then plane_stride is set and ldb unused); part_stride: the TN product's
struct Facts {
    int M = 0, N = 0, K = 0, lda = 0, ldb = 0, ldc = 0, ldy = 0;
    long part_stride = 0, plane_stride = 0;
    uintptr_t a = 0, b = 0, c = 0, bias = 0, y = 0, bias_grad = 0;
};

struct Selection {
    Kind kind = NONE;
    unsigned grid_x = 0, grid_y = 1, block = 256;
    size_t lds = 0;
    int vecA = 0, vecB = 0;                                  // f32: 16-byte loads of A / B allowed
    int rows_per_block = 0, narrow_is_a = 0, sbk = 0, sbn = 0;      // the memory-bound kernels' arguments
    int remap = 0, k_chunk = 0, tiles = 0;                   // gemm_kernel's (k_chunk, tiles: TN only)
    int rows_fastest = 0;                                    // xgemm
    bool lik = false;                                        // x6: the LIK instantiation is the one chosen
};

// ---- how a weight-gradient product C[M][N] = A[K][M]^T B[K][N] (K = all rows) is cut along K: every slice writes its own partial
// [M][N] (and partial column sums of A, [M]) and reduce_partials adds the slices in order
struct TnPlan {
    bool skinny;
    int tiles, splits, chunk;      // MFMA path: output tiles, grid splits (whole splits per XCD; padding ones exit), rows per split
    int slices;                    // partials actually written
};
inline int imin(int a, int b) { return a < b ? a : b; }
inline int imax(int a, int b) { return a > b ? a : b; }
inline TnPlan tn_plan(int M, int N, int K) {
    TnPlan p{};
    if (M <= SKINNY || N <= SKINNY) {
        p.skinny = true;
        p.chunk = 64;
        p.slices = (K + p.chunk - 1) / p.chunk;
        return p;
    }
    // about three workgroups per CU in flight, 64-row output tiles (less padding, half the splits of 128-row tiles);
    // at most 768 workgroups = three per CU in ONE round (a 769th would make some CU run four)
    p.tiles = ((M + 63) / 64) * ((N + BN - 1) / BN);
    const int splits = imax(1, imin((K + BK - 1) / BK, 768 / imax(p.tiles, 1)));
    p.chunk = ((K + splits - 1) / splits + BK - 1) / BK * BK;
    p.slices = (K + p.chunk - 1) / p.chunk;
    p.splits = (p.slices + 7) / 8 * 8;
    return p;
}
struct X6TnPlan { int tiles, splits, chunk, slices; };
// x6tn_kernel: 128 x 128 tiles, two workgroups per CU: as many slices of the rows as fill `slots` (512) in ONE round
inline X6TnPlan x6tn_plan(int M, int N, int K, int slots) {
    X6TnPlan p{};
    p.tiles = ((M + 127) / 128) * ((N + 127) / 128);
    const int splits = imax(1, imin((K + XBK - 1) / XBK, slots / imax(p.tiles, 1)));
    p.chunk = ((K + splits - 1) / splits + XBK - 1) / XBK * XBK;
    p.slices = (K + p.chunk - 1) / p.chunk;
    p.splits = p.slices;
    return p;
}
// the exact-data weight gradient (xgemm_nt_glds_kernel<128, true>): Rp = R rounded up to 64 rows, cut into slices of whole k steps
struct XdwPlan { int Rp, steps, steps_per_split, slices, grid_splits, tiles; };
inline XdwPlan xdw_plan(int P, int n_out, size_t R) {
    XdwPlan p{};
    p.Rp = (int)((R + 63) / 64 * 64);
    p.steps = p.Rp / XBK;
    p.tiles = ((P + 127) / 128) * ((n_out + 127) / 128);
    const int want = imax(1, imin(p.steps, 512 / imax(p.tiles, 1)));     // two workgroups per CU, one round
    p.steps_per_split = (p.steps + want - 1) / want;
    p.slices = (p.steps + p.steps_per_split - 1) / p.steps_per_split;
    p.grid_splits = p.slices;
    while ((p.grid_splits * p.tiles) % 8) ++p.grid_splits;       // whole XCD shares; the padding workgroups exit
    return p;
}
// does that kernel's 32-bit byte offset reach every element of its operands at R rows?
inline bool xdw_fits(uint32_t n_out, uint32_t n_in, size_t R) {
    const size_t Rp = (R + 63) / 64 * 64, widest = 3 * (size_t)n_out > n_in ? 3 * (size_t)n_out : n_in;
    return widest * Rp * 2 < 0xF0000000ull;
}
inline size_t align4(size_t n) { return (n + 3) / 4 * 4; }      // partial regions start on 16-byte boundaries
// floats of a layer's slice partials (weights, then bias): room for the f32 plan and for the six-piece form's own number of slices
inline size_t tn_partial_floats(int M, int N, int K, bool bias, int slots) {
    const TnPlan p = tn_plan(M, N, K);
    const size_t x6 = (size_t)x6tn_plan(M, N, K, slots).slices;
    const size_t slices = p.skinny || (size_t)p.slices > x6 ? (size_t)p.slices : x6;
    return align4(slices * M * N) + (bias ? align4(slices * M) : 0);
}

// ---- the f32-input products (mode: MODE_NT forward, MODE_NN input gradient, MODE_TN weight gradient)
inline bool al16(uintptr_t p) { return (p & 15) == 0; }
inline bool al16(uintptr_t p, int ld) { return (p & 15) == 0 && (ld & 3) == 0; }
inline Selection select_f32(int mode, const Facts& f, const Switches& sw) {
    Selection s;
    if (f.M <= 0 || f.N <= 0 || f.K <= 0) return s;
    s.vecA = al16(f.a, f.lda);
    s.vecB = al16(f.b, f.ldb);
    const int deep = sw.pf[mode] == 2 ? 1 : 0;
    if (mode == MODE_TN && (f.M <= SKINNY || f.N <= SKINNY)) {      // a side of width <= 8: the memory-bound kernels
        s.narrow_is_a = f.M <= f.N ? 1 : 0;
        const int wide = s.narrow_is_a ? f.N : f.M, narrow = s.narrow_is_a ? f.M : f.N;
        s.rows_per_block = tn_plan(f.M, f.N, f.K).chunk;
        const bool wide_vec = s.narrow_is_a ? s.vecB : s.vecA, narrow_vec = s.narrow_is_a ? s.vecA : s.vecB;
        const bool out_vec = !s.narrow_is_a || (f.ldc % 4 == 0 && al16(f.c) && f.part_stride % 4 == 0);
        const bool bias_vec = !f.bias_grad || s.narrow_is_a || (f.M % 4 == 0 && al16(f.bias_grad));
        // (the padded leading dimension of the narrow operand covers the 16-byte loads: ld >= 4 ceil(narrow / 4))
        const bool outer = sw.second_generation && wide % 4 == 0 && wide_vec && narrow_vec && out_vec && bias_vec;
        s.kind = !outer ? SKINNY_TN : narrow <= 4 ? OUTER4 : OUTER8;
        s.grid_x = (unsigned)(((outer ? wide / 4 : wide) + 255) / 256);
        s.grid_y = (unsigned)((f.K + s.rows_per_block - 1) / s.rows_per_block);
        return s;
    }
    if (mode != MODE_TN) {
        s.sbk = mode == MODE_NT ? 1 : f.ldb;
        s.sbn = mode == MODE_NT ? f.ldb : 1;
        if (sw.second_generation && f.N <= SKINNY && f.K % 4 == 0 && s.vecA && (size_t)f.K * SKINNY * sizeof(float) <= 64 * 1024) {
            const int w = f.N <= 2 ? 2 : f.N <= 4 ? 4 : 8;
            s.kind = w == 2 ? ROWDOT2 : w == 4 ? ROWDOT4 : ROWDOT8;
            s.rows_per_block = 32;
            s.grid_x = (unsigned)((f.M + 31) / 32);
            s.lds = (size_t)w * f.K * sizeof(float);
            return s;
        }
        if (f.N <= SKINNY && (size_t)f.N * f.K <= 8192) {
            s.kind = SKINNY_N;
            s.rows_per_block = sw.skinny_rows;
            s.grid_x = (unsigned)((f.M + s.rows_per_block - 1) / s.rows_per_block);
            s.lds = (size_t)f.N * f.K * sizeof(float);
            return s;
        }
        if (f.K <= SKINNY && (uint64_t)f.M * (uint64_t)f.N < (1ull << 32) - 256) {      // (32-bit index arithmetic in these kernels)
            const bool out4 = (f.N & 3) == 0 && al16(f.b) && (f.ldc & 3) == 0 && al16(f.c) && (!f.bias || al16(f.bias));
            const unsigned quads = (unsigned)(((long)f.M * (f.N >> 2) + 255) / 256);
            if (sw.second_generation && mode == MODE_NT && f.ldb == f.K && out4) {
                s.kind = (Kind)(SKINNY_K4NT_1 + f.K - 1);
                s.grid_x = quads;
                return s;
            }
            // (B stored [N][K], the forward layout, would need strided scalar loads per output: measured slower)
            if (s.sbn == 1 && (s.sbk & 3) == 0 && out4 && (!f.y || ((f.ldy & 3) == 0 && al16(f.y)))) {
                s.kind = SKINNY_K4;
                s.grid_x = quads;
                return s;
            }
            s.kind = SKINNY_K;
            s.grid_x = (unsigned)(((long)f.M * f.N + 255) / 256);
            return s;
        }
    }
    const int tiles_n = (f.N + BN - 1) / BN;
    if (mode == MODE_TN) {
        const TnPlan plan = tn_plan(f.M, f.N, f.K);
        s.kind = deep ? GEMM_TN_64_PF2 : GEMM_TN_64_PF1;
        s.k_chunk = plan.chunk;
        s.tiles = plan.tiles;
        s.remap = 1;
        s.grid_x = (unsigned)(plan.tiles * plan.splits);
        return s;
    }
    // 64-row tiles when 128-row tiles would leave most CUs with one or two workgroups
    int tiles = ((f.M + BM - 1) / BM) * tiles_n;
    const bool half = tiles < sw.half_below && f.M > 64;
    if (half) tiles = ((f.M + 63) / 64) * tiles_n;
    s.kind = (Kind)((mode == MODE_NT ? GEMM_NT_64_PF1 : GEMM_NN_64_PF1) + (half ? 0 : 2) + deep);
    s.remap = tiles % 8 == 0 ? 1 : 0;
    s.grid_x = (unsigned)tiles;
    return s;
}

// ---- six products of exact bf16 pieces (nn: the input gradient; otherwise the forward product, which may carry the likelihood).
// Round 6's kernel (LDS-DMA staging, 16-byte stores) wants 16-byte aligned rows of every matrix it touches with wide accesses and
// 31-bit byte offsets into A and the pieces; anything else — and BSVI_X6_V=5 — takes round 5's kernel, which stages through registers
inline Selection select_x6(bool nn, const Facts& f, bool want_lik, const Switches& sw) {
    Selection s;
    s.grid_x = (unsigned)(((f.M + 127) / 128) * ((f.N + 127) / 128));
    const bool wide_ok = sw.x6_v6 && (f.N & 3) == 0 && al16(f.a, f.lda) && al16(f.c, f.ldc) && (!f.y || al16(f.y, f.ldy)) && al16(f.b);
    if (!(wide_ok && ((size_t)(f.M - 1) * f.lda + f.K) * sizeof(float) < 0x7fffffffull && 3 * (size_t)f.plane_stride * 2 < 0x7fffffffull)) {
        s.kind = nn ? X6_R5_NN : X6_R5_NT;
        return s;
    }
    const int dbg = sw.x6_debug;
    if (!nn && (dbg == 2 || dbg == 3 || dbg == 4 || dbg == 5)) s.kind = (Kind)(X6_NT_DBG2 + dbg - 2);
    else if (!nn && dbg == 9) s.kind = X6_NT_DBG9;
    else if (nn && (dbg == 12 || dbg == 13)) s.kind = (Kind)(X6_NN_DBG2 + dbg - 12);
    else if (!nn && want_lik) s.kind = X6_NT_LIK;
    else if (sw.x6_var == 1) s.kind = nn ? X6_NN_VAR1 : X6_NT_VAR1;
    else s.kind = nn ? X6_NN : X6_NT;
    s.lik = s.kind == X6_NT_LIK;
    return s;
}

// ---- the exact-data forward product (three bf16 MFMAs on the pieces of W)
// (measured, cfg 4's two products: 256-row tiles 66 us each at two waves per SIMD — fewer LDS reads per MFMA, but one workgroup per
//  CU at these shapes — against 45 us with 128-row tiles at three; BSVI_XGEMM_TALL=1 selects the tall tile)
inline Selection select_xgemm(int M, int N, const Switches& sw) {
    Selection s;
    s.rows_fastest = 3L * N > (long)M ? 1 : 0;      // which operand is the larger one (both have Kp columns)
    const bool tall = sw.xgemm_tall && M >= 256;
    const int tbm = tall ? 256 : 128;
    s.grid_x = (unsigned)(((M + tbm - 1) / tbm) * ((N + 127) / 128));
    s.kind = sw.xgemm_glds ? (tall ? XGEMM_GLDS_256 : XGEMM_GLDS_128) : (tall ? XGEMM_REG_256 : XGEMM_REG_128);
    return s;
}

// ---- which product path a layer of bsvi_amort_fwd_bwd takes.  x6_on: the network has six-piece layers and the call at least
// kX6MinRows rows; from_data: the layer reads the gathered data rows
inline bool x6_rows(size_t R) { return R >= (size_t)kX6MinRows; }
enum ForwardPath { FWD_EXACT_DATA, FWD_X6, FWD_F32 };
// data_pieces / x6_pieces: the layer's weight pieces for the exact-data / the six-piece forward product exist
inline ForwardPath forward_path(bool from_data, bool data_exact, bool data_pieces, bool x6_on, bool x6_pieces, const Switches& sw) {
    if (from_data && data_exact && data_pieces) return FWD_EXACT_DATA;
    return x6_on && (sw.x6_modes & 1) && !from_data && x6_pieces ? FWD_X6 : FWD_F32;
}
enum WeightGradPath { WG_X6TN_DATA, WG_XDW, WG_X6TN, WG_F32 };      // x6tn_kernel<., true> / the exact-piece product / x6tn_kernel / gemm<TN>
// the data layer's weight gradient through x6tn_kernel<., true> (no transposed minibatch rows, no pieces of dY in memory)?
inline bool data_x6tn(bool x6_on, const Switches& sw) { return x6_on && sw.x6_tn && sw.x6_tn_data; }
// xdw_ok: the layer has the exact-data product's pieces, its transposed rows, and xdw_fits; M = n_out, N = n_in of dW [M][N]
// (from 64 on both sides: never tn_plan's skinny form)
inline WeightGradPath weight_grad_path(bool from_data, bool xdw_ok, bool x6_on, int M, int N, const Switches& sw) {
    if (from_data && xdw_ok) return data_x6tn(x6_on, sw) ? WG_X6TN_DATA : WG_XDW;
    return x6_on && sw.x6_tn && !from_data && M >= 64 && N >= 64 ? WG_X6TN : WG_F32;
}
enum InputGradPath { IG_X6, IG_F32 };
// x6_pieces: the transposed weight's pieces exist; layer_id: 10 * net + layer (what BSVI_X6_NN_ONLY names)
inline InputGradPath input_grad_path(bool x6_on, bool x6_pieces, int layer_id, const Switches& sw) {
    return x6_on && (sw.x6_modes & 2) && x6_pieces && (sw.x6_nn_only < 0 || sw.x6_nn_only == layer_id) ? IG_X6 : IG_F32;
}

}  // namespace bsvi_amort_select
