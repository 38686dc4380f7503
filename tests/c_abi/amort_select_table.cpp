// The kernel selection of the amortised path (brancher_amd/csrc/amort_select.h): the rows that tests/test_gpu_amortized.py runs on the
// device (one per kind that bsvi_debug_gemm reaches with the default switches, printed so that the two lists are compared), both sides
// of every threshold, a sweep of the plans' invariants, every switch flipped once, and the rule of the fused likelihood.  The expected
// kinds and numbers were worked out by hand from the launchers' conditions as they stood before the header — not from the functions
// under test.  Exit status 0: everything holds; 1 otherwise, with each row that does not printed.
#include <stdio.h>
#include <string.h>

#include <initializer_list>

#include "amort_select.h"

using namespace bsvi_amort_select;

static int g_failures = 0;
static void expect(const char* what, bool ok) {
    if (ok) return;
    ++g_failures;
    printf("FAILED: %s\n", what);
}
static void kind_is(const char* id, const Selection& s, Kind expected) {
    if (s.kind == expected) return;
    ++g_failures;
    printf("FAILED: %s: expected %s, got %s\n", id, name(expected), name(s.kind));
}

constexpr uintptr_t AL = 1u << 20, OFF4 = AL + 4;      // an aligned address, and one 4 bytes beyond
// the facts bsvi_debug_gemm hands over with aligned buffers: modes 0 / 1 as given; mode 2 with the partials in its own buffer
// (ldc = N, slices of M N floats, the bias partials 16-byte aligned behind them); modes 5 / 6 with the pieces [3][N][Kp]
static Facts hook(int mode, int M, int N, int K, int lda, int ldb, int ldc, int ldy, bool extra) {
    Facts f;
    f.M = M; f.N = N; f.K = K; f.lda = lda; f.ldb = ldb; f.ldc = ldc; f.ldy = ldy;
    f.a = f.b = f.c = AL;
    if (mode == 0 || mode == 5) f.bias = extra ? AL : 0;
    if (mode == 1 || mode == 6) f.y = extra ? AL : 0;
    if (mode == 2) { f.ldc = N; f.part_stride = (long)M * N; f.bias_grad = extra ? AL : 0; }
    if (mode == 5 || mode == 6) { f.ldb = 0; f.plane_stride = (long)N * ((K + XBK - 1) / XBK * XBK); }
    return f;
}
static Selection pick(int mode, const Facts& f, const Switches& sw = Switches(), bool want_lik = false) {
    if (mode == 3) return select_xgemm(f.M, f.N, sw);
    if (mode == 5 || mode == 6) return select_x6(mode == 6, f, want_lik, sw);
    return select_f32(mode, f, sw);
}
static void device_row(const char* id, int mode, int M, int N, int K, int lda, int ldb, int ldc, int ldy, Kind expected, unsigned gx, unsigned gy, size_t lds) {
    const Selection s = pick(mode, hook(mode, M, N, K, lda, ldb, ldc, ldy, true));
    kind_is(id, s, expected);
    if (s.grid_x != gx || s.grid_y != gy || s.lds != lds || s.block != 256) {
        ++g_failures;
        printf("FAILED: %s: grid %u x %u, %zu bytes; expected %u x %u, %zu\n", id, s.grid_x, s.grid_y, s.lds, gx, gy, lds);
    }
    printf("device-row %s %d %d %d %d %d %d %d %d %s\n", id, mode, M, N, K, lda, ldb, ldc, ldy, name(expected));
}

int main() {
    const Switches def;
    // ---- one row per kind bsvi_debug_gemm reaches with the default switches, at a small shape with tails (the device test's rows).
    // mode 2 (C[M][N] = A[K][M]^T B[K][N]): lda is A's, ldb B's leading dimension; 64 rows of K per workgroup on the narrow kernels
    device_row("outer4", 2, 3, 260, 130, 4, 260, 260, 0, OUTER4, 1, 3, 0);               // narrow A (3 <= 4, rows padded to 4), 65 quads of B
    device_row("outer8", 2, 260, 6, 130, 260, 8, 6, 0, OUTER8, 1, 3, 0);                 // narrow B (rows padded to 8), M % 4 == 0 for the bias partials
    device_row("skinny_tn", 2, 257, 3, 130, 257, 3, 3, 0, SKINNY_TN, 2, 3, 0);           // 257 % 4 != 0
    device_row("gemm_tn", 2, 70, 50, 300, 70, 50, 50, 0, GEMM_TN_64_PF2, 48, 1, 0);      // 2 tiles, 19 k steps: 19 slices of 16 rows, 24 splits each
    // mode 0 (C = act(A[rows] B^T + bias)), mode 1 (C += (A B) act'(Y))
    device_row("rowdot2", 0, 70, 2, 12, 12, 12, 2, 0, ROWDOT2, 3, 1, 96);
    device_row("rowdot4", 0, 70, 3, 12, 12, 12, 3, 0, ROWDOT4, 3, 1, 192);
    device_row("rowdot8", 1, 70, 7, 12, 12, 7, 7, 7, ROWDOT8, 3, 1, 384);
    device_row("skinny_n", 0, 70, 5, 13, 13, 13, 5, 0, SKINNY_N, 5, 1, 260);             // K % 4 != 0; 16 rows per workgroup
    device_row("skinny_k4nt1", 0, 257, 12, 1, 1, 1, 12, 0, SKINNY_K4NT_1, 4, 1, 0);      // 257 * 3 = 771 quads
    device_row("skinny_k4nt3", 0, 257, 12, 3, 3, 3, 12, 0, SKINNY_K4NT_3, 4, 1, 0);
    device_row("skinny_k4nt8", 0, 257, 12, 8, 8, 8, 16, 0, SKINNY_K4NT_8, 4, 1, 0);
    device_row("skinny_k4", 1, 257, 12, 5, 5, 12, 12, 12, SKINNY_K4, 4, 1, 0);
    device_row("skinny_k", 0, 257, 12, 2, 2, 2, 15, 0, SKINNY_K, 13, 1, 0);              // ldc % 4 != 0: 3084 outputs
    device_row("gemm_nt64", 0, 300, 70, 50, 50, 50, 73, 0, GEMM_NT_64_PF2, 5, 1, 0);
    device_row("gemm_nt128", 0, 50, 20, 18, 18, 18, 23, 0, GEMM_NT_128_PF2, 1, 1, 0);    // M <= 64
    device_row("gemm_nn64", 1, 300, 70, 50, 50, 70, 70, 70, GEMM_NN_64_PF2, 5, 1, 0);
    device_row("gemm_nn128", 1, 50, 20, 18, 18, 20, 20, 20, GEMM_NN_128_PF2, 1, 1, 0);
    // modes 5 / 6: the same products as six bf16 MFMAs
    device_row("x6_nt", 5, 300, 72, 100, 100, 100, 76, 0, X6_NT_VAR1, 3, 1, 0);
    device_row("x6_nn", 6, 300, 72, 100, 100, 72, 72, 72, X6_NN_VAR1, 3, 1, 0);
    device_row("x6_r5_nt", 5, 256, 130, 64, 64, 64, 134, 0, X6_R5_NT, 4, 1, 0);          // N % 4 != 0
    device_row("x6_r5_nn", 6, 256, 130, 64, 64, 130, 130, 130, X6_R5_NN, 4, 1, 0);
    // mode 3: the exact-data forward product
    device_row("xgemm", 3, 300, 70, 50, 50, 50, 73, 0, XGEMM_GLDS_128, 3, 1, 0);
    {   // the derived arguments of some of them
        const Selection o = pick(2, hook(2, 3, 260, 130, 4, 260, 260, 0, true)), p = pick(2, hook(2, 260, 6, 130, 260, 8, 6, 0, true));
        expect("outer4: A is the narrow side, 64 rows per workgroup", o.narrow_is_a == 1 && o.rows_per_block == 64 && o.vecA && o.vecB);
        expect("outer8: B is the narrow side", p.narrow_is_a == 0 && p.rows_per_block == 64);
        const Selection t = pick(2, hook(2, 70, 50, 300, 70, 50, 50, 0, true));
        expect("gemm_tn: 2 tiles, chunks of 16 rows, remapped", t.tiles == 2 && t.k_chunk == 16 && t.remap == 1 && !t.vecA && !t.vecB);
        const Selection r = pick(1, hook(1, 70, 7, 12, 12, 7, 7, 7, true)), q = pick(0, hook(0, 70, 2, 12, 12, 12, 2, 0, true));
        expect("rowdot NN: B's k stride is ldb, its n stride 1; 32 rows per workgroup", r.sbk == 7 && r.sbn == 1 && r.rows_per_block == 32);
        expect("rowdot NT: B's k stride is 1, its n stride ldb", q.sbk == 1 && q.sbn == 12);
        expect("skinny_n: 16 rows per workgroup", pick(0, hook(0, 70, 5, 13, 13, 13, 5, 0, true)).rows_per_block == 16);
        expect("gemm_nt64: 5 tiles are not remapped, k_chunk and tiles stay 0", pick(0, hook(0, 300, 70, 50, 50, 50, 73, 0, true)).remap == 0 &&
               pick(0, hook(0, 300, 70, 50, 50, 50, 73, 0, true)).k_chunk == 0 && pick(0, hook(0, 300, 70, 50, 50, 50, 73, 0, true)).tiles == 0);
        expect("xgemm: W is the smaller operand at 300 x 70", pick(3, hook(3, 300, 70, 50, 50, 50, 73, 0, true)).rows_fastest == 0 &&
               select_xgemm(300, 101, def).rows_fastest == 1);
        expect("an empty product launches nothing", pick(0, hook(0, 0, 5, 5, 5, 5, 5, 0, true)).kind == NONE && pick(1, hook(1, 5, 0, 5, 5, 5, 5, 0, true)).kind == NONE &&
               pick(2, hook(2, 5, 5, 0, 5, 5, 5, 0, true)).kind == NONE);
    }
    // what the suite's older mode-0 row (257, 784, 2) with ldc = N + 3 runs: not skinny_k4nt
    kind_is("(257, 784, 2) at ldc 787", pick(0, hook(0, 257, 784, 2, 2, 2, 787, 0, true)), SKINNY_K);

    // ---- both sides of every threshold
    // (1) a side of width 8
    kind_is("TN M = 8", pick(2, hook(2, 8, 260, 130, 8, 260, 0, 0, false)), OUTER8);
    kind_is("TN M = 9, N = 9", pick(2, hook(2, 9, 9, 130, 9, 9, 0, 0, false)), GEMM_TN_64_PF2);
    kind_is("TN M = 9, N = 8", pick(2, hook(2, 9, 8, 130, 9, 8, 0, 0, false)), SKINNY_TN);       // (wide = 9)
    kind_is("NT N = 8", pick(0, hook(0, 70, 8, 12, 12, 12, 8, 0, false)), ROWDOT8);
    kind_is("NT N = 9", pick(0, hook(0, 70, 9, 12, 12, 12, 9, 0, false)), GEMM_NT_64_PF2);
    kind_is("NT K = 8", pick(0, hook(0, 70, 12, 8, 8, 8, 12, 0, false)), SKINNY_K4NT_8);
    kind_is("NT K = 9", pick(0, hook(0, 70, 12, 9, 9, 9, 12, 0, false)), GEMM_NT_64_PF2);
    // (2) the narrow widths 2 / 4 / 8
    const Kind rowdots[9] = {NONE, ROWDOT2, ROWDOT2, ROWDOT4, ROWDOT4, ROWDOT8, ROWDOT8, ROWDOT8, ROWDOT8};
    for (int n = 1; n <= 8; ++n) {
        kind_is("rowdot width", pick(0, hook(0, 70, n, 12, 12, 12, n, 0, false)), rowdots[n]);
        expect("rowdot stages its width times K floats", pick(0, hook(0, 70, n, 12, 12, 12, n, 0, false)).lds == (size_t)(n <= 2 ? 2 : n <= 4 ? 4 : 8) * 12 * 4);
        kind_is("outer width", pick(2, hook(2, n, 260, 130, (n + 3) / 4 * 4, 260, 0, 0, false)), n <= 4 ? OUTER4 : OUTER8);
    }
    // (3) K % 4, (4) K * 8 * 4 <= 64 KiB, (5) N K <= 8192
    kind_is("K = 12", pick(0, hook(0, 70, 2, 12, 12, 12, 2, 0, false)), ROWDOT2);
    kind_is("K = 13, lda 16", pick(0, hook(0, 70, 2, 13, 16, 13, 2, 0, false)), SKINNY_N);
    kind_is("K = 2048", pick(0, hook(0, 70, 2, 2048, 2048, 2048, 2, 0, false)), ROWDOT2);
    kind_is("K = 2052, N = 2", pick(0, hook(0, 70, 2, 2052, 2052, 2052, 2, 0, false)), SKINNY_N);
    kind_is("K = 2052, N = 8", pick(0, hook(0, 70, 8, 2052, 2052, 2052, 8, 0, false)), GEMM_NT_64_PF2);
    kind_is("N K = 8184", pick(0, hook(0, 70, 8, 1023, 1023, 1023, 8, 0, false)), SKINNY_N);
    kind_is("N K = 8200", pick(0, hook(0, 70, 8, 1025, 1025, 1025, 8, 0, false)), GEMM_NT_64_PF2);
    kind_is("N K = 8192, K = 8", pick(1, hook(1, 70, 1024, 8, 8, 1024, 1024, 0, false)), SKINNY_K4);      // (N > 8: not skinny_n's business)
    // (6) M N < 2^32 - 256 = 256 * 255 * 65793
    kind_is("M N = 2^32 - 256 - 255", pick(0, hook(0, 16843007, 255, 2, 2, 2, 255, 0, false)), SKINNY_K);
    kind_is("M N = 2^32 - 256", pick(0, hook(0, 16843008, 255, 2, 2, 2, 255, 0, false)), GEMM_NT_128_PF2);
    expect("grids at that size", pick(0, hook(0, 16843007, 255, 2, 2, 2, 255, 0, false)).grid_x == 16777215u && pick(0, hook(0, 16843008, 255, 2, 2, 2, 255, 0, false)).grid_x == 263172u);
    // (7) 64-row tiles below half_below 128-row tiles, from 65 rows
    kind_is("M = 64", pick(0, hook(0, 64, 16, 16, 16, 16, 16, 0, false)), GEMM_NT_128_PF2);
    kind_is("M = 65", pick(0, hook(0, 65, 16, 16, 16, 16, 16, 0, false)), GEMM_NT_64_PF2);
    kind_is("1535 tiles", pick(1, hook(1, 128 * 1535, 128, 16, 16, 128, 128, 0, false)), GEMM_NN_64_PF2);
    kind_is("1536 tiles", pick(1, hook(1, 128 * 1536, 128, 16, 16, 128, 128, 0, false)), GEMM_NN_128_PF2);
    expect("grids at those", pick(1, hook(1, 128 * 1535, 128, 16, 16, 128, 128, 0, false)).grid_x == 3070u && pick(1, hook(1, 128 * 1536, 128, 16, 16, 128, 128, 0, false)).grid_x == 1536u);
    // (8) tiles % 8: the XCD-aware order
    expect("8 tiles are remapped, 7 are not", pick(0, hook(0, 512, 16, 16, 16, 16, 16, 0, false)).remap == 1 && pick(0, hook(0, 448, 16, 16, 16, 16, 16, 0, false)).remap == 0 &&
           pick(0, hook(0, 448, 16, 16, 16, 16, 16, 0, false)).grid_x == 7u);
    // (9) each alignment predicate on its own
    {
        auto f = [] { return hook(2, 3, 260, 130, 4, 260, 0, 0, true); };       // outer4: A narrow
        Facts x = f(); x.N = 262; kind_is("outer: wide % 4", pick(2, x), SKINNY_TN);
        x = f(); x.b = OFF4; kind_is("outer: wide operand's address", pick(2, x), SKINNY_TN);
        x = f(); x.ldb = 261; kind_is("outer: wide operand's leading dimension", pick(2, x), SKINNY_TN);
        x = f(); x.a = OFF4; kind_is("outer: narrow operand's address", pick(2, x), SKINNY_TN);
        x = f(); x.lda = 3; kind_is("outer: narrow operand's leading dimension", pick(2, x), SKINNY_TN);
        x = f(); x.c = OFF4; kind_is("outer: C's address", pick(2, x), SKINNY_TN);
        x = f(); x.ldc = 261; kind_is("outer: C's leading dimension", pick(2, x), SKINNY_TN);
        x = f(); x.part_stride = 781; kind_is("outer: the partials' stride", pick(2, x), SKINNY_TN);
        x = f(); x.bias_grad = OFF4; kind_is("outer, A narrow: the bias partials' address does not matter", pick(2, x), OUTER4);
        auto g = [] { return hook(2, 260, 6, 130, 260, 8, 0, 0, true); };       // outer8: B narrow
        x = g(); x.c = OFF4; x.ldc = 7; x.part_stride = 1561; kind_is("outer, B narrow: C does not matter", pick(2, x), OUTER8);
        x = g(); x.bias_grad = OFF4; kind_is("outer, B narrow: the bias partials' address", pick(2, x), SKINNY_TN);
        x = g(); x.M = 262; x.lda = 264; kind_is("outer, B narrow: M % 4 with bias partials", pick(2, x), SKINNY_TN);
        x = g(); x.M = 262; x.lda = 264; x.bias_grad = 0; kind_is("outer, B narrow: M % 4 without", pick(2, x), SKINNY_TN);      // (wide % 4)
        auto r = [] { return hook(0, 70, 2, 12, 12, 12, 2, 0, true); };
        x = r(); x.a = OFF4; kind_is("rowdot: A's address", pick(0, x), SKINNY_N);
        x = r(); x.lda = 13; kind_is("rowdot: A's leading dimension", pick(0, x), SKINNY_N);
        x = r(); x.b = OFF4; x.ldb = 13; x.c = OFF4; x.bias = OFF4; kind_is("rowdot: nothing else", pick(0, x), ROWDOT2);
        auto k = [] { return hook(0, 257, 12, 3, 3, 3, 12, 0, true); };
        x = k(); x.ldb = 4; kind_is("k4nt: B dense", pick(0, x), SKINNY_K);
        x = k(); x.N = 13; x.ldc = 16; kind_is("k4nt: N % 4", pick(0, x), SKINNY_K);
        x = k(); x.b = OFF4; kind_is("k4nt: B's address", pick(0, x), SKINNY_K);
        x = k(); x.ldc = 13; kind_is("k4nt: C's leading dimension", pick(0, x), SKINNY_K);
        x = k(); x.c = OFF4; kind_is("k4nt: C's address", pick(0, x), SKINNY_K);
        x = k(); x.bias = OFF4; kind_is("k4nt: the bias' address", pick(0, x), SKINNY_K);
        x = k(); x.bias = 0; x.a = OFF4; x.lda = 5; kind_is("k4nt: no bias, A anywhere", pick(0, x), SKINNY_K4NT_3);
        auto q = [] { return hook(1, 257, 12, 5, 5, 12, 12, 12, true); };
        x = q(); x.ldb = 13; kind_is("k4: B's leading dimension", pick(1, x), SKINNY_K);
        x = q(); x.b = OFF4; kind_is("k4: B's address", pick(1, x), SKINNY_K);
        x = q(); x.N = 13; x.ldb = x.ldc = x.ldy = 16; kind_is("k4: N % 4", pick(1, x), SKINNY_K);
        x = q(); x.ldc = 13; kind_is("k4: C's leading dimension", pick(1, x), SKINNY_K);
        x = q(); x.c = OFF4; kind_is("k4: C's address", pick(1, x), SKINNY_K);
        x = q(); x.y = OFF4; kind_is("k4: Y's address", pick(1, x), SKINNY_K);
        x = q(); x.ldy = 13; kind_is("k4: Y's leading dimension", pick(1, x), SKINNY_K);
        x = q(); x.y = 0; x.ldy = 13; kind_is("k4: no Y", pick(1, x), SKINNY_K4);
        x = hook(0, 257, 12, 5, 5, 8, 12, 0, true); kind_is("k4: the forward layout never", pick(0, x), SKINNY_K);
        expect("vecA / vecB follow address and leading dimension", pick(0, hook(0, 300, 70, 52, 52, 52, 70, 0, false)).vecA == 1 &&
               pick(0, hook(0, 300, 70, 52, 52, 52, 70, 0, false)).vecB == 1 && pick(0, hook(0, 300, 70, 52, 53, 52, 70, 0, false)).vecA == 0 &&
               pick(0, hook(0, 300, 70, 52, 52, 53, 70, 0, false)).vecB == 0);
        // (10) the six-piece kernel: N & 3 and every operand
        auto s = [] { return hook(6, 300, 72, 100, 100, 0, 72, 72, true); };
        x = s(); x.N = 74; x.ldc = x.ldy = 76; kind_is("x6: N & 3", pick(6, x), X6_R5_NN);
        x = s(); x.a = OFF4; kind_is("x6: A's address", pick(6, x), X6_R5_NN);
        x = s(); x.lda = 101; kind_is("x6: A's leading dimension", pick(6, x), X6_R5_NN);
        x = s(); x.c = OFF4; kind_is("x6: C's address", pick(6, x), X6_R5_NN);
        x = s(); x.ldc = 73; kind_is("x6: C's leading dimension", pick(6, x), X6_R5_NN);
        x = s(); x.y = OFF4; kind_is("x6: Y's address", pick(6, x), X6_R5_NN);
        x = s(); x.ldy = 73; kind_is("x6: Y's leading dimension", pick(6, x), X6_R5_NN);
        x = s(); x.y = 0; x.ldy = 73; kind_is("x6: no Y", pick(6, x), X6_NN_VAR1);
        x = s(); x.b = AL + 8; kind_is("x6: the pieces' address", pick(6, x), X6_R5_NN);
        x = hook(5, 300, 72, 100, 100, 0, 76, 0, true); x.bias = OFF4; kind_is("x6: the bias anywhere", pick(5, x), X6_NT_VAR1);
    }
    // (11) both 2^31 guards of the six-piece kernel: ((M - 1) lda + K) 4 and 6 plane_stride bytes below 2^31 - 1
    {
        Facts x = hook(5, 1048575, 512, 512, 512, 0, 512, 0, true);
        kind_is("A of 2^31 - 2048 bytes", pick(5, x), X6_NT_VAR1);
        x.M = 1048576; kind_is("A of 2^31 bytes (1M rows at lda 512)", pick(5, x), X6_R5_NT);
        expect("that grid", pick(5, x).grid_x == 8192u * 4u);
        x = hook(6, 300, 72, 100, 100, 0, 72, 72, true);
        x.plane_stride = 357913941; kind_is("pieces of 2^31 - 2 bytes", pick(6, x), X6_NN_VAR1);
        x.plane_stride = 357913942; kind_is("pieces of 2^31 + 4 bytes", pick(6, x), X6_R5_NN);
    }
    // (12) the layer paths: xdw's 0xF0000000 bound (784 columns: 2 567 936 rows fit, one more rounds up to 2 568 000), 256 rows, 64 units
    expect("xdw fits 784 x 2 567 936", xdw_fits(256, 784, 2567936) && !xdw_fits(256, 784, 2567937));
    expect("xdw's widest side is 3 n_out or n_in", xdw_fits(262, 784, 2561344) && !xdw_fits(262, 784, 2561345));      // 786 columns: below 2 561 407.02 rows
    expect("the six-piece kernels from 256 rows", !x6_rows(255) && x6_rows(256));
    expect("x6tn from 64 units on both sides", weight_grad_path(false, false, true, 64, 64, def) == WG_X6TN && weight_grad_path(false, false, true, 63, 64, def) == WG_F32 &&
           weight_grad_path(false, false, true, 64, 63, def) == WG_F32 && weight_grad_path(false, false, false, 64, 64, def) == WG_F32);
    expect("the data layer's weight gradient", weight_grad_path(true, true, true, 256, 784, def) == WG_X6TN_DATA && weight_grad_path(true, true, false, 256, 784, def) == WG_XDW &&
           weight_grad_path(true, false, true, 256, 784, def) == WG_F32);
    expect("the forward paths", forward_path(true, true, true, true, true, def) == FWD_EXACT_DATA && forward_path(true, false, true, true, true, def) == FWD_F32 &&
           forward_path(true, true, false, true, true, def) == FWD_F32 && forward_path(false, true, true, true, true, def) == FWD_X6 &&
           forward_path(false, true, true, false, true, def) == FWD_F32 && forward_path(false, true, true, true, false, def) == FWD_F32);
    expect("the input-gradient paths", input_grad_path(true, true, 11, def) == IG_X6 && input_grad_path(false, true, 11, def) == IG_F32 && input_grad_path(true, false, 11, def) == IG_F32);

    // ---- the plans' invariants over M, N in 1 .. 1024 and K in 1 .. 70 000
    long plans = 0;
    for (int slots : {512, 64, 2048})
        for (int M = 1; M <= 1024; M += (M < 12 ? 1 : 61))
            for (int N = 1; N <= 1024; N += (N < 12 ? 1 : 67))
                for (int K = 1; K <= 70000; K += (K < 70 ? 1 : 997)) {
                    ++plans;
                    const TnPlan t = tn_plan(M, N, K);
                    const X6TnPlan x = x6tn_plan(M, N, K, slots);
                    const XdwPlan w = xdw_plan(M, N, (size_t)K);
                    bool ok = (long)t.slices * t.chunk >= K && K > (long)(t.slices - 1) * t.chunk && t.skinny == (M <= 8 || N <= 8);
                    // at most 768 workgroups do work (or one per tile); the grid pads every tile's splits to whole XCD shares, fewer than 8 more each
                    if (!t.skinny) ok = ok && t.splits % 8 == 0 && t.splits >= t.slices && t.splits - t.slices < 8 && t.chunk % BK == 0 &&
                                        t.tiles == ((M + 63) / 64) * ((N + 127) / 128) && t.tiles * t.slices <= (t.tiles > 768 ? t.tiles : 768) &&
                                        (t.tiles > 1 || t.tiles * t.splits <= 768 + 7);
                    else ok = ok && t.chunk == 64;
                    ok = ok && (long)x.slices * x.chunk >= K && K > (long)(x.slices - 1) * x.chunk && x.chunk % XBK == 0 && x.splits == x.slices &&
                         x.tiles * x.slices <= (slots > x.tiles ? slots : x.tiles);
                    ok = ok && w.Rp % 64 == 0 && w.Rp >= K && w.Rp - K < 64 && w.slices * w.steps_per_split >= w.steps && w.steps > (w.slices - 1) * w.steps_per_split &&
                         (w.grid_splits * w.tiles) % 8 == 0 && w.grid_splits >= w.slices && w.tiles * w.slices <= (w.tiles > 512 ? w.tiles : 512);
                    for (int bias = 0; bias < 2; ++bias) {
                        const size_t have = tn_partial_floats(M, N, K, bias != 0, slots);
                        const size_t most = !t.skinny && x.slices > t.slices ? (size_t)x.slices : (size_t)t.slices;
                        ok = ok && have == align4(most * M * N) + (bias ? align4(most * M) : 0);
                    }
                    if (!ok) { if (++g_failures < 20) printf("FAILED: plans at M %d N %d K %d slots %d\n", M, N, K, slots); }
                }
    printf("plans: %ld shapes\n", plans);
    expect("cfg 5's weight gradient at 25 600 rows", tn_plan(512, 784, 25600).tiles == 56 && tn_plan(512, 784, 25600).slices == 13 && tn_plan(512, 784, 25600).chunk == 1984 &&
           tn_plan(512, 784, 25600).splits == 16 && x6tn_plan(512, 784, 25600, 512).tiles == 28 && x6tn_plan(512, 784, 25600, 512).slices == 18 &&
           x6tn_plan(512, 784, 25600, 512).chunk == 1440);

    // ---- every switch flipped once: the rows that change, and rows that must not
    {
        Switches sw;
        sw.second_generation = false;      // BSVI_NARROW_GEN=1
        kind_is("gen 1: outer", pick(2, hook(2, 3, 260, 130, 4, 260, 0, 0, true), sw), SKINNY_TN);
        kind_is("gen 1: rowdot", pick(0, hook(0, 70, 2, 12, 12, 12, 2, 0, true), sw), SKINNY_N);
        kind_is("gen 1: k4nt", pick(0, hook(0, 257, 12, 3, 3, 3, 12, 0, true), sw), SKINNY_K);
        kind_is("gen 1: k4 stays", pick(1, hook(1, 257, 12, 5, 5, 12, 12, 12, true), sw), SKINNY_K4);
        kind_is("gen 1: gemm stays", pick(0, hook(0, 300, 70, 50, 50, 50, 73, 0, true), sw), GEMM_NT_64_PF2);
        sw = Switches(); sw.skinny_rows = 8;      // BSVI_SKINNY_ROWS=8
        expect("skinny rows: skinny_n's grid and argument", pick(0, hook(0, 70, 5, 13, 13, 13, 5, 0, true), sw).grid_x == 9u && pick(0, hook(0, 70, 5, 13, 13, 13, 5, 0, true), sw).rows_per_block == 8);
        expect("skinny rows: rowdot keeps 32", pick(0, hook(0, 70, 2, 12, 12, 12, 2, 0, true), sw).rows_per_block == 32 && pick(0, hook(0, 70, 2, 12, 12, 12, 2, 0, true), sw).grid_x == 3u);
        sw = Switches(); sw.half_below = 0;       // BSVI_GEMM_HALF_BELOW=0
        kind_is("half below 0: NT", pick(0, hook(0, 300, 70, 50, 50, 50, 73, 0, true), sw), GEMM_NT_128_PF2);
        kind_is("half below 0: NN", pick(1, hook(1, 300, 70, 50, 50, 70, 70, 70, true), sw), GEMM_NN_128_PF2);
        kind_is("half below 0: TN stays", pick(2, hook(2, 70, 50, 300, 70, 50, 0, 0, true), sw), GEMM_TN_64_PF2);
        sw = Switches(); sw.pf[0] = 1;            // BSVI_GEMM_PF=122
        kind_is("pf 122: NT", pick(0, hook(0, 300, 70, 50, 50, 50, 73, 0, true), sw), GEMM_NT_64_PF1);
        kind_is("pf 122: NT 128", pick(0, hook(0, 50, 20, 18, 18, 18, 23, 0, true), sw), GEMM_NT_128_PF1);
        kind_is("pf 122: NN stays", pick(1, hook(1, 300, 70, 50, 50, 70, 70, 70, true), sw), GEMM_NN_64_PF2);
        kind_is("pf 122: TN stays", pick(2, hook(2, 70, 50, 300, 70, 50, 0, 0, true), sw), GEMM_TN_64_PF2);
        sw = Switches(); sw.pf[1] = 1;            // 212
        kind_is("pf 212: NN", pick(1, hook(1, 300, 70, 50, 50, 70, 70, 70, true), sw), GEMM_NN_64_PF1);
        kind_is("pf 212: NN 128", pick(1, hook(1, 50, 20, 18, 18, 20, 20, 20, true), sw), GEMM_NN_128_PF1);
        kind_is("pf 212: NT stays", pick(0, hook(0, 300, 70, 50, 50, 50, 73, 0, true), sw), GEMM_NT_64_PF2);
        sw = Switches(); sw.pf[2] = 1;            // 221
        kind_is("pf 221: TN", pick(2, hook(2, 70, 50, 300, 70, 50, 0, 0, true), sw), GEMM_TN_64_PF1);
        kind_is("pf 221: NT stays", pick(0, hook(0, 300, 70, 50, 50, 50, 73, 0, true), sw), GEMM_NT_64_PF2);
        const Facts nt = hook(5, 300, 72, 100, 100, 0, 76, 0, true), nn = hook(6, 300, 72, 100, 100, 0, 72, 72, true), odd = hook(5, 256, 130, 64, 64, 0, 134, 0, true);
        sw = Switches(); sw.x6_v6 = false;        // BSVI_X6_V=5
        kind_is("v5: NT", pick(5, nt, sw), X6_R5_NT);
        kind_is("v5: NN", pick(6, nn, sw), X6_R5_NN);
        kind_is("v5: f32 stays", pick(0, hook(0, 300, 70, 50, 50, 50, 73, 0, true), sw), GEMM_NT_64_PF2);
        sw = Switches(); sw.x6_var = 0;           // BSVI_X6_VAR=0
        kind_is("var 0: NT", pick(5, nt, sw), X6_NT);
        kind_is("var 0: NN", pick(6, nn, sw), X6_NN);
        kind_is("var 0: LIK stays", pick(5, nt, sw, true), X6_NT_LIK);
        kind_is("var 0: r5 stays", pick(5, odd, sw), X6_R5_NT);
        sw.x6_var = 2;
        kind_is("var 2 is var 0", pick(5, nt, sw), X6_NT);
        const int dbgs[] = {2, 3, 4, 5, 9, 12, 13, 1, 6, 10, 14};
        const Kind nt_kinds[] = {X6_NT_DBG2, X6_NT_DBG3, X6_NT_DBG4, X6_NT_DBG5, X6_NT_DBG9, X6_NT_VAR1, X6_NT_VAR1, X6_NT_VAR1, X6_NT_VAR1, X6_NT_VAR1, X6_NT_VAR1};
        const Kind nn_kinds[] = {X6_NN_VAR1, X6_NN_VAR1, X6_NN_VAR1, X6_NN_VAR1, X6_NN_VAR1, X6_NN_DBG2, X6_NN_DBG3, X6_NN_VAR1, X6_NN_VAR1, X6_NN_VAR1, X6_NN_VAR1};
        for (int i = 0; i < 11; ++i) {            // BSVI_X6_DEBUG
            sw = Switches(); sw.x6_debug = dbgs[i];
            kind_is("dbg: NT", pick(5, nt, sw), nt_kinds[i]);
            kind_is("dbg: NN", pick(6, nn, sw), nn_kinds[i]);
            kind_is("dbg: r5 stays", pick(5, odd, sw), X6_R5_NT);
        }
        sw = Switches(); sw.xgemm_tall = true;    // BSVI_XGEMM_TALL=1
        kind_is("tall: 256 rows", select_xgemm(256, 70, sw), XGEMM_GLDS_256);
        kind_is("tall: 255 rows", select_xgemm(255, 70, sw), XGEMM_GLDS_128);
        expect("tall: grids", select_xgemm(300, 130, sw).grid_x == 4u && select_xgemm(300, 130, def).grid_x == 6u);
        sw.xgemm_glds = false;                    // and BSVI_XGEMM_GLDS=0
        kind_is("tall, register-staged", select_xgemm(256, 70, sw), XGEMM_REG_256);
        sw = Switches(); sw.xgemm_glds = false;
        kind_is("register-staged", select_xgemm(300, 70, sw), XGEMM_REG_128);
        expect("register-staged: the same grid", select_xgemm(300, 130, sw).grid_x == 6u);
        sw = Switches(); sw.x6tn_slots = 256;     // BSVI_X6TN_SLOTS=256
        expect("slots: x6tn's slices", x6tn_plan(512, 784, 25600, 256).slices == 9 && tn_plan(512, 784, 25600).slices == 13 &&
               tn_partial_floats(512, 784, 25600, false, 256) == (size_t)13 * 512 * 784 && tn_partial_floats(512, 784, 25600, false, 512) == (size_t)18 * 512 * 784);
        sw = Switches(); sw.x6_modes = 1;         // BSVI_X6_MODES=1
        expect("modes 1: forward on, input gradient off", forward_path(false, true, true, true, true, sw) == FWD_X6 && input_grad_path(true, true, 11, sw) == IG_F32);
        sw.x6_modes = 2;
        expect("modes 2: forward off, input gradient on", forward_path(false, true, true, true, true, sw) == FWD_F32 && input_grad_path(true, true, 11, sw) == IG_X6 &&
               forward_path(true, true, true, true, true, sw) == FWD_EXACT_DATA && weight_grad_path(false, false, true, 64, 64, sw) == WG_X6TN);
        sw = Switches(); sw.x6_nn_only = 11;      // BSVI_X6_NN_ONLY=11
        expect("nn only: the decoder's layer 1 alone", input_grad_path(true, true, 11, sw) == IG_X6 && input_grad_path(true, true, 10, sw) == IG_F32 &&
               input_grad_path(true, true, 1, sw) == IG_F32 && forward_path(false, true, true, true, true, sw) == FWD_X6);
        sw = Switches(); sw.x6_tn = false;        // BSVI_X6_TN=0
        expect("x6 tn off: both six-piece weight gradients", weight_grad_path(false, false, true, 64, 64, sw) == WG_F32 && weight_grad_path(true, true, true, 256, 784, sw) == WG_XDW &&
               !data_x6tn(true, sw) && input_grad_path(true, true, 11, sw) == IG_X6);
        sw = Switches(); sw.x6_tn_data = false;   // BSVI_X6_TN_DATA=0
        expect("x6 tn data off: the data layer's alone", weight_grad_path(false, false, true, 64, 64, sw) == WG_X6TN && weight_grad_path(true, true, true, 256, 784, sw) == WG_XDW &&
               !data_x6tn(true, sw) && data_x6tn(true, def) && !data_x6tn(false, def));
        sw = Switches(); sw.fuse_lik = false;     // BSVI_AMORT_FUSE_LIK=0: the caller stops asking; the selection itself does not read it
        kind_is("fuse off, still asked", pick(5, nt, sw, true), X6_NT_LIK);
    }

    // ---- the fused likelihood: `lik` exactly when the LIK kernel is the one chosen — never with a DBG form, round 5's kernel or NN
    {
        const int dbgs[] = {0, 2, 3, 4, 5, 9};
        long asked = 0, fused = 0;
        for (int v6 = 0; v6 < 2; ++v6)
            for (int dbg : dbgs)
                for (int guard = 0; guard < 11; ++guard)
                    for (int want = 0; want < 2; ++want)
                        for (int nn = 0; nn < 2; ++nn)
                            for (int var = 0; var < 2; ++var) {
                                Switches sw;
                                sw.x6_v6 = v6 != 0; sw.x6_debug = dbg; sw.x6_var = var;
                                Facts x = hook(nn ? 6 : 5, 512, 784, 512, 512, 0, 784, 784, true);
                                switch (guard) {      // 0: none fails
                                case 1: x.N = 786; x.ldc = 788; break;
                                case 2: x.a = OFF4; break;
                                case 3: x.lda = 513; break;
                                case 4: x.c = OFF4; break;
                                case 5: x.ldc = 785; break;
                                case 6: x.b = AL + 2; break;
                                case 7: x.M = 1048576; break;
                                case 8: x.plane_stride = 357913942; break;
                                case 9: x.y = nn ? OFF4 : 0; break;
                                case 10: x.ldy = 785; break;      // (Y is the input gradient's alone)
                                }
                                const Selection s = select_x6(nn != 0, x, want != 0, sw);
                                const bool falls_back = !v6 || (guard >= 1 && guard <= 8) || (nn && guard >= 9);
                                const bool expected = want && !nn && !falls_back && dbg == 0;
                                asked += want; fused += s.lik;
                                if (s.lik != expected || s.lik != (s.kind == X6_NT_LIK) || (falls_back && s.kind != (nn ? X6_R5_NN : X6_R5_NT))) {
                                    ++g_failures;
                                    printf("FAILED: lik at v6 %d dbg %d guard %d want %d nn %d var %d: %s, lik %d\n", v6, dbg, guard, want, nn, var, name(s.kind), (int)s.lik);
                                }
                            }
        printf("fused likelihood: asked %ld times, answered %ld\n", asked, fused);
        expect("the likelihood is fused in 6 of the 528 asked combinations", asked == 528 && fused == 6);
    }
    for (int k = 0; k < KIND_COUNT; ++k)
        for (int j = 0; j < k; ++j) expect("kind names are distinct", strcmp(name(k), name(j)) != 0);
    expect("unknown kinds have no name", !strcmp(name(-1), "?") && !strcmp(name(KIND_COUNT), "?"));
    printf("%d failures\n", g_failures);
    return g_failures ? 1 : 0;
}
