// local_plan (brancher_amd/csrc/dense_local_select.h) from the header alone, without a GPU: at the shapes the device tests run and at
// BASELINE config 4's size every tile and split covers B, P and N exactly once, the LDS of both kernels fits, and the workspace regions
// are disjoint and large enough.  tests/test_dense_local_cpu.py compiles and runs this.
#include <initializer_list>
#include <stdio.h>

#include "dense_local_select.h"

using namespace bsvi_dense_local;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

static void shape(uint32_t C, uint32_t P, uint32_t B, uint32_t N, uint32_t n_cu, uint32_t forced) {
    const Plan L = local_plan(C, P, B, N, n_cu, 2u * C * P, forced);
    // rows: the tiles [32 t, 32 t + 32) cover [0, B) inside the head's padding
    CHECK(L.row_tiles * ROWS >= B && (L.row_tiles - 1u) * ROWS < B && L.row_tiles * ROWS <= L.B_pad && L.B_pad % 64u == 0u);
    CHECK(L.k_chunks * KC >= P && (L.k_chunks - 1u) * KC < P && L.k_chunks * KC <= L.P_pad);
    CHECK(L.col_tiles * COLS >= P && (L.col_tiles - 1u) * COLS < P && L.col_tiles * COLS <= L.P_pad && L.P_pad % 64u == 0u);
    // samples: split i takes [i sps, min(N, (i + 1) sps)), lane l of it the samples l, l + 8, ...: every sample once, no empty split
    CHECK(L.samples_per_split % LANES == 0u && L.splits >= 1u && (uint64_t)(L.splits - 1u) * L.samples_per_split < N);
    uint32_t seen = 0;
    for (uint32_t s = 0; s < L.splits; ++s) {
        const uint32_t n0 = s * L.samples_per_split, n1 = n0 + L.samples_per_split < N ? n0 + L.samples_per_split : N;
        for (uint32_t l = 0; l < LANES; ++l)
            for (uint32_t n = n0 + l; n < n1; n += LANES) ++seen;
    }
    CHECK(seen == N && (!forced || L.splits <= forced) && L.CT >= C && (L.CT == 1u || L.CT == 4u || L.CT == 10u || L.CT == 16u));
    CHECK(fwd_lds_bytes() <= LDS_LIMIT && bwd_lds_bytes() <= LDS_LIMIT && 2u * fwd_lds_bytes() <= 160u * 1024u);
    const size_t at[] = {L.rowp, L.idx, L.Xb, L.XbT, L.lab, L.partial, L.rowg, L.hpart, L.dM, L.dV, L.jM, L.jV, L.likp, L.total};
    for (size_t i = 0; i + 1 < sizeof(at) / sizeof(at[0]); ++i) CHECK(at[i] < at[i + 1] && at[i] % 256u == 0u);
    const size_t tile = (size_t)L.row_tiles * ROWS * 32u * 4u;
    CHECK(L.idx - L.rowp >= 6u * (size_t)C * P * 4u && L.XbT - L.Xb >= (size_t)L.B_pad * L.P_pad * 4u && L.lab - L.XbT >= (size_t)L.B_pad * L.P_pad * 4u);
    CHECK(L.hpart - L.rowg >= 4u * (size_t)C * P * 4u && L.dM - L.hpart >= L.col_tiles * 4u);
    CHECK(L.dV - L.dM >= L.splits * tile && L.jM - L.dV >= L.splits * tile && L.jV - L.jM >= tile && L.likp - L.jV >= tile);
    CHECK(L.total - L.likp >= (size_t)L.splits * L.row_tiles * 4u);
}

int main() {
    for (uint32_t n_cu : {1u, 64u, 256u}) {
        shape(1, 3, 5, 3, n_cu, 0);
        shape(3, 5, 33, 9, n_cu, 0);
        shape(10, 70, 64, 40, n_cu, 0);
        shape(10, 70, 64, 40, n_cu, 3);
        shape(16, 130, 40, 17, n_cu, 0);
        shape(10, 784, 512, 1024, n_cu, 0);
        shape(16, 784, 1, 65536, n_cu, 7);
    }
    // config 4 on the 256 CUs of an MI355X fills the chip with two workgroups a CU; the knob
    const Plan L = local_plan(10, 784, 512, 1024, 256, 15680, 0);
    CHECK(L.row_tiles == 16u && L.splits == 32u && L.samples_per_split == 32u && L.k_chunks == 25u && L.col_tiles == 25u && L.CT == 10u);
    CHECK(local_plan(10, 70, 64, 40, 256, 0, 3).splits == 3u && local_plan(10, 70, 64, 40, 256, 0, 1).splits == 1u);
    printf("%s\n", failures ? "dense_local_plan: FAILED" : "dense_local_plan: ok");
    return failures ? 1 : 0;
}
