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

// the shapes of tests/test_gpu_dense_local_branches.py and the branches they claim to reach: what the plan must say of each, at the 256
// CUs of an MI355X and at 32 (the splits are the clamp ceil(N / 8) at both, so the cases reach their branches on either chip)
struct Named { uint32_t C, P, B, N, row_tiles, k_chunks, rounds, col_tiles, CT, splits, sps; };
static const Named NAMED[] = {
    {2, 32, 32, 8, 1, 1, 1, 1, 4, 1, 8},            // everything exact, two dead classes of tier 4, P_pad > P
    {4, 64, 64, 16, 2, 2, 1, 2, 4, 2, 8},           // tier 4 full, P = P_pad, B = B_pad
    {5, 128, 96, 24, 3, 4, 1, 4, 10, 3, 8},         // lower edge of tier 10, one chunk a wave, three row tiles
    {11, 260, 160, 81, 5, 9, 3, 9, 16, 11, 8},      // lower edge of tier 16, three rounds, wave 0 of bwd twice, the join's second group
    {1, 40, 130, 20, 5, 2, 1, 2, 1, 3, 8},          // Bernoulli over five row tiles, split and joined
    {3, 5, 33, 1, 2, 1, 1, 1, 4, 1, 8},             // N = 1
    {10, 70, 64, 40, 2, 3, 1, 3, 10, 5, 8},         // the tail's shared-entry loop at R = 700
    {11, 8, 40, 17, 2, 1, 1, 1, 16, 3, 8},          // the drawn normals against the host reference
    {1, 8, 40, 17, 2, 1, 1, 1, 1, 3, 8},
    {3, 5, 33, 9, 2, 1, 1, 1, 4, 2, 8},             // the training trajectory
};

static void named_shapes() {
    for (const Named& s : NAMED) {
        const uint32_t clamp = (s.N + LANES - 1u) / LANES;
        for (uint32_t n_cu : {256u, 32u}) {
            shape(s.C, s.P, s.B, s.N, n_cu, 0);
            const Plan L = local_plan(s.C, s.P, s.B, s.N, n_cu, 2u * s.C * s.P, 0);
            CHECK(L.row_tiles == s.row_tiles && L.k_chunks == s.k_chunks && (L.k_chunks + 3u) / 4u == s.rounds && L.col_tiles == s.col_tiles);
            CHECK(L.CT == s.CT && L.splits == s.splits && L.samples_per_split == s.sps && L.splits == clamp);
            if (!(L.row_tiles == s.row_tiles && L.k_chunks == s.k_chunks && L.col_tiles == s.col_tiles && L.CT == s.CT && L.splits == s.splits && L.samples_per_split == s.sps))
                printf("  shape (%u, %u, %u, %u) at %u CUs: row_tiles %u k_chunks %u col_tiles %u CT %u splits %u sps %u\n", s.C, s.P, s.B, s.N, n_cu,
                       L.row_tiles, L.k_chunks, L.col_tiles, L.CT, L.splits, L.samples_per_split);
            // the knob from 1 up to the clamp: the workspace never shrinks, grows whenever the number of splits does, stays aligned
            Plan before = local_plan(s.C, s.P, s.B, s.N, n_cu, 2u * s.C * s.P, 1);
            CHECK(before.splits == 1u);
            for (uint32_t forced = 1; forced <= clamp; ++forced) {
                shape(s.C, s.P, s.B, s.N, n_cu, forced);
                const Plan F = local_plan(s.C, s.P, s.B, s.N, n_cu, 2u * s.C * s.P, forced);
                CHECK(F.splits >= before.splits && F.splits <= forced && F.total >= before.total && (F.splits == before.splits || F.total > before.total));
                CHECK(F.total % 256u == 0u);
                before = F;
            }
            CHECK(before.splits == clamp && before.total == L.total);
        }
    }
    // the split counts the split-invariance and the workspace-cache tests ask for at (11, 260, 160, 81): 1, 3, 8, 9 -> 1, 3, 6, 6 splits
    const uint32_t asked[] = {1, 3, 8, 9}, given[] = {1, 3, 6, 6};
    for (int i = 0; i < 4; ++i) CHECK(local_plan(11, 260, 160, 81, 256, 0, asked[i]).splits == given[i]);
    CHECK(local_plan(11, 260, 160, 81, 256, 0, 9).total > local_plan(11, 260, 160, 81, 256, 0, 1).total);
    for (const Named& s : NAMED) printf("named shape %u %u %u %u\n", s.C, s.P, s.B, s.N);
}

int main() {
    named_shapes();
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
