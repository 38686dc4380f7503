// The host functions of the posterior-predictive pass (brancher_amd/csrc/bnn_select.h: predict_lds_bytes, predict_lds,
// predict_rows_per_pass, predict_layout) from the header alone, without a GPU: the LDS arm at its boundary, the default pass at its
// limits, the workspace monotone in rows and samples.  tests/test_bnn_predict_cpu.py compiles and runs this with the sanitizers.
#include <initializer_list>
#include <stdio.h>

#include "bnn_select.h"

using namespace bsvi_bnn_select;

static int failures = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

int main() {
    // the formula: the staging tile [Rs][65], then two buffers of the widest layer [2 w][256], in floats
    CHECK(predict_lds_bytes(230, 20) == (230u * 65u + 2u * 20u * 256u) * 4u);
    CHECK(predict_lds_bytes(0, 3) == (65u + 2u * 3u * 256u) * 4u);          // no small tensors: staged as one row
    // the rows the device tests run: 784-20-10 and 32-16-16-4 in LDS, 32-64-8 through global memory
    CHECK(predict_lds(230, 20));
    CHECK(predict_lds_bytes(356, 16) == 125328u && predict_lds(356, 16));
    CHECK(predict_lds_bytes(584, 64) == 282912u && !predict_lds(584, 64));
    // the boundary: the largest Rs that fits beside a width, and the next one
    for (uint32_t w : {1u, 8u, 16u, 32u, 64u}) {
        const uint32_t fits = (uint32_t)((LDS_LIMIT / 4u - 2u * w * 256u) / 65u);
        CHECK(predict_lds(fits, w) && predict_lds_bytes(fits, w) <= LDS_LIMIT);
        CHECK(!predict_lds(fits + 1u, w) && predict_lds_bytes(fits + 1u, w) > LDS_LIMIT);
    }
    CHECK(predict_lds(1, 74) && !predict_lds(1, 75));                       // (65 + 2 * 74 * 256) * 4 = 151 812 <= 153 600 < 153 860
    // forward only needs less than the training kernel's tile wherever there is more than one layer
    CHECK(predict_lds_bytes(356, 16) < upper_lds_bytes(356, 36));
    // the default pass: a multiple of 32, at least 32, no more than the rows rounded up, a1 within its budget and the index range
    for (uint32_t h1 : {1u, 20u, 64u, 512u})
        for (uint32_t n_pad : {64u, 128u, 4096u, 65536u})
            for (uint32_t rows : {1u, 31u, 32u, 33u, 10000u, 1000000u}) {
                const uint32_t r = predict_rows_per_pass(h1, n_pad, rows);
                CHECK(r % 32u == 0u && r >= 32u && r <= (rows + 31u) / 32u * 32u);
                CHECK(r == 32u || (uint64_t)r * h1 * n_pad * 4u <= PREDICT_A1_BYTES);
                CHECK(r == 32u || (uint64_t)r * h1 * n_pad < (1ull << 31));
            }
    CHECK(predict_rows_per_pass(20, 64, 10000) == 10016u);                  // a whole test set of 784-20-10 at 64 samples: one pass
    CHECK(predict_rows_per_pass(20, 64, 1) == 32u);
    // the workspace: monotone in the rows (up to the pass) and in the samples; a given pass bounds it whatever the rows
    size_t last = 0;
    for (uint32_t rows : {1u, 33u, 70u, 1000u, 10000u}) {
        const PredictLayout L = predict_layout(15910, 230, 784, 10, 20, 20, 64, rows, 0);
        CHECK(L.total >= last && L.total % 256u == 0u && L.rows_pass == predict_rows_per_pass(20, 64, rows));
        CHECK(L.rowp < L.sg && L.sg < L.flag && L.flag < L.Wsm && L.Wsm < L.W1 && L.W1 < L.part && L.part < L.X && L.X < L.a1 && L.a1 <= L.act && L.act <= L.p && L.p < L.total);
        last = L.total;
    }
    last = 0;
    for (uint32_t n : {1u, 64u, 65u, 700u, 4000u}) {
        const PredictLayout L = predict_layout(15910, 230, 784, 10, 20, 20, n, 96, 32);
        CHECK(L.total > last && L.n_pad == (n + 63u) / 64u * 64u && L.NC == 20u * L.n_pad && L.rows_pass == 32u);
        last = L.total;
    }
    CHECK(predict_layout(15910, 230, 784, 10, 20, 20, 64, 100000, 32).total == predict_layout(15910, 230, 784, 10, 20, 20, 64, 64, 32).total);
    // the global arm's activations are part of the workspace, the LDS arm's are not
    CHECK(predict_layout(2632, 584, 32, 8, 64, 64, 70, 33, 0).p - predict_layout(2632, 584, 32, 8, 64, 64, 70, 33, 0).act == 2u * 64u * 64u * 128u * 4u);
    CHECK(predict_layout(868, 356, 32, 4, 16, 16, 70, 33, 0).p == predict_layout(868, 356, 32, 4, 16, 16, 70, 33, 0).act);
    printf("%s\n", failures ? "bnn_predict_select: FAILED" : "bnn_predict_select: ok");
    return failures ? 1 : 0;
}
