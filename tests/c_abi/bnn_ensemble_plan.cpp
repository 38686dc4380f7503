// brancher_amd/csrc/bnn_select.h, ensemble_plan, from the header alone (tests/test_bnn_ensemble_cpu.py compiles and runs this)
#include <initializer_list>
#include <stdio.h>
#include "bnn_select.h"
using namespace bsvi_bnn_select;
static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

int main() {
    CHECK(ENS_MAX_WIDTH >= 256u);
    for (uint32_t w = 1; w <= ENS_MAX_WIDTH + 1u; ++w)
        for (uint32_t c : {1u, 3u, 10u, w})
            for (uint32_t depth : {1u, 2u, 3u})
                for (uint32_t n : {2u, 9u, 256u})
                    for (uint32_t m : {1u, 129u, 100000u}) {
                        uint32_t widths[3] = {w, w, w};
                        widths[depth - 1u] = c;
                        const EnsemblePlan E = ensemble_plan(widths, depth, n, m);
                        const bool wide = w > ENS_MAX_WIDTH && (depth > 1u || c == w);
                        CHECK(E.served == (wide ? 0u : 1u));
                        if (!E.served) { CHECK(E.widest == w); continue; }
                        CHECK(E.lds_bytes <= 160u * 1024u && E.lds_bytes <= LDS_LIMIT);
                        CHECK(E.rows == 128u || E.rows == 64u || E.rows == 32u);
                        CHECK(E.group >= 1u && E.group <= n && E.blocks >= 1u && E.blocks <= ENS_BLOCKS);
                        CHECK(E.n_groups == (n + E.group - 1u) / E.group && E.row_tiles == (m + E.rows - 1u) / E.rows);
                        CHECK(E.splits >= 1u && E.splits <= E.n_groups);
                        CHECK(E.stride[0] % 2u == 1u && E.stride[1] % 2u == 1u && E.stride[(depth - 1u) & 1u] > c && E.stride[depth & 1u] > c + 1u);
                        CHECK(E.tile[0] == ENS_STAGE_FLOATS && E.tile[1] == E.tile[0] + E.group * E.rows * E.stride[0]);
                        CHECK(E.workspace_bytes >= E.probs + (size_t)n * m * c * 4u && E.sigma + c * 4u <= E.probs);
                    }
    // the rows the device tests run: 784-20-10 keeps 128 rows and several particles a group; 256 units shrink the row tile
    const uint32_t mnist[2] = {20u, 10u}, wide[2] = {256u, 1u}, wide2[3] = {256u, 256u, 1u};
    CHECK(ensemble_plan(mnist, 2, 64, 10000).rows == 128u && ensemble_plan(mnist, 2, 64, 10000).group >= 4u);
    CHECK(ensemble_plan(mnist, 2, 64, 1).splits == ensemble_plan(mnist, 2, 64, 1).n_groups);      // the one-row call: dealt over grid.y
    CHECK(ensemble_plan(mnist, 2, 64, 100000).splits == 1u);
    CHECK(ensemble_plan(wide, 2, 4, 5).rows == 64u && ensemble_plan(wide2, 3, 4, 5).rows == 32u);
    printf("%s\n", failures ? "bnn_ensemble_plan: FAILED" : "bnn_ensemble_plan: ok");
    return failures ? 1 : 0;
}
