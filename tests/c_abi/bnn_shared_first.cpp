// The selection of the shared first layer of the Bayesian-neural-network family (brancher_amd/csrc/bnn_select.h, shared_first): every one
// of the first R1 point bytes set -> shared; one of them unset -> per sample, wherever it stands; the switch off -> per sample; no point
// bytes at all -> per sample; the bytes behind R1 (b1 and the upper tensors) do not enter.  The expectations are the rule as
// include/bsvi.h states it, not the function under test.  Exit status 0: everything holds; 1 otherwise, with each row that does not printed.
#include <stdio.h>

#include <vector>

#include "bnn_select.h"

using namespace bsvi_bnn_select;

static int g_failures = 0;

static void row(const char* id, const uint8_t* bytes, uint32_t R1, bool off, bool expected) {
    const bool got = shared_first(bytes, R1, off);
    if (got == expected) return;
    ++g_failures;
    printf("%s (R1 %u, switch %s): expected %s, got %s\n", id, R1, off ? "off" : "on", expected ? "shared" : "per_sample", got ? "shared" : "per_sample");
}

int main() {
    const uint32_t R1 = 9 * 64, R = R1 + 9 + 9 + 1;      // 64-9-1
    std::vector<uint8_t> trunk(R, 0), head(R, 0), all(R, 1), none(R, 0);
    for (uint32_t r = 0; r < R1 + 9; ++r) trunk[r] = 1;      // weights1 and b1
    for (uint32_t r = R1 + 9; r < R; ++r) head[r] = 1;       // weights2 and b2
    row("trunk", trunk.data(), R1, false, true);
    row("all", all.data(), R1, false, true);
    row("head", head.data(), R1, false, false);
    row("none", none.data(), R1, false, false);
    row("no bytes", nullptr, R1, false, false);
    row("trunk, switch off", trunk.data(), R1, true, false);
    row("all, switch off", all.data(), R1, true, false);
    // weights1 alone (b1 random) is enough; one unset byte anywhere in weights1 is not
    std::vector<uint8_t> w1(R, 0);
    for (uint32_t r = 0; r < R1; ++r) w1[r] = 1;
    row("weights1 alone", w1.data(), R1, false, true);
    for (uint32_t at : {0u, 1u, R1 / 2u, R1 - 1u}) {
        std::vector<uint8_t> holed(all);
        holed[at] = 0;
        row("one byte of weights1 unset", holed.data(), R1, false, false);
    }
    std::vector<uint8_t> behind(all);
    behind[R1] = 0;                                            // the first byte of b1
    row("a byte behind weights1 unset", behind.data(), R1, false, true);
    // exactly the first R1 bytes are read: a vector of that length, under the address sanitizer
    const std::vector<uint8_t> exact(R1, 1);
    row("R1 bytes", exact.data(), R1, false, true);
    printf("%d failures\n", g_failures);
    return g_failures ? 1 : 0;
}
