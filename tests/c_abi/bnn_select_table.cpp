// The selection of the Bayesian-neural-network family's middle kernel (brancher_amd/csrc/bnn_select.h): the rows of the table that
// tests/test_gpu_bnn_middle.py runs on the device, both sides of each of the three thresholds, and a sweep over every realisable
// network of one to eight layers with widths 1 .. 64 for a shape that lands on bnn_upper<true> with both generators switched on.
// The expected kinds were worked out by hand from the rules as bnn_mid_ready, bnn_upper_ready and bsvi_bnn_create spelled them —
// not from the function under test.  Exit status 0: everything holds; 1 otherwise, with each row that does not printed.
#include <stdio.h>

#include <initializer_list>
#include <vector>

#include "bnn_select.h"

using namespace bsvi_bnn_select;

static int g_failures = 0;

struct Net { uint32_t Rs, act; };
// widths: features first, outputs last; every layer with a bias.  Rs: every bias and every weight matrix above the first
static Net net(std::initializer_list<uint32_t> widths, bool bias = true) {
    std::vector<uint32_t> w(widths);
    Net n{0, 0};
    for (size_t l = 1; l < w.size(); ++l) {
        n.act += w[l];
        if (bias) n.Rs += w[l];
        if (l > 1) n.Rs += w[l] * w[l - 1];
    }
    return n;
}
static uint32_t pad32(uint32_t B) { return (B + 31u) / 32u * 32u; }

static void row(const char* id, Net n, uint32_t B_pad, bool exact, bool mid_off, bool jit_off, BnnMiddle expected) {
    Switches sw;
    sw.mid_off = mid_off; sw.jit_off = jit_off;
    const BnnMiddle got = middle(n.Rs, n.act, B_pad, exact, sw);
    if (got == expected) return;
    ++g_failures;
    printf("%s (Rs %u, act %u, B_pad %u, %s, mid %s, jit %s): expected %s, got %s\n", id, n.Rs, n.act, B_pad, exact ? "exact" : "f32",
           mid_off ? "off" : "on", jit_off ? "off" : "on", name(expected), name(got));
}
static void expect(const char* what, bool ok) {
    if (ok) return;
    ++g_failures;
    printf("%s\n", what);
}

int main() {
    // ---- the rows of the device tests (P = 32 throughout; the features do not enter)
    const Net a = net({32, 48, 44, 4}), b = net({32, 48, 44, 5}), c = net({32, 16, 16, 4}), d = net({32, 16, 14, 4}), e = net({32, 32, 8}),
              g = net({32, 18, 18, 1}), h = net({32, 18, 18, 3}), i = net({32, 6, 6, 6, 6, 6, 6, 6, 3});
    expect("case a is Rs 2384, act 96", a.Rs == 2384 && a.act == 96);
    expect("case c is Rs 356, act 36", c.Rs == 356 && c.act == 36);
    expect("case d is Rs 314, act 34", d.Rs == 314 && d.act == 34);
    expect("case e is Rs 296, act 40", e.Rs == 296 && e.act == 40);
    expect("case i is Rs 279, act 45", i.Rs == 279 && i.act == 45);
    row("a", a, pad32(17), true, false, false, MID_GEN);
    row("b", b, pad32(17), true, false, false, UPPER_MEM);
    row("c", c, pad32(17), false, false, false, UPPER_MEM);
    row("d", d, pad32(17), false, false, false, UPPER_GEN);
    row("e", e, pad32(448), true, false, false, MID_GEN);
    expect("case e asks for 145 824 bytes", mid_lds_bytes(e.Rs, e.act, pad32(448)) == 145824u);
    row("f", e, pad32(449), true, false, false, UPPER_GEN);
    expect("case f would ask for 156 064 bytes", pad32(449) == 480u && mid_lds_bytes(e.Rs, e.act, 480) == 156064u);
    row("g", g, pad32(33), false, false, false, UPPER_MEM);
    row("h", h, pad32(33), false, false, false, UPPER_MEM);
    row("i", i, pad32(17), true, false, false, MID_GEN);
    row("i, BSVI_BNN_MID=0", i, pad32(17), true, true, false, UPPER_GEN);
    row("i, BSVI_BNN_MID=0 BSVI_BNN_JIT=0", i, pad32(17), true, true, true, UPPER_MEM);      // (279 * 65 + 90 * 256) * 4 = 164 700 bytes
    // the networks of the suite before this table: 784-20-10 (Rs 230, act 30) at B = 30 and B = 512, and its static kernel
    const Net ex = net({784, 20, 10});
    expect("784-20-10 is Rs 230, act 30", ex.Rs == 230 && ex.act == 30);
    row("784-20-10", ex, 32, true, false, false, MID_GEN);
    row("784-20-10, 512 rows", ex, 512, true, false, false, MID_GEN);
    row("784-20-10, f32", ex, 32, false, false, false, UPPER_GEN);
    row("784-20-10, both off", ex, 32, true, true, true, UPPER_LDS);

    // ---- the three thresholds, both sides of each, at the boundary values
    // (1) bnn_mid_gen: the tile within 150 KiB = 153 600 bytes (Rs4 + 2 act (B_pad + 4) <= 38 400 floats), and act <= 96
    expect("mid tile of exactly 153 600 bytes", mid_lds_bytes(2240, 40, 448) == 153600u);
    row("mid tile at the limit", Net{2240, 40}, 448, true, false, false, MID_GEN);
    row("mid tile one row quad beyond", Net{2241, 40}, 448, true, false, false, UPPER_MEM);      // Rs4 = 2244: 153 616 bytes
    row("mid tile at the limit, f32 data", Net{2240, 40}, 448, false, false, false, UPPER_MEM);
    row("96 units", Net{96, 96}, 32, true, false, false, MID_GEN);
    row("97 units", Net{97, 97}, 32, true, false, false, UPPER_GEN);                             // 97 + 194 = 291 floats
    // (2) bnn_upper_gen: Rs + 2 act <= 400 floats (its staging tile, Rs <= 590 rows, cannot bind below that)
    row("400 floats", Net{330, 35}, 32, false, false, false, UPPER_GEN);
    row("401 floats", Net{331, 35}, 32, false, false, false, UPPER_MEM);                         // (331 * 65 + 70 * 256) * 4 = 157 740 bytes
    row("400 floats, few rows", Net{0, 200}, 32, false, false, false, UPPER_GEN);
    row("402 floats, few rows", Net{0, 201}, 32, false, false, false, UPPER_MEM);
    expect("staging tile of 590 rows fits, of 591 does not", upper_gen_lds_bytes(590) <= LDS_LIMIT && upper_gen_lds_bytes(591) > LDS_LIMIT);
    // (3) bnn_upper<true>: 65 Rs + 512 act <= 38 400 floats
    expect("static tile of exactly 153 600 bytes", upper_lds_bytes(512, 10) == 153600u);
    row("static tile at the limit", Net{512, 10}, 32, false, false, false, UPPER_LDS);           // 512 + 20 > 400: the generator declines
    row("static tile one row beyond", Net{513, 10}, 32, false, false, false, UPPER_MEM);
    row("static tile at the limit, generators off", Net{330, 33}, 32, false, true, true, UPPER_LDS);      // 21 450 + 16 896 = 38 346
    row("static tile one unit beyond, generators off", Net{330, 34}, 32, false, true, true, UPPER_MEM);   // 21 450 + 17 408 = 38 858
    expect("a network without small tensors stages one row", upper_lds_bytes(0, 1) == upper_lds_bytes(1, 1) && mid_lds_bytes(0, 1, 32) == mid_lds_bytes(1, 1, 32));

    // ---- the sweep: every (Rs, act) that a network of 1 .. 8 layers with widths 1 .. 64 can have (with biases on every layer or on
    // none), every B_pad 32 .. 512, both data paths, both switches on.  Rows beyond RS_CAP and units beyond ACT_CAP share one cell each:
    // every rule is monotone in both, the cells are asked at their smallest member (where a static tile is smallest) and at the largest.
    const uint32_t W = 64, LAYERS = 8, RS_CAP = 640, ACT_CAP = 201, NR = RS_CAP + 2, NA = ACT_CAP + 1;
    unsigned long counts[4] = {0, 0, 0, 0}, shapes = 0;
    for (int bias = 0; bias < 2; ++bias) {
        // reach[(last * NA + act) * NR + Rs]
        std::vector<char> reach((size_t)(W + 1) * NA * NR, 0), next;
        std::vector<char> seen((size_t)NA * NR, 0);
        for (uint32_t w = 1; w <= W; ++w) reach[((size_t)w * NA + w) * NR + (bias ? w : 0u)] = 1;      // the first layer: its weights are not small tensors
        for (uint32_t depth = 1; depth <= LAYERS; ++depth) {
            next.assign(reach.size(), 0);
            for (uint32_t last = 1; last <= W; ++last)
                for (uint32_t act = 0; act < NA; ++act)
                    for (uint32_t Rs = 0; Rs < NR; ++Rs) {
                        if (!reach[((size_t)last * NA + act) * NR + Rs]) continue;
                        seen[(size_t)act * NR + Rs] = 1;
                        if (depth == LAYERS) continue;
                        for (uint32_t w = 1; w <= W; ++w) {
                            uint32_t a2 = act + w, r2 = Rs + w * last + (bias ? w : 0u);
                            if (a2 > ACT_CAP) a2 = ACT_CAP;
                            if (r2 > RS_CAP) r2 = RS_CAP + 1;
                            next[((size_t)w * NA + a2) * NR + r2] = 1;
                        }
                    }
            reach.swap(next);
        }
        for (uint32_t act = 0; act < NA; ++act)
            for (uint32_t Rs = 0; Rs < NR; ++Rs) {
                if (!seen[(size_t)act * NR + Rs]) continue;
                ++shapes;
                const uint32_t rs_members[2] = {Rs, Rs > RS_CAP ? 7u * W * W + 8u * W : Rs}, act_members[2] = {act, act >= ACT_CAP ? 8u * W : act};
                for (uint32_t B_pad = 32; B_pad <= 512; B_pad += 32)
                    for (int exact = 0; exact < 2; ++exact)
                        for (int m = 0; m < 2; ++m) ++counts[middle(rs_members[m], act_members[m], B_pad, exact != 0, Switches())];
            }
    }
    printf("sweep: %lu (Rs, act) cells; mid_gen %lu, upper_gen %lu, upper_lds %lu, upper_mem %lu\n", shapes, counts[MID_GEN], counts[UPPER_GEN],
           counts[UPPER_LDS], counts[UPPER_MEM]);
    printf("upper_lds reachable with both switches on: %s\n", counts[UPPER_LDS] ? "yes" : "no");
    expect("the sweep reaches the three other kinds", counts[MID_GEN] && counts[UPPER_GEN] && counts[UPPER_MEM]);
    return g_failures ? 1 : 0;
}
