// The decision table of the specialised kernels' selection (brancher_amd/csrc/spec_select.h), row by row.  The expected values
// were derived by reading the selection as it was spread over geo(), launch() and applies() of specialize.cpp — not from the
// function under test.  Exit status 0: every row holds; 1 otherwise, with each row that does not printed.
#include <stdio.h>

#include "spec_select.h"

using namespace bsvi_spec;

static int g_failures = 0;

// defaults of the table: 8 waves in the one-workgroup geometry, 256-thread many-workgroup geometry with 2 per CU, 256 CUs,
// draw waves allowed, 20 noise rows, every switch on, nothing failed, loop mode, no diagnostics, exchange or gather
static SelectInput base(uint32_t n) {
    SelectInput in;
    in.max_waves_one = 8; in.many_threads = 256; in.many_per_cu = 2; in.n_cus = 256;
    in.draw_wave_ok = true; in.n_noise = 20; in.exchange_ok = true; in.has_previous = true;
    in.n_local = n; in.mode = SELECT_MODE_LOOP;
    return in;
}

static void served(const char* row, const SelectInput& in, uint32_t blocks, uint32_t threads, int variant, int fallback = -1,
                   uint32_t fallback_threads = 0) {
    const Selection r = select(in);
    const uint32_t waves = (in.n_local + 63) / 64;
    const bool ok = r.status == SELECT_OK && r.applies && r.blocks == blocks && r.threads == threads && r.variant == variant
                    && r.fallback_variant == fallback && r.fallback_threads == fallback_threads && r.geometry == (variant == 2 || variant == 3 ? 1 : 0)
                    && (blocks != 1 || r.extra_waves == threads / 64 - waves);
    if (ok) return;
    ++g_failures;
    printf("%s (n = %u): expected %u x %u variant %d fallback %d at %u; got status %d applies %d %u x %u variant %d fallback %d at %u, %u extra waves\n",
           row, in.n_local, blocks, threads, variant, fallback, fallback_threads, (int)r.status, (int)r.applies, r.blocks, r.threads,
           r.variant, r.fallback_variant, r.fallback_threads, r.extra_waves);
}

static void refused(const char* row, const SelectInput& in, SelectStatus why) {
    const Selection r = select(in);
    if (r.status == why && r.reason[0]) return;
    ++g_failures;
    printf("%s (n = %u): expected status %d with a reason; got %d, variant %d\n", row, in.n_local, (int)why, (int)r.status, r.variant);
}

static void applies(const char* row, const SelectInput& in, bool expected) {
    if (select(in).applies == expected) return;
    ++g_failures;
    printf("%s (n = %u): applies is %d\n", row, in.n_local, (int)!expected);
}

int main() {
    // one to three sample waves: one draw wave; the kernel without it is the fallback
    served("one sample wave", base(1), 1, 128, V_DRAW_WAVE, V_ONE, 64);
    served("one sample wave", base(64), 1, 128, V_DRAW_WAVE, V_ONE, 64);
    served("two sample waves", base(65), 1, 192, V_DRAW_WAVE, V_ONE, 128);
    served("three sample waves", base(192), 1, 256, V_DRAW_WAVE, V_ONE, 192);
    // four and five: the draw service with the owners on a draw wave
    const uint32_t service_sizes[] = {193u, 256u, 257u, 320u};
    for (uint32_t n : service_sizes) served("draw service, owners' wave", base(n), 1, 512, V_OWNERS);
    // six to eight: no extra wave; beyond: the many-workgroup geometry
    served("six sample waves", base(321), 1, 384, V_ONE);
    served("eight sample waves", base(512), 1, 512, V_ONE);
    served("nine sample waves", base(513), 3, 256, V_MANY);
    served("every workgroup resident", base(200000), 512, 256, V_MANY);
    { SelectInput in = base(513); in.loop_many = false; applies("BSVI_SPEC_LOOP_MANY=0", in, false); }
    { SelectInput in = base(512); in.loop_many = false; applies("BSVI_SPEC_LOOP_MANY=0, one workgroup", in, true); }
    { SelectInput in = base(513); in.loop_many = false; in.mode = 1; applies("BSVI_SPEC_LOOP_MANY=0, step mode", in, true); }
    // the draw waves' tiles hold the sets: 4 x 68 rows for four sample waves (and one more set for the owners' wave), 3 x 68 for five
    { SelectInput in = base(256); in.n_noise = 54; served("54 noise rows", in, 1, 512, V_OWNERS); }
    { SelectInput in = base(256); in.n_noise = 55; served("55 noise rows", in, 1, 512, V_DRAW_WAVE, V_ONE, 256); }
    { SelectInput in = base(300); in.n_noise = 34; served("34 noise rows", in, 1, 512, V_OWNERS); }
    { SelectInput in = base(300); in.n_noise = 35; served("35 noise rows", in, 1, 512, V_DRAW_WAVE, V_ONE, 320); }
    { SelectInput in = base(300); in.n_noise = 40; served("40 noise rows", in, 1, 512, V_DRAW_WAVE, V_ONE, 320); }
    { SelectInput in = base(300); in.n_noise = 41; served("41 noise rows", in, 1, 320, V_ONE); }
    // kernels compiled for four waves
    { SelectInput in = base(64); in.max_waves_one = 4; served("4-wave geometry", in, 1, 128, V_DRAW_WAVE, V_ONE, 64); }
    { SelectInput in = base(192); in.max_waves_one = 4; served("4-wave geometry", in, 1, 256, V_DRAW_WAVE, V_ONE, 192); }
    { SelectInput in = base(193); in.max_waves_one = 4; served("4-wave geometry", in, 1, 256, V_ONE); }
    { SelectInput in = base(257); in.max_waves_one = 4; served("4-wave geometry", in, 2, 256, V_MANY); }
    // a program that allows no draw waves
    { SelectInput in = base(64); in.draw_wave_ok = false; served("no draw waves", in, 1, 64, V_ONE); }
    { SelectInput in = base(256); in.draw_wave_ok = false; served("no draw waves", in, 1, 256, V_ONE); }
    // one evaluation, one step: no extra waves; the diagnostic kernel by the launch's arguments
    for (int mode = 0; mode < 2; ++mode)
        for (int diag = 0; diag < 2; ++diag) {
            SelectInput in = base(256); in.mode = mode; in.diagnostic = diag != 0; served("sums / step", in, 1, 256, diag ? V_ONE_DIAG : V_ONE);
            in.n_local = 513; served("sums / step", in, 3, 256, diag ? V_MANY_DIAG : V_MANY);
        }
    { SelectInput in = base(128); in.diagnostic = true; served("loop, diagnostic", in, 1, 128, V_ONE_DIAG); }
    { SelectInput in = base(256); in.diagnostic = true; served("loop, diagnostic", in, 1, 256, V_ONE_DIAG); }
    // the switches
    { SelectInput in = base(128); in.draw_wave = false; served("BSVI_SPEC_DRAW_WAVE=0", in, 1, 128, V_ONE); }
    { SelectInput in = base(256); in.draw_wave = false; served("BSVI_SPEC_DRAW_WAVE=0", in, 1, 256, V_ONE); }
    { SelectInput in = base(256); in.draw_service = false; served("BSVI_SPEC_DRAW_SERVICE=0", in, 1, 320, V_DRAW_WAVE, V_ONE, 256); }
    { SelectInput in = base(300); in.draw_service = false; served("BSVI_SPEC_DRAW_SERVICE=0", in, 1, 320, V_ONE); }
    { SelectInput in = base(256); in.owner_wave = false; served("BSVI_SPEC_OWNER_WAVE=0", in, 1, 512, V_DRAW_WAVE, V_ONE, 256); }
    { SelectInput in = base(256); in.lean_chain = false; served("BSVI_SPEC_LEAN_CHAIN=0", in, 1, 512, V_OWNERS_PREVIOUS); }
    { SelectInput in = base(256); in.lean_chain = false; in.has_previous = false; refused("BSVI_SPEC_LEAN_CHAIN=0, no previous source", in, SELECT_NO_PREVIOUS); }
    // the in-loop exchange
    { SelectInput in = base(128); in.exchange = true; served("exchange", in, 1, 192, V_EXCHANGE); }
    { SelectInput in = base(256); in.exchange = true; served("exchange", in, 1, 512, V_EXCHANGE); }
    { SelectInput in = base(256); in.exchange = true; in.diagnostic = true; refused("exchange, diagnostic", in, SELECT_NO_EXCHANGE); }
    { SelectInput in = base(513); in.exchange = true; refused("exchange, many workgroups", in, SELECT_NO_EXCHANGE); }
    { SelectInput in = base(256); in.exchange = true; in.mode = 1; refused("exchange, step mode", in, SELECT_NO_EXCHANGE); }
    // kernels that did not compile: the draw-wave kernel is not asked for again; the owners' kernel is (its error is the launch's)
    { SelectInput in = base(128); in.failed[V_DRAW_WAVE] = true; served("failed[4]", in, 1, 128, V_ONE); }
    { SelectInput in = base(256); in.failed[V_DRAW_WAVE] = true; served("failed[4]", in, 1, 256, V_ONE); }
    { SelectInput in = base(256); in.failed[V_OWNERS] = true; served("failed[6]", in, 1, 512, V_OWNERS); }
    // the gather phase: the same variant numbers (of the minibatch table)
    { SelectInput in = base(256); in.gather = true; served("gather", in, 1, 512, V_OWNERS); }
    { SelectInput in = base(256); in.gather = true; in.diagnostic = true; refused("gather, diagnostic", in, SELECT_NO_GATHER); }
    { SelectInput in = base(256); in.gather = true; in.exchange = true; refused("gather, exchange", in, SELECT_NO_GATHER); }
    { SelectInput in = base(256); in.gather = true; in.mode = 1; refused("gather, step mode", in, SELECT_NO_GATHER); }
    { SelectInput in = base(256); in.gather = true; in.mode = 0; refused("gather, sums mode", in, SELECT_NO_GATHER); }
    // served at all
    { SelectInput in = base(64); in.jit = false; applies("BSVI_JIT=0", in, false); }
    { SelectInput in = base(64); in.failed[V_ONE] = true; applies("failed[0]", in, false); }
    { SelectInput in = base(64); in.failed[V_ONE_DIAG] = true; applies("failed[1]", in, false); }
    { SelectInput in = base(513); in.failed[V_MANY] = true; applies("failed[2]", in, false); }
    { SelectInput in = base(64); in.failed[V_MANY] = true; applies("failed[2], one workgroup", in, true); }
    if (g_failures) printf("%d rows of the decision table do not hold\n", g_failures);
    return g_failures ? 1 : 0;
}
