// spec_select.h — which specialised kernel a launch gets, and in which shape: the kernel variants by name and ONE pure
// function from what the program, the launch and the environment say to the decision.  Host only: no HIP, no
// getenv — specialize.cpp fills the input; tests/c_abi/spec_select_table.cpp walks the decision table without a GPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace bsvi_spec {

// The kernel variants.  The values are public: bsvi_program_source / bsvi_program_source_minibatch take them and
// bsvi_spec_last_variant returns them.  How each is built from a generated base source: kVariants (specialize.cpp).
enum VariantId {
    V_ONE = 0,              // one workgroup: the training kernel (Philox noise, no per-sample outputs)
    V_ONE_DIAG = 1,         // one workgroup: the diagnostic kernel (noise in / samples, noise and per-sample values out)
    V_MANY = 2,             // many workgroups: the training kernel
    V_MANY_DIAG = 3,        // many workgroups: the diagnostic kernel
    V_DRAW_WAVE = 4,        // V_ONE with waves that carry no samples and draw the normals (one draw wave, or the draw service)
    V_EXCHANGE = 5,         // V_ONE with the cross-rank exchange inside the training loop (draw waves when the program allows them)
    V_OWNERS = 6,           // V_DRAW_WAVE with the owners' epilogue on a draw wave of the draw service
    V_OWNERS_PREVIOUS = 7,  // V_OWNERS as it was before the lean chain (comparisons; exists when BSVI_SPEC_LEAN_CHAIN was set at creation)
    V_COUNT = 8
};

// the two launch geometries, each with its own compiled kernels (specialize.cpp, Geom)
enum { GEOM_ONE = 0, GEOM_MANY = 1 };

constexpr int SELECT_MODE_LOOP = 2;     // bsvi_spec::MODE_LOOP (bsvi_internal.h): the training loop inside the kernel

struct SelectInput {
    // what the program's specialisation knows
    uint32_t max_waves_one = 0;         // waves of the one-workgroup geometry's kernels (4 or 8)
    uint32_t many_threads = 256;        // threads of a workgroup of the many-workgroup geometry
    uint32_t many_per_cu = 2;           // such workgroups per CU: what the kernels are compiled for, reduced until they fit a CU's LDS
    uint32_t n_cus = 256;
    bool draw_wave_ok = false;          // the program allows draw waves (Spec::draw_wave_ok)
    uint32_t n_noise = 0;
    bool exchange_ok = false;
    bool has_previous = false;          // V_OWNERS_PREVIOUS has a source
    bool failed[V_COUNT] = {};          // variants that did not compile — of the PLAIN table, also for a launch with the gather phase (*)
    // what the launch asks
    uint32_t n_local = 0;
    int mode = 0;                       // bsvi_spec::Mode
    bool diagnostic = false;            // caller noise, per-sample outputs or caller weights
    bool exchange = false;              // the in-loop cross-rank exchange
    bool gather = false;                // the minibatch gather phase (kernels of the minibatch table)
    // the switches BSVI_JIT, BSVI_SPEC_LOOP_MANY, _DRAW_WAVE, _DRAW_SERVICE, _OWNER_WAVE, _LEAN_CHAIN: on unless the value starts with '0'
    bool jit = true, loop_many = true, draw_wave = true, draw_service = true, owner_wave = true, lean_chain = true;
};

enum SelectStatus { SELECT_OK = 0, SELECT_NO_EXCHANGE, SELECT_NO_GATHER, SELECT_NO_PREVIOUS };

struct Selection {
    bool applies = false;               // the specialised kernels serve n_local samples in this mode at all (the interpreter otherwise)
    SelectStatus status = SELECT_OK;    // not SELECT_OK: this launch is not served; `reason` says why
    const char* reason = "";
    int variant = V_ONE;
    uint32_t blocks = 1, threads = 0;
    int geometry = GEOM_ONE;            // the compile-time geometry of the variant
    uint32_t extra_waves = 0;           // waves of `threads` that carry no samples
    int fallback_variant = -1;          // what the launch gets when `variant` does not compile (-1: its error is the launch's)
    uint32_t fallback_threads = 0;
};

// Oddities of the decision, kept as they are:
//  (*) with `gather` the kernels come from the minibatch table, but "did the draw-wave kernel fail" is asked of the plain table: a
//      minibatch twin that does not compile is tried, and fallen back from, at every launch;
//  (+) only V_DRAW_WAVE has a fallback: a V_OWNERS, V_OWNERS_PREVIOUS or V_EXCHANGE that does not compile is an error of the launch;
//  (#) a query without the launch's details (bsvi_program_engine) reports the extra waves a diagnostic launch then takes off again.
inline Selection select(const SelectInput& in) {
    Selection r;
    const uint32_t waves = (in.n_local + 63) / 64;
    const bool loop = in.mode == SELECT_MODE_LOOP;
    bool owners = false;
    if (waves <= in.max_waves_one) {
        // The in-kernel loop is given waves beyond those the samples need: they carry no samples and draw the next iteration's
        // normals (spec_main.h).  Up to four sample waves — one per SIMD — one draw wave, drawing for the owners' wave, whose chain
        // is what an iteration takes; beyond that two sample waves share a SIMD and their draws set the pace.
        const bool draws = loop && in.draw_wave_ok && in.draw_wave && !in.failed[in.exchange ? V_EXCHANGE : V_DRAW_WAVE];
        const bool single = draws && waves <= 4 && waves + 1 <= in.max_waves_one;
        // four or five sample waves: four / three draw waves draw for ALL of them (the draw service; switched off: the single draw
        // wave up to four sample waves, none at five); the sets are handed over in the draw waves' transpose tiles of 64 x 68 floats.
        // (Three sample waves: 3.89 us with the single draw wave, 3.94 with the service; one and two: the single draw wave.)
        const uint32_t n_service = waves == 4 ? 4u : 3u;
        const size_t room = (size_t)n_service * 64u * 68u;
        const bool service = draws && in.draw_service && waves >= 4 && waves <= 5 && waves + n_service <= in.max_waves_one
                             && (size_t)in.n_noise * 64u * waves <= room;
        r.extra_waves = service ? n_service : single ? 1u : 0u;
        // the owners on a draw wave: one more buffer, for the set the owners' wave draws — and a full workgroup: the lean epilogue
        // adds the rows of all waves the kernel is compiled for
        owners = service && (size_t)in.n_noise * 64u * (waves + 1u) <= room && waves + n_service == in.max_waves_one;
        r.threads = (waves + r.extra_waves) * 64u;
    } else {
        // many samples: workgroups of one wave per SIMD, as many per CU as the kernels are compiled for; beyond that every
        // workgroup walks several chunks of samples
        r.geometry = GEOM_MANY;
        r.threads = in.many_threads;
        r.blocks = (in.n_local + r.threads - 1) / r.threads;
        if (r.blocks > in.many_per_cu * in.n_cus) r.blocks = in.many_per_cu * in.n_cus;
    }
    const int base = 2 * r.geometry + (in.diagnostic ? 1 : 0);
    r.variant = base;
    // several workgroups in loop mode: workgroup 0 owns the iteration, the others wait on its generation number (spec_main.h);
    // every workgroup must be resident — never more are asked for than fit the chip (loop_many off: launch per iteration)
    r.applies = in.n_local != 0 && in.jit && !in.failed[2 * r.geometry] && !in.failed[2 * r.geometry + 1]
                && (!(loop && r.blocks != 1) || in.loop_many);
    auto refuse = [&r](SelectStatus why, const char* text) { r.status = why; r.reason = text; return r; };
    if (in.exchange && !(loop && r.blocks == 1 && base == V_ONE && in.exchange_ok))
        return refuse(SELECT_NO_EXCHANGE, "the in-loop exchange serves the one-workgroup training loop with Philox noise and no per-sample outputs");
    // the loop with the gather phase: Philox noise, no per-sample outputs, one rank — everything else trains launch by launch
    if (in.gather && (!loop || in.diagnostic || in.exchange))
        return refuse(SELECT_NO_GATHER, "the in-kernel minibatch gather serves the training loop with Philox noise, no per-sample outputs and one rank");
    if (in.exchange) {
        r.variant = V_EXCHANGE;
    } else if (owners && base == V_ONE && in.owner_wave) {
        r.variant = in.lean_chain ? V_OWNERS : V_OWNERS_PREVIOUS;
        if (r.variant == V_OWNERS_PREVIOUS && !in.has_previous)
            return refuse(SELECT_NO_PREVIOUS, "BSVI_SPEC_LEAN_CHAIN=0 needs the variable set when the program is created (the previous source is generated then)");
    } else if (r.extra_waves && base == V_ONE) {
        r.variant = V_DRAW_WAVE;
        r.fallback_variant = V_ONE;
        r.fallback_threads = r.threads - 64u * r.extra_waves;
    } else if (r.extra_waves) {          // the diagnostic kernel has no draw waves
        r.threads -= 64u * r.extra_waves;
        r.extra_waves = 0;
    }
    return r;
}

}  // namespace bsvi_spec
