// spec_main.h — second half of the frame around a program-specialised ELBO kernel (see spec_prelude.h): the kernel.
//
// One workgroup = up to SPEC_MAX_WAVES waves of 64 Monte-Carlo samples.  Per iteration:
//   prologue   U[k] = a + b*g(theta | const), 1/U[k], log U[k]     (geometric_ranges.py transforms: once per launch for
//              every entry, then per iteration by the thread that owns the parameter)
//   body       spec_draw() + spec_body(): GENERATED straight-line forward / reverse sweep of one sample per lane,
//              registers only; per-lane gradient contributions leave through the transpose tile (SPEC_DU)
//   reduce     wave (DPP) -> workgroup (LDS) -> grid (partials + arrival ticket, last workgroup finishes); fixed
//              order everywhere, no float atomics: bitwise reproducible
//   epilogue   chain rule U -> theta through the CSR map; by mode: sums only (the caller all-reduces them over the
//              sample shards of other GPUs), or loss / finite flag / scaled gradients / fused SGD-Adam step
//              (inference.py:96-108), or that whole loop n_iterations times inside this one launch.
#pragma once
// The gather phase of the in-kernel training loop (SPEC_MINIBATCH, a define of the generated source with the sources' geometry
// as literals — specialize.cpp, set_minibatches): observations that are a minibatch of a dataset take other rows in every
// iteration, drawn by the keyed bijection of minibatch_index.h from (key, offset0 + it).  SPEC_DEBUG_NO_GATHER compiles the
// phase out (measurements: what it costs; the rows then stay those of the observation buffer).
#if defined(SPEC_MINIBATCH) && !SPEC_DIAG && !defined(SPEC_WITH_EXCHANGE) && !defined(SPEC_DEBUG_NO_GATHER)
#define SPEC_MB 1
#include "minibatch_index.h"
#else
#define SPEC_MB 0
#endif

namespace bsvi {

// Scalar-register discipline (as in the interpreter's persistent kernels): SpecArgs is ~50 dwords.  Read as `A.x`
// they are all loaded at entry and stay live through the body, whose Philox key schedule and exec masks then spill
// through v_writelane / v_readlane.  So every phase re-reads what it needs from the kernarg segment, through a
// pointer the optimiser cannot see through.
#if defined(__HIP_DEVICE_COMPILE__)
#define SPEC_CONST_AS __attribute__((address_space(4)))
#define SPEC_GLOBAL_AS __attribute__((address_space(1)))
#define SPEC_RELOAD_ARGS() asm volatile("" : "+s"(ka))
#else
#define SPEC_CONST_AS
#define SPEC_GLOBAL_AS
#define SPEC_RELOAD_ARGS()
#endif

// TAB (words): uniform entries [4 * NU] | CSR row pointers [NP + 1] | positions [NUG] | uniform indices [NUG] |
//              per parameter: bit 0 active, bit 1 active while iteration <= pretraining_iterations [NP]
#define SPEC_TAB_PTR (4 * SPEC_N_UNIFORM)
#define SPEC_TAB_POS (SPEC_TAB_PTR + SPEC_N_PARAMS + 1)
#define SPEC_TAB_IDX (SPEC_TAB_POS + SPEC_N_POS)
#define SPEC_TAB_MASK (SPEC_TAB_IDX + SPEC_N_POS)

// The barriers of the iteration loop order LDS traffic only (sums, uniform table, theta all live in LDS), so they wait
// for the LDS counter and not for global memory: __syncthreads() also drains vmcnt, i.e. every iteration would wait
// for the write acknowledgements of its loss / gradient stores — 1.3 of 6.3 us per iteration at BASELINE config 1.
__device__ __forceinline__ void spec_lds_barrier() {
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
#endif
}

// U[k] = a + b * g(x) and its companions, from the LDS copy of entry k
// The transforms of the uniform table: values through the library forms of dist_math.h (softplusf_ / sigmoidf_, see
// there), derivatives on the hardware transcendental units (their rounding moves a gradient by 1e-7).  The transform id is
// data: written as one switch the compiler evaluates EVERY case and selects — tanh polynomial, sqrt refinement and all;
// the rare ones stay out of line behind a real branch.
__device__ __noinline__ float spec_utransform_rare(uint32_t t, float x) { return utransform((int)t, x); }
__device__ __noinline__ float spec_utransform_grad_rare(uint32_t t, float x) { return utransform_grad((int)t, x); }
#ifndef SPEC_RARE_TRANSFORMS
#define SPEC_RARE_TRANSFORMS 1
#endif
#ifndef SPEC_UT_MASK
#define SPEC_UT_MASK 0xFFu
#endif
__device__ __forceinline__ float utransform_common(uint32_t t, float x) {
#if SPEC_RARE_TRANSFORMS
    if (t > BSVI_UT_SIGMOID) return spec_utransform_rare(t, x);
#endif
    // (both evaluated and selected — unless the program's table has no entry of the kind: SPEC_UT_MASK)
    const float soft = ((SPEC_UT_MASK >> BSVI_UT_SOFTPLUS) & 1u) ? softplusf_(x) : x;
    const float sig = ((SPEC_UT_MASK >> BSVI_UT_SIGMOID) & 1u) ? sigmoidf_(x) : x;
    return t == BSVI_UT_IDENTITY ? x : (t == BSVI_UT_SOFTPLUS ? soft : sig);
}
__device__ __forceinline__ float spec_utransform_grad(uint32_t t, float x) {
#if SPEC_RARE_TRANSFORMS
    if (t > BSVI_UT_SIGMOID) return spec_utransform_grad_rare(t, x);
#endif
    const float s = spec_rcp(1.0f + __expf(-x));               // sigmoid(x) = softplus'(x)
    const float soft = x > 20.0f ? 1.0f : s;
    return t == BSVI_UT_IDENTITY ? 1.0f : (t == BSVI_UT_SOFTPLUS ? soft : s * (1.0f - s));
}
// An entry's three values go to its homes.  SPEC_HOME(k) is what a writer keeps of entry k (the owners' rows hold it in the place
// of k): k itself in the compact layout; SPEC_QUADS: the homes of U and of the pair (1 / U, log U) in float offsets, 16 bits each,
// from the generated map — two stores, as in the compact layout.
#if SPEC_QUADS
__constant__ uint32_t spec_q_homes[SPEC_N_UNIFORM] = SPEC_Q_HOMES;
#define SPEC_HOME(k) spec_q_homes[k]
__device__ __forceinline__ void spec_store_uniform(uint32_t home, float u) {
    float* const pair = spec_lds + (home >> 16);
    spec_lds[home & 0xFFFFu] = u;
    pair[0] = spec_rcp(u);
    pair[1] = spec_log(u);
}
#else
#define SPEC_HOME(k) (k)
__device__ __forceinline__ void spec_store_uniform(uint32_t k, float u) {
    spec_lds[k] = u;
    spec_lds[SPEC_OFF_UR + k] = spec_rcp(u);
    spec_lds[SPEC_OFF_UL + k] = spec_log(u);
}
#endif
__device__ __forceinline__ void spec_publish_uniform(const uint32_t* TAB, uint32_t k, float x) {
    const uint32_t w1 = TAB[4 * k + 1];
    spec_store_uniform(SPEC_HOME(k), __uint_as_float(TAB[4 * k + 2]) + __uint_as_float(TAB[4 * k + 3]) * utransform_common(w1 & 0xFFu, x));
}

// The most uniform entries a parameter of this program owns, 1 or 2 (specialize.cpp): the owners' code handles that many.
// Every parameter of a scalar model owns one — the second position's row of sums, its chain-rule factor and its guarded
// store were read, multiplied and not selected in every iteration.
#ifndef SPEC_OWN_ENTRIES
#define SPEC_OWN_ENTRIES 2
#endif
// rows of sums already in registers, added waves in order (every row is a wave's: the caller runs with a full workgroup)
__device__ __forceinline__ float spec_rows_total(const float (&r)[SPEC_MAX_WAVES]) {
    float s = 0.0f;
#pragma unroll
    for (uint32_t w = 0; w < SPEC_MAX_WAVES; ++w) s += r[w];
    return s;
}
// What the thread that owns parameter `tid` keeps in registers across the iterations of a launch (parameters beyond
// the workgroup size, or with more than two uniform entries, go through the LDS working copy instead)
struct SpecOwn {
    float theta, s0, s1, s2, st;     // parameter and optimizer state
    float a[2], b[2];                // its uniform entries: U = a + b * g(theta)
    uint32_t pos[2], k[2], tr[2];
    uint32_t n, mask;                // entries (0..2); mask bits (SPEC_TAB_MASK)
    double p1, p2;                   // Adam, AdamW, Adamax: beta1^st, beta2^st as running products (optimizer_apply_running)
};
__device__ __forceinline__ void spec_own_store_products(spec_f4* row, const SpecOwn& o) {
    const unsigned long long a = __double_as_longlong(o.p1), b = __double_as_longlong(o.p2);
    row[4] = spec_f4{__uint_as_float((uint32_t)a), __uint_as_float((uint32_t)(a >> 32)), __uint_as_float((uint32_t)b), __uint_as_float((uint32_t)(b >> 32))};
}
__device__ __forceinline__ void spec_own_store(spec_f4* row, const SpecOwn& o) {
    row[0] = spec_f4{o.theta, o.s0, o.s1, o.s2};
    row[1] = spec_f4{o.st, o.a[0], o.b[0], o.a[1]};
    row[2] = spec_f4{o.b[1], __uint_as_float(o.pos[0]), __uint_as_float(o.pos[1]), __uint_as_float(o.k[0])};
    row[3] = spec_f4{__uint_as_float(o.k[1]), __uint_as_float(o.tr[0] | (o.tr[1] << 8) | (o.n << 16) | (o.mask << 24)), 0.0f, 0.0f};
    spec_own_store_products(row, o);
}
__device__ __forceinline__ SpecOwn spec_own_load(const spec_f4* row) {
    const spec_f4 q0 = row[0], q1 = row[1], q2 = row[2], q3 = row[3], q4 = row[4];
    SpecOwn o;
    o.p1 = __longlong_as_double((long long)(((unsigned long long)__float_as_uint(q4.y) << 32) | __float_as_uint(q4.x)));
    o.p2 = __longlong_as_double((long long)(((unsigned long long)__float_as_uint(q4.w) << 32) | __float_as_uint(q4.z)));
    o.theta = q0.x; o.s0 = q0.y; o.s1 = q0.z; o.s2 = q0.w;
    o.st = q1.x; o.a[0] = q1.y; o.b[0] = q1.z; o.a[1] = q1.w;
    o.b[1] = q2.x; o.pos[0] = __float_as_uint(q2.y); o.pos[1] = __float_as_uint(q2.z); o.k[0] = __float_as_uint(q2.w);
    o.k[1] = __float_as_uint(q3.x);
    const uint32_t meta = __float_as_uint(q3.y);
    o.tr[0] = meta & 0xFFu; o.tr[1] = (meta >> 8) & 0xFFu; o.n = (meta >> 16) & 0xFFu; o.mask = meta >> 24;
    return o;
}

// ---- the cross-rank sum INSIDE the in-kernel training loop (SPEC_WITH_EXCHANGE: a kernel variant of its own, compiled
//      when a multi-rank run first asks for it).  Monte-Carlo samples are sharded over the GPUs of a node; per
//      iteration every rank holds its loss sum, its non-finite count and, after the chain rule, one gradient sum per
//      parameter, and all ranks need the totals before the (replicated) optimizer step.  The protocol is the one-shot
//      direct-write exchange of collective.hip — same regions and abort word, its own area and call count, so launches of
//      that kernel and of this one can follow each other on the same bsvi_exchange — run by the OWNERS' WAVE alone: lane i owns parameter i
//      (SPEC_GENERIC_OWNERS == 0: every parameter has an owner in that one wave), so
//        1. lane i stores its parameter's sum (lane 0 also the two loss words) into this rank's row of EVERY region,
//        2. lane i reads every rank's entry of its parameter (and the loss words) in this rank's region until all carry the
//           call's number (bounded; anybody's abort ends it) and adds them in rank order: bit-identical totals on every rank.
//      No workgroup barrier: the other waves go on to the next iteration's first barrier (drawing its normals on the way),
//      where they wait for the owners to publish the new table as always.
#if defined(SPEC_WITH_EXCHANGE) && !SPEC_DIAG && !SPEC_ACCUMULATE_CHUNKS
#define SPEC_EXCHANGE 1
// An entry of the region's second area carries its value AND the number of the call that wrote it in one 8-byte word
// (xchg_ll_entry), stored with a single 64-bit store: a reader that finds the call's number has the value — no fence and no
// separate flag between "data written" and "data may be read", one store -> one load across the link instead of store, fence,
// flag, poll, load.  (Measured with one rank exchanging with itself, fine-grained memory: the flagged form of
// collective.hip's kernel added 2.5 us to a 4.8 us iteration.)
__device__ __forceinline__ unsigned long long* spec_xentry(unsigned char* region, uint32_t parity, uint32_t r, uint32_t capacity, uint32_t world) {
    return reinterpret_cast<unsigned long long*>(region + XCHG_HEADER_WORDS * 4 + (size_t)2 * world * capacity * 4) + ((size_t)parity * world + r) * capacity;
}
// Programs whose parameters do not all have an owner in one wave (more than 64 of them, or more than two table entries each:
// SPEC_GENERIC_OWNERS): the same entries, written and awaited PER THREAD — a tagged entry needs no rendezvous, so the thread
// that forms a parameter's sum stores it to every region and later polls that one entry of every rank, wherever in the
// workgroup it sits.  Every thread also polls the loss words: each owner gates its own step on the total's finiteness.
__device__ __forceinline__ void spec_xput(const SpecExchange* xg, uint32_t seq, uint32_t k, float v) {
    const uint32_t world = xg->world, rank = xg->rank, cap = xg->capacity, parity = seq & 1u;
    const unsigned long long e = ((unsigned long long)seq << 32) | __float_as_uint(v);
    for (uint32_t p = 0; p < world; ++p)
        __hip_atomic_store(spec_xentry(xg->peer[p], parity, rank, cap, world) + k, e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ bool spec_xget(const SpecExchange* xg, uint32_t seq, uint32_t k, float& v) {
    const uint32_t world = xg->world, rank = xg->rank, cap = xg->capacity, parity = seq & 1u;
    unsigned char* const region = xg->peer[rank];
    uint32_t* const abort_word = reinterpret_cast<uint32_t*>(region) + XCHG_MAX_RANKS * XCHG_FLAG_STRIDE;
    unsigned long long t0 = 0;
    for (uint32_t round = 0;; ++round) {
        unsigned long long e[XCHG_MAX_RANKS];
#pragma unroll
        for (uint32_t r = 0; r < XCHG_MAX_RANKS; ++r) {
            e[r] = (unsigned long long)seq << 32;
            if (r < world) e[r] = __hip_atomic_load(spec_xentry(region, parity, r, cap, world) + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        bool all = true;
        float t = 0.0f;
#pragma unroll
        for (uint32_t r = 0; r < XCHG_MAX_RANKS; ++r) {
            all = all && (uint32_t)(e[r] >> 32) == seq;
            if (r < world) t += __uint_as_float((uint32_t)e[r]);
        }
        if (all) {
            v = t;
            return __hip_atomic_load(abort_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) == 0u;
        }
        if (round == 0u) t0 = wall_clock64();
        if (__hip_atomic_load(abort_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0u) return false;
        if (wall_clock64() - t0 > xg->timeout_ticks) {
            for (uint32_t p = 0; p < world; ++p)
                __hip_atomic_store(reinterpret_cast<uint32_t*>(xg->peer[p]) + XCHG_MAX_RANKS * XCHG_FLAG_STRIDE, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            return false;
        }
        __builtin_amdgcn_s_sleep(1);
    }
}
#if !SPEC_GENERIC_OWNERS
// returns false when the call was abandoned (this rank or a peer gave up waiting: sticky, csrc/collective.hip)
__device__ __forceinline__ bool spec_exchange(const SpecExchange* xg, uint32_t seq, uint32_t l, bool has_param, float& vs, float& vb, float& gsum) {
    const uint32_t world = xg->world, rank = xg->rank, cap = xg->capacity, parity = seq & 1u;
    uint32_t* const abort_word = reinterpret_cast<uint32_t*>(xg->peer[rank]) + XCHG_MAX_RANKS * XCHG_FLAG_STRIDE;
    const uint32_t aborted = __hip_atomic_load(abort_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);       // (needed at the end only)
    const unsigned long long tag = (unsigned long long)seq << 32;
    // 1. this rank's sums into its row of EVERY region (its own included): lane l its parameter's, lane 0 the loss words too
    for (uint32_t p = 0; p < world; ++p) {
        unsigned long long* const row = spec_xentry(xg->peer[p], parity, rank, cap, world);
        if (l == 0u) {
            __hip_atomic_store(row, tag | __float_as_uint(vs), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(row + 1, tag | __float_as_uint(vb), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        if (has_param) __hip_atomic_store(row + BSVI_OUT_HEADER + l, tag | __float_as_uint(gsum), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    // 2. every rank's row of THIS region, until all of them carry the call's number; added in rank order
    unsigned char* const region = xg->peer[rank];
    unsigned long long t0 = 0;
    bool gave_up = false;
    float ts, tb, tg;
    for (uint32_t round = 0;; ++round) {
        unsigned long long e0[XCHG_MAX_RANKS], e1[XCHG_MAX_RANKS], eg[XCHG_MAX_RANKS];
#pragma unroll
        for (uint32_t r = 0; r < XCHG_MAX_RANKS; ++r) {
            e0[r] = e1[r] = eg[r] = tag;
            if (r < world) {
                const unsigned long long* const row = spec_xentry(region, parity, r, cap, world);
                e0[r] = __hip_atomic_load(row, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                e1[r] = __hip_atomic_load(row + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                if (has_param) eg[r] = __hip_atomic_load(row + BSVI_OUT_HEADER + l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
        bool all = true;
        ts = 0.0f; tb = 0.0f; tg = 0.0f;
#pragma unroll
        for (uint32_t r = 0; r < XCHG_MAX_RANKS; ++r) {
            all = all && (uint32_t)(e0[r] >> 32) == seq && (uint32_t)(e1[r] >> 32) == seq && (uint32_t)(eg[r] >> 32) == seq;
            if (r < world) { ts += __uint_as_float((uint32_t)e0[r]); tb += __uint_as_float((uint32_t)e1[r]); tg += __uint_as_float((uint32_t)eg[r]); }
        }
        if (__all((int)all)) break;
        // somebody is late: bounded, and ended by anybody's abort
        if (round == 0u) t0 = wall_clock64();
        if (__hip_atomic_load(abort_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0u) { gave_up = true; break; }
        if (wall_clock64() - t0 > xg->timeout_ticks) {
            gave_up = true;
            if (l < world) __hip_atomic_store(reinterpret_cast<uint32_t*>(xg->peer[l]) + XCHG_MAX_RANKS * XCHG_FLAG_STRIDE, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            if (l == 0u) atomicAdd(abort_word + 1, 1u);
            break;
        }
        __builtin_amdgcn_s_sleep(1);
    }
    if (gave_up || aborted != 0u) return false;
    vs = ts; vb = tb; gsum = tg;
    return true;
}
#endif
#else
#define SPEC_EXCHANGE 0
#endif

#if defined(SPEC_WAVES_PER_EU)
#define SPEC_VGPR_ATTR __attribute__((amdgpu_waves_per_eu(SPEC_WAVES_PER_EU, SPEC_WAVES_PER_EU)))
#elif defined(SPEC_NUM_VGPR)
#define SPEC_VGPR_ATTR __attribute__((amdgpu_num_vgpr(SPEC_NUM_VGPR)))
#else
#define SPEC_VGPR_ATTR
#endif
// SPEC_BOUND_THREADS (>= SPEC_MAX_THREADS): the launch bound the register allocator sees.  A bound of 768 / 1024 threads
// caps a lane at 168 / 128 registers, so that 3 / 4 workgroups of 256 threads share a CU (the throughput regime).
#ifndef SPEC_BOUND_THREADS
#define SPEC_BOUND_THREADS SPEC_MAX_THREADS
#endif
extern "C" __global__ void __launch_bounds__(SPEC_BOUND_THREADS) SPEC_VGPR_ATTR bsvi_spec_kernel(const SpecArgs A_unused) {
    (void)A_unused;
    const SPEC_CONST_AS char* ka = (const SPEC_CONST_AS char*)__builtin_amdgcn_kernarg_segment_ptr();
#define SPEC_A ((const SPEC_CONST_AS SpecArgs*)ka)
    const uint32_t tid = threadIdx.x, nthreads = blockDim.x, W = nthreads >> 6, wave = tid >> 6, lane = tid & 63u;
    const uint32_t G = gridDim.x;
    float* const WS = spec_lds + SPEC_OFF_WS;
    float* const RED = spec_lds + SPEC_OFF_RED;
    float* const PS = spec_lds + SPEC_OFF_PS;
    uint32_t* const TAB = reinterpret_cast<uint32_t*>(spec_lds + SPEC_OFF_TAB);
    float* const WSw = WS + wave * SPEC_WS_PAD;

    SpecLane T;
    T.lane = lane;
    T.n = blockIdx.x * nthreads + tid;
    T.active = false; T.nc = 0; T.nidx = 0;
    T.vz = SPEC_VZ(T.n);
    T.tile = wave * SPEC_TR_FLOATS + lane;
    const uint32_t sample_base = SPEC_A->sample_base;
    const uint32_t n_chunks = (SPEC_A->n_local + G * nthreads - 1u) / (G * nthreads);
    const uint32_t mode = SPEC_A->mode;
    const bool step = mode != SPEC_MODE_SUMS;
    const uint32_t n_it = (mode == SPEC_MODE_LOOP) ? SPEC_A->n_iterations : 1u;

#if defined(SPEC_DEBUG_STAMPS)
    const unsigned long long stamp_entry = __builtin_amdgcn_s_memtime();
#endif
    // ---- once per launch: tables, observed data, theta and the optimizer state into LDS; the uniform table
    {
        const uint32_t* uniform = reinterpret_cast<const uint32_t*>(SPEC_A->uniform);
        const uint32_t* pu_ptr = SPEC_A->pu_ptr;
        const uint32_t* pu_pos = SPEC_A->pu_pos;
        const uint32_t* pu_idx = SPEC_A->pu_idx;
        const float* obs = SPEC_A->obs;
        const float* params = SPEC_A->params;
        const float* state = SPEC_A->state;
        const uint8_t* mask = SPEC_A->mask;
        const uint8_t* mask_first = SPEC_A->mask_first;
        // The first trip of every copy loop is REQUESTED before any of them is stored: eight dependent global round trips
        // (~1 us each, the tables are cold) in a row were most of the launch's prologue — a third of a 20-iteration launch.
        const bool h_uni = tid < 4u * SPEC_N_UNIFORM, h_ptr = tid < SPEC_N_PARAMS + 1u, h_pos = tid < SPEC_N_POS,
                   h_obs = tid < SPEC_N_OBS, h_par = tid < SPEC_N_PARAMS;
        uint32_t r_uni = 0, r_ptr = 0, r_pos = 0, r_idx = 0, r_mask = 0;
        float r_obs = 0.0f, r_par = 0.0f, r_st[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        const bool h_uni2 = tid + nthreads < 4u * SPEC_N_UNIFORM;            // (four words per entry: the table is the long one)
        uint32_t r_uni2 = 0;
        if (h_uni) r_uni = uniform[tid];
        if (h_uni2) r_uni2 = uniform[tid + nthreads];
        if (h_ptr) r_ptr = pu_ptr[tid];
        if (h_pos) { r_pos = pu_pos[tid]; r_idx = pu_idx[tid]; }
        if (h_obs) r_obs = obs[tid];
        if (h_par) {
            r_par = params[tid];
            if (step) {
                if (state) {
#pragma unroll
                    for (uint32_t s = 0; s < 4u; ++s) r_st[s] = state[(size_t)s * SPEC_N_PARAMS + tid];
                }
                r_mask = (mask[tid] ? 1u : 0u) | (mask_first[tid] ? 2u : 0u);
            }
        }
        asm volatile("" ::: "memory");        // (the loads stay in front of the stores: the compiler would pair them up again)
        if (h_uni) TAB[tid] = r_uni;
        if (h_uni2) TAB[tid + nthreads] = r_uni2;
        if (h_ptr) TAB[SPEC_TAB_PTR + tid] = r_ptr;
        if (h_pos) { TAB[SPEC_TAB_POS + tid] = r_pos; TAB[SPEC_TAB_IDX + tid] = r_idx; }
        if (h_obs) spec_lds[SPEC_OBS0 + tid] = r_obs;
        if (h_par) {
            PS[tid] = r_par;
            if (step) {
#pragma unroll
                for (uint32_t s = 0; s < 4u; ++s) PS[(1u + s) * SPEC_NP_PAD + tid] = r_st[s];      // no state buffer: a fresh optimizer (all zeros), nothing written back
                TAB[SPEC_TAB_MASK + tid] = r_mask;
            }
        }
        for (uint32_t i = tid + 2u * nthreads; i < 4u * SPEC_N_UNIFORM; i += nthreads) TAB[i] = uniform[i];
        for (uint32_t i = tid + nthreads; i < SPEC_N_PARAMS + 1u; i += nthreads) TAB[SPEC_TAB_PTR + i] = pu_ptr[i];
        for (uint32_t j = tid + nthreads; j < SPEC_N_POS; j += nthreads) { TAB[SPEC_TAB_POS + j] = pu_pos[j]; TAB[SPEC_TAB_IDX + j] = pu_idx[j]; }
        for (uint32_t i = tid + nthreads; i < SPEC_N_OBS; i += nthreads) spec_lds[SPEC_OBS0 + i] = obs[i];
        for (uint32_t i = tid + nthreads; i < SPEC_N_PARAMS; i += nthreads) {
            PS[i] = params[i];
            if (step) {
#pragma unroll
                for (uint32_t s = 0; s < 4u; ++s)
                    PS[(1u + s) * SPEC_NP_PAD + i] = state ? state[(size_t)s * SPEC_N_PARAMS + i] : 0.0f;
                TAB[SPEC_TAB_MASK + i] = (mask[i] ? 1u : 0u) | (mask_first[i] ? 2u : 0u);
            }
        }
        __syncthreads();
        const float* consts = SPEC_A->consts;
        for (uint32_t k = tid; k < SPEC_N_UNIFORM; k += nthreads) {
            const uint32_t src = TAB[4 * k], w1 = TAB[4 * k + 1];
            spec_publish_uniform(TAB, k, ((w1 >> 8) & 0xFFu) ? PS[src] : consts[src]);
        }
    }

    // the owner rows: built once, read back with four 16-byte LDS loads per iteration (kept in registers across the body
    // they are the first values the allocator spills to scratch: 2.2 us of scratch round trips per iteration)
    spec_f4* const OWN = reinterpret_cast<spec_f4*>(spec_lds + SPEC_OFF_OWN);
    // The owners are the first threads of wave SPEC_OWNER_WAVE when the workgroup has that wave and every parameter has an
    // owner (wave 1 by default: with five waves on four SIMDs wave 0 shares its SIMD with the fifth, and the serial epilogue
    // should not compete with that wave's work), else of wave 0.
#ifndef SPEC_OWNER_WAVE
#define SPEC_OWNER_WAVE 1u
#endif
    // The draw wave.  An iteration takes as long as the chain of the owners' wave: its draw, its body, the sums, the epilogue
    // (a single wave alone runs at nearly the speed of five, tools/wave_scaling.sh).  The in-kernel loop of a one-workgroup
    // launch is therefore given one wave more than the samples need (specialize.cpp, geo): it carries no samples and, beside
    // the epilogue, draws the NEXT iteration's normals of the owners' wave into its own — otherwise unused — transpose tile,
    // where the owners' wave picks them up behind the next barrier; every other wave draws beside the epilogue too, none
    // ahead of the barrier.  (Measured, tools/draw_wave_probe.sh: 64 samples 4.68 -> 3.83 us per iteration, 128: 4.79 -> 3.89,
    // 256: 4.91 -> 4.64; with five and more sample waves two of them share a SIMD and their late draws, not the owners'
    // chain, set the pace: 300 samples 5.0 -> 5.0.  The roles are a kernel variant of their own, SPEC_WITH_DRAW_WAVE, used
    // for up to four sample waves: merely compiled in they cost the plain loop 3 %.)  The draws are a function of (seed,
    // offset, sample index, row) only: who computes them does not change a bit of the result.
#if SPEC_TILE && SPEC_KEEP_NOISE && SPEC_KEEP_NOISE <= 68 && !SPEC_GENERIC_OWNERS && !SPEC_DIAG && !SPEC_ACCUMULATE_CHUNKS \
    && !defined(SPEC_DEBUG_NO_DRAW) && !defined(SPEC_NO_EARLY_DRAW) && !defined(SPEC_DEBUG_LATE_FREE) && defined(SPEC_WITH_DRAW_WAVE)
#define SPEC_DRAW_WAVE 1
    const uint32_t WSN = (SPEC_A->n_local + 63u) / 64u;     // waves that carry samples
    const bool has_draw_wave = mode == SPEC_MODE_LOOP && G == 1u && W >= 2u && WSN < W;
    const uint32_t fed_index = W == 2u ? 0u : 1u;         // the owners' wave, as without a draw wave (SPEC_OWNER_WAVE)
    // The draw SERVICE (round 5): five sample waves and three draw waves.  One wave issues a vector instruction every ~3.1 ns whether
    // or not a second wave shares its SIMD (profiles/r5/cfg1_wave_rate_notes.txt), so an iteration is the chain of one wave: body,
    // flush, sums — barrier — the owners' epilogue; with five sample waves the owners' wave also had to draw its own next noise in
    // front of that barrier (470 of its 1 650 instructions), and two late draws on one SIMD took longer than the epilogue they ran
    // beside (the Philox multiplies and the transcendentals are quarter-rate: a draw is 1.5 us of a SIMD's pipe).  Here NO sample wave
    // draws after the first iteration: the extra waves draw for all of them — draw wave k one set for sample wave k while the bodies
    // run (kept in registers, stored behind the barrier: a sample wave reads its buffer at the top of its body), and, when there are
    // more sample waves than draw waves, a second set beside the epilogue unless it sits on the owners' SIMD — into one buffer per
    // sample wave in the draw waves' own, otherwise unused, transpose tiles.  (300 samples: waves 5, 6, 7 for 0 | 1, 3 | 2, 4.)
    // The draws are functions of (seed, offset, sample, row): who computes them does not change a bit.
    const bool draw_service = has_draw_wave && W - WSN >= 3u;      // (three or more extra waves: the host asked for the service)
    const bool draw_wave = __builtin_amdgcn_readfirstlane((has_draw_wave && (draw_service ? wave >= WSN : wave == W - 1u)) ? 1 : 0) != 0;
    const bool fed_wave = __builtin_amdgcn_readfirstlane((has_draw_wave && (draw_service ? wave < WSN : wave == fed_index)) ? 1 : 0) != 0;
    // (one wave's set: SPEC_KEEP_NOISE rows of 64 lanes; the service's five buffers lie in the three draw waves' tiles)
    float* const NZ = spec_lds + SPEC_OFF_TR + (draw_service ? WSN * SPEC_TR_FLOATS + wave * (SPEC_KEEP_NOISE * 64u) : (W - 1u) * SPEC_TR_FLOATS) + lane;
    float* const NZB = spec_lds + SPEC_OFF_TR + WSN * SPEC_TR_FLOATS + lane;           // (service: buffer w at NZB + w * SPEC_KEEP_NOISE * 64)
    if (draw_wave) for (uint32_t k = lane; k < SPEC_WS_PAD; k += 64u) WSw[k] = 0.0f;     // its row of sums stays zero
#else
#define SPEC_DRAW_WAVE 0
    const bool has_draw_wave = false, draw_wave = false, fed_wave = false;
    const uint32_t fed_index = 1u;
#endif
    // The owners on a draw wave (round 7; a kernel variant of its own, SPEC_WITH_DRAW_OWNERS, launched with the draw service only):
    // the owners' epilogue leaves sample wave 1 for the service's draw wave on the same SIMD (wave 5), whose loop of its own keeps
    // the owner state in registers for the whole launch, evaluates what depends on theta and the step count alone while the bodies
    // run, and after the second barrier is left with the sums -> gradient -> step -> new table.  The sample waves go straight from
    // the second barrier to the next first one.  Every set of normals is drawn while the bodies run (see the draw loop below).
#if SPEC_DRAW_WAVE && defined(SPEC_WITH_DRAW_OWNERS) && !SPEC_EXCHANGE
#define SPEC_DRAW_OWNERS 1
    const uint32_t own_wave = WSN + ((1u - WSN) & 3u);        // the first draw wave on the owners' SIMD (wave & 3 == 1)
#else
#define SPEC_DRAW_OWNERS 0
#endif
// The lean chain (SPEC_LEAN_CHAIN, a define of the generated source): behind the second barrier the owners' wave is the
// iteration, so it does there only what the next table needs — the argument words are loaded beside the bodies and kept, the
// LDS rows are requested in one batch, and the loss bookkeeping (a full-precision division, the stores) follows the table.
// Programs with a two-entry parameter keep the epilogue as it was.
#if SPEC_DRAW_OWNERS && defined(SPEC_LEAN_CHAIN) && !defined(SPEC_DEBUG_NO_LEAN_CHAIN) && SPEC_OWN_ENTRIES == 1
#define SPEC_LEAN_OWNERS 1
#else
#define SPEC_LEAN_OWNERS 0
#endif
// The tail of the lean chain (SPEC_LEAN_TAIL, a define of the generated source): two arrangements of the lean owners' loop,
// each with a switch of its own for measurements (BSVI_SPEC_DEFINES)
//   SPEC_DEFER_BOOK    what follows the table store — the loss division, the curve and flag stores — waits in two registers
//                      and is done beside the NEXT iteration's bodies; the launch's last iteration does it at once
//   SPEC_PLAIN_SGD     SGD without momentum, weight decay or maximize (launch-uniform, decided beside the bodies) is one
//                      multiply-add on theta and the step count: its own scalar branch, not optimizer_apply's dispatch
#if SPEC_LEAN_OWNERS && defined(SPEC_LEAN_TAIL) && !defined(SPEC_DEBUG_NO_DEFER_BOOK)
#define SPEC_DEFER_BOOK 1
#else
#define SPEC_DEFER_BOOK 0
#endif
#if SPEC_LEAN_OWNERS && defined(SPEC_LEAN_TAIL) && !defined(SPEC_DEBUG_NO_PLAIN_SGD)
#define SPEC_PLAIN_SGD 1
#else
#define SPEC_PLAIN_SGD 0
#endif
// The optimizer as a literal (SPEC_OPT_LITERAL, a define the LAUNCH puts in front of the variant's source: specialize.cpp,
// opt_literal): the kind and the on/off options cannot change inside a launch, so a code object of its own has them as
// constants — the other kinds' arms are not compiled, nothing is dispatched and no arm's registers are merged.  The arithmetic
// is the same functions on a configuration whose launch-invariant words are constants; learning rate, betas and eps stay data.
//   0 (or not defined)  generic: every kind, dispatched on cfg
//   1                   SGD without momentum, weight decay, maximize or nesterov
//   2                   Adam without amsgrad, weight decay or maximize
#if defined(SPEC_OPT_LITERAL) && (SPEC_OPT_LITERAL < 0 || SPEC_OPT_LITERAL > 2)
#error "SPEC_OPT_LITERAL: 0, 1 and 2 exist"
#endif
#if SPEC_LEAN_OWNERS && defined(SPEC_OPT_LITERAL) && SPEC_OPT_LITERAL == 1
#define SPEC_OPT_FIX(c) do { (c).kind = BSVI_OPT_SGD; (c).momentum = 0.0f; (c).weight_decay = 0.0f; (c).nesterov = 0u; (c).maximize = 0u; } while (0)
#elif SPEC_LEAN_OWNERS && defined(SPEC_OPT_LITERAL) && SPEC_OPT_LITERAL == 2
#define SPEC_OPT_FIX(c) do { (c).kind = BSVI_OPT_ADAM; (c).weight_decay = 0.0f; (c).amsgrad = 0u; (c).maximize = 0u; } while (0)
#else      // (generic; a kernel without the lean owners' loop has no literal form: the define changes nothing there)
#define SPEC_OPT_FIX(c) do { } while (0)
#endif
#if defined(SPEC_TAIL_MUST_BE_OFF) && (SPEC_DEFER_BOOK || SPEC_PLAIN_SGD)
#error "the tail's arrangements are compiled into a kernel that keeps the previous epilogue"
#endif
#if SPEC_DRAW_OWNERS
    const uint32_t own_base = own_wave * 64u;
#else
    const uint32_t own_base = has_draw_wave ? fed_index * 64u
                            : (!SPEC_GENERIC_OWNERS && SPEC_OWNER_WAVE * 64u + SPEC_N_PARAMS <= nthreads) ? SPEC_OWNER_WAVE * 64u : 0u;
#endif
    const uint32_t oid = tid - own_base;                      // the parameter this thread owns (if < SPEC_N_PARAMS)
    bool own_fast = false;
#if SPEC_DRAW_OWNERS
    SpecOwn own = {};                                         // (the owners' registers: never written to LDS)
#endif
    if (oid < SPEC_N_PARAMS) {
        const uint32_t j0 = TAB[SPEC_TAB_PTR + oid], j1 = TAB[SPEC_TAB_PTR + oid + 1];
        if (j1 - j0 <= 2u) {
            own_fast = true;
#if !SPEC_DRAW_OWNERS
            SpecOwn own;
#endif
            own.n = j1 - j0;
            own.mask = 0;
            own.theta = PS[oid];
            own.s0 = own.s1 = own.s2 = own.st = 0.0f;
            own.p1 = own.p2 = 1.0;
            own.a[0] = own.a[1] = own.b[0] = own.b[1] = 0.0f;
            own.pos[0] = own.pos[1] = own.k[0] = own.k[1] = own.tr[0] = own.tr[1] = 0;
            if (step) {
                own.s0 = PS[SPEC_NP_PAD + oid]; own.s1 = PS[2 * SPEC_NP_PAD + oid];
                own.s2 = PS[3 * SPEC_NP_PAD + oid]; own.st = PS[4 * SPEC_NP_PAD + oid];
                own.mask = TAB[SPEC_TAB_MASK + oid];
                const bsvi_opt_cfg cfg0 = SPEC_A->cfg;       // once per launch: the running products start at beta^st
                if (own.st != 0.0f) {                        // (the kinds with a beta^step factor: Adam, AdamW; Adamax beta1 only)
                    if (optimizer_has_p1(cfg0.kind)) own.p1 = pow((double)cfg0.beta1, (double)own.st);
                    if (optimizer_has_p2(cfg0.kind)) own.p2 = pow((double)cfg0.beta2, (double)own.st);
                }
            }
#pragma unroll
            for (uint32_t e = 0; e < SPEC_OWN_ENTRIES; ++e) {
                if (e < own.n) {
                    const uint32_t k = TAB[SPEC_TAB_IDX + j0 + e];
                    own.pos[e] = TAB[SPEC_TAB_POS + j0 + e];
                    own.k[e] = SPEC_HOME(k);
                    own.tr[e] = TAB[4 * k + 1] & 0xFFu;
                    own.a[e] = __uint_as_float(TAB[4 * k + 2]);
                    own.b[e] = __uint_as_float(TAB[4 * k + 3]);
                }
            }
#if !SPEC_DRAW_OWNERS
            spec_own_store(OWN + 5 * oid, own);
#endif
        }
    }

    // ---- what the iterations read of the argument block, once: a scalar load per iteration and phase is a round trip
    //      to the scalar cache on the critical path of a ~5 us iteration
    SPEC_RELOAD_ARGS();
    SpecBody B0;
    B0.n_local = SPEC_A->n_local;
    B0.seed_lo = SPEC_A->seed_lo;
    B0.seed_hi = SPEC_A->seed_hi;
#if SPEC_DIAG
    B0.noise = SPEC_A->noise;
    B0.samples_out = SPEC_A->samples_out;
    B0.noise_out = SPEC_A->noise_out;
    B0.fvalue_out = SPEC_A->fvalue_out;
    B0.f_weight = SPEC_A->f_weight;
    B0.q_weight = SPEC_A->q_weight;
#else
    B0.noise = nullptr; B0.samples_out = nullptr; B0.noise_out = nullptr; B0.fvalue_out = nullptr;
    B0.f_weight = nullptr; B0.q_weight = nullptr;
#endif
    unsigned long long off0 = ((unsigned long long)SPEC_A->offset_hi << 32) | SPEC_A->offset_lo;
    if (const unsigned long long* const offset_dev = SPEC_A->offset_dev) off0 += *offset_dev;
    const uint32_t n_global = SPEC_A->n_global;
    const uint32_t pretraining = SPEC_A->pretraining_iterations;
#if SPEC_MB
    // ---- the gather phase.  Source s rewrites its stretch obs[o : o + B * r] of the LDS observation table with the rows
    //      dataset_s[minibatch_index(key_s, offset, b)][0 .. r) — ONE wave does it, lane l the rows b = l, l + 64, ...: the row's
    //      index once per key group (sources that share a RandomIndices variable share the walk), then r floats per source, held
    //      in SPEC_MB_REGS registers between `mb_fetch` (index walk + global loads: issued beside the bodies where the wave has
    //      no body of its own) and `mb_store` (the LDS stores).  The bodies read the stretch between an iteration's first and
    //      second barrier, so the stores lie between the second barrier and the next first one — no race, by construction.
    //      Every geometry number is a literal of the generated source (SPEC_MB_SOURCES), the offsets of the body stay literals.
    struct SpecGather { float v[SPEC_MB_REGS]; };
    const uint32_t mb_seed_lo = B0.seed_lo, mb_seed_hi = B0.seed_hi;
    auto mb_fetch = [&](unsigned long long offn, SpecGather& Gv) {
        SPEC_RELOAD_ARGS();
        const uint32_t olo = (uint32_t)offn, ohi = (uint32_t)(offn >> 32);
#define SPEC_MB_INDEX(s, o, B, r, DS, g, leader, base) uint32_t idx_##s[SPEC_MB_MAXQ] = {}; (void)idx_##s;
        SPEC_MB_SOURCES(SPEC_MB_INDEX)
#undef SPEC_MB_INDEX
#define SPEC_MB_FETCH(s, o, B, r, DS, g, leader, base)                                                              \
        {                                                                                                           \
            const float* const data = SPEC_A->mb_data[s];                                                           \
            uint32_t klo, khi;                                                                                      \
            minibatch_group_key(mb_seed_lo, mb_seed_hi, g, klo, khi);                                               \
            _Pragma("unroll") for (uint32_t q = 0; q < ((B) + 63u) / 64u; ++q) {                                    \
                const uint32_t b = lane + 64u * q;                                                                  \
                if ((leader) == (s)) idx_##s[q] = b < (B) ? minibatch_index_keyed(DS, klo, khi, olo, ohi, b) : 0u;  \
                const float* const row = data + (size_t)idx_##leader[q] * (r);                                      \
                _Pragma("unroll") for (uint32_t e = 0; e < (r); ++e) Gv.v[(base) + q * (r) + e] = b < (B) ? row[e] : 0.0f; \
            }                                                                                                       \
        }
        SPEC_MB_SOURCES(SPEC_MB_FETCH)
#undef SPEC_MB_FETCH
    };
    auto mb_store = [&](const SpecGather& Gv) {
#define SPEC_MB_STORE(s, o, B, r, DS, g, leader, base)                                                              \
        _Pragma("unroll") for (uint32_t q = 0; q < ((B) + 63u) / 64u; ++q) {                                        \
            const uint32_t b = lane + 64u * q;                                                                      \
            if (b < (B)) {                                                                                          \
                _Pragma("unroll") for (uint32_t e = 0; e < (r); ++e) spec_lds[SPEC_OBS0 + (o) + b * (r) + e] = Gv.v[(base) + q * (r) + e]; \
            }                                                                                                       \
        }
        SPEC_MB_SOURCES(SPEC_MB_STORE)
#undef SPEC_MB_STORE
    };
    // Who gathers (wave-uniform).  The draw service: its last draw wave that is not on the owners' SIMD (wave & 3 == 1) — beside
    // the bodies it draws one or two sets of normals and waits.  A single draw wave: that wave, idle beside the bodies.  No draw
    // wave (the plain loop, several workgroups): the last wave that is not the owners', behind the second barrier, beside the
    // owners' epilogue — every workgroup of a many-workgroup launch its own copy (the rows are a function of the key alone).
    const bool mb_loop = mode == SPEC_MODE_LOOP;
#if SPEC_DRAW_WAVE
    const uint32_t mb_service_wave = ((W - 1u) & 3u) != 1u ? W - 1u : W - 2u;
    const bool mb_in_service = draw_service;
#else
    const uint32_t mb_service_wave = 0u;
    const bool mb_in_service = false;
#endif
    const uint32_t mb_plain_wave = (W - 1u) != (own_base >> 6) ? W - 1u : (W > 1u ? W - 2u : 0u);
    const uint32_t mb_wave = mb_in_service ? mb_service_wave : has_draw_wave ? W - 1u : mb_plain_wave;
    const bool mb_gatherer = __builtin_amdgcn_readfirstlane((mb_loop && wave == mb_wave) ? 1 : 0) != 0;
    const bool mb_beside_bodies = has_draw_wave;      // (the gathering wave carries no samples: it fetches in front of the second barrier)
    // iteration 0's rows: behind the prologue's barrier (the whole observation table is in LDS), in front of the first barrier
    if (mb_gatherer) {
        SpecGather G0;
        mb_fetch(off0, G0);
        mb_store(G0);
    }
#endif
    // several workgroups in loop mode (the many-workgroup geometry only: the one-workgroup kernels are never launched with
    // more, and the extra live scalars cost BASELINE config 1's kernel 30 more spilled scalar registers).  The arrival ticket
    // and the generation number of the launch are ZERO when it starts (the host clears both words on the launch's stream,
    // specialize.cpp): iteration `it` is released as generation it + 1, and SPEC_GEN_OVER says "this launch is over" — a
    // workgroup that only becomes resident after workgroup 0 gave up on it leaves without touching the ticket.
#if SPEC_ACCUMULATE_CHUNKS
#define SPEC_LOOP_MANY 1
#define SPEC_GEN_OVER 0x7fff0000u
    const unsigned int gen0 = 0;
    if (G > 1 && mode == SPEC_MODE_LOOP && blockIdx.x != 0 &&
        __hip_atomic_load(SPEC_A->ticket + 64, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= SPEC_GEN_OVER) return;
#else
#define SPEC_LOOP_MANY 0
#endif
#if SPEC_EXCHANGE
    // (this rank's call count lives in its region and is touched by this rank's kernels only: stream order makes it current)
    uint32_t xseq0 = 0;
    if (const SpecExchange* const xg0 = SPEC_A->xchg) xseq0 = reinterpret_cast<const uint32_t*>(xg0->peer[xg0->rank])[XCHG_CALLS_WORD + 1];
#endif

#if defined(SPEC_DEBUG_STAMPS)        // timing experiment (tools/spec_stamps.py): s_memtime at the phase boundaries of one iteration
    unsigned long long stamp[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#define SPEC_STAMP(i) if (it == n_it / 2) stamp[i] = __builtin_amdgcn_s_memtime()
    // per wave, whatever its role (tools/spec_role_stamps.py): 0 past the first barrier, 1 at the second, 2 past it, 3 the owners'
    // sums read, 4 the iteration's work done, 5 past the NEXT first barrier; written by lane 0 of every wave at the end
    // (6: the owners' new table published — lean chain: what is left behind it is bookkeeping)
    unsigned long long rstamp[7] = {0, 0, 0, 0, 0, 0, 0};
#define SPEC_RSTAMP(i) if (it == n_it / 2) rstamp[i] = __builtin_amdgcn_s_memtime()
#define SPEC_RSTAMP_NEXT() if (it == n_it / 2 + 1u) rstamp[5] = __builtin_amdgcn_s_memtime(); else if (it == 0u) stamp_first = __builtin_amdgcn_s_memtime()
    unsigned long long stamp_first = 0;     // (7: the launch's first barrier passed, counted from the kernel's entry)
#define SPEC_RSTAMP_WRITE()                                                                                              \
    if (lane == 0u && SPEC_A->loss_slot && n_it > 16u + 8u * SPEC_MAX_WAVES) {                                           \
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                                                 \
        for (int i = 1; i < 7; ++i) SPEC_A->loss_slot[16u + 8u * wave + i] = rstamp[i] ? (float)(rstamp[i] - rstamp[0]) : 0.0f; \
        SPEC_A->loss_slot[16u + 8u * wave + 7] = (float)(stamp_first - stamp_entry);                                     \
        SPEC_A->loss_slot[16u + 8u * wave] = 1.0f;                                                                       \
    }
#else
#define SPEC_STAMP(i)
#define SPEC_RSTAMP(i)
#define SPEC_RSTAMP_NEXT()
#define SPEC_RSTAMP_WRITE()
#endif
    // One workgroup, noise kept in registers, lean build: the NEXT iteration's standard normals do not depend on anything
    // this iteration computes, and most waves have idle time right after their body — N = 300 is five waves on four SIMDs,
    // the hardware favours the older wave of a SIMD, so waves 0-3 wait at the barrier below for wave 4 — so the first wave
    // of each SIMD draws its next noise THERE.  What is left after the barrier is the owners' epilogue (threads of wave 0)
    // with only the late waves' draws beside it, instead of the epilogue followed by wave 0's own draw.
#if SPEC_KEEP_NOISE && !SPEC_DIAG && !SPEC_ACCUMULATE_CHUNKS && !defined(SPEC_DEBUG_NO_DRAW) && !defined(SPEC_NO_EARLY_DRAW)
#define SPEC_EARLY_DRAW 1
    SpecNoise Z;                       // lives across iterations: the early draw overwrites it once the body is done with it
    bool noise_ready = false;
#else
#define SPEC_EARLY_DRAW 0
#endif
#if SPEC_DRAW_WAVE
    if (draw_service && draw_wave) {
        // The service's draw waves run a loop of their OWN with the main loop's two barriers per iteration (a set drawn beside the
        // bodies would otherwise be live across spec_body in the register allocation of EVERY wave: 15 spilled registers and
        // 4.7 -> 6.5 us per iteration for every user of this kernel variant).  Their rows of the sums stay zero.
        if (lane == 0u) { RED[8 + 2 * wave] = 0.0f; RED[9 + 2 * wave] = 0.0f; }
        const uint32_t n_draw = W - WSN, k = wave - WSN;
        const uint32_t first = k;                              // (k < WSN or nothing: `has_first`)
        uint32_t before = 0;                                   // draw waves in front of this one that take a second set
        for (uint32_t j = 0; j < k; ++j) before += (((WSN + j) & 3u) != 1u) ? 1u : 0u;
        const uint32_t second = n_draw + before;
        const bool has_first = first < WSN, has_second = (wave & 3u) != 1u && second < WSN;      // (wave & 3 == 1: the owners' SIMD)
        auto draw_for = [&](uint32_t target, unsigned long long offn, SpecNoise& Zd) {
            SpecLane Tn = T;
            Tn.n = target * 64u + lane;
            Tn.active = Tn.n < B0.n_local;
            Tn.nc = Tn.active ? Tn.n : (B0.n_local - 1u);
            Tn.nidx = sample_base + Tn.nc;
            Tn.off_lo = (uint32_t)offn;
            Tn.off_hi = (uint32_t)(offn >> 32);
            Tn.vz = T.vz;
            spec_draw(B0, Tn, Zd);
        };
#if SPEC_DRAW_OWNERS
        (void)has_first; (void)has_second;
        // Whole sets, all drawn while the bodies run (tools/spec_role_stamps.py: a set of 21 rows is ~3 000 cycles of a draw
        // wave, the bodies ~6 500): the owners' wave draws set 0 in front of its epilogue work and stores it at once, into the
        // buffer of the iteration's parity (set 0 has two, the second behind the WSN sets: sample wave 0 reads the other one
        // meanwhile), so nothing of the draws is left on the owners' chain; the other draw waves share the remaining sets
        // evenly (five sample waves: 1, 2 | 3, 4; four: one each), keep them in registers and store them behind the second
        // barrier, beside the owners' epilogue.
        const uint32_t kown = own_wave - WSN, n_other = n_draw - 1u, rest = WSN - 1u;
        const uint32_t j = k < kown ? k : k - 1u, per = rest / n_other, extra = rest % n_other;
        const uint32_t set_a = __builtin_amdgcn_readfirstlane(1u + j * per + (j < extra ? j : extra));
        const uint32_t n_sets = __builtin_amdgcn_readfirstlane(per + (j < extra ? 1u : 0u));     // (<= 2: rest <= 4, n_other >= 2)
        const bool owners = __builtin_amdgcn_readfirstlane(wave == own_wave ? 1 : 0) != 0;     // (wave-uniform: the branches below are scalar)
        const float own_scale = -1.0f / (float)n_global;       // (the loop mode always steps)
        (void)own_scale;
#if SPEC_LEAN_OWNERS
        // (the lean epilogue adds the rows of all SPEC_MAX_WAVES waves: the host launches the service with a full workgroup only)
        if (W != SPEC_MAX_WAVES) __builtin_trap();
#endif
#if SPEC_DEFER_BOOK
        float book_vs = 0.0f, book_finite = 0.0f;             // the last iteration's loss sum and flag, until they are written
#endif
        for (uint32_t it = 0; it < n_it; ++it) {
            const bool more = it + 1u < n_it, last = !more;
            spec_lds_barrier();                                // (the main loop's first barrier: the sample waves read their buffers behind it)
            SPEC_RSTAMP(0);
            SPEC_RSTAMP_NEXT();
#if SPEC_MB
            SpecGather Gn;
            if (mb_gatherer && more) mb_fetch(off0 + it + 1u, Gn);      // (the loads fly while the sets are drawn)
#endif
            SpecNoise Za, Zb;
            float fac[2] = {0.0f, 0.0f};
            AdamBias bias = {1.0, 1.0, 0.0f, 0.0f};
            if (owners) {
                // ---- beside the bodies: what depends on this iteration's theta and the step count only, then set 0
                SPEC_RELOAD_ARGS();
                bsvi_opt_cfg cfg = SPEC_A->cfg;
                SPEC_OPT_FIX(cfg);
#pragma unroll
                for (uint32_t e = 0; e < SPEC_OWN_ENTRIES; ++e) fac[e] = own.b[e] * spec_utransform_grad(own.tr[e], own.theta);
                if (cfg.kind == BSVI_OPT_ADAM) bias = optimizer_adam_bias(cfg, own.p1, own.p2);     // (kept when the step is taken)
                else if (cfg.kind > BSVI_OPT_ADAM) bias = optimizer_more_bias(cfg, own.p1, own.p2, own.st);
                if (more) {
                    draw_for(0u, off0 + it + 1u, Za);
                    float* const buf = NZB + (((it + 1u) & 1u) ? WSN * (SPEC_KEEP_NOISE * 64u) : 0u);
#pragma unroll
                    for (uint32_t r = 0; r < SPEC_KEEP_NOISE; ++r) buf[64u * r] = Za.z[r];
                }
            } else if (more) {
                draw_for(set_a, off0 + it + 1u, Za);          // in registers
                if (n_sets > 1u) draw_for(set_a + 1u, off0 + it + 1u, Zb);
            }
#if SPEC_LEAN_OWNERS
            // The epilogue's words of the argument block, loaded HERE (behind the draw: they are not live across its key
            // schedule) and kept in scalar registers across the barrier — a scalar load behind it is a round trip to the
            // scalar cache in front of the LDS reads, which wait on the same counter.  This loop has no spec_body, which is
            // what the main loop re-reads them for.  (Through an empty statement: the loads cannot sink to their uses.)
            //  The pointers as global-memory pointers: behind the empty statement the compiler no longer knows where they came
            //  from, and a store through a generic pointer also counts on the LDS counter the next barrier waits for.)
            typedef SPEC_GLOBAL_AS float* spec_gptr;
            spec_gptr e_out = nullptr, e_loss = nullptr, e_finite = nullptr, e_params = nullptr, e_state = nullptr;
            bsvi_opt_cfg e_cfg = {};
#if SPEC_PLAIN_SGD
            bool plain_sgd = false;
#endif
            if (owners) {
                SPEC_RELOAD_ARGS();
                e_out = (spec_gptr)SPEC_A->out; e_loss = (spec_gptr)SPEC_A->loss_slot; e_finite = (spec_gptr)SPEC_A->finite_slot;
                e_params = (spec_gptr)SPEC_A->params; e_state = (spec_gptr)SPEC_A->state;
                e_cfg = SPEC_A->cfg;
#if defined(__HIP_DEVICE_COMPILE__)
                asm volatile("" : "+s"(e_out), "+s"(e_loss), "+s"(e_finite), "+s"(e_params), "+s"(e_state));
                asm volatile("" : "+s"(e_cfg.kind), "+s"(e_cfg.lr), "+s"(e_cfg.momentum), "+s"(e_cfg.dampening), "+s"(e_cfg.weight_decay),
                             "+s"(e_cfg.nesterov), "+s"(e_cfg.beta1), "+s"(e_cfg.beta2), "+s"(e_cfg.eps), "+s"(e_cfg.amsgrad), "+s"(e_cfg.maximize));
#endif
                SPEC_OPT_FIX(e_cfg);
#if SPEC_PLAIN_SGD
                plain_sgd = __builtin_amdgcn_readfirstlane((e_cfg.kind == BSVI_OPT_SGD && e_cfg.momentum == 0.0f && e_cfg.weight_decay == 0.0f
                                                            && !e_cfg.maximize) ? 1 : 0) != 0;
#endif
#if SPEC_DEFER_BOOK
                // ---- the bookkeeping of the iteration before, beside this one's bodies (the pointers have just arrived)
                if (it > 0u && oid == 0u) {
                    const float loss = -book_vs / (float)n_global;
                    if (e_loss) e_loss[it - 1u] = loss;
                    if (e_finite) e_finite[it - 1u] = book_finite;
                }
#endif
            }
#endif
            SPEC_RSTAMP(1);
            spec_lds_barrier();                                // (the second: every wave's sums are in WS / RED, the buffers are free)
            SPEC_RSTAMP(2);
#if SPEC_MB
            if (mb_gatherer && more) mb_store(Gn);
#endif
#if SPEC_LEAN_OWNERS
            if (owners) {
                // ---- the owners' epilogue, lean: every LDS word it needs requested in one batch — the waves' loss rows and
                //      the position's rows (literal addresses; the service fills the workgroup, W == SPEC_MAX_WAVES, checked at
                //      the top of this loop: every row is a wave's, none is read and not selected) — then sums (waves in order)
                //      -> gradient -> step -> the new table, and only then the bookkeeping.  One entry per parameter.
                float ra[SPEC_MAX_WAVES], rb[SPEC_MAX_WAVES], rp[SPEC_MAX_WAVES];
                spec_f4 rq[SPEC_MAX_WAVES / 2];               // (RED + 8: value and non-finite count per wave, two waves per 16 bytes)
#pragma unroll
                for (uint32_t q = 0; q < SPEC_MAX_WAVES / 2; ++q) rq[q] = reinterpret_cast<const spec_f4*>(RED + 8)[q];
#pragma unroll
                for (uint32_t w = 0; w < SPEC_MAX_WAVES; ++w) rp[w] = WS[w * SPEC_WS_PAD + own.pos[0]];
                // (one statement that needs them all: every read is issued in front of it and waited for once — left to itself
                //  the compiler sinks the position rows into the branch below and waits for each pair of them in turn)
#if defined(__HIP_DEVICE_COMPILE__) && SPEC_MAX_WAVES == 8
#define SPEC_PIN8(a) "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]), "+v"(a[5]), "+v"(a[6]), "+v"(a[7])
                asm volatile("" : "+v"(rq[0]), "+v"(rq[1]), "+v"(rq[2]), "+v"(rq[3]), SPEC_PIN8(rp));
#undef SPEC_PIN8
#endif
#pragma unroll
                for (uint32_t w = 0; w < SPEC_MAX_WAVES; ++w) {
                    ra[w] = (w & 1u) ? rq[w / 2].z : rq[w / 2].x;
                    rb[w] = (w & 1u) ? rq[w / 2].w : rq[w / 2].y;
                }
                const float tot = spec_rows_total(rp);
                const float vs = spec_rows_total(ra);
                const float finite = isfinite(vs) ? 1.0f : 0.0f;       // (all the step needs of the loss)
                const uint32_t mask_bit = it <= pretraining ? 2u : 1u;
                float grad = 0.0f;
                if (own_fast) {
                    float gsum = 0.0f;
                    const float term = tot * fac[0];
                    gsum += own.n > 0u ? term : 0.0f;
                    grad = gsum * own_scale;
                    SPEC_RSTAMP(3);
#if SPEC_PLAIN_SGD
                    if (plain_sgd) {                           // (optimizer_apply's SGD branch with its options off)
                        if (finite != 0.0f && (own.mask & mask_bit)) {
                            own.st = own.st + 1.0f;
                            own.theta = own.theta - e_cfg.lr * grad;
                        }
                    } else
#endif
                    if (finite != 0.0f && (own.mask & mask_bit)) {
                        if (e_cfg.kind == BSVI_OPT_SGD) {
                            optimizer_apply(e_cfg, own.theta, own.s0, own.s1, own.s2, own.st, grad);
                        } else if (e_cfg.kind == BSVI_OPT_ADAM) {
                            optimizer_apply_adam_biased(e_cfg, own.theta, own.s0, own.s1, own.s2, own.st, grad, bias);
                            own.p1 = bias.p1;
                            own.p2 = bias.p2;
                        } else {                               // AdamW, RMSprop, Adagrad, Adamax: a scalar branch of their own
                            optimizer_apply_more(e_cfg, own.theta, own.s0, own.s1, own.s2, own.st, grad, bias);
                            own.p1 = bias.p1;
                            own.p2 = bias.p2;
                        }
                    }
                    if (more) {
                        const float g0 = utransform_common(own.tr[0], own.theta);
                        if (own.n > 0u) spec_store_uniform(own.k[0], own.a[0] + own.b[0] * g0);
                    }
                }
                asm volatile("" ::: "memory");                 // (the table's stores stay in front of the bookkeeping's)
                SPEC_RSTAMP(6);
                // ---- behind the table: the loss (a full-precision division), the curve, the launch's output block
#if SPEC_DEFER_BOOK
                book_vs = vs; book_finite = finite;
                if (more) { SPEC_RSTAMP(4); continue; }        // (written beside the next bodies, above)
#endif
                const float loss = -vs / (float)n_global;
                if (oid == 0u) {
                    const float vb = spec_rows_total(rb);
                    if (last) { e_out[0] = vs; e_out[1] = vb; e_out[2] = loss; e_out[3] = finite; }
                    if (e_loss) e_loss[it] = loss;
                    if (e_finite) e_finite[it] = finite;
                }
                if (own_fast && last) {
                    e_out[BSVI_OUT_HEADER + oid] = grad;
                    e_params[oid] = own.theta;
                    if (e_state) {
                        e_state[oid] = own.s0;
                        e_state[(size_t)SPEC_N_PARAMS + oid] = own.s1;
                        e_state[2 * (size_t)SPEC_N_PARAMS + oid] = own.s2;
                        e_state[3 * (size_t)SPEC_N_PARAMS + oid] = own.st;
                    }
                }
            } else if (more) {
#pragma unroll
                for (uint32_t r = 0; r < SPEC_KEEP_NOISE; ++r) NZB[set_a * (SPEC_KEEP_NOISE * 64u) + 64u * r] = Za.z[r];
                if (n_sets > 1u) {
#pragma unroll
                    for (uint32_t r = 0; r < SPEC_KEEP_NOISE; ++r) NZB[(set_a + 1u) * (SPEC_KEEP_NOISE * 64u) + 64u * r] = Zb.z[r];
                }
            }
#else
            if (owners) {
                // ---- the owners' epilogue (as the main loop's below, on registers): the loss rows and both positions' rows
                //      requested together, gradient, step, the new table
                SPEC_RELOAD_ARGS();
                float* const out = SPEC_A->out;
                float* const loss_slot = SPEC_A->loss_slot;
                float* const finite_slot = SPEC_A->finite_slot;
                const bsvi_opt_cfg cfg = SPEC_A->cfg;
                float vs = 0.0f, vb = 0.0f;
#pragma unroll
                for (uint32_t w = 0; w < SPEC_MAX_WAVES; ++w) {
                    const float a = RED[8 + 2 * w], b = RED[9 + 2 * w];
                    vs += w < W ? a : 0.0f;
                    vb += w < W ? b : 0.0f;
                }
                float tot[2];
#pragma unroll
                for (uint32_t e = 0; e < SPEC_OWN_ENTRIES; ++e) tot[e] = spec_pos_total(WS, own.pos[e], W);
                const float finite = isfinite(vs) ? 1.0f : 0.0f;
                const float loss = -vs / (float)n_global;
                if (oid == 0u) {
                    if (last) { out[0] = vs; out[1] = vb; out[2] = loss; out[3] = finite; }
                    if (loss_slot) loss_slot[it] = loss;
                    if (finite_slot) finite_slot[it] = finite;
                }
                const float scale = -1.0f / (float)n_global;   // (the loop mode always steps)
                const uint32_t mask_bit = it <= pretraining ? 2u : 1u;
                if (own_fast) {
                    float gsum = 0.0f;
#pragma unroll
                    for (uint32_t e = 0; e < SPEC_OWN_ENTRIES; ++e) {
                        const float term = tot[e] * fac[e];
                        gsum += e < own.n ? term : 0.0f;
                    }
                    const float grad = gsum * scale;
                    SPEC_RSTAMP(3);
                    if (last) out[BSVI_OUT_HEADER + oid] = grad;
                    if (finite != 0.0f && (own.mask & mask_bit)) {
                        if (cfg.kind == BSVI_OPT_SGD) {
                            optimizer_apply(cfg, own.theta, own.s0, own.s1, own.s2, own.st, grad);
                        } else if (cfg.kind == BSVI_OPT_ADAM) {
                            optimizer_apply_adam_biased(cfg, own.theta, own.s0, own.s1, own.s2, own.st, grad, bias);
                            own.p1 = bias.p1;
                            own.p2 = bias.p2;
                        } else {                               // AdamW, RMSprop, Adagrad, Adamax: a scalar branch of their own
                            optimizer_apply_more(cfg, own.theta, own.s0, own.s1, own.s2, own.st, grad, bias);
                            own.p1 = bias.p1;
                            own.p2 = bias.p2;
                        }
                    }
                    if (last) {
                        float* const params = SPEC_A->params;
                        float* const state = SPEC_A->state;
                        params[oid] = own.theta;
                        if (state) {
                            state[oid] = own.s0;
                            state[(size_t)SPEC_N_PARAMS + oid] = own.s1;
                            state[2 * (size_t)SPEC_N_PARAMS + oid] = own.s2;
                            state[3 * (size_t)SPEC_N_PARAMS + oid] = own.st;
                        }
                    } else {
                        // g(theta) once when both entries carry the same transform (the prior's scale entries reuse the
                        // posterior's parameter): the same function of the same value
                        const float g0 = utransform_common(own.tr[0], own.theta);
                        float g1 = g0;
                        if (own.n == 2u && own.tr[1] != own.tr[0]) g1 = utransform_common(own.tr[1], own.theta);
                        if (own.n > 0u) spec_store_uniform(own.k[0], own.a[0] + own.b[0] * g0);
                        if (own.n > 1u) spec_store_uniform(own.k[1], own.a[1] + own.b[1] * g1);
                    }
                }
            } else if (more) {
#pragma unroll
                for (uint32_t r = 0; r < SPEC_KEEP_NOISE; ++r) NZB[set_a * (SPEC_KEEP_NOISE * 64u) + 64u * r] = Za.z[r];
                if (n_sets > 1u) {
#pragma unroll
                    for (uint32_t r = 0; r < SPEC_KEEP_NOISE; ++r) NZB[(set_a + 1u) * (SPEC_KEEP_NOISE * 64u) + 64u * r] = Zb.z[r];
                }
            }
#endif
            SPEC_RSTAMP(4);
        }
        SPEC_RSTAMP_WRITE();
        return;
#else
        for (uint32_t it = 0; it < n_it; ++it) {
            const bool more = it + 1u < n_it;
            spec_lds_barrier();                                // (the main loop's first barrier: the sample waves read their buffers behind it)
            SPEC_RSTAMP(0);
            SPEC_RSTAMP_NEXT();
#if SPEC_MB
            SpecGather Gn;
            if (mb_gatherer && more) mb_fetch(off0 + it + 1u, Gn);      // (the loads fly while the set is drawn)
#endif
            SpecNoise Za;
            if (more && has_first) draw_for(first, off0 + it + 1u, Za);     // beside the bodies, in registers
            SPEC_RSTAMP(1);
            spec_lds_barrier();                                // (the second: the buffers are free)
            SPEC_RSTAMP(2);
#if SPEC_MB
            if (mb_gatherer && more) mb_store(Gn);
#endif
            if (more) {
                if (has_first) {
#pragma unroll
                    for (uint32_t r = 0; r < SPEC_KEEP_NOISE; ++r) NZB[first * (SPEC_KEEP_NOISE * 64u) + 64u * r] = Za.z[r];
                }
                if (has_second) {
                    SpecNoise Zb;
                    draw_for(second, off0 + it + 1u, Zb);
#pragma unroll
                    for (uint32_t r = 0; r < SPEC_KEEP_NOISE; ++r) NZB[second * (SPEC_KEEP_NOISE * 64u) + 64u * r] = Zb.z[r];
                }
            }
            SPEC_RSTAMP(4);
        }
        SPEC_RSTAMP_WRITE();
        return;
#endif
    }
#endif
    for (uint32_t it = 0; it < n_it; ++it) {
        SPEC_STAMP(0);
        // ---- one Monte-Carlo sample per lane and chunk (a workgroup of a large shard walks several chunks of samples, so
        //      that the launch's fixed costs — tables, prologue, the row of sums — are paid once per workgroup, not once
        //      per 256 samples).  The standard normals do not depend on the uniform table: the first chunk's are drawn
        //      ahead of the barrier that publishes it.
        float lane_value = 0.0f, lane_bad = 0.0f;
        for (uint32_t chunk = 0; chunk < n_chunks; ++chunk) {
            SpecBody B = B0;
#if SPEC_DIAG
            // a given-noise sequence is laid out [iteration][row][n_local]
            if (B.noise) B.noise += (size_t)it * SPEC_N_NOISE * B.n_local;
#endif
            T.n = (chunk * G + blockIdx.x) * nthreads + tid;
            T.active = T.n < B.n_local;
            T.nc = T.active ? T.n : (B.n_local - 1u);
            T.nidx = sample_base + T.nc;
            const unsigned long long off = off0 + it;
            T.f = 0.0f;
            T.lq = 0.0f;
#if SPEC_DIAG
            T.gw = B.f_weight ? B.f_weight[T.nc] : 1.0f;
#else
            T.gw = 1.0f;
#endif
            T.off_lo = (uint32_t)off;
            T.off_hi = (uint32_t)(off >> 32);
#if !SPEC_EARLY_DRAW
            SpecNoise Z;
#endif
#if defined(SPEC_DEBUG_NO_DRAW)                                // timing experiment (BSVI_SPEC_DEFINES): what the noise costs
            for (uint32_t r = 0; r < (SPEC_KEEP_NOISE ? SPEC_KEEP_NOISE : 1); ++r) Z.z[r] = 0.25f;
#elif SPEC_EARLY_DRAW
#if defined(SPEC_DEBUG_LATE_FREE)                              // timing experiment: what the late waves' own draw costs
            if (!noise_ready && (!((SPEC_DEBUG_LATE_FREE >> wave) & 1u) || it == 0u)) spec_draw(B, T, Z);   // mask of waves whose draws are skipped
#else
            if (!noise_ready && !draw_wave && !(fed_wave && it > 0u)) spec_draw(B, T, Z);
#endif
#else
            spec_draw(B, T, Z);
#endif
            SPEC_STAMP(1);
            if (chunk == 0) {
                spec_lds_barrier();                            // the uniform table of this iteration is complete ...
                SPEC_RSTAMP(0);
                SPEC_RSTAMP_NEXT();
#if SPEC_ACCUMULATE_CHUNKS
                for (uint32_t k = lane; k < SPEC_WS_CELLS; k += 64u) WSw[k] = 0.0f;     // ... and the last one's sums are consumed
#endif
            }
#if SPEC_DRAW_WAVE
            if (fed_wave && it > 0u) {                         // drawn by the draw wave beside the last epilogue
#if SPEC_DRAW_OWNERS
                const float* const nz = NZ + ((wave == 0u && (it & 1u)) ? WSN * (SPEC_KEEP_NOISE * 64u) : 0u);     // (set 0: two buffers)
#else
                const float* const nz = NZ;
#endif
#pragma unroll
                for (uint32_t r = 0; r < SPEC_KEEP_NOISE; ++r) Z.z[r] = nz[64u * r];
            }
#endif
            SPEC_STAMP(2);
#if !defined(SPEC_DEBUG_NO_BODY)
            if (!draw_wave) {
                spec_body(B, T, Z, WSw);
#if SPEC_TILE
                {
                    // the lanes of this wave with a sample of this chunk (the samples fill the lanes in order)
                    const uint32_t first = T.n - lane;
                    const uint32_t live = __builtin_amdgcn_readfirstlane(first < B.n_local ? (B.n_local - first < 64u ? B.n_local - first : 64u) : 0u);
                    spec_du_flush(spec_lds + SPEC_OFF_TR + wave * SPEC_TR_FLOATS, WSw, lane, live);
                }
#endif
            }
#endif
            SPEC_STAMP(3);
            const float value = (SPEC_ESTIMATOR == BSVI_EST_BLACKBOX) ? (T.lq * T.f + T.f) : T.f;
            lane_value += T.active ? value : 0.0f;
            lane_bad += (T.active && !isfinite(value)) ? 1.0f : 0.0f;
        }
        const float vsum = wave_sum(lane_value);
        const float bad = wave_sum(lane_bad);
        if (lane == 0) { RED[8 + 2 * wave] = vsum; RED[9 + 2 * wave] = bad; }
        SPEC_STAMP(4);
#if SPEC_EARLY_DRAW
        noise_ready = false;
#ifndef SPEC_EARLY_MASK
#define SPEC_EARLY_MASK (1u | (1u << SPEC_OWNER_WAVE))          // wave 0 (idle at the barrier) and the owners' wave (busy after it)
#endif
#if defined(SPEC_DEBUG_LATE_FREE)
        if (((SPEC_EARLY_MASK >> wave) & 1u) && !((SPEC_DEBUG_LATE_FREE >> wave) & 1u) && n_chunks == 1u && it + 1u < n_it) {
#else
        if (((SPEC_EARLY_MASK >> wave) & 1u) && !has_draw_wave && n_chunks == 1u && it + 1u < n_it) {
#endif
            const unsigned long long off = off0 + it + 1u;
            SpecLane Tn = T;
            Tn.off_lo = (uint32_t)off;
            Tn.off_hi = (uint32_t)(off >> 32);
            spec_draw(B0, Tn, Z);
            noise_ready = true;
        }
#endif
#if SPEC_MB && !SPEC_DRAW_OWNERS
        // the gather: a single draw wave fetches the next rows here, beside the bodies; without one the wave fetches behind the
        // barrier, beside the owners' epilogue (several workgroups: while thread 0 waits for the grid, below)
        SpecGather Gn;
        const bool mb_more = mb_gatherer && it + 1u < n_it;
        if (mb_more && mb_beside_bodies) mb_fetch(off0 + it + 1u, Gn);
#endif
        SPEC_RSTAMP(1);
        spec_lds_barrier();                                    // every wave's sums are in WS / RED
        SPEC_STAMP(5);
        SPEC_RSTAMP(2);
#if SPEC_MB && !SPEC_DRAW_OWNERS
        const bool mb_with_grid = SPEC_LOOP_MANY && G > 1 && mode == SPEC_MODE_LOOP;
        if (mb_more && !mb_with_grid) {
            if (!mb_beside_bodies) mb_fetch(off0 + it + 1u, Gn);
            mb_store(Gn);
        }
#endif
#if SPEC_DRAW_OWNERS
        SPEC_RSTAMP(4);
        continue;                                              // (the epilogue runs on the owners' draw wave)
#endif
#if SPEC_DRAW_WAVE
        if (draw_wave && it + 1u < n_it) {                     // (the owners' wave read the last set behind the barrier before the body)
            const unsigned long long off = off0 + it + 1u;
            SpecLane Tn = T;
            Tn.n = fed_index * 64u + lane;
            Tn.active = Tn.n < B0.n_local;
            Tn.nc = Tn.active ? Tn.n : (B0.n_local - 1u);
            Tn.nidx = sample_base + Tn.nc;
            Tn.off_lo = (uint32_t)off;
            Tn.off_hi = (uint32_t)(off >> 32);
            SpecNoise Zf;
            spec_draw(B0, Tn, Zf);
#pragma unroll
            for (uint32_t r = 0; r < SPEC_KEEP_NOISE; ++r) NZ[64u * r] = Zf.z[r];
        }
#endif

        // ---- several workgroups: every one publishes its row of sums, the last to arrive adds the rows in order
        uint32_t rows = W;                                     // rows of WS / RED that hold sums
        if (G > 1) {
            SPEC_RELOAD_ARGS();
            float* const partials = SPEC_A->partials;
            unsigned int* const ticket = SPEC_A->ticket;
            const uint32_t stride = 2u + SPEC_N_POS;
            float* mine = partials + (size_t)blockIdx.x * stride;
            for (uint32_t k = tid; k < SPEC_N_POS; k += nthreads) mine[2 + k] = spec_pos_total(WS, k, W);
            if (tid == 0) {
                float s = 0.0f, c = 0.0f;
                for (uint32_t w = 0; w < W; ++w) { s += RED[8 + 2 * w]; c += RED[9 + 2 * w]; }
                mine[0] = s;
                mine[1] = c;
            }
            __syncthreads();                                   // every wave's stores issued and drained
#if SPEC_LOOP_MANY
            if (mode == SPEC_MODE_LOOP) {
                // The loop of inference.py:95-108 over SEVERAL workgroups in one launch (round 4; before: one launch per
                // iteration, every workgroup staging the tables again — 70 x the algorithmic traffic at BASELINE config 2).
                // Workgroup 0 is the iteration's owner: it waits for the other G - 1 rows, adds them, runs the epilogue on ITS
                // copy of the parameters and the optimizer state, writes the new parameters to memory and releases the
                // iteration's generation number; the others wait for that number, read the parameters back and rebuild their
                // copy of the uniform table.  Generation numbers only grow (base read at the start of the launch), the waits
                // are bounded (a launch whose workgroups are not all resident must not hang: it ends with a NaN loss).
                unsigned int* const gen = ticket + 64;
                const unsigned int target = gen0 + it + 1u;
#if SPEC_MB && !SPEC_DRAW_OWNERS
                // every workgroup rebuilds its own copy of the minibatch stretches, while its thread 0 waits for the grid
                if (mb_more) { mb_fetch(off0 + it + 1u, Gn); mb_store(Gn); }
#endif
                if (blockIdx.x != 0) {
                    if (tid == 0) {
                        __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
                        const unsigned long long t0 = wall_clock64();
                        unsigned int seen;
                        bool over = false;
                        while ((int)((seen = __hip_atomic_load(gen, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT)) - target) < 0) {
                            if (wall_clock64() - t0 > 400000000ull) { over = true; break; }      // 4 s of the 100 MHz clock
                            __builtin_amdgcn_s_sleep(2);
                        }
                        // (workgroup 0 gave up on a workgroup and ended the launch, or this one waited in vain: leave — going on
                        //  would mean K more waits of four seconds)
                        RED[3] = (over || seen >= SPEC_GEN_OVER) ? 1.0f : 0.0f;
                    }
                    __syncthreads();
                    if (RED[3] != 0.0f) return;
                    if (it + 1u == n_it) return;
                    float* const params = SPEC_A->params;
                    for (uint32_t i = tid; i < SPEC_N_PARAMS; i += nthreads)
                        PS[i] = __hip_atomic_load(params + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __syncthreads();
                    const float* const consts = SPEC_A->consts;
                    (void)consts;
                    for (uint32_t k = tid; k < SPEC_N_UNIFORM; k += nthreads) {
                        const uint32_t src = TAB[4 * k], w1 = TAB[4 * k + 1];
                        if ((w1 >> 8) & 0xFFu) spec_publish_uniform(TAB, k, PS[src]);
                    }
                    continue;                                  // (the next iteration's first barrier publishes the table)
                }
                if (tid == 0) {
                    const unsigned long long t0 = wall_clock64();
                    bool late = false;
                    while (__hip_atomic_load(ticket, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) != G - 1u) {
                        if (wall_clock64() - t0 > 400000000ull) { late = true; break; }
                        __builtin_amdgcn_s_sleep(2);
                    }
                    RED[3] = late ? 1.0f : 0.0f;
                }
                __syncthreads();
                if (RED[3] != 0.0f) {
                    // A workgroup never arrived (not resident: a shared GPU, a CU mask, another stream's kernels).  The launch ends
                    // HERE: this and every remaining iteration get a NaN loss and no step (the parameters in memory are those of
                    // the last good iteration), the output block says so, and the generation number is set to "over" so that
                    // every waiting workgroup — and any that starts later — leaves at once.  (Round 4 went on to the next
                    // iteration and waited four seconds again: a K-iteration call took K x 4 s to fail.)
                    SPEC_RELOAD_ARGS();
                    float* const loss_slot = SPEC_A->loss_slot;
                    float* const finite_slot = SPEC_A->finite_slot;
                    float* const out = SPEC_A->out;
                    const float nanv = __int_as_float(0x7fc00000);
                    for (uint32_t k = it + tid; k < n_it; k += nthreads) {
                        if (loss_slot) loss_slot[k] = nanv;
                        if (finite_slot) finite_slot[k] = 0.0f;
                    }
                    if (tid == 0) {
                        out[0] = nanv; out[1] = 1.0f; out[2] = nanv; out[3] = 0.0f;
                        __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        __hip_atomic_store(gen, SPEC_GEN_OVER, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
                    }
                    return;
                }
            } else
#endif
            {
                if (tid == 0) {
                    const unsigned int t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
                    RED[2] = (t == G - 1u) ? 1.0f : 0.0f;
                }
                __syncthreads();
                if (RED[2] == 0.0f) return;
            }
            // column c of the G rows: four interleaved slices per column (G can be hundreds of workgroups), then the slices
            float* const SL = spec_lds + SPEC_OFF_SCR;
            for (uint32_t i = tid; i < 4u * stride; i += nthreads) {
                const uint32_t sl = i & 3u, c = i >> 2;
                // eight loads in flight, added in row order (the same association as one load at a time: with hundreds of
                // workgroups the one-at-a-time form made this the longest phase of the launch — a serial tail in ONE
                // workgroup of ~130 dependent L2 round trips while the rest of the chip was idle)
                float s = 0.0f;
                uint32_t b = sl;
                for (; b + 28u < G; b += 32u) {
                    float v[8];
#pragma unroll
                    for (uint32_t u = 0; u < 8u; ++u)
                        v[u] = __hip_atomic_load(&partials[(size_t)(b + 4u * u) * stride + c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
                    for (uint32_t u = 0; u < 8u; ++u) s += v[u];
                }
                for (; b < G; b += 4u)
                    s += __hip_atomic_load(&partials[(size_t)b * stride + c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                SL[i] = s;
            }
            __syncthreads();
            for (uint32_t c = tid; c < stride; c += nthreads) {
                const float s = (SL[4 * c] + SL[4 * c + 1]) + (SL[4 * c + 2] + SL[4 * c + 3]);
                if (c < 2u) {
                    RED[8 + c] = s;
                } else {                                       // the grid total in the first wave's cell of the position
                    WS[SPEC_WS_CELL(c - 2u)] = s;
#if !SPEC_TILE
                    WS[4u * (c - 2u) + 1u] = 0.0f; WS[4u * (c - 2u) + 2u] = 0.0f; WS[4u * (c - 2u) + 3u] = 0.0f;
#endif
                }
            }
            if (tid == 0) {
                __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            __syncthreads();
            rows = 1;
        }

        // ---- epilogue.  The thread that owns parameter i does everything that depends on it: adds the waves' sums of
        //      its uniform entries, applies the chain rule, the optimizer step on the LDS working copy, and publishes
        //      the entries' new values for the next iteration — so an iteration of the in-kernel loop has two
        //      barriers: after the body, and before the next one.
        // (the epilogue's own words of the argument block: requested here, they arrive while the LDS reads below are in flight)
        SPEC_RELOAD_ARGS();
        float* const out = SPEC_A->out;
        float* const loss_slot = SPEC_A->loss_slot;
        float* const finite_slot = SPEC_A->finite_slot;
        const bsvi_opt_cfg cfg = SPEC_A->cfg;
        // (literal trip counts and literal addresses — every row of RED exists, the rows of waves this launch does not have are
        //  read and not selected: the LDS reads are one base register + immediates and issue back to back)
        float vs = 0.0f, vb = 0.0f;
#pragma unroll
        for (uint32_t w = 0; w < SPEC_MAX_WAVES; ++w) {
            const float a = RED[8 + 2 * w], b = RED[9 + 2 * w];
            vs += w < rows ? a : 0.0f;
            vb += w < rows ? b : 0.0f;
        }
#if SPEC_EXCHANGE
        // several ranks: the owners' wave exchanges [loss sum, non-finite count, gradient sum per parameter] with its peers
        // (spec_exchange above); everything below runs on the TOTALS, as bsvi_finalize_step does behind the exchange kernel
        const SpecExchange* const xg = SPEC_A->xchg;
#if SPEC_GENERIC_OWNERS
        const bool xrun = xg != nullptr && mode == SPEC_MODE_LOOP;
        float xgsum = 0.0f;
        if (xrun) {                                            // per thread: see spec_xput / spec_xget
            const uint32_t xseq = xseq0 + it + 1u;
            if (tid == own_base) { spec_xput(xg, xseq, 0u, vs); spec_xput(xg, xseq, 1u, vb); }
            if (own_fast) {
                const SpecOwn own = spec_own_load(OWN + 5 * oid);
                float g = 0.0f;
#pragma unroll
                for (uint32_t e = 0; e < SPEC_OWN_ENTRIES; ++e) {
                    const float term = spec_pos_total(WS, own.pos[e], rows) * (own.b[e] * spec_utransform_grad(own.tr[e], own.theta));
                    g += e < own.n ? term : 0.0f;
                }
                spec_xput(xg, xseq, BSVI_OUT_HEADER + oid, g);
            }
            for (uint32_t i = tid; i < SPEC_N_PARAMS; i += nthreads) {
                if (i == oid && own_fast) continue;
                const float theta = PS[i];
                const uint32_t j0 = TAB[SPEC_TAB_PTR + i], j1 = TAB[SPEC_TAB_PTR + i + 1];
                float g = 0.0f;
                for (uint32_t j = j0; j < j1; ++j) {
                    const uint32_t pos = TAB[SPEC_TAB_POS + j], k = TAB[SPEC_TAB_IDX + j];
                    g += spec_pos_total(WS, pos, rows) * (__uint_as_float(TAB[4 * k + 3]) * spec_utransform_grad(TAB[4 * k + 1] & 0xFFu, theta));
                }
                spec_xput(xg, xseq, BSVI_OUT_HEADER + i, g);
            }
            bool ok = spec_xget(xg, xseq, 0u, vs);
            ok = spec_xget(xg, xseq, 1u, vb) && ok;
            if (own_fast) ok = spec_xget(xg, xseq, BSVI_OUT_HEADER + oid, xgsum) && ok;
            if (!ok) vs = __int_as_float(0x7fc00000);         // abandoned: NaN loss, no step
            if (tid == own_base && it + 1u == n_it) reinterpret_cast<uint32_t*>(xg->peer[xg->rank])[XCHG_CALLS_WORD + 1] = xseq0 + n_it;
        }
#else
        const bool xrun = xg != nullptr && mode == SPEC_MODE_LOOP && (tid >> 6) == (own_base >> 6);
        float xgsum = 0.0f;
        if (xrun) {
            if (own_fast) {
                const SpecOwn own = spec_own_load(OWN + 5 * oid);
                float tot[2];
#pragma unroll
                for (uint32_t e = 0; e < SPEC_OWN_ENTRIES; ++e) tot[e] = spec_pos_total(WS, own.pos[e], rows);
#pragma unroll
                for (uint32_t e = 0; e < SPEC_OWN_ENTRIES; ++e) {
                    const float term = tot[e] * (own.b[e] * spec_utransform_grad(own.tr[e], own.theta));
                    xgsum += e < own.n ? term : 0.0f;
                }
            }
            if (!spec_exchange(xg, xseq0 + it + 1u, oid, own_fast, vs, vb, xgsum)) vs = __int_as_float(0x7fc00000);     // abandoned: NaN loss, no step
            if (oid == 0u && it + 1u == n_it) reinterpret_cast<uint32_t*>(xg->peer[xg->rank])[XCHG_CALLS_WORD + 1] = xseq0 + n_it;
        }
#endif
#endif
        // -vs / n is finite exactly when vs is (n >= 1): the optimizer step does not wait for the division
        const float finite = isfinite(vs) ? 1.0f : 0.0f;
        const float loss = -vs / (float)n_global;
        SPEC_STAMP(7);
        if (tid == own_base) {
            if (it + 1u == n_it) { out[0] = vs; out[1] = vb; }     // (the output block of the launch's last iteration)
            if (step) {
                if (it + 1u == n_it) { out[2] = loss; out[3] = finite; }
                if (loss_slot) loss_slot[it] = loss;
                if (finite_slot) finite_slot[it] = finite;
            }
        }
        const float scale = step ? -1.0f / (float)n_global : 1.0f;
        const bool last = it + 1u == n_it;
        const uint32_t mask_bit = (mode == SPEC_MODE_LOOP && it <= pretraining) ? 2u : 1u;
        if (own_fast) {
            SpecOwn own = spec_own_load(OWN + 5 * oid);
            // (both positions' rows requested before either sum: an unused entry has position 0, read and not selected)
            float tot[2];
#pragma unroll
            for (uint32_t e = 0; e < SPEC_OWN_ENTRIES; ++e) tot[e] = spec_pos_total(WS, own.pos[e], rows);
            float gsum = 0.0f;
#pragma unroll
            for (uint32_t e = 0; e < SPEC_OWN_ENTRIES; ++e) {
                const float term = tot[e] * (own.b[e] * spec_utransform_grad(own.tr[e], own.theta));
                gsum += e < own.n ? term : 0.0f;
            }
#if SPEC_EXCHANGE
            if (xrun) gsum = xgsum;
#endif
            const float grad = gsum * scale;
            SPEC_STAMP(8);
            SPEC_RSTAMP(3);
            if (last || !step) out[BSVI_OUT_HEADER + oid] = grad;
            if (step) {
                if (finite != 0.0f && (own.mask & mask_bit))
                    optimizer_apply_running(cfg, own.theta, own.s0, own.s1, own.s2, own.st, grad, own.p1, own.p2);
                SPEC_STAMP(9);
#if SPEC_LOOP_MANY
                if (G > 1 && !last) __hip_atomic_store(SPEC_A->params + oid, own.theta, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
                if (last) {
                    float* const params = SPEC_A->params;
                    float* const state = SPEC_A->state;
                    params[oid] = own.theta;
                    if (state) {
                        state[oid] = own.s0;
                        state[(size_t)SPEC_N_PARAMS + oid] = own.s1;
                        state[2 * (size_t)SPEC_N_PARAMS + oid] = own.s2;
                        state[3 * (size_t)SPEC_N_PARAMS + oid] = own.st;
                    }
                } else {
#pragma unroll
                    for (uint32_t e = 0; e < SPEC_OWN_ENTRIES; ++e)
                        if (e < own.n) spec_store_uniform(own.k[e], own.a[e] + own.b[e] * utransform_common(own.tr[e], own.theta));
                    OWN[5 * oid] = spec_f4{own.theta, own.s0, own.s1, own.s2};
                    spec_lds[SPEC_OFF_OWN + SPEC_OWN_WORDS * oid + 4] = own.st;
                    if (optimizer_has_p1(cfg.kind)) spec_own_store_products(OWN + 5 * oid, own);     // (Adam, AdamW, Adamax)
                }
            }
        }
#if SPEC_GENERIC_OWNERS      // parameters beyond the workgroup size or with more than two uniform entries: the LDS working copy
        for (uint32_t i = tid; i < SPEC_N_PARAMS; i += nthreads) {
            if (i == oid && own_fast) continue;
            const float theta = PS[i];
            const uint32_t j0 = TAB[SPEC_TAB_PTR + i], j1 = TAB[SPEC_TAB_PTR + i + 1];
            float gsum = 0.0f;
            for (uint32_t j = j0; j < j1; ++j) {
                const uint32_t pos = TAB[SPEC_TAB_POS + j], k = TAB[SPEC_TAB_IDX + j];
                gsum += spec_pos_total(WS, pos, rows) * (__uint_as_float(TAB[4 * k + 3]) * spec_utransform_grad(TAB[4 * k + 1] & 0xFFu, theta));
            }
#if SPEC_EXCHANGE
            bool xok = true;
            if (xrun) xok = spec_xget(xg, xseq0 + it + 1u, BSVI_OUT_HEADER + i, gsum);      // the ranks' sums of this parameter, in rank order
#else
            const bool xok = true;
#endif
            const float grad = gsum * scale;
            if (last || !step) out[BSVI_OUT_HEADER + i] = grad;
            if (step && xok && finite != 0.0f && (TAB[SPEC_TAB_MASK + i] & mask_bit))
                optimizer_update(cfg, PS, PS + SPEC_NP_PAD, SPEC_NP_PAD, i, grad);
            if (!step) continue;
            if (last) {
                float* const params = SPEC_A->params;
                float* const state = SPEC_A->state;
                params[i] = PS[i];
                if (state) {
#pragma unroll
                    for (uint32_t s = 0; s < 4u; ++s) state[(size_t)s * SPEC_N_PARAMS + i] = PS[(1u + s) * SPEC_NP_PAD + i];
                }
            } else {
                const float theta2 = PS[i];
                for (uint32_t j = j0; j < j1; ++j) spec_publish_uniform(TAB, TAB[SPEC_TAB_IDX + j], theta2);
#if SPEC_LOOP_MANY
                if (G > 1) __hip_atomic_store(SPEC_A->params + i, theta2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
            }
        }
#endif
#if SPEC_LOOP_MANY
        if (G > 1 && mode == SPEC_MODE_LOOP) {                  // (only workgroup 0 gets here) the new parameters are out: release the iteration
            __threadfence();
            __syncthreads();
            if (tid == 0) __hip_atomic_store(SPEC_A->ticket + 64, gen0 + it + 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        }
#endif
        SPEC_STAMP(6);
        SPEC_RSTAMP(4);
    }
    SPEC_RSTAMP_WRITE();
#if defined(SPEC_DEBUG_STAMPS)
    float* const loss_slot = SPEC_A->loss_slot;
    if (tid == 0 && loss_slot && n_it > 16) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        for (int i = 1; i < 12; ++i) loss_slot[i] = (float)(stamp[i] - stamp[0]);
    }
#endif
#undef SPEC_A
}

}  // namespace bsvi
