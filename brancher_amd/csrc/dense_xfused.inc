// dense_xfused.inc — the exact-data iteration of the dense-link path as TWO fused launches (DESIGN 4.8; included by
// dense_kernel.inc between the round-3 exact-data kernels and the host side; same translation unit as elbo_kernel.hip).
//
// The iteration (examples/MNIST_logistic_regression.py:15-54 through brancher/variables.py:843-870) multiplies twice by the
// minibatch x, whose values are exactly bf16 numbers, so both products run on v_mfma_f32_32x32x16_bf16 / 16x16x32 as three
// MFMAs on the exact pieces hi + mid + lo of the f32 operand (dense_split3).  Round 3 ran them as library calls between
// four elementwise launches and materialised every intermediate (W pieces 49 MB, logits 21 MB, dlog pieces 31 MB,
// GT 32 MB at BASELINE config 4).  Here:
//
//   dense_xfwd   one workgroup = NS samples x all minibatch rows of a 512-row tile.  Waves 4-7 DRAW the weights of those
//                samples (Philox, W = mu + s * eps, split in three) straight into LDS, k chunk by k chunk; waves 0-3 multiply
//                the chunk before it (A fragments of x from global memory: 16 bytes per lane IS a fragment), so the vector
//                work of the draw runs beside the matrix work on every SIMD.  The logits never leave the chip: the epilogue
//                turns the accumulators through LDS, takes the log-softmax cross-entropy and stores d f / d logits as pieces
//                [3][(c, n)][B_pad] — class-major, so that the sum over samples is a sum over neighbouring columns below.
//   dense_xbwd   GT[p][(c, n)] = sum_b x[b][p] dlog[(c, n)][b] with the 112 x B_pad tile of x^T RESIDENT in LDS for the
//                life of the workgroup; every wave on its own takes column blocks of 16 samples off the workgroup's queue
//                (fragments of dlog from global memory, no barrier in the loop), redraws the normals of its 7 x 64 feature
//                quads in registers and reduces eps * GT, GT, eps, eps^2 over the 16 samples with DPP row sums.  GT is never
//                stored; eps is never stored.
//
// HBM traffic per iteration at config 4: the dlog pieces once out and (through L2) once in, 2 x 31 MB, plus 8 MB of partial
// sums — against 300-500 MB in round 3.  No atomics on floats; every sum has a fixed order.

#include "dense_select.h"
// the tile constants the launch plan shares with the kernels live there: XF_ROWS (sample, class) rows of a dense_xfwd workgroup and
// its XF_FWD_LDS bytes (the epilogue's share: xf_epilogue_lds), XF_MT / XF_MT9 rows of x^T resident in dense_xbwd
using bsvi_dense_select::XF_ROWS;
using bsvi_dense_select::XF_FWD_LDS;

typedef __bf16 xf_bf16x8 __attribute__((ext_vector_type(8)));
typedef float xf_f32x16 __attribute__((ext_vector_type(16)));
typedef float xf_f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t xf_u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t xf_u32x2 __attribute__((ext_vector_type(2)));

constexpr uint32_t XF_KC = 64;                       // features per chunk of W in LDS (two k steps of 32)
constexpr uint32_t XF_WS = 2 * XF_KC + 16;           // row stride in bytes: 9 x 16, so 16 rows sit on 16 different bank quads
constexpr uint32_t XF_PLANE = XF_ROWS * XF_WS;
constexpr uint32_t XF_BUF = 3 * XF_PLANE;
constexpr uint32_t XF_DRAW_LDS = 2 * XF_BUF;         // two chunks of W: one being drawn, one being multiplied (55 296 B)
constexpr uint32_t XF_XSLOT = 8192;                  // the A fragments of one k step of one product wave: 2 k chunks x 4 row blocks x 1 KB
constexpr uint32_t XF_XRING = 3;                     // ... three steps deep per wave (two steps = 64 KB per CU in flight)
constexpr uint32_t XF_LOOP_LDS = XF_DRAW_LDS + 4 * XF_XRING * XF_XSLOT;      // 153 600 B
static_assert(XF_LOOP_LDS <= XF_FWD_LDS, "the product loop's LDS");      // (after the loop: xf_epilogue_lds, dense_select.h)

__device__ __forceinline__ xf_u32x2 xf_pack4(const uint16_t v[4]) {
    return xf_u32x2{(uint32_t)v[0] | ((uint32_t)v[1] << 16), (uint32_t)v[2] | ((uint32_t)v[3] << 16)};
}
typedef __bf16 xb_bf16x2 __attribute__((ext_vector_type(2)));
typedef float xb_f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t xb_pack(float a, float b) {       // (v_cvt_pk_bf16_f32, round to nearest even: dense_bf16_bits of both)
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(xb_f32x2{a, b}, xb_bf16x2));
}
__device__ __forceinline__ xf_u32x4 xf_pack8(const uint16_t v[8]) {
    return xf_u32x4{(uint32_t)v[0] | ((uint32_t)v[1] << 16), (uint32_t)v[2] | ((uint32_t)v[3] << 16),
                    (uint32_t)v[4] | ((uint32_t)v[5] << 16), (uint32_t)v[6] | ((uint32_t)v[7] << 16)};
}

// DBG (profiling only, BSVI_XF_DEBUG): 1 = the drawing waves store constants (no Philox, no split), 2 = the product waves
// skip the LDS reads and the MFMAs, 3 = no epilogue (and with it no MFMAs: the accumulators are dead code then), 4 = 1 and 2 (the DMA
// of the minibatch fragments alone), 5 = no DMA (draw and products on whatever LDS holds).
// Read of the variants at the round's end (us): whole 47.2; without Philox 40; loop without MFMAs 24.6, with them 35.4;
// the accumulators through LDS 3; log-softmax, gradient pieces and their stores 8.8 (the stores 7)
// The barriers of the product loop: LDS traffic only.  (__syncthreads() carries a workgroup-scope fence, which on gfx950 is an
// s_waitcnt vmcnt(0): every chunk barrier drained the product waves' DMA ring — and dense_xbwd's staging barrier its first fragment
// groups.)
__device__ __forceinline__ void xf_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

template <int DBG, int NCB, bool WEIGHTED = false>      // (WEIGHTED: caller weights a_n on d f / d logits — its own instantiation: the check cost cfg 4 1.2 us)
__global__ void __launch_bounds__(512) dense_xfwd(const DParams D, const uint32_t NS) {
    unsigned char* const lds = reinterpret_cast<unsigned char*>(g_lds);
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));   // (scalar: the roles branch below)
    const uint32_t n0 = blockIdx.x * NS, b0 = blockIdx.y * 512u;
    const uint32_t NSC = NS * D.C;
    const uint32_t n_steps = D.Kp / 32u, n_chunks = (D.Kp + XF_KC - 1) / XF_KC;
    for (uint32_t i = tid; i < XF_DRAW_LDS / 16; i += 512) reinterpret_cast<xf_u32x4*>(lds)[i] = xf_u32x4{0u, 0u, 0u, 0u};
    __syncthreads();

    // (DBG 6: cycle stamps of workgroups 0 and 133, rows 16.. of the debug buffer — tools/r6/xfwd_stamps.py)
    unsigned long long* const stamp = (DBG == 6 && D.stamps && lane == 0 && (blockIdx.x == 0 || blockIdx.x == 133)) ? D.stamps + (16u + (blockIdx.x ? 8u : 0u) + wave) * 32u : nullptr;
    uint32_t n_stamp = 0;
    auto mark = [&]() __attribute__((always_inline)) { if (DBG == 6 && stamp && n_stamp < 32) stamp[n_stamp++] = __builtin_readcyclecounter(); };
    mark();
    xf_f32x16 acc[4][NCB];          // (set by the product waves only: the drawing waves must not carry 128 live registers through their loop)
    const uint32_t lm = lane & 31u, lk = lane >> 5;

    if (wave >= 4) {
        // ---- the draw: quad (row, kq) of a chunk = features k0 + 4 kq .. + 3 of weight row (sample n0 + row / C, class row % C)
        const uint32_t gtid = tid - 256u;
        const float2* const ms = reinterpret_cast<const float2*>(D.rowp + 4 * (size_t)D.R);      // {loc, scale} per row
        auto produce = [&](uint32_t chunk) __attribute__((always_inline)) {
            unsigned char* const buf = lds + (chunk & 1u) * XF_BUF;
            const uint32_t k0 = chunk * XF_KC, klen = min(XF_KC, D.Kp - k0), qpr = klen / 4u, rstep = 256u / qpr;
            const uint32_t rsub = gtid / qpr, kq = gtid - rsub * qpr, p = k0 + 4u * kq;
            if (rsub >= rstep) return;
            uint32_t ni = rsub / D.C, c = rsub - ni * D.C;
            if (DBG != 1 && DBG != 4 && !D.noise_in && !D.noise_out) {
                // the product path: RU rows of this lane at a time, no branch between their Philox chains — ONE drawing wave per
                // SIMD has nobody to hide the latency of the dependent v_mad_u64_u32 / transcendental chain behind but itself
                constexpr int RU = 3;
                const bool inp = p < D.P;
                for (uint32_t row0 = rsub; row0 < NSC; row0 += RU * rstep) {
                    float e[RU][4];
                    uint32_t rr[RU];
                    bool ok[RU], lv[RU];
#pragma unroll
                    for (int u = 0; u < RU; ++u) {
                        const uint32_t row = row0 + u * rstep, n = n0 + ni;
                        ok[u] = row < NSC && inp;
                        lv[u] = ok[u] && n < D.n_local;
                        rr[u] = ok[u] ? c * D.P + p : 0u;
                        dense_eps4(D, n, rr[u] >> 2, e[u]);
                        c += rstep;
                        while (c >= D.C) { c -= D.C; ++ni; }
                    }
#pragma unroll
                    for (int u = 0; u < RU; ++u) {
                        const uint32_t row = row0 + u * rstep;
                        const xf_f32x4 m01 = *reinterpret_cast<const xf_f32x4*>(ms + rr[u]), m23 = *reinterpret_cast<const xf_f32x4*>(ms + rr[u] + 2);
                        const float w[4] = {m01[0] + m01[1] * (lv[u] ? e[u][0] : 0.0f), m01[2] + m01[3] * (lv[u] ? e[u][1] : 0.0f),
                                            m23[0] + m23[1] * (lv[u] ? e[u][2] : 0.0f), m23[2] + m23[3] * (lv[u] ? e[u][3] : 0.0f)};
                        uint16_t hi[4], mid[4], lo[4];
#pragma unroll
                        for (int j = 0; j < 4; ++j) dense_split3(ok[u] ? w[j] : 0.0f, hi[j], mid[j], lo[j]);
                        if (row < NSC) {
                            unsigned char* const at = buf + row * XF_WS + kq * 8u;
                            *reinterpret_cast<xf_u32x2*>(at) = xf_pack4(hi);
                            *reinterpret_cast<xf_u32x2*>(at + XF_PLANE) = xf_pack4(mid);
                            *reinterpret_cast<xf_u32x2*>(at + 2 * XF_PLANE) = xf_pack4(lo);
                        }
                    }
                }
                return;
            }
            for (uint32_t row = rsub; row < NSC; row += rstep) {
                const uint32_t n = n0 + ni;
                uint16_t hi[4] = {0, 0, 0, 0}, mid[4] = {0, 0, 0, 0}, lo[4] = {0, 0, 0, 0};
                if (DBG == 1 || DBG == 4) { hi[0] = (uint16_t)row; mid[1] = (uint16_t)p; }
                if (DBG != 1 && DBG != 4 && p < D.P) {
                    const uint32_t r = c * D.P + p;
                    float e[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                    if (n < D.n_local) {
                        if (D.noise_in) {
#pragma unroll
                            for (int j = 0; j < 4; ++j) e[j] = D.noise_in[(size_t)(r + j) * D.n_local + n];
                        } else {
                            dense_eps4(D, n, r >> 2, e);
                        }
                        if (D.noise_out && blockIdx.y == 0) {
#pragma unroll
                            for (int j = 0; j < 4; ++j) D.noise_out[(size_t)(r + j) * D.n_local + n] = e[j];
                        }
                    }
                    const xf_f32x4 m01 = *reinterpret_cast<const xf_f32x4*>(ms + r), m23 = *reinterpret_cast<const xf_f32x4*>(ms + r + 2);
                    const float w[4] = {m01[0] + m01[1] * e[0], m01[2] + m01[3] * e[1], m23[0] + m23[1] * e[2], m23[2] + m23[3] * e[3]};
#pragma unroll
                    for (int j = 0; j < 4; ++j) dense_split3(w[j], hi[j], mid[j], lo[j]);
                }
                unsigned char* const at = buf + row * XF_WS + kq * 8u;
                *reinterpret_cast<xf_u32x2*>(at) = xf_pack4(hi);
                *reinterpret_cast<xf_u32x2*>(at + XF_PLANE) = xf_pack4(mid);
                *reinterpret_cast<xf_u32x2*>(at + 2 * XF_PLANE) = xf_pack4(lo);
                c += rstep;
                while (c >= D.C) { c -= D.C; ++ni; }
            }
        };
        const uint32_t passes = (NSC + 15u) / 16u;
        if (DBG != 1 && DBG != 4 && !D.noise_in && !D.noise_out && passes <= 4u) {
            // Round 6: the {loc, scale} of a quad were loaded where they were used — two loads, 71 vector instructions of Philox,
            // s_waitcnt vmcnt(0): every 16-row pass of every chunk waited out what was left of an L2 round trip under the product waves'
            // DMA traffic.  A lane's rows are the same in every whole chunk, so the values of chunk c + 1 are requested before chunk c
            // is drawn and have a whole chunk (and the barrier) to arrive: config 4 102.5 -> 100.5 us per iteration.
            auto run = [&](auto ru_tag) __attribute__((always_inline)) {
                constexpr int RU = decltype(ru_tag)::value;
                const uint32_t rsub = gtid >> 4, kq = gtid & 15u;
                uint32_t cb[RU], nn[RU], rw[RU];
                bool rok[RU];
#pragma unroll
                for (int u = 0; u < RU; ++u) {
                    rw[u] = rsub + 16u * u;
                    rok[u] = rw[u] < NSC;
                    const uint32_t ni = rw[u] / D.C;
                    cb[u] = (rw[u] - ni * D.C) * D.P;
                    nn[u] = n0 + ni;
                }
                xf_f32x4 m01[RU], m23[RU];
                auto fetch = [&](uint32_t chunk) __attribute__((always_inline)) {
                    const uint32_t p = chunk * XF_KC + 4u * kq;
#pragma unroll
                    for (int u = 0; u < RU; ++u) {
                        const uint32_t rr = (rok[u] && p < D.P) ? cb[u] + p : 0u;
                        m01[u] = *reinterpret_cast<const xf_f32x4*>(ms + rr);
                        m23[u] = *reinterpret_cast<const xf_f32x4*>(ms + rr + 2);
                    }
                };
                auto whole = [&](uint32_t chunk) __attribute__((always_inline)) {
                    unsigned char* const buf = lds + (chunk & 1u) * XF_BUF;
                    const uint32_t p = chunk * XF_KC + 4u * kq;
                    const bool inp = p < D.P;
                    // (the empty asm READS the registers: the compiler's wait for the loads of a chunk ago sits here, in front of the new
                    //  requests — left to itself it put the requests first and an s_waitcnt vmcnt(0), which counts in order, behind them)
                    xf_f32x4 a01[RU], a23[RU];
#pragma unroll
                    for (int u = 0; u < RU; ++u) {
                        asm volatile("" : "+v"(m01[u]), "+v"(m23[u]));
                        a01[u] = m01[u];
                        a23[u] = m23[u];
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    if ((chunk + 2u) * XF_KC <= D.Kp) fetch(chunk + 1u);
                    __builtin_amdgcn_sched_barrier(0);
                    float e[RU][4];
#pragma unroll
                    for (int u = 0; u < RU; ++u) dense_eps4(D, nn[u], ((rok[u] && inp) ? cb[u] + p : 0u) >> 2, e[u]);
#pragma unroll
                    for (int u = 0; u < RU; ++u) {
                        const bool ok = rok[u] && inp, lv = ok && nn[u] < D.n_local;
                        const float w[4] = {a01[u][0] + a01[u][1] * (lv ? e[u][0] : 0.0f), a01[u][2] + a01[u][3] * (lv ? e[u][1] : 0.0f),
                                            a23[u][0] + a23[u][1] * (lv ? e[u][2] : 0.0f), a23[u][2] + a23[u][3] * (lv ? e[u][3] : 0.0f)};
                        uint16_t hi[4], mid[4], lo[4];
#pragma unroll
                        for (int j = 0; j < 4; ++j) dense_split3(ok ? w[j] : 0.0f, hi[j], mid[j], lo[j]);
                        if (rok[u]) {
                            unsigned char* const at = buf + rw[u] * XF_WS + kq * 8u;
                            *reinterpret_cast<xf_u32x2*>(at) = xf_pack4(hi);
                            *reinterpret_cast<xf_u32x2*>(at + XF_PLANE) = xf_pack4(mid);
                            *reinterpret_cast<xf_u32x2*>(at + 2 * XF_PLANE) = xf_pack4(lo);
                        }
                    }
                };
                if (XF_KC <= D.Kp) fetch(0);
                for (uint32_t chunk = 0; chunk < n_chunks; ++chunk) {
                    if ((chunk + 1u) * XF_KC <= D.Kp) whole(chunk); else produce(chunk);       // (a short last chunk: other quads per lane)
                    mark();
                    xf_barrier();
                    mark();
                }
                xf_barrier();
            };
            if (passes == 1u) run(std::integral_constant<int, 1>{});
            else if (passes == 2u) run(std::integral_constant<int, 2>{});
            else if (passes == 3u) run(std::integral_constant<int, 3>{});
            else run(std::integral_constant<int, 4>{});
        } else {
            produce(0);
            xf_barrier();
            for (uint32_t chunk = 0; chunk < n_chunks; ++chunk) {
                if (chunk + 1 < n_chunks) produce(chunk + 1);
                xf_barrier();
            }
        }
    } else {
        // ---- the product: wave w multiplies minibatch rows b0 + 128 w .. + 127 (four 32-row blocks) by the 64 rows of W
        const uint32_t rbase = b0 + wave * 128u;
        // (no guards in the hot loop: row blocks beyond B_pad read row B_pad - 1 and are not stored; NCB = column blocks of 32)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < NCB; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
        // x in FRAGMENT-MAJOR order (dense_head, fused form): the 64 x 16 bytes of the A fragment of (32-row block, k chunk of 16)
        // are contiguous, so a fragment is one fully coalesced 1 KB load.  (From the row-major copy a fragment touched 32
        // rows x 32 bytes: 32 half-used lines per load, 64 KB of lines per step against 32 KB of L1 — the product ran at a
        // quarter of the MFMA rate.)
        const unsigned char* xrow[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t rbi = min((rbase >> 5) + (uint32_t)i, (D.B_pad >> 5) - 1u);
            xrow[i] = reinterpret_cast<const unsigned char*>(D.Xb_bf) + ((size_t)rbi * (D.Kp / 16u) * 64u + lane) * 16u;
        }
        // ... and travels global -> LDS by DMA (no registers) into a ring of XF_XRING step slots PRIVATE to the wave: the fragments
        // of steps gs + 1 and gs + 2 are in flight while step gs is multiplied, 64 KB per CU.  (With the fragments prefetched
        // one step ahead in registers — all a 256-register budget allows beside 128 accumulators — 32 KB per CU were in
        // flight against ~1.3 us of L2 latency under this load: 24 GB/s per CU, the product at half the MFMA rate.)  Only the
        // wave's own vmcnt orders its LDS reads behind its DMA; nobody else touches the slots, so no barrier.
        unsigned char* const xring = lds + XF_DRAW_LDS + wave * (XF_XRING * XF_XSLOT);
        auto dma = [&](uint32_t gs, uint32_t slot) {
            if (DBG == 5) return;
#pragma unroll
            for (int kc = 0; kc < 2; ++kc)
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(xrow[i] + (size_t)(2u * gs + kc) * 1024u),
                                                     (__attribute__((address_space(3))) void*)(xring + slot * XF_XSLOT + (kc * 4 + i) * 1024), 16, 0, 0);
        };
        // One step = 2 k chunks x 3 planes x 4 x NCB = 48 MFMAs of 32 cycles, and that is what the product waves spend per step: 1 900-2 250
        // cycles on pixel data (whose toggling costs the clock a quarter against zeros: tools/r6/mfma_feed.hip, xfwd_stamps.py) — the loop
        // is bound by the matrix pipe, padding included (40 live of 64 columns), not by the draw.  Round 6 tried, and measured no gain from:
        // the fragments of piece q + 1 requested ahead of the MFMAs of piece q, the next step's first fragments ahead of piece 3 (the
        // in-order wave had the pipe's queue full either way); the last, partly filled pass of the draw on the product waves
        // (tools/r5/experiments/xfwd_product_wave_draw_share.patch).
        auto multiply = [&](uint32_t gs, uint32_t slot) {
            const unsigned char* const buf = lds + ((gs >> 1) & 1u) * XF_BUF + (gs & 1u) * 64u + lk * 16u + lm * XF_WS;
            const unsigned char* const xa = xring + slot * XF_XSLOT + lane * 16u;
#pragma unroll
            for (int kc = 0; kc < 2; ++kc) {
                xf_bf16x8 A[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) A[i] = *reinterpret_cast<const xf_bf16x8*>(xa + (kc * 4 + i) * 1024);
#pragma unroll
                for (int pl = 0; pl < 3; ++pl) {
                    xf_bf16x8 b[NCB];
#pragma unroll
                    for (int j = 0; j < NCB; ++j) b[j] = *reinterpret_cast<const xf_bf16x8*>(buf + pl * XF_PLANE + j * 32u * XF_WS + kc * 32u);
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int j = 0; j < NCB; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[i], b[j], acc[i][j], 0, 0, 0);
                }
            }
        };
        dma(0, 0);
        if (1 < n_steps) dma(1, 1);
        xf_barrier();                                   // chunk 0 is drawn
        uint32_t slot = 0;
        for (uint32_t gs = 0; gs < n_steps; ++gs) {
            if ((gs & 1u) == 0 && gs > 0) xf_barrier();     // the chunk of steps gs, gs + 1 is drawn, the one before it is free
            if (gs + 2 < n_steps) {
                dma(gs + 2, slot == 0 ? 2u : slot - 1u);        // (into the slot of step gs - 1, whose reads the MFMAs have consumed)
                asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
            } else if (gs + 1 < n_steps) {
                asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
            } else {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            if (DBG == 6 && gs < 12) mark();
            if (DBG != 2 && DBG != 4) multiply(gs, slot);
            if (DBG == 6 && gs < 12) mark();
            slot = slot == 2 ? 0u : slot + 1u;
        }
        mark();
        xf_barrier();                                   // (the drawing waves' last barrier)
    }

    // ---- epilogue: the logits tile through LDS, log-softmax cross-entropy, d f / d logits as pieces.  One work item =
    // (4 consecutive minibatch rows, one sample): the 4 values of a class leave as ONE 8-byte store per piece (2-byte stores
    // along b, one per value, took 55 of this kernel's 77 us).  Row r of the tile sits at position (r & 3) * n_quad + (r >> 2),
    // so the lanes of a wave — consecutive quads — read consecutive tile rows (odd stride: distinct banks).
    // (Round 4, second version.  The first took items of 8 rows: 256 of the 512 threads had one — four waves, one per SIMD,
    //  each walking 80 logits TWICE (the exponentials of the gradient were computed again: 160 registers could not be kept) —
    //  and the epilogue was 27 of the kernel's 52 us, 20 of them arithmetic and LDS latency, 7 the stores (profiling variants).
    //  With 4 rows per item every thread has one, the 40 exponentials stay in registers, and two waves share a SIMD.)
    if (DBG == 3) return;
    mark();
    float* const tile = g_lds;
    const uint32_t TS = NSC | 1u;
    constexpr uint32_t n_quad = 128u;                      // quads of the 512-row tile (ONE pass: the accumulators die here)
    float* const likbuf = tile + 512u * TS;                // [sample][quad]
    // d f / d logits leaves as F32, class-major [(c, n)][B_pad] (round 6; three bf16 planes before): 4 bytes per element instead of 6 on
    // the way out and on dense_xbwd's way in — which is bound by what a CU takes in from its L2 — and no split here; dense_xbwd splits
    // the fragment it is about to multiply in registers (the same hi + mid + lo: bit-identical sums)
    float* const dlogf = reinterpret_cast<float*>(D.dlogp);
    {
        __syncthreads();
        if (wave < 4) {
            const uint32_t wrow = wave * 128u;
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < NCB; ++j) {
                    const uint32_t col = 32u * j + lm;
                    if (col < NSC) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const uint32_t row = wrow + 32u * i + 8u * (r >> 2) + 4u * lk + (r & 3u);
                            tile[((row & 3u) * n_quad + (row >> 2)) * TS + col] = acc[i][j][r];
                        }
                    }
                }
        }
        __syncthreads();
        for (uint32_t it = tid; it < n_quad * NS; it += 512) {
            const uint32_t ni = it / n_quad, o = it - ni * n_quad, n = n0 + ni, b = b0 + 4u * o;
            const bool live = n < D.n_local;
            float lik = 0.0f;
            if (b < D.B_pad && n < D.n_pad) {
                const float* const trow = tile + o * TS + ni * D.C;          // + k * n_quad * TS: row 4 o + k
                float lab[4], wk[4];
                const float wn = WEIGHTED ? D.lik_weight * (live ? D.f_weight[n] : 1.0f) : D.lik_weight;       // (a_n: caller-weighted gradients)
#pragma unroll
                for (int k = 0; k < 4; ++k) { lab[k] = D.lab[b + k]; wk[k] = (b + k < D.B) ? wn : 0.0f; }
                if (D.likelihood == BSVI_LIK_CATEGORICAL) {
                    // (loops over the classes unrolled to 16 with guards: a run-time loop waits for every single LDS read)
                    float e[4][16], wr[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const float* const t = trow + k * n_quad * TS;
                        float m = -INFINITY, zl = 0.0f, se = 0.0f;
#pragma unroll
                        for (int c = 0; c < 16; ++c) {
                            e[k][c] = c < (int)D.C ? t[c] : -INFINITY;
                            m = fmaxf(m, e[k][c]);
                        }
#pragma unroll
                        for (int c = 0; c < 16; ++c) {
                            zl = (lab[k] == (float)c) ? e[k][c] : zl;
                            e[k][c] = c < (int)D.C ? __expf(e[k][c] - m) : 0.0f;
                            se += e[k][c];
                        }
                        lik += wk[k] * (zl - (m + __builtin_amdgcn_logf(se) * 0.6931471805599453f));
                        wr[k] = wk[k] * __builtin_amdgcn_rcpf(se);
                    }
#pragma unroll
                    for (int c = 0; c < 16; ++c) {
                        if (c < (int)D.C) {
                            xf_f32x4 g4;
#pragma unroll
                            for (int k = 0; k < 4; ++k) g4[k] = live ? ((lab[k] == (float)c) ? wk[k] : 0.0f) - wr[k] * e[k][c] : 0.0f;
                            *reinterpret_cast<xf_f32x4*>(dlogf + ((size_t)c * D.n_pad + n) * D.B_pad + b) = g4;
                        }
                    }
                } else {   // Bernoulli / Binomial(1): -binary_cross_entropy_with_logits(l, k)
                    xf_f32x4 g4;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const float l = trow[k * n_quad * TS];
                        lik += wk[k] * (lab[k] * l - (fmaxf(l, 0.0f) + log1pf(expf(-fabsf(l)))));
                        g4[k] = live ? wk[k] * (lab[k] - sigmoidf_(l)) : 0.0f;
                    }
                    *reinterpret_cast<xf_f32x4*>(dlogf + (size_t)n * D.B_pad + b) = g4;
                }
            }
            likbuf[ni * n_quad + o] = live ? lik : 0.0f;
        }
    }
    __syncthreads();
    // the quads of a sample in row order: eight threads per sample take sixteen each, the first adds the eight partial sums
    float* const likpart = likbuf + NS * n_quad;
    if (tid < 8u * NS) {
        const uint32_t ni = tid >> 3, part = tid & 7u;
        float sp = 0.0f;
#pragma unroll
        for (uint32_t o = 0; o < 16u; ++o) sp += likbuf[ni * n_quad + part * 16u + o];
        likpart[tid] = sp;
    }
    __syncthreads();
    if (tid < NS && n0 + tid < D.n_pad) {
        float sp = 0.0f;
#pragma unroll
        for (uint32_t q = 0; q < 8u; ++q) sp += likpart[tid * 8u + q];
        D.lik_part[(size_t)blockIdx.y * D.n_pad + n0 + tid] = sp;
    }
    mark();
}

// 16 sums over the 16 lanes of a DPP row in 15 exchanges: at every step a lane keeps the half of its values that its own
// lane bit selects and adds the partner's copy of that half (partners: lane ^ 8, the mirror lane of the half row — which
// has bit 2 flipped —, lane ^ 2, lane ^ 1); lane q of the row ends with the row total of v[q].  (Sixteen separate row sums
// would be 64 DPP adds per MFMA block.)
__device__ __forceinline__ float xf_row16_reduce16(float (&v)[16], uint32_t lane) {
    const bool b3 = (lane & 8u) != 0, b2 = (lane & 4u) != 0, b1 = (lane & 2u) != 0, b0 = (lane & 1u) != 0;
    float a[8], c[4], d[2];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float keep = b3 ? v[8 + i] : v[i], give = b3 ? v[i] : v[8 + i];
        a[i] = keep + dpp_f<0x128>(give);              // row_ror:8
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float keep = b2 ? a[4 + i] : a[i], give = b2 ? a[i] : a[4 + i];
        c[i] = keep + dpp_f<0x141>(give);              // row_half_mirror: lane 7 - i of the half row (the other quad: bit 2 flipped)
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const float keep = b1 ? c[2 + i] : c[i], give = b1 ? c[i] : c[2 + i];
        d[i] = keep + dpp_f<0x4E>(give);               // quad_perm [2,3,0,1]: lane ^ 2
    }
    const float keep = b0 ? d[1] : d[0], give = b0 ? d[0] : d[1];
    return keep + dpp_f<0xB1>(give);                   // quad_perm [1,0,3,2]: lane ^ 1
}

// DBG (profiling only): 1 = no redraw in the epilogue, 2 = no MFMAs (the fragments are still loaded), 3 = no dlog loads
// RB: 16-row blocks of x^T per feature tile.  The P / 16 row blocks are dealt out evenly: tile m has base + (m < extra) of them.
// (Round 5: 9 instead of 7 — six feature tiles re-read a group's dlog columns instead of seven, 40 column groups of 16 blocks are
//  exactly two blocks per wave, and 240 workgroups fit the XCDs' 8 x 32 CUs: L2 -> CU traffic 275 -> 221 MB.)
// NOISE: the caller-supplied-noise form is its OWN instantiation (round 6): with its loads of the normals in the block epilogue the compiler put
// an s_waitcnt vmcnt(0) in front of the Philox path's redraw too — the ring's next three groups were waited for at every block's end
template <int DBG, int NR, int RB, bool NOISE = false>     // NR: sets of the fragment ring = groups of two k steps in flight (4 when B_pad is a multiple of 256, else 2)
__global__ void __launch_bounds__(512) dense_xbwd(const DParams D, const uint32_t tiles_m, const uint32_t groups, const uint32_t rb_base, const uint32_t rb_extra) {
    unsigned char* const lds = reinterpret_cast<unsigned char*>(g_lds);
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    // the tiles_m workgroups of one column group run on ONE XCD (blocks b and b + 8 share one): the group's dlog columns
    // enter that L2 once and are read tiles_m times from it
    const uint32_t xcd = blockIdx.x & 7u, slot = blockIdx.x >> 3, gi = slot / tiles_m, m = slot - gi * tiles_m, g = gi * 8u + xcd;
    if (g >= groups) return;
    const uint32_t rb0 = m * rb_base + min(m, rb_extra), rows_m = 16u * (rb_base + (m < rb_extra ? 1u : 0u));
    const uint32_t p0 = 16u * rb0, rowbytes = D.B_pad * 2u, stride = rowbytes + 32u, pieces = rowbytes / 16u;   // (66 x 16 B at B_pad = 512: the four 16-lane groups of a ds_read_b128 on 16 distinct bank quads)
    const uint32_t wave = tid >> 6;
    unsigned long long* const stamp = (D.stamps && lane == 0 && (blockIdx.x == 0 || blockIdx.x == 133)) ? D.stamps + ((blockIdx.x ? 8u : 0u) + wave) * 32u : nullptr;
    uint32_t n_stamp = 0;
    auto mark = [&]() { if (stamp && n_stamp < 32) stamp[n_stamp++] = __builtin_readcyclecounter(); };
    const uint32_t per_class = D.n_pad / 16u, total_cb = D.C * per_class;
    const uint32_t cb_lo = (uint32_t)(((uint64_t)g * total_cb) / groups), cb_hi = (uint32_t)(((uint64_t)(g + 1) * total_cb) / groups);
    const uint32_t lc = lane & 15u, lq = lane >> 4;
    const size_t plane = (size_t)D.n_pad * D.C * D.B_pad;
    const unsigned char* const abase = lds + lc * stride + lq * 16u;

    // column blocks off the workgroup's queue; the dlog fragments of a block travel in groups of two k steps through a ring
    // of four register sets (three groups = six steps = ~2 000 MFMA cycles ahead), and the first three groups of the NEXT block
    // are requested before this block's epilogue — the redraw — so that no block starts on a cold load
    // (round 6: the blocks of a wave are static — cb_lo + wave, + 8, ...: in front of the queue's LDS atomic the compiler put an
    //  s_waitcnt vmcnt(0), which drained the fragment ring once per block; the grid gives every wave the same number of blocks anyway)
    auto next_block = [&](uint32_t cb_now) { return cb_now + 8u; };
    // (buffer loads: ONE 32-bit lane offset per block, the piece and the k step in the scalar offset — with 64-bit lane
    //  addresses per piece the ring below ran out of registers and the compiler drained every load before issuing the next)
    auto source_of = [&](uint32_t cb) {
        const uint32_t c = cb / per_class, nb = (cb - c * per_class) * 16u;
        return (((c * D.n_pad + nb + lc) * D.B_pad) + lq * 8u) * 4u;         // (f32: the lane's eight values of a k step are 32 bytes)
    };
    // The ring holds raw 128-bit words (as <8 x bf16> values the compiler took every set that crosses a branch apart into 16-bit
    // pieces: 24 shifts and v_perm per fetch behind an s_waitcnt vmcnt(0)), and NOTHING about it is conditional: set k is
    // multiplied and at once requested again for the group NR further on — of this block or, at its end, of the wave's next
    // block, whose ticket is taken a block ahead (a wave without a next block requests one cache line again and again instead).
    // (Round 4's ring sat behind `if (g + 3 < n_groups)` guards.  s_waitcnt counts are static: the compiler has to assume that
    // any guarded fetch was skipped, so every multiply waited for all loads but the five youngest — the ring never had more than
    // one group in flight, and the kernel ran on exposed L2 latency.)
    // (round 6: the fragments are F32 — two 16-byte words per lane and k step instead of three — and are split into hi | mid | lo where
    //  they are multiplied: eleven vector instructions per pair of values beside the 27 MFMAs of the step)
    // The loads are written as assembly and waited for by hand (ring_wait): whatever the source looked like, the compiler ended up
    // with ONE s_waitcnt vmcnt(0) at the top of the ring's loop — every trip drained the three groups it had just requested.  Behind
    // `=v` the compiler knows nothing about a load in flight; what orders things is that ring_wait takes the set as an in-out operand
    // (nothing of the set is read before it) and that a set is overwritten only behind the MFMAs that read its split.
    xf_u32x4 S[NR][2][2];
    const xf_u32x4 rs = {(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(uintptr_t)D.dlogp),
                         (uint32_t)__builtin_amdgcn_readfirstlane((int)((uint32_t)((uintptr_t)D.dlogp >> 32) & 0xFFFFu)),
                         (uint32_t)__builtin_amdgcn_readfirstlane((int)((uint32_t)plane * 4u)), 0x00020000u};
    auto fetch = [&](xf_u32x4 (&B)[2][2], uint32_t src, uint32_t g) {
        const uint32_t voff = DBG == 3 ? lane * 16u : src;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const uint32_t soff = DBG == 3 ? 0u : (uint32_t)__builtin_amdgcn_readfirstlane((int)((g * 2u + u) * 128u));
            asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen" : "=v"(B[u][0]) : "v"(voff), "s"(rs), "s"(soff) : "memory");
            if (DBG == 3) asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen" : "=v"(B[u][1]) : "v"(voff), "s"(rs), "s"(soff) : "memory");
            else asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen offset:16" : "=v"(B[u][1]) : "v"(voff), "s"(rs), "s"(soff) : "memory");
        }
    };
    // set k is the oldest of the NR sets in flight: all but the 4 (NR - 1) youngest loads have landed
    auto ring_wait = [&](xf_u32x4 (&B)[2][2]) {
        if (NR == 4) asm volatile("s_waitcnt vmcnt(12)" : "+v"(B[0][0]), "+v"(B[0][1]), "+v"(B[1][0]), "+v"(B[1][1]) :: "memory");
        else asm volatile("s_waitcnt vmcnt(4)" : "+v"(B[0][0]), "+v"(B[0][1]), "+v"(B[1][0]), "+v"(B[1][1]) :: "memory");
    };
    auto split8 = [&](const xf_u32x4 (&raw)[2], xf_u32x4 (&P)[3]) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float u0 = __uint_as_float(raw[q >> 1][(q & 1) * 2]), u1 = __uint_as_float(raw[q >> 1][(q & 1) * 2 + 1]);
            const uint32_t h = xb_pack(u0, u1);
            u0 -= __uint_as_float(h << 16); u1 -= __uint_as_float(h & 0xFFFF0000u);
            const uint32_t m = xb_pack(u0, u1);
            u0 -= __uint_as_float(m << 16); u1 -= __uint_as_float(m & 0xFFFF0000u);
            P[0][q] = h; P[1][q] = m; P[2][q] = xb_pack(u0, u1);
        }
    };
    xf_f32x4 acc[RB];
    // The A fragments (x^T from LDS) of k step t + 1 are requested as soon as step t's last MFMA on that fragment has issued:
    // the products run feature block by feature block (three pieces on one accumulator back to back — the 16x16x32 form
    // needs no interleaving of accumulators), and block rb's register is reloaded while the 18 MFMAs of the other blocks
    // run.  A wave alone on its SIMD then runs at the MFMA rate with no register beyond round 4's (254, nothing to spare:
    // a second set of fragments spilled) instead of read -> wait -> 21 MFMAs per step.
    xf_u32x4 a[RB];
    auto a_load = [&](uint32_t step) {
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) a[rb] = *reinterpret_cast<const xf_u32x4*>(abase + rb * 16u * stride + step * 64u);
    };
    const uint32_t n_steps = D.B_pad / 32u;
    auto multiply = [&](const xf_u32x4 (&B)[2][2], uint32_t g) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const uint32_t next = 2u * g + u + 1u == n_steps ? 0u : 2u * g + u + 1u;
            const unsigned char* const an = abase + next * 64u;
            xf_u32x4 P[3];
            split8(B[u], P);
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) {
#pragma unroll
                for (int pl = 0; pl < 3; ++pl) {
                    // (rows beyond P are zero in LDS: no guard in the hot loop — a guard per block made every MFMA wait for its own read)
                    if (DBG == 2) acc[rb][0] += __builtin_bit_cast(float, a[rb][0]) * __builtin_bit_cast(float, P[pl][0]);
                    else acc[rb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(xf_bf16x8, a[rb]), __builtin_bit_cast(xf_bf16x8, P[pl]), acc[rb], 0, 0, 0);
                }
                a[rb] = *reinterpret_cast<const xf_u32x4*>(an + rb * 16u * stride);        // (the last step reads step 0 again: no branch in the loop)
#if defined(XB_SCHED)
                __builtin_amdgcn_sched_group_barrier(0x008, 3, 0);
                __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
#endif
            }
        }
    };
    const uint32_t n_groups = D.B_pad / 64u;            // (a multiple of NR: call_plan, dense_select.h, picks the instantiation)
    // x^T rows p0 .. p0 + 111 -> LDS by DMA (global_load_lds, 16 bytes per lane: one instruction = 1 KB = one row at
    // B_pad = 512), wave w takes rows w, w + 8, ...: all of a wave's rows in flight at once, no registers.  (Round 4 staged
    // through registers, seven loads in flight per lane: 9 500 cycles before the first MFMA.)  Rows beyond P are zeros.
    for (uint32_t row = wave; row < 16u * RB; row += 8u) {
        const uint32_t p = p0 + row;
        if (row < rows_m && p < D.P) {
            for (uint32_t pc = 0; pc < pieces; pc += 64u) {
                if (pc + lane < pieces)
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(reinterpret_cast<const unsigned char*>(D.XbT_bf + (size_t)p * D.B_pad) + (size_t)(pc + lane) * 16u),
                                                     (__attribute__((address_space(3))) void*)(lds + row * stride + pc * 16u), 16, 0, 0);
            }
        } else {
            for (uint32_t pc = lane; pc < pieces; pc += 64u) *reinterpret_cast<xf_u32x4*>(lds + row * stride + pc * 16u) = xf_u32x4{0u, 0u, 0u, 0u};
        }
    }
    // the FIRST block of a wave is static (block cb_lo + wave), so that its first fragment groups are requested while
    // the x^T tile is on its way (requested first: every wave waits for the tile, only one for a fragment group)
    uint32_t cb = cb_lo + wave;
    const bool any = cb < cb_hi;
    uint32_t bsrc = source_of(any ? cb : cb_lo);
    if (any) {
#pragma unroll
        for (int k = 0; k < NR; ++k) fetch(S[k], bsrc, k);
    }
    mark();
    // (the tile only: the wave's 4 NR fragment loads were issued behind it and stay in flight)
    if (any) { if (NR == 4) asm volatile("s_waitcnt vmcnt(16)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); }
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    xf_barrier();                      // (not __syncthreads(): its fence would drain the fragment loads)
    mark();
    if (!any) return;
    for (;;) {
        mark();
        const uint32_t cb_next = next_block(cb);
        const bool more = cb_next < cb_hi;
        const uint32_t src_next = more ? source_of(cb_next) : 0u;      // (no next block: every lane requests the SAME 16 bytes — one line per load, served by the L1)
        a_load(0u);
        const uint32_t c = cb / per_class, nb = (cb - c * per_class) * 16u, n = nb + lc;
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) acc[rb] = xf_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        for (uint32_t g = 0; g < n_groups; g += NR) {
            const bool last = g + NR >= n_groups;
            const uint32_t fsrc = last ? src_next : bsrc, fg = last ? 0u : g + NR;
#pragma unroll
            for (int k = 0; k < NR; ++k) {
                ring_wait(S[k]);
                multiply(S[k], g + k);
                __builtin_amdgcn_sched_barrier(0);      // (or the scheduler sinks all NR fetches to the end of the body: the first multiply
                fetch(S[k], fsrc, fg + k);              //  of the next trip then waits for a load issued a few cycles before it)
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        mark();
        // acc[rb][j] = GT[p0 + 16 rb + 4 lq + j][(c, n)]: four consecutive features of ONE weight-row quad of sample n
        const bool live = n < D.n_local;
        const uint32_t grp = nb / 16u;
        float e[RB][4];
        if (DBG == 1) {
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) e[rb][0] = e[rb][1] = e[rb][2] = e[rb][3] = 1.0f;
        } else if (NOISE) {
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) {
                const uint32_t p = p0 + 16u * rb + 4u * lq, r = c * D.P + p;
#pragma unroll
                for (int j = 0; j < 4; ++j) e[rb][j] = (live && p < D.P && 16u * rb < rows_m) ? D.noise_in[(size_t)(r + j) * D.n_local + n] : 0.0f;
            }
        } else {
            // RB independent Philox chains with no branch between them (the wave's only latency cover is its own other chains).
            // (Measured instead: the normals stored by dense_xfwd, [n][c][p], and loaded here — 64 MB more traffic and the
            // epilogue no shorter: the loads' latency took the place of the chains'.)
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) {
                const uint32_t p = p0 + 16u * rb + 4u * lq, r = c * D.P + (p < D.P ? p : 0u);
                dense_eps4(D, n, r >> 2, e[rb]);
            }
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) {
                const bool on = live && p0 + 16u * rb + 4u * lq < D.P && 16u * rb < rows_m;
#pragma unroll
                for (int j = 0; j < 4; ++j) e[rb][j] = on ? e[rb][j] : 0.0f;
            }
        }
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {
            const uint32_t p = p0 + 16u * rb + 4u * lq, r = c * D.P + p;
            float v[16];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float gt = acc[rb][j];
                v[j] = e[rb][j] * gt;
                v[4 + j] = gt;
                v[8 + j] = e[rb][j];
                v[12 + j] = e[rb][j] * e[rb][j];
            }
            const float s = xf_row16_reduce16(v, lane);
            // lane lc of the row holds the total of v[lc]: four arrays x the quad's four features
            if (p < D.P && 16u * rb < rows_m) {      // (a short tile's last block slot belongs to the next tile: zero rows, nothing stored)
                float* const dst = (lc < 4u) ? D.ds_part : (lc < 8u ? D.dmu_part : (lc < 12u ? D.s1 : D.s2));
                dst[(size_t)grp * D.R + r + (lc & 3u)] = s;
            }
        }
        mark();
        if (!more) break;
        cb = cb_next;
        bsrc = src_next;
    }
}
