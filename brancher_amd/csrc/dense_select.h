// dense_select.h — which launches an iteration of the dense-link path (dense_kernel.inc, dense_xfused.inc) makes, in which order, with
// which grids, dynamic LDS and derived arguments, and how its workspace is laid out: pure functions of the model, the switches and
// the call.  Host only: no HIP, no look at the environment — dense_kernel.inc fills Switches from the environment
// (dense_read_switches), Model from the descriptor and the device, Call from the launch arguments;
// tests/c_abi/dense_select_table.cpp walks the table without a GPU.
//
// Oddities kept as they were found (the launchers' behaviour is this header's specification):
//  - a knob counts as "off" by its first character being '0' (BSVI_DENSE_XGEMM, _FUSED, _FOLD); BSVI_XF_DEBUG / BSVI_XB_DEBUG are their
//    first character minus '0', masked with 7 / 3; the other three go through atoi.
//  - BSVI_XF_DEBUG applies only to the unweighted forward form with NS * C > 32; values other than 1..6 are the plain kernel.
//  - BSVI_XB_DEBUG applies only without supplied noise, with RB == 7 and B_pad % 256 == 0 — but any non-zero value also forces RB = 7
//    for every form (BSVI_XB_RB: only the value 7 means anything).
//  - BSVI_XF_NS is applied before the epilogue-LDS cap, and ignored when NS * C > 64 (in 32-bit arithmetic).
//  - BSVI_XB_GROUPS is applied before the clamp to C * n_pad / 16; the backward grid is 8 * ceil(groups / 8) * tiles_m (whole XCD
//    shares: the padding workgroups find no column group).
//  - the f32 path's ksplit is 4 or 2, never 1, because n_pad is a multiple of 64; the exact six-launch path's is kXGroups, the fused
//    one's n_pad / 16.
//  - an exact-data model pads the minibatch to 128 rows even when it ends up on the six-launch sequence (B_pad >= 768, BSVI_DENSE_FUSED=0,
//    a refused LDS attribute, or dlog pieces of 4 GB and more).
//  - that 4 GB guard still counts three bf16 planes of dlog although the fused launches now carry f32 (fused_fits: kept, not re-derived).
//  - nine-block tiles of x^T (xb9) need B_pad % 256 == 0 beside their LDS; the LDS bound of create is 150 KiB, the grant 160 KiB.
//  - the sample sums fold into the parameter kernel only on the fused path, with every row parameter on an entry of its own, no
//    BlackBox entropy term, no per-sample values and no caller weights (call_plan's last lines: the conditions as the launchers had them).
//  - the two products of the six-launch sequence are launched by bsvi_xgemm_nt, which selects its own kernel and grid
//    (amort_select.h): their grid and block are 0 here.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace bsvi_dense_select {

// ---- tile constants of the kernels (dense_kernel.inc, dense_xfused.inc use them from here)
constexpr uint32_t XF_ROWS = 64;                     // (sample, class) rows of a dense_xfwd workgroup: two 32-column MFMA blocks
// dense_xfwd after its loop: the 512-row logits tile (row stride NS C | 1 words) + per-quad likelihoods [NS][128] + their partial sums [NS][8]
constexpr uint32_t xf_epilogue_lds(uint32_t NS, uint32_t C) { return (512u * ((NS * C) | 1u) + NS * 136u) * 4u; }
constexpr uint32_t XF_FWD_LDS = 160u * 1024u;        // (the samples per workgroup are capped so that the epilogue fits: call_plan)
constexpr uint32_t XF_MT = 112;                      // rows of x^T resident in dense_xbwd with 7 MFMA blocks of 16 per tile (784 = 7 x 112)
constexpr uint32_t XF_MT9 = 144;                     // ... with 9: 49 row blocks as tiles of 9, 8, 8, 8, 8, 8 (152 KB of LDS at B_pad = 512)
constexpr uint32_t kXbLdsLimit = 150u * 1024u;       // the x^T tile of dense_xbwd must stay below this for the fused launches to be wanted
constexpr uint32_t kXGroups = 4;                     // sample groups of dense_xreduce (dense_rows adds them in order)
constexpr uint32_t kDenseRowChunk = 64;
constexpr uint32_t kDenseKSplit = 4;                 // upper bound; the workspace is sized for it

// One kind per launch the path can make.  The values are public: bsvi_dense_plan returns them.
enum Kind {
    WEIGHTED_SUMS = 0, HEAD, PROLOGUE, GATHER, NOISE,
    FORWARD_1, FORWARD_4, FORWARD_10, FORWARD_16, BACKWARD,
    WSPLIT, XGEMM_LOGITS, CE, XGEMM_GRAD, XREDUCE,
    XFWD_0_1, XFWD_0_2, XFWD_1_2, XFWD_2_2, XFWD_3_2, XFWD_4_2, XFWD_5_2, XFWD_6_2, XFWD_0_1_W, XFWD_0_2_W,
    XBWD_0_2_7, XBWD_0_4_7, XBWD_1_4_7, XBWD_2_4_7, XBWD_3_4_7, XBWD_0_4_9, XBWD_0_2_7_N, XBWD_0_4_7_N, XBWD_0_4_9_N,
    ROWS, ROWS_SLICED, SAMPLE_SUMS, EPILOGUE, PARAM, PARAM_FOLD,
    KIND_COUNT
};
constexpr int XFWD_FIRST = XFWD_0_1, XFWD_COUNT = XFWD_0_2_W - XFWD_0_1 + 1;
constexpr int XBWD_FIRST = XBWD_0_2_7, XBWD_COUNT = XBWD_0_4_9_N - XBWD_0_2_7 + 1;
constexpr int FORWARD_FIRST = FORWARD_1, FORWARD_COUNT = 4;

inline const char* name(int kind) {
    static const char* const names[KIND_COUNT] = {
        "dense_weighted_sums", "dense_head", "dense_prologue", "dense_gather", "dense_noise",
        "dense_forward<1>", "dense_forward<4>", "dense_forward<10>", "dense_forward<16>", "dense_backward",
        "dense_wsplit", "xgemm_nt<logits>", "dense_ce", "xgemm_nt<grad>", "dense_xreduce",
        "dense_xfwd<0,1>", "dense_xfwd<0,2>", "dense_xfwd<1,2>", "dense_xfwd<2,2>", "dense_xfwd<3,2>", "dense_xfwd<4,2>", "dense_xfwd<5,2>",
        "dense_xfwd<6,2>", "dense_xfwd<0,1,w>", "dense_xfwd<0,2,w>",
        "dense_xbwd<0,2,7>", "dense_xbwd<0,4,7>", "dense_xbwd<1,4,7>", "dense_xbwd<2,4,7>", "dense_xbwd<3,4,7>", "dense_xbwd<0,4,9>",
        "dense_xbwd<0,2,7,noise>", "dense_xbwd<0,4,7,noise>", "dense_xbwd<0,4,9,noise>",
        "dense_rows", "dense_rows<sliced>", "dense_sample_sums", "dense_epilogue", "dense_param_kernel", "dense_param_fold_kernel"};
    return kind >= 0 && kind < KIND_COUNT ? names[kind] : "?";
}

// every knob the path reads, at its default
struct Switches {
    bool xgemm = true;          // BSVI_DENSE_XGEMM != 0: exact data on the bf16 matrix cores
    bool fused = true;          // BSVI_DENSE_FUSED != 0: ... as the two fused launches
    bool fold = true;           // BSVI_DENSE_FOLD != 0: the sample sums inside the parameter kernel when the call allows
    uint32_t xf_ns = 0;         // BSVI_XF_NS: samples per dense_xfwd workgroup (0: chosen here)
    int xf_debug = 0;           // BSVI_XF_DEBUG: a profiling form of dense_xfwd
    int xb_debug = 0;           // BSVI_XB_DEBUG: ... of dense_xbwd
    int xb_rb = 0;              // BSVI_XB_RB=7: seven-block tiles of x^T where nine would fit
    uint32_t xb_groups = 0;     // BSVI_XB_GROUPS: column groups of dense_xbwd (0: chosen here)
};

// what bsvi_dense_create knows
struct Model {
    uint32_t C = 1, P = 1, B = 1, DS = 1;
    uint32_t n_params = 0, n_uniform_grad = 0;
    bool exact_data = false;            // every dataset value is exactly a bf16 number (looked at only if wants_exact_scan)
    bool blackbox = false;              // the estimator
    uint32_t base[4] = {0, 0, 0, 0};    // q loc, q scale, prior loc, prior scale: the rows' entries of the uniform table
    uint32_t stride[4] = {0, 0, 0, 0};
    float entropy_weight = 1.0f;
    uint32_t n_cu = 256;
    // device facts, filled after create has walked ModelPlan::attr: did the runtime grant the dynamic LDS?
    bool fused_ok = true, xb9_ok = true;
};

// what a launch knows
struct Call {
    uint32_t n_local = 1;
    bool fvalue_out = false, f_weight = false, q_weight = false, logq_out = false, noise_in = false;
};

enum Path { F32, EXACT_SIX, EXACT_FUSED };
enum AttrClass { ATTR_REGULAR, ATTR_NINE, ATTR_PROFILING };      // refused: no fused launches / no nine-block tiles / nothing happens
struct Attr { Kind kind; uint32_t lds; AttrClass cls; };
struct ModelPlan {
    Path path = F32;            // EXACT_FUSED: wanted — Model::fused_ok and the 4 GB guard of the call decide
    uint32_t P_pad = 0, B_pad = 0, Kp = 0;
    bool xb9 = false;           // nine-block tiles wanted
    uint32_t n_attr = 0;
    Attr attr[XFWD_COUNT + XBWD_COUNT];
};

// is the dataset worth a look?  (the exact-data path needs whole Philox quads of features and a full k step)
inline bool wants_exact_scan(const Model& m, const Switches& sw) { return sw.xgemm && m.P % 4 == 0 && m.P >= 32; }

inline ModelPlan model_plan(const Model& m, const Switches& sw) {
    ModelPlan mp;
    mp.P_pad = (m.P + 63) / 64 * 64;
    mp.B_pad = (m.B + 63) / 64 * 64;
    mp.Kp = (m.P + 31) / 32 * 32;
    if (!(wants_exact_scan(m, sw) && m.exact_data)) return mp;
    mp.B_pad = (m.B + 127) / 128 * 128;          // dense_xbwd walks the minibatch axis in steps of 128
    const uint32_t row = mp.B_pad * 2 + 32;      // bytes of a row of the x^T tile
    mp.path = sw.fused && (size_t)XF_MT * row <= kXbLdsLimit ? EXACT_FUSED : EXACT_SIX;
    mp.xb9 = (size_t)XF_MT9 * row <= kXbLdsLimit && mp.B_pad % 256u == 0u;
    if (mp.path != EXACT_FUSED) return mp;
    auto want = [&](int kind, uint32_t lds, AttrClass cls) { mp.attr[mp.n_attr++] = Attr{(Kind)kind, lds, cls}; };
    for (int k = XFWD_0_1; k <= XFWD_0_2_W; ++k) want(k, XF_FWD_LDS, k >= XFWD_3_2 && k <= XFWD_6_2 ? ATTR_PROFILING : ATTR_REGULAR);
    for (int k = XBWD_0_2_7; k <= XBWD_0_4_9_N; ++k) {
        const bool nine = k == XBWD_0_4_9 || k == XBWD_0_4_9_N;
        if (!nine || mp.xb9) want(k, (uint32_t)((nine ? XF_MT9 : XF_MT) * row), nine ? ATTR_NINE : ATTR_REGULAR);
    }
    return mp;
}

// the fused launches address the dlog pieces with 32-bit buffer offsets: beyond 4 GB of pieces the six-launch sequence serves
inline bool fused_fits(uint32_t n_pad, uint32_t C, uint32_t B_pad) { return 3ull * n_pad * C * B_pad * 2ull < (1ull << 32); }

// arg: dense_head {n_noise, n_tiles}; dense_xfwd {NS}; dense_xbwd {tiles_m, groups, rb_base, rb_extra}; dense_sample_sums {with_q};
// dense_param_fold_kernel {row_blocks}
struct Launch {
    Kind kind;
    uint32_t grid_x, grid_y, block, lds;
    uint32_t arg[4];
};
struct Plan {
    bool exact = false, xfused = false;      // the path this call takes: f32 kernels / six launches / two fused launches
    uint32_t P_pad = 0, B_pad = 0, Kp = 0, R = 0, n_pad = 0;
    uint32_t ksplit = 0, lik_parts = 0, per_sample = 0;
    bool sums_folded = false;                // the DParams of dense_epilogue / dense_param_fold_kernel carry sums_folded = 1
    uint32_t n = 0;
    Launch launch[12];
};

inline Plan call_plan(const Model& m, const Switches& sw, const Call& c) {
    const ModelPlan mp = model_plan(m, sw);
    Plan pl;
    const uint32_t C = m.C, P = m.P, Bp = pl.B_pad = mp.B_pad, Pp = pl.P_pad = mp.P_pad;
    const uint32_t R = pl.R = (uint32_t)((uint64_t)C * P), np = pl.n_pad = (c.n_local + 63) / 64 * 64;
    pl.Kp = mp.Kp;
    pl.exact = mp.path != F32;
    pl.xfused = mp.path == EXACT_FUSED && m.fused_ok && fused_fits(np, C, Bp);
    pl.per_sample = (c.fvalue_out || m.blackbox) ? 1u : 0u;
    pl.sums_folded = pl.exact || pl.per_sample;      // dense_wsplit / dense_sample_sums wrote the per-sample sums whole
    // f32: as many sample splits (<= kDenseKSplit) as keep each a multiple of the 32-sample step
    pl.ksplit = 1;
    for (uint32_t k = kDenseKSplit; k >= 1; k >>= 1)
        if (np % (32 * k) == 0) { pl.ksplit = k; break; }
    if (pl.exact) pl.ksplit = kXGroups;
    if (pl.xfused) pl.ksplit = np / 16;              // dense_xbwd: one partial per block of 16 samples (dense_rows adds them in order)
    pl.lik_parts = pl.xfused ? (Bp + 511) / 512 : Bp / 64;
    auto add = [&](int kind, uint32_t grid_x, uint32_t block = 256) -> Launch& {
        Launch& l = pl.launch[pl.n++];
        l = Launch{(Kind)kind, grid_x, 1, block, 0, {0, 0, 0, 0}};
        return l;
    };
    const uint32_t n_tiles = (Bp / 64) * (Pp / 64), n_rowp = (R + 255) / 256, n_param = ((m.n_params ? m.n_params : 1) + 255) / 256;
    const uint32_t with_q = (m.blackbox && m.entropy_weight != 0.0f) ? 1u : 0u;
    // (caller-weighted gradients: the weighted row sums depend on nothing the iteration writes)
    if (c.f_weight) add(WEIGHTED_SUMS, n_rowp);
    if (!pl.exact) {
        const uint32_t noise_x = np / 256 ? (np + 255) / 256 : 1, noise_y = (R + kDenseRowChunk - 1) / kDenseRowChunk;
        if (!pl.per_sample) {
            // the three heads are independent: one launch of heterogeneous workgroups
            Launch& h = add(HEAD, noise_x * noise_y + n_tiles + n_rowp);
            h.arg[0] = noise_x * noise_y; h.arg[1] = n_tiles;
        } else {
            // per-sample prior values wanted: the noise kernel reads the row parameters, so the heads run in order
            const uint32_t work0 = R > Bp ? R : Bp, work1 = Bp * Pp;
            add(PROLOGUE, (work0 + 255) / 256);
            add(GATHER, (work1 + 255) / 256 > 2048 ? 2048 : (work1 + 255) / 256);
            add(NOISE, noise_x).grid_y = noise_y;
        }
        add(C == 1 ? FORWARD_1 : C <= 4 ? FORWARD_4 : C <= 10 ? FORWARD_10 : FORWARD_16, (np / 16) * (Bp / 64));
        add(BACKWARD, C * ((P + 63) / 64) * pl.ksplit * (Bp / 64));
        add(ROWS, n_rowp);
        if (pl.per_sample) add(SAMPLE_SUMS, np / 64).arg[0] = with_q;
        add(EPILOGUE, 1, 1024);
        add(PARAM, n_param);
        return pl;
    }
    // row parameters and the minibatch (with its bf16 copies) in one launch of heterogeneous workgroups, no noise blocks
    add(HEAD, n_tiles + n_rowp).arg[1] = n_tiles;
    if (!pl.xfused) {
        // W pieces | logits product | likelihood and dlog pieces | gradient product | reduction against eps | the common tail
        add(WSPLIT, np);
        add(XGEMM_LOGITS, 0, 0);
        add(CE, (Bp / 64) * (np / 8));
        add(XGEMM_GRAD, 0, 0);
        add(XREDUCE, (P / 4) * kXGroups);
        add(ROWS, n_rowp);
        add(EPILOGUE, 1, 1024);
        add(PARAM, n_param);
        return pl;
    }
    // [per-sample prior sums] | draw + logits product + likelihood | gradient product + reduction against eps | the tail
    if (pl.per_sample) add(WSPLIT, np);      // (sums only)
    // samples per workgroup: as many as fill the 64 rows of W, but no fewer workgroups than CUs
    // (BSVI_XF_NS: measurements.  cfg 4, C = 10: NS = 3 / 4 / 5 / 6 -> 154.7 / 138.1 / 147.6 / 148.4 us per iteration — one workgroup
    //  per CU beats fuller 64-row tiles on fewer CUs, and 32-row tiles on 1.33 rounds of workgroups)
    uint32_t NS = XF_ROWS / C;
    const uint32_t want = np / m.n_cu;
    if (NS > want) NS = want ? want : 1u;
    if (sw.xf_ns && sw.xf_ns * C <= XF_ROWS) NS = sw.xf_ns;
    while (NS > 1u && xf_epilogue_lds(NS, C) > XF_FWD_LDS) --NS;
    const bool one_block = NS * C <= 32u;
    const int fdbg = sw.xf_debug >= 1 && sw.xf_debug <= 6 ? sw.xf_debug : 0;
    Launch& f = add(c.f_weight ? (one_block ? XFWD_0_1_W : XFWD_0_2_W) : one_block ? XFWD_0_1 : XFWD_0_2 + fdbg, (np + NS - 1) / NS, 512);
    f.grid_y = (Bp + 511) / 512; f.lds = XF_FWD_LDS; f.arg[0] = NS;
    // feature tiles of RB 16-row blocks of x^T: nine when they fit LDS (BSVI_XB_RB=7: seven), the P / 16 blocks dealt out evenly
    const uint32_t RB = (mp.xb9 && m.xb9_ok && sw.xb_debug == 0 && sw.xb_rb != 7) ? 9u : 7u;
    const uint32_t nrb = (P + 15u) / 16u, tiles_m = (nrb + RB - 1u) / RB;
    // One workgroup per CU (its x^T tile takes 118 / 152 KB of LDS), and workgroup i runs on XCD i % 8: the column groups of ONE XCD
    // times the feature tiles must fit that XCD's n_cu / 8 CUs (36 -> 32 groups at cfg 4: 66.3 -> 36.9 us, profiles/r5/xbwd_groups.txt)
    const uint32_t cu_per_xcd = m.n_cu >= 8u ? m.n_cu / 8u : 1u, total_cb = C * (np / 16);
    uint32_t groups = 8u * (cu_per_xcd / tiles_m);
    if (!groups) groups = m.n_cu / tiles_m;
    if (sw.xb_groups) groups = sw.xb_groups;
    if (groups > total_cb) groups = total_cb;
    if (!groups) groups = 1;
    // (groups of two k steps in a ring of four register sets when B_pad is a multiple of 256; B_pad = 128 (mod 256): a ring of two)
    const bool ring4 = Bp % 256u == 0u;
    const int bdbg = sw.xb_debug >= 1 && sw.xb_debug <= 3 ? sw.xb_debug : 0;
    Launch& b = add(c.noise_in ? (RB == 9u ? XBWD_0_4_9_N : ring4 ? XBWD_0_4_7_N : XBWD_0_2_7_N)
                               : RB == 9u ? XBWD_0_4_9 : ring4 ? XBWD_0_4_7 + bdbg : XBWD_0_2_7,
                    8 * ((groups + 7) / 8) * tiles_m, 512);
    b.lds = 16u * RB * (Bp * 2 + 32);
    b.arg[0] = tiles_m; b.arg[1] = groups; b.arg[2] = nrb / tiles_m; b.arg[3] = nrb % tiles_m;
    add(ROWS_SLICED, (R + 63) / 64);         // 64 rows per workgroup
    // the epilogue's sums inside the parameter kernel when nothing but the plain value is asked of it
    const uint32_t nug = m.n_uniform_grad;
    bool own_entries = true;
    for (int i = 0; i < 4; ++i) own_entries = own_entries && (m.stride[i] || m.base[i] >= nug);
    if (sw.fold && own_entries && !with_q && !pl.per_sample && !c.f_weight && !c.fvalue_out && !c.logq_out) {
        add(PARAM_FOLD, n_param).arg[0] = (R + 63) / 64;
        return pl;
    }
    add(EPILOGUE, 1, 1024);
    add(PARAM, n_param);
    return pl;
}

// ---- the workspace: byte offsets of every region, in this order, each 256-byte aligned
struct Layout {
    size_t rowp, idx, Xb, XbT, lab, eps, pv_part, qv_part, s1, s2, lik_part, dlog;
    size_t Xb_bf, XbT_bf, Wp, logitsT, dlogp, GT;      // the exact-data paths' (0 on the f32 path)
    size_t ds_part, dmu_part, rowg, hpart, partial, wsum, ws1, ws2, total;
};
inline Layout layout(const Model& m, const Plan& pl) {
    Layout L;
    const size_t R = pl.R, np = pl.n_pad, Bp = pl.B_pad, Pp = pl.P_pad, C = m.C;
    const bool fused = pl.xfused;
    size_t o = 0;
    auto take = [&](size_t floats) { size_t at = o; o += (floats * 4 + 255) / 256 * 256; return at; };
    L.rowp = take(6 * R + 64);                 // mu, s, mu0, s0, {mu, s} interleaved (+ slack rows)
    L.idx = take(Bp);
    L.Xb = take(Bp * Pp);
    L.XbT = take(Pp * Bp + 128);               // forward tiles are 128 columns wide: slack is only read
    L.lab = take(Bp);
    // (the exact-data path stores neither eps nor the f32 dlog: it has the pieces below instead)
    L.eps = take(pl.exact ? 64 : (R + 32) * np);                // 32 rows of slack: the last feature chunk reads past P
    L.pv_part = take(((R + kDenseRowChunk - 1) / kDenseRowChunk) * np);
    L.qv_part = take(m.blackbox ? ((R + kDenseRowChunk - 1) / kDenseRowChunk) * np : 1);
    const size_t xgroups = fused ? np / 16 : kDenseKSplit;       // sample groups of dense_xbwd's partial sums
    L.s1 = take(xgroups * R);
    L.s2 = take(xgroups * R);
    L.lik_part = take((Bp / 32) * np);
    L.dlog = take(pl.exact ? 64 : C * np * Bp);
    if (pl.exact) {
        const size_t Kp = pl.Kp, NC = np * C;
        L.Xb_bf = take((Bp * Kp + 1) / 2 + 64);
        L.XbT_bf = take(((size_t)m.P * Bp + 1) / 2 + 64);
        L.Wp = take(fused ? 64 : (3 * NC * Kp + 1) / 2 + 64);
        L.logitsT = take(fused ? 64 : Bp * NC);
        L.dlogp = take((3 * NC * Bp + 1) / 2 + 64);
        L.GT = take(fused ? 64 : (size_t)m.P * NC);
    } else {
        L.Xb_bf = L.XbT_bf = L.Wp = L.logitsT = L.dlogp = L.GT = 0;
    }
    L.ds_part = take((fused ? xgroups : kDenseKSplit * (Bp / 64)) * R);
    L.dmu_part = take((fused ? xgroups : kDenseKSplit * (Bp / 64)) * R);
    L.rowg = take(4 * R);
    L.hpart = take(3 * ((R + 63) / 64));
    L.partial = take(2 + (size_t)m.n_uniform_grad);
    L.wsum = take(2);                          // caller-weighted gradients: A, B and the weighted row sums (dense_weighted_sums)
    L.ws1 = take(R + 4);
    L.ws2 = take(R + 4);
    L.total = o + 256;
    return L;
}

}  // namespace bsvi_dense_select
