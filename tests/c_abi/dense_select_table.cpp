// The launch plan of the dense-link path (brancher_amd/csrc/dense_select.h): the rows that tests/test_gpu_dense_fused.py runs on the
// device (printed so that the two lists are compared), both sides of every threshold, a sweep of the plan's invariants and every
// switch flipped once.  The expected kinds and numbers were worked out by hand from the launchers' conditions as they stood before
// the header — not from the functions under test.  Exit status 0: everything holds; 1 otherwise, with each row that does not printed.
#include <stdio.h>
#include <string.h>

#include <initializer_list>
#include <string>

#include "dense_select.h"

using namespace bsvi_dense_select;

static int g_failures = 0;
static void expect(const char* what, bool ok) {
    if (ok) return;
    if (++g_failures < 40) printf("FAILED: %s\n", what);
}

// a logistic-regression model as the device test builds it: pixel data (exactly bf16), every row parameter on an entry of its own,
// on a device of 256 CUs that grants every LDS attribute
static Model model(uint32_t DS, uint32_t B, uint32_t P, uint32_t C) {
    Model m;
    m.C = C; m.P = P; m.B = B; m.DS = DS;
    m.exact_data = true;
    m.n_params = 2 * C * P; m.n_uniform_grad = 2 * C * P;
    for (int i = 0; i < 4; ++i) { m.base[i] = (i & 1) * C * P; m.stride[i] = 1; }
    return m;
}
static Call call(uint32_t n, const char* what = "plain") {
    Call c;
    c.n_local = n;
    c.fvalue_out = strstr(what, "fvalues") != nullptr;
    c.noise_in = strstr(what, "noise") != nullptr;
    c.f_weight = strstr(what, "weighted") != nullptr;
    return c;
}
static std::string kinds_of(const Plan& pl) {
    std::string s;
    for (uint32_t i = 0; i < pl.n; ++i) s += std::string(i ? " " : "") + name(pl.launch[i].kind);
    return s;
}
static const Launch* find(const Plan& pl, int first, int last) {
    for (uint32_t i = 0; i < pl.n; ++i)
        if (pl.launch[i].kind >= first && pl.launch[i].kind <= last) return &pl.launch[i];
    return nullptr;
}
static const Launch* find(const Plan& pl, int kind) { return find(pl, kind, kind); }
static bool has(const Plan& pl, int kind) { return find(pl, kind) != nullptr; }
static bool launch_is(const Launch* l, uint32_t gx, uint32_t gy, uint32_t block, uint32_t lds, uint32_t a0 = 0, uint32_t a1 = 0, uint32_t a2 = 0, uint32_t a3 = 0) {
    return l && l->grid_x == gx && l->grid_y == gy && l->block == block && l->lds == lds && l->arg[0] == a0 && l->arg[1] == a1 && l->arg[2] == a2 && l->arg[3] == a3;
}
static Plan device_row(uint32_t DS, uint32_t B, uint32_t P, uint32_t C, uint32_t n, const char* env, const Switches& sw, const char* what, const char* expected) {
    const Plan pl = call_plan(model(DS, B, P, C), sw, call(n, what));
    if (kinds_of(pl) != expected) {
        ++g_failures;
        printf("FAILED: row (%u, %u, %u, %u, %u) %s %s: expected %s, got %s\n", DS, B, P, C, n, env, what, expected, kinds_of(pl).c_str());
    }
    printf("device-row %u %u %u %u %u %s %s %s\n", DS, B, P, C, n, env, what, expected);
    return pl;
}

int main() {
    const Switches def;
    // ---- the device test's rows: (dataset, batch, features, classes, samples), the environment, the call, the launches in order
    {
        Switches rb7, ns4, f32, nofold;
        rb7.xb_rb = 7; ns4.xf_ns = 4; f32.xgemm = false; nofold.fold = false;
        // B_pad = 128: a ring of two, seven-block tiles; 64 samples on 256 CUs: one sample per workgroup
        Plan pl = device_row(64, 32, 32, 1, 50, "-", def, "fvalues",
                             "dense_head dense_wsplit dense_xfwd<0,1> dense_xbwd<0,2,7> dense_rows<sliced> dense_epilogue dense_param_kernel");
        expect("row 1: head of 2 minibatch tiles and 1 block of row parameters", launch_is(find(pl, HEAD), 3, 1, 256, 0, 0, 2));
        expect("row 1: wsplit per padded sample", launch_is(find(pl, WSPLIT), 64, 1, 256, 0));
        expect("row 1: xfwd, 64 workgroups of one sample", launch_is(find(pl, XFWD_0_1), 64, 1, 512, 160 * 1024, 1));
        expect("row 1: xbwd, 2 row blocks in one tile, 4 column groups, a grid of 8", launch_is(find(pl, XBWD_0_2_7), 8, 1, 512, 16 * 7 * (128 * 2 + 32), 1, 4, 2, 0));
        expect("row 1: tail", launch_is(find(pl, ROWS_SLICED), 1, 1, 256, 0) && launch_is(find(pl, EPILOGUE), 1, 1, 1024, 0) && launch_is(find(pl, PARAM), 1, 1, 256, 0));
        expect("row 1: scalars", pl.exact && pl.xfused && pl.B_pad == 128 && pl.P_pad == 64 && pl.Kp == 32 && pl.n_pad == 64 && pl.ksplit == 4 && pl.lik_parts == 1 &&
               pl.per_sample == 1 && pl.sums_folded);
        // B_pad = 256: nine-block tiles fit (144 * 544 bytes), a ring of four
        pl = device_row(256, 200, 32, 3, 24, "-", def, "fvalues", "dense_head dense_wsplit dense_xfwd<0,1> dense_xbwd<0,4,9> dense_rows<sliced> dense_epilogue dense_param_kernel");
        expect("row 2: xbwd<0,4,9>: 2 row blocks in one tile, 3 * 4 column groups, 16 workgroups", launch_is(find(pl, XBWD_0_4_9), 16, 1, 512, 16 * 9 * 544, 1, 12, 2, 0));
        pl = device_row(256, 200, 32, 3, 24, "BSVI_XB_RB=7", rb7, "fvalues", "dense_head dense_wsplit dense_xfwd<0,1> dense_xbwd<0,4,7> dense_rows<sliced> dense_epilogue dense_param_kernel");
        expect("row 3: seven-block LDS", launch_is(find(pl, XBWD_0_4_7), 16, 1, 512, 16 * 7 * 544, 1, 12, 2, 0));
        device_row(256, 200, 32, 3, 24, "-", def, "fvalues+noise", "dense_head dense_wsplit dense_xfwd<0,1> dense_xbwd<0,4,9,noise> dense_rows<sliced> dense_epilogue dense_param_kernel");
        // config 4's forward instantiation at 24 samples: four samples of ten classes per workgroup
        pl = device_row(96, 40, 784, 10, 24, "BSVI_XF_NS=4", ns4, "fvalues", "dense_head dense_wsplit dense_xfwd<0,2> dense_xbwd<0,2,7> dense_rows<sliced> dense_epilogue dense_param_kernel");
        expect("row 5: head of 2 x 13 tiles and 31 blocks of row parameters", launch_is(find(pl, HEAD), 57, 1, 256, 0, 0, 26));
        expect("row 5: xfwd<0,2>, 16 workgroups of four samples", launch_is(find(pl, XFWD_0_2), 16, 1, 512, 160 * 1024, 4));
        expect("row 5: xbwd, 49 row blocks in 7 tiles of 7, 8 * (32 / 7) = 32 groups", launch_is(find(pl, XBWD_0_2_7), 224, 1, 512, 32256, 7, 32, 7, 0));
        expect("row 5: rows in slices of 64", launch_is(find(pl, ROWS_SLICED), 123, 1, 256, 0) && launch_is(find(pl, PARAM), 62, 1, 256, 0));
        // B_pad = 768: 112 * 1568 bytes of x^T pass 150 KiB — the six-launch sequence, by itself
        pl = device_row(700, 650, 32, 1, 20, "-", def, "fvalues",
                        "dense_head dense_wsplit xgemm_nt<logits> dense_ce xgemm_nt<grad> dense_xreduce dense_rows dense_epilogue dense_param_kernel");
        expect("row 6: scalars", pl.exact && !pl.xfused && pl.B_pad == 768 && pl.ksplit == 4 && pl.lik_parts == 12 && pl.sums_folded);
        expect("row 6: grids", launch_is(find(pl, HEAD), 13, 1, 256, 0, 0, 12) && launch_is(find(pl, WSPLIT), 64, 1, 256, 0) && launch_is(find(pl, CE), 12 * 8, 1, 256, 0) &&
               launch_is(find(pl, XREDUCE), 8 * 4, 1, 256, 0) && launch_is(find(pl, ROWS), 1, 1, 256, 0) && launch_is(find(pl, XGEMM_LOGITS), 0, 1, 0, 0));
        // 30 features: no whole k step — the f32 kernels; three heads in order with per-sample values, one launch without
        pl = device_row(64, 32, 30, 3, 20, "-", def, "fvalues",
                        "dense_prologue dense_gather dense_noise dense_forward<4> dense_backward dense_rows dense_sample_sums dense_epilogue dense_param_kernel");
        expect("row 7: grids", launch_is(find(pl, PROLOGUE), 1, 1, 256, 0) && launch_is(find(pl, GATHER), 16, 1, 256, 0) && launch_is(find(pl, NOISE), 1, 2, 256, 0) &&
               launch_is(find(pl, FORWARD_4), 4, 1, 256, 0) && launch_is(find(pl, BACKWARD), 3 * 1 * 2 * 1, 1, 256, 0) && launch_is(find(pl, SAMPLE_SUMS), 1, 1, 256, 0, 0));
        expect("row 7: scalars", !pl.exact && !pl.xfused && pl.B_pad == 64 && pl.P_pad == 64 && pl.ksplit == 2 && pl.lik_parts == 1 && pl.per_sample == 1 && pl.sums_folded);
        pl = device_row(64, 32, 30, 3, 20, "-", def, "plain", "dense_head dense_forward<4> dense_backward dense_rows dense_epilogue dense_param_kernel");
        expect("row 8: one head: 2 noise blocks, 1 tile, 1 block of row parameters; sums not folded", launch_is(find(pl, HEAD), 4, 1, 256, 0, 2, 1) && !pl.sums_folded && !pl.per_sample);
        device_row(64, 32, 32, 16, 20, "BSVI_DENSE_XGEMM=0", f32, "fvalues",
                   "dense_prologue dense_gather dense_noise dense_forward<16> dense_backward dense_rows dense_sample_sums dense_epilogue dense_param_kernel");
        // nothing but the plain value asked: the sample sums inside the parameter kernel
        pl = device_row(96, 40, 784, 10, 24, "-", def, "plain", "dense_head dense_xfwd<0,1> dense_xbwd<0,2,7> dense_rows<sliced> dense_param_fold_kernel");
        expect("row 10: the folded parameter kernel over 123 row blocks", launch_is(find(pl, PARAM_FOLD), 62, 1, 256, 0, 123) && pl.sums_folded && !pl.per_sample);
        device_row(96, 40, 784, 10, 24, "BSVI_DENSE_FOLD=0", nofold, "plain", "dense_head dense_xfwd<0,1> dense_xbwd<0,2,7> dense_rows<sliced> dense_epilogue dense_param_kernel");
    }
    // the weighted instantiations (caller weights: no device row)
    expect("weighted, one block", kinds_of(call_plan(model(96, 40, 784, 10), def, call(24, "weighted"))) ==
           "dense_weighted_sums dense_head dense_xfwd<0,1,w> dense_xbwd<0,2,7> dense_rows<sliced> dense_epilogue dense_param_kernel");
    expect("weighted, two blocks", has(call_plan(model(96, 40, 784, 10), def, call(1024, "weighted")), XFWD_0_2_W));
    {
        const Plan pl = call_plan(model(64, 32, 30, 3), def, call(20, "weighted"));
        expect("weighted sums first on the f32 path too", pl.launch[0].kind == WEIGHTED_SUMS && launch_is(&pl.launch[0], 1, 1, 256, 0));
    }

    // ---- both sides of every threshold
    // (1) 32 features and whole quads of them
    expect("P = 28 is not exact data's", model_plan(model(64, 32, 28, 3), def).path == F32 && model_plan(model(64, 32, 32, 3), def).path == EXACT_FUSED);
    expect("P % 4", model_plan(model(64, 32, 34, 3), def).path == F32 && model_plan(model(64, 32, 36, 3), def).path == EXACT_FUSED);
    expect("paddings: 64 rows on the f32 path, 128 on the exact ones; features to 64 and to the k step of 32", model_plan(model(64, 32, 34, 3), def).B_pad == 64 &&
           model_plan(model(64, 32, 36, 3), def).B_pad == 128 && model_plan(model(64, 32, 36, 3), def).P_pad == 64 && model_plan(model(64, 32, 36, 3), def).Kp == 64 &&
           model_plan(model(200, 130, 100, 3), def).B_pad == 256 && model_plan(model(200, 129, 100, 3), def).Kp == 128);
    {   // inexact data
        Model m = model(64, 32, 32, 3);
        m.exact_data = false;
        expect("inexact data", model_plan(m, def).path == F32 && model_plan(m, def).n_attr == 0);
    }
    // (2) nine-block tiles: 144 * (2 B_pad + 32) <= 150 KiB and B_pad % 256 == 0; (3) the fused launches: 112 * (2 B_pad + 32) <= 150 KiB
    expect("xb9 at B_pad = 512, not at 768", model_plan(model(2048, 512, 64, 3), def).xb9 && !model_plan(model(2048, 768, 64, 3), def).xb9);
    expect("xb9 not at B_pad = 384 or 640", !model_plan(model(2048, 384, 64, 3), def).xb9 && !model_plan(model(2048, 640, 64, 3), def).xb9);
    expect("fused at B_pad = 640, six launches at 768", model_plan(model(2048, 640, 64, 3), def).path == EXACT_FUSED && model_plan(model(2048, 641, 64, 3), def).path == EXACT_SIX &&
           model_plan(model(2048, 641, 64, 3), def).B_pad == 768);
    expect("attributes: 17 kinds without the nine-block pair, 19 with; none off the fused path", model_plan(model(2048, 640, 64, 3), def).n_attr == 17 &&
           model_plan(model(2048, 512, 64, 3), def).n_attr == 19 && model_plan(model(2048, 768, 64, 3), def).n_attr == 0);
    {
        const ModelPlan mp = model_plan(model(2048, 512, 64, 3), def);
        int regular = 0, nine = 0, prof = 0;
        for (uint32_t i = 0; i < mp.n_attr; ++i) {
            const Attr& a = mp.attr[i];
            regular += a.cls == ATTR_REGULAR; nine += a.cls == ATTR_NINE; prof += a.cls == ATTR_PROFILING;
            const bool fwd = a.kind >= XFWD_FIRST && a.kind < XFWD_FIRST + XFWD_COUNT;
            expect("attribute sizes", a.lds == (fwd ? 160u * 1024u : a.cls == ATTR_NINE ? 144u * 1056u : 112u * 1056u));
            expect("attribute classes", (a.cls == ATTR_NINE) == (a.kind == XBWD_0_4_9 || a.kind == XBWD_0_4_9_N) && (a.cls == ATTR_PROFILING) == (a.kind >= XFWD_3_2 && a.kind <= XFWD_6_2));
        }
        expect("13 regular, 2 nine-block, 4 profiling kinds", regular == 13 && nine == 2 && prof == 4);
    }
    {   // a refused attribute
        Model m = model(2048, 512, 64, 3);
        m.xb9_ok = false;
        expect("nine-block tiles refused: seven", has(call_plan(m, def, call(64)), XBWD_0_4_7));
        m.fused_ok = false;
        expect("fused launches refused: six launches, still 128-row padding", has(call_plan(m, def, call(64)), XREDUCE) && call_plan(m, def, call(64)).B_pad == 512 &&
               call_plan(model(64, 32, 32, 3), def, call(64)).B_pad == 128);
    }
    // (4) one or two 32-column blocks of (sample, class) rows: NS * C = 32 / 33
    {
        Switches sw;
        sw.xf_ns = 2;
        expect("NS C = 32", launch_is(find(call_plan(model(64, 32, 32, 16), sw, call(1024)), XFWD_0_1), 512, 1, 512, 160 * 1024, 2));
        sw.xf_ns = 3;
        expect("NS C = 33", launch_is(find(call_plan(model(64, 32, 32, 11), sw, call(1024)), XFWD_0_2), 342, 1, 512, 160 * 1024, 3));
    }
    // (5) samples per workgroup: n_pad / n_cu = 0, 1, 2 (and at most 64 / C)
    expect("n_pad / n_cu = 0 and 1: one sample", find(call_plan(model(64, 32, 32, 3), def, call(192)), XFWD_FIRST, XFWD_0_2_W)->arg[0] == 1 &&
           find(call_plan(model(64, 32, 32, 3), def, call(256)), XFWD_FIRST, XFWD_0_2_W)->arg[0] == 1);
    expect("n_pad / n_cu = 2", find(call_plan(model(64, 32, 32, 3), def, call(512)), XFWD_FIRST, XFWD_0_2_W)->arg[0] == 2);
    expect("64 / C caps it", find(call_plan(model(64, 32, 32, 10), def, call(4096)), XFWD_FIRST, XFWD_0_2_W)->arg[0] == 6 && has(call_plan(model(64, 32, 32, 10), def, call(4096)), XFWD_0_2));
    // (6) the f32 path's sample splits: n_pad = 64 / 128 / 192
    expect("ksplit 2 / 4 / 2", call_plan(model(64, 32, 30, 3), def, call(64)).ksplit == 2 && call_plan(model(64, 32, 30, 3), def, call(65)).ksplit == 4 &&
           call_plan(model(64, 32, 30, 3), def, call(192)).ksplit == 2 && call_plan(model(64, 32, 32, 3), def, call(192)).ksplit == 12);
    // (7) the 4 GB guard: 3 * n_pad * 16 * 128 * 2 bytes of dlog pieces below 2^32: n_pad = 349 504 passes, 349 568 does not
    {
        const Plan in = call_plan(model(64, 32, 32, 16), def, call(349504)), out = call_plan(model(64, 32, 32, 16), def, call(349505));
        expect("4 GB guard", in.xfused && in.ksplit == 349504 / 16 && !out.xfused && out.exact && out.ksplit == 4 && out.n_pad == 349568 && has(out, XREDUCE) && !has(in, XREDUCE));
        expect("fused_fits", fused_fits(349504, 16, 128) && !fused_fits(349568, 16, 128));
        const Layout a = layout(model(64, 32, 32, 16), in), b = layout(model(64, 32, 32, 16), out);
        expect("the six-launch sequence stores W, logits and GT", a.logitsT - a.Wp == 256 && a.total < b.total && b.logitsT - b.Wp > (size_t)3 * 349568 * 16 * 32);
    }
    // (8) the forward kernel of the f32 path by classes: 1 / 2, 4 / 5, 10 / 11
    {
        const int want[17] = {0, FORWARD_1, FORWARD_4, FORWARD_4, FORWARD_4, FORWARD_10, FORWARD_10, FORWARD_10, FORWARD_10, FORWARD_10, FORWARD_10,
                              FORWARD_16, FORWARD_16, FORWARD_16, FORWARD_16, FORWARD_16, FORWARD_16};
        for (uint32_t C = 1; C <= 16; ++C) expect("dense_forward<CT>", has(call_plan(model(64, 32, 30, C), def, call(20)), want[C]));
    }
    // (9) the fold: every condition on its own
    {
        Model m = model(96, 40, 784, 10);
        expect("fold", has(call_plan(m, def, call(24)), PARAM_FOLD));
        expect("no fold with per-sample values", !has(call_plan(m, def, call(24, "fvalues")), PARAM_FOLD));
        expect("no fold with caller weights", !has(call_plan(m, def, call(24, "weighted")), PARAM_FOLD));
        expect("fold with supplied noise", has(call_plan(m, def, call(24, "noise")), PARAM_FOLD));
        m.blackbox = true;
        expect("no fold under BlackBox (per-sample values)", !has(call_plan(m, def, call(24)), PARAM_FOLD) && has(call_plan(m, def, call(24)), WSPLIT));
        m = model(96, 40, 784, 10); m.stride[2] = 0; m.base[2] = m.n_uniform_grad - 1;
        expect("no fold with a shared learnable entry", !has(call_plan(m, def, call(24)), PARAM_FOLD));
        m.base[2] = m.n_uniform_grad;
        expect("fold with a shared constant", has(call_plan(m, def, call(24)), PARAM_FOLD));
        expect("no fold off the fused path", !has(call_plan(model(64, 32, 30, 3), def, call(24)), PARAM_FOLD) && !has(call_plan(model(2048, 768, 64, 3), def, call(24)), PARAM_FOLD));
        m = model(64, 32, 30, 3); m.blackbox = true;
        expect("with_q: BlackBox with an entropy term", find(call_plan(m, def, call(20)), SAMPLE_SUMS)->arg[0] == 1);
        m.entropy_weight = 0.0f;
        expect("with_q: not without", find(call_plan(m, def, call(20)), SAMPLE_SUMS)->arg[0] == 0);
    }

    // ---- a sweep of the invariants
    long plans = 0;
    const uint32_t Bs[] = {1, 64, 65, 128, 129, 256, 300, 512, 640, 641, 2048}, Ps[] = {1, 28, 32, 36, 100, 236, 784, 4096}, Ns[] = {1, 64, 65, 300, 1024, 5000, 200000};
    const uint32_t cus[] = {1, 7, 8, 64, 256, 304};
    for (uint32_t C = 1; C <= 16; ++C)
        for (uint32_t P : Ps)
            for (uint32_t B : Bs)
                for (uint32_t n : Ns)
                    for (uint32_t n_cu : cus)
                        for (int v = 0; v < 16; ++v) {
                            Model m = model(2048, B, P, C);
                            m.n_cu = n_cu; m.blackbox = v & 1; m.xb9_ok = !(v & 2); m.fused_ok = v != 7;
                            Switches sw;
                            if (v & 4) { sw.xf_ns = 1 + (v >> 2) * 3; sw.xb_groups = v == 12 ? 1000000u : 5u; }
                            if (v & 8) { sw.xb_debug = v & 3; sw.xf_debug = v & 7; }
                            Call c = call(n, v % 3 == 0 ? "plain" : v % 3 == 1 ? "fvalues" : "noise");
                            c.f_weight = c.q_weight = v == 5;
                            const ModelPlan mp = model_plan(m, sw);
                            const Plan pl = call_plan(m, sw, c);
                            const Layout L = layout(m, pl);
                            ++plans;
                            bool ok = pl.n >= 5 && pl.n <= 10 && pl.n_pad % 64 == 0 && pl.n_pad >= n && pl.n_pad - n < 64;
                            for (uint32_t i = 0; i < pl.n; ++i) {
                                const Launch& l = pl.launch[i];
                                if (l.lds) {      // the plan never lists a kind whose attribute model_plan did not request, nor asks for more
                                    bool asked = false;
                                    for (uint32_t j = 0; j < mp.n_attr; ++j) asked = asked || (mp.attr[j].kind == l.kind && mp.attr[j].lds >= l.lds);
                                    ok = ok && asked && l.lds <= 160u * 1024u;
                                }
                                if (l.kind >= XFWD_FIRST && l.kind < XFWD_FIRST + XFWD_COUNT) {
                                    const uint32_t NS = l.arg[0];
                                    ok = ok && NS >= 1 && NS * C <= XF_ROWS && (NS == 1 || xf_epilogue_lds(NS, C) <= XF_FWD_LDS) && l.grid_x * NS >= pl.n_pad && (l.grid_x - 1) * NS < pl.n_pad &&
                                         l.grid_y * 512 >= pl.B_pad && l.lds == XF_FWD_LDS;
                                }
                                if (l.kind >= XBWD_FIRST && l.kind < XBWD_FIRST + XBWD_COUNT) {
                                    const uint32_t tiles_m = l.arg[0], groups = l.arg[1], rb_base = l.arg[2], rb_extra = l.arg[3];
                                    const uint32_t RB = l.kind == XBWD_0_4_9 || l.kind == XBWD_0_4_9_N ? 9 : 7;
                                    ok = ok && l.grid_x % 8 == 0 && l.grid_x >= groups * tiles_m && groups >= 1 && rb_base * tiles_m + rb_extra == (P + 15) / 16 &&
                                         rb_base + (rb_extra ? 1 : 0) <= RB && rb_extra < tiles_m && l.lds == 16 * RB * (pl.B_pad * 2 + 32) && l.lds <= 160u * 1024u &&
                                         (RB == 7 || (mp.xb9 && m.xb9_ok));
                                }
                            }
                            const size_t at[] = {L.rowp, L.idx, L.Xb, L.XbT, L.lab, L.eps, L.pv_part, L.qv_part, L.s1, L.s2, L.lik_part, L.dlog};
                            const size_t ex[] = {L.Xb_bf, L.XbT_bf, L.Wp, L.logitsT, L.dlogp, L.GT};
                            const size_t tail[] = {L.ds_part, L.dmu_part, L.rowg, L.hpart, L.partial, L.wsum, L.ws1, L.ws2, L.total};
                            size_t last = 0;
                            bool first = true;
                            auto walk = [&](const size_t* o, int count) {
                                for (int i = 0; i < count; ++i) { ok = ok && o[i] % 256 == 0 && (first || o[i] > last); last = o[i]; first = false; }
                            };
                            walk(at, 12);
                            if (pl.exact) walk(ex, 6);
                            else for (size_t o : ex) ok = ok && o == 0;
                            walk(tail, 9);
                            ok = ok && L.rowp == 0 && pl.exact == (mp.path != F32) && (!pl.xfused || (mp.path == EXACT_FUSED && m.fused_ok));
                            if (!ok && ++g_failures < 40) printf("FAILED: invariants at C %u P %u B %u n %u n_cu %u v %d: %s\n", C, P, B, n, n_cu, v, kinds_of(pl).c_str());
                        }
    printf("plans: %ld\n", plans);

    // ---- every switch flipped once: what changes, and what must not
    {
        const Model cfg = model(2048, 512, 784, 10);       // nine-block tiles, B_pad % 256 == 0, two blocks of (sample, class) rows from 1024 samples
        Switches sw;
        expect("defaults", kinds_of(call_plan(cfg, def, call(1024))) == "dense_head dense_xfwd<0,2> dense_xbwd<0,4,9> dense_rows<sliced> dense_param_fold_kernel");
        expect("defaults: 4 samples per workgroup, 49 row blocks as 9 + 5 * 8, 8 * (32 / 6) = 40 groups", launch_is(find(call_plan(cfg, def, call(1024)), XFWD_0_2), 256, 1, 512, 160 * 1024, 4) &&
               launch_is(find(call_plan(cfg, def, call(1024)), XBWD_0_4_9), 240, 1, 512, 144 * 1056, 6, 40, 8, 1));
        sw.xgemm = false;       // BSVI_DENSE_XGEMM=0
        expect("xgemm off: the f32 kernels, 64-row padding", kinds_of(call_plan(cfg, sw, call(1024))) == "dense_head dense_forward<10> dense_backward dense_rows dense_epilogue dense_param_kernel" &&
               model_plan(cfg, sw).path == F32 && model_plan(cfg, sw).n_attr == 0 && !wants_exact_scan(cfg, sw));
        sw = Switches(); sw.fused = false;      // BSVI_DENSE_FUSED=0
        expect("fused off: six launches, no attributes", kinds_of(call_plan(cfg, sw, call(1024))) ==
               "dense_head dense_wsplit xgemm_nt<logits> dense_ce xgemm_nt<grad> dense_xreduce dense_rows dense_epilogue dense_param_kernel" && model_plan(cfg, sw).n_attr == 0);
        sw = Switches(); sw.fold = false;       // BSVI_DENSE_FOLD=0
        expect("fold off", kinds_of(call_plan(cfg, sw, call(1024))) == "dense_head dense_xfwd<0,2> dense_xbwd<0,4,9> dense_rows<sliced> dense_epilogue dense_param_kernel");
        sw = Switches(); sw.xf_ns = 3;          // BSVI_XF_NS
        expect("xf_ns 3: one block", launch_is(find(call_plan(cfg, sw, call(1024)), XFWD_0_1), 342, 1, 512, 160 * 1024, 3));
        sw.xf_ns = 7;
        expect("xf_ns 7: 70 rows are ignored", find(call_plan(cfg, sw, call(1024)), XFWD_0_2)->arg[0] == 4);
        sw.xf_ns = 6;
        expect("xf_ns 6 beyond the CU rule", find(call_plan(cfg, sw, call(64)), XFWD_0_2)->arg[0] == 6);
        {   // the epilogue-LDS cap comes after the knob: C = 1, NS = 64 needs (512 * 65 + 64 * 136) * 4 = 167 936 bytes, 63 samples 163 296
            Switches big; big.xf_ns = 64;
            expect("xf_ns 64 at one class is capped to 63", find(call_plan(model(64, 32, 32, 1), big, call(64)), XFWD_0_2)->arg[0] == 63 &&
                   xf_epilogue_lds(64, 1) > XF_FWD_LDS && xf_epilogue_lds(63, 1) <= XF_FWD_LDS);
        }
        for (int dbg = 0; dbg <= 7; ++dbg) {    // BSVI_XF_DEBUG
            sw = Switches(); sw.xf_debug = dbg;
            expect("xf_debug: the unweighted two-block form", has(call_plan(cfg, sw, call(1024)), dbg >= 1 && dbg <= 6 ? XFWD_0_2 + dbg : XFWD_0_2));
            expect("xf_debug: not the one-block form", has(call_plan(cfg, sw, call(64)), XFWD_0_1));
            expect("xf_debug: not the weighted form", has(call_plan(cfg, sw, call(1024, "weighted")), XFWD_0_2_W));
        }
        for (int dbg = 1; dbg <= 3; ++dbg) {    // BSVI_XB_DEBUG
            sw = Switches(); sw.xb_debug = dbg;
            expect("xb_debug: seven-block tiles and its form", has(call_plan(cfg, sw, call(1024)), XBWD_0_4_7 + dbg));
            expect("xb_debug: with noise only the seven blocks", has(call_plan(cfg, sw, call(1024, "noise")), XBWD_0_4_7_N));
            expect("xb_debug: a ring of two has no form", has(call_plan(model(2048, 384, 784, 10), sw, call(1024)), XBWD_0_2_7));
        }
        sw = Switches(); sw.xb_rb = 7;          // BSVI_XB_RB=7
        expect("xb_rb 7", launch_is(find(call_plan(cfg, sw, call(1024)), XBWD_0_4_7), 224, 1, 512, 112 * 1056, 7, 32, 7, 0) && has(call_plan(cfg, sw, call(1024, "noise")), XBWD_0_4_7_N));
        sw.xb_rb = 9;
        expect("xb_rb 9 means nothing", has(call_plan(cfg, sw, call(1024)), XBWD_0_4_9) && has(call_plan(model(2048, 384, 784, 10), sw, call(1024)), XBWD_0_2_7));
        sw = Switches(); sw.xb_groups = 33;     // BSVI_XB_GROUPS
        expect("xb_groups 33: 40 column-group slots of 6 tiles", launch_is(find(call_plan(cfg, sw, call(1024)), XBWD_0_4_9), 240, 1, 512, 144 * 1056, 6, 33, 8, 1));
        sw.xb_groups = 100000;
        expect("xb_groups clamped to C * n_pad / 16", find(call_plan(cfg, sw, call(1024)), XBWD_0_4_9)->arg[1] == 640 && find(call_plan(cfg, sw, call(1024)), XBWD_0_4_9)->grid_x == 3840);
    }
    for (int k = 0; k < KIND_COUNT; ++k)
        for (int j = 0; j < k; ++j) expect("kind names are distinct", strcmp(name(k), name(j)) != 0);
    expect("unknown kinds have no name", !strcmp(name(-1), "?") && !strcmp(name(KIND_COUNT), "?"));
    printf("%d failures\n", g_failures);
    return g_failures ? 1 : 0;
}
