// bnn_source.h — the text of the two kernels the library generates for ONE Bayesian neural network: bnn_upper_gen (lanes along the
// samples, the sample's small tensors and the activations in registers) and bnn_mid_gen (a workgroup per sample, lanes along the
// minibatch rows).  Host only: no HIP, no getenv — bnn_kernel.inc fills the Net (bnn_source_net) and compiles what comes back
// (bnn_gen_ready); tests/c_abi/bnn_source_text.cpp writes the same text without a GPU, and tests/golden/bnn_source/digests.json holds
// what the text was before this header existed.
// Both kernels walk one (sample, minibatch row) the same way — forward sweep, likelihood and its seeds, reverse sweep, the three bf16
// pieces of d f / d a1 — so every one of those is written ONCE here, parametrised by the name of the weights (`w`: registers, `wl`: LDS)
// and by how a1 is loaded.  What differs stays in upper_source / mid_source: staging, the pk[][] pairs, the tile, GEN_DU / GEN_YU.
// The text is layer sizes, offsets and activations as literals with every loop unrolled; same arithmetic in the same order as the static
// bnn_upper.
#pragma once
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include <string>
#include <vector>

#include "bsvi.h"

namespace bsvi_bnn_source {

constexpr uint32_t MAX_LAYERS = 8;
constexpr uint32_t NO_BIAS = 0xFFFFFFFFu;

// one network, as bnn_create derives it
struct Net {
    uint32_t n_layers = 0;
    bsvi_bnn_layer layer[MAX_LAYERS] = {};
    uint32_t act_off[MAX_LAYERS] = {};       // first unit of layer l among the act_floats units of a (sample, row)
    uint32_t R1 = 0, Rs = 0;                 // rows of weights1; rows behind them (the small tensors)
    uint32_t act_floats = 0;                 // the sum of all layer widths
    uint32_t C = 0;                          // targets per minibatch row (a scale head: half the last layer's rows)
    uint32_t B_pad = 0;
    uint32_t likelihood = BSVI_LIK_CATEGORICAL, family = BSVI_DIST_NORMAL;
    bool scale_learn = false;
    uint32_t heads = 0, head_a_bits = 0, head_b_bits = 0;      // a scale head's BSVI_UT_* transform (0: none), a and b of sigma = a + b g(raw) as bits
    bool cauchy_log1p = false;               // BSVI_BNN_CAUCHY_LOG=log1p, read by the caller
    // the parameters of the layers' activations (bsvi_bnn_set_activation_params); act_params_set false: torch's defaults (act_default)
    bool act_params_set = false;
    float act_p[MAX_LAYERS][2] = {};
};

// torch's defaults of the parametrised activations: leaky_relu's negative_slope, elu's alpha, hardtanh's (min_val, max_val)
inline void act_default(uint32_t a, float p[2]) {
    p[0] = a == BSVI_BNN_ACT_LEAKY_RELU ? 0.01f : (a == BSVI_BNN_ACT_ELU ? 1.0f : (a == BSVI_BNN_ACT_HARDTANH ? -1.0f : 0.0f));
    p[1] = a == BSVI_BNN_ACT_HARDTANH ? 1.0f : 0.0f;
}
// SILU and GELU are not monotone: their derivative is taken from the pre-activation, where every other kind's is a function of the output
inline bool act_grad_from_input(uint32_t a) { return a == BSVI_BNN_ACT_SILU || a == BSVI_BNN_ACT_GELU; }
// selu's two constants as torch holds them, and their product
#define BSVI_SELU_SCALE 1.0507009873554804934193349852946
#define BSVI_SELU_ALPHA 1.6732632423543772848170429916717
// gelu's 1 / sqrt(2) and 1 / sqrt(2 pi): ONE spelling for the static kernels (bnn_kernel.inc) and, as text, for the generated ones
#define BSVI_INV_SQRT2 0.707106781f
#define BSVI_INV_SQRT_2PI 0.398942280f
#define BSVI_TEXT_(x) #x
#define BSVI_TEXT(x) BSVI_TEXT_(x)

// the activation of layer l with its parameters
struct Act { uint32_t kind; float p[2]; };
inline Act act_of(const Net& N, uint32_t l) {
    Act a;
    a.kind = N.layer[l].activation;
    if (N.act_params_set) { a.p[0] = N.act_p[l][0]; a.p[1] = N.act_p[l][1]; }
    else act_default(a.kind, a.p);
    return a;
}

inline std::string fmt(const char* f, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, f);
    vsnprintf(buf, sizeof buf, f, ap);
    va_end(ap);
    return std::string(buf);
}

// a finite float as a literal that reads back to the same bits (nine significant digits)
inline std::string flit(float x) {
    std::string s = fmt("%.9g", (double)x);
    if (s.find_first_of(".e") == std::string::npos) s += ".0";
    return s + "f";
}

// v: the NAME of the pre-activation (it is read more than once)
inline std::string act_text(const Act& a, const std::string& v) {
    switch (a.kind) {
    case BSVI_BNN_ACT_TANH: return "tanhf(" + v + ")";
    case BSVI_BNN_ACT_RELU: return "fmaxf(" + v + ", 0.0f)";
    case BSVI_BNN_ACT_SIGMOID: return "sigmoidf_(" + v + ")";
    case BSVI_BNN_ACT_SOFTPLUS: return "((" + v + ") > 20.0f ? (" + v + ") : log1pf(expf(" + v + ")))";
    case BSVI_BNN_ACT_LEAKY_RELU: return "(" + v + " > 0.0f ? " + v + " : " + flit(a.p[0]) + " * " + v + ")";
    case BSVI_BNN_ACT_ELU: return "(" + v + " > 0.0f ? " + v + " : " + flit(a.p[0]) + " * expm1f(" + v + "))";
    case BSVI_BNN_ACT_SELU:
        return "(" + flit((float)BSVI_SELU_SCALE) + " * (" + v + " > 0.0f ? " + v + " : " + flit((float)BSVI_SELU_ALPHA) + " * expm1f(" + v + ")))";
    case BSVI_BNN_ACT_SOFTSIGN: return "(" + v + " / (1.0f + fabsf(" + v + ")))";
    case BSVI_BNN_ACT_HARDTANH: return "fminf(fmaxf(" + v + ", " + flit(a.p[0]) + "), " + flit(a.p[1]) + ")";
    case BSVI_BNN_ACT_SILU: return "(" + v + " * sigmoidf_(" + v + "))";
    case BSVI_BNN_ACT_GELU: return "(" + v + " * (0.5f * (1.0f + erff(" + v + " * " BSVI_TEXT(BSVI_INV_SQRT2) "))))";
    default: return v;
    }
}
// through the OUTPUT of the activation
inline std::string act_grad_text(const Act& a, const std::string& y) {
    switch (a.kind) {
    case BSVI_BNN_ACT_TANH: return "(1.0f - " + y + " * " + y + ")";
    case BSVI_BNN_ACT_RELU: return "(" + y + " > 0.0f ? 1.0f : 0.0f)";
    case BSVI_BNN_ACT_SIGMOID: return "(" + y + " * (1.0f - " + y + "))";
    case BSVI_BNN_ACT_SOFTPLUS: return "(" + y + " > 20.0f ? 1.0f : -expm1f(-" + y + "))";
    case BSVI_BNN_ACT_LEAKY_RELU: return "(" + y + " > 0.0f ? 1.0f : " + flit(a.p[0]) + ")";
    case BSVI_BNN_ACT_ELU: return "(" + y + " > 0.0f ? 1.0f : " + y + " + " + flit(a.p[0]) + ")";
    case BSVI_BNN_ACT_SELU:
        return "(" + y + " > 0.0f ? " + flit((float)BSVI_SELU_SCALE) + " : " + y + " + " + flit((float)(BSVI_SELU_SCALE * BSVI_SELU_ALPHA)) + ")";
    case BSVI_BNN_ACT_SOFTSIGN: return "((1.0f - fabsf(" + y + ")) * (1.0f - fabsf(" + y + ")))";
    case BSVI_BNN_ACT_HARDTANH: return "(" + y + " > " + flit(a.p[0]) + " && " + y + " < " + flit(a.p[1]) + " ? 1.0f : 0.0f)";
    default: return std::string("1.0f");
    }
}
// SILU | GELU: the statement that leaves act(v) in `y` and act'(v) in `d`, the unit's delta slot, which nothing reads before the reverse
// sweep multiplies it in place (sigma (1 + v (1 - sigma)) | Phi(v) + v phi(v))
inline std::string act_pair_text(const Act& a, const std::string& v, const std::string& y, const std::string& d) {
    if (a.kind == BSVI_BNN_ACT_SILU)
        return "{ const float sg = sigmoidf_(" + v + "); " + y + " = " + v + " * sg; " + d + " = sg * (1.0f + " + v + " * (1.0f - sg)); }";
    return "{ const float cdf = 0.5f * (1.0f + erff(" + v + " * " BSVI_TEXT(BSVI_INV_SQRT2) ")); " + y + " = " + v + " * cdf; " + d + " = cdf + " + v +
           " * (" BSVI_TEXT(BSVI_INV_SQRT_2PI) " * expf(-0.5f * " + v + " * " + v + ")); }";
}

// what both translation units open with, up to their argument struct
inline std::string preamble() {
    return "// generated by libbsvi (bnn_kernel.inc) for one Bayesian neural network: do not edit\n"
           "#include \"bsvi_device.h\"\nusing namespace bsvi;\n";
}
const char* const GEN_BF16 =
    "__device__ __forceinline__ uint16_t gen_bf16(float x) { const uint32_t u = __float_as_uint(x); return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16); }\n";
// g -> its three exact bf16 pieces hi, mid, lo (dense_split3)
const char* const SPLIT3 =
    "            const uint16_t hi = gen_bf16(g);\n"
    "            const float r1 = g - __uint_as_float((uint32_t)hi << 16);\n"
    "            const uint16_t mid = gen_bf16(r1);\n"
    "            const uint16_t lo = gen_bf16(r1 - __uint_as_float((uint32_t)mid << 16));\n";

// y[] of every layer; w: the name of the sample's small tensors, a1: the load of product 1's element (h, n, b)
inline std::string forward_sweep(const Net& N, const char* w, const char* a1) {
    const bsvi_bnn_layer& L0 = N.layer[0];
    std::string s = "#pragma unroll\n";
    s += fmt("        for (uint32_t h = 0; h < %uu; ++h) {\n            float v = %s;\n", L0.rows, a1);
    if (L0.bias_row0 != NO_BIAS) s += fmt("            v += %s[%uu + h];\n", w, L0.bias_row0 - N.R1);
    // (a kind whose derivative needs the pre-activation leaves it in the unit's delta slot: act_pair_text)
    auto store = [&](uint32_t l, const char* unit, const char* v) {
        const std::string at = fmt("[%uu + %s]", N.act_off[l], unit);
        const Act a = act_of(N, l);
        if (act_grad_from_input(a.kind)) return "            " + act_pair_text(a, v, "y" + at, "d" + at) + "\n        }\n";
        return "            y" + at + " = " + act_text(a, v) + ";\n        }\n";
    };
    s += store(0, "h", "v");
    for (uint32_t l = 1; l < N.n_layers; ++l) {
        const bsvi_bnn_layer& L = N.layer[l];
        s += "#pragma unroll\n";
        s += fmt("        for (uint32_t i = 0; i < %uu; ++i) {\n", L.rows);
        s += L.bias_row0 != NO_BIAS ? fmt("            float sm = %s[%uu + i];\n", w, L.bias_row0 - N.R1) : std::string("            float sm = 0.0f;\n");
        s += "#pragma unroll\n";
        s += fmt("            for (uint32_t j = 0; j < %uu; ++j) sm += %s[%uu + i * %uu + j] * y[%uu + j];\n", L.cols, w, L.weight_row0 - N.R1, L.cols, N.act_off[l - 1]);
        s += store(l, "i", "sm");
    }
    return s;
}

// delta_l = d f / d (pre-activation of layer l), from the last layer's d[] down; the last layer's activation is the identity
inline std::string reverse_sweep(const Net& N, const char* w) {
    std::string s;
    for (uint32_t l = N.n_layers - 1; l >= 1; --l) {
        const bsvi_bnn_layer& L = N.layer[l];
        const Act ap = act_of(N, l - 1);
        const std::string below = fmt("[%uu + j]", N.act_off[l - 1]);
        s += "#pragma unroll\n";
        s += fmt("        for (uint32_t j = 0; j < %uu; ++j) {\n            float sm = 0.0f;\n#pragma unroll\n", L.cols);
        s += fmt("            for (uint32_t i = 0; i < %uu; ++i) sm += %s[%uu + i * %uu + j] * d[%uu + i];\n", L.rows, w, L.weight_row0 - N.R1, L.cols, N.act_off[l]);
        s += "            d" + below + " = sm * " + (act_grad_from_input(ap.kind) ? "d" + below : act_grad_text(ap, "y" + below)) + ";\n        }\n";
    }
    return s;
}

// the classifiers: log-softmax cross-entropy over `rows` logits, or Bernoulli logits on the one
inline std::string classifier_epilogue(uint32_t likelihood, uint32_t rows, uint32_t yl) {
    std::string s;
    if (likelihood == BSVI_LIK_CATEGORICAL) {
        s += "        {\n            float m = -INFINITY;\n#pragma unroll\n";
        s += fmt("            for (uint32_t c = 0; c < %uu; ++c) m = fmaxf(m, y[%uu + c]);\n", rows, yl);
        s += "            float se = 0.0f, zl = 0.0f;\n#pragma unroll\n";
        s += fmt("            for (uint32_t c = 0; c < %uu; ++c) { const float z = y[%uu + c]; se += expf(z - m); if (label == (float)c) zl = z; }\n", rows, yl);
        s += "            const float lse = m + logf(se);\n            lik = wgt * (zl - lse);\n#pragma unroll\n";
        s += fmt("            for (uint32_t c = 0; c < %uu; ++c) d[%uu + c] = wgt * ((label == (float)c ? 1.0f : 0.0f) - expf(y[%uu + c] - lse));\n        }\n", rows, yl, yl);
    } else {
        s += fmt("        {\n            const float z = y[%uu];\n            lik = wgt * (label * z - (fmaxf(z, 0.0f) + log1pf(expf(-fabsf(z)))));\n            d[%uu] = wgt * (label - sigmoidf_(z));\n        }\n", yl, yl);
    }
    return s;
}

// the loc-scale likelihoods in u = (y - z) / sigma (DESIGN.md's table): the line that defines psi (none: psi is u itself), the value
// without its constant, u psi(u), the score's name, and the constant as it follows -logf(sigma).  Every site seeds
//     d f / d z = wgt psi / sigma,      d f / d sigma = wgt (u psi - 1) / sigma
struct Family { const char* psi_line; const char* value; const char* upsi; const char* score; const char* log_const; };
inline Family family_text(uint32_t family, bool cauchy_log1p) {
    static const Family table[3] = {
        {nullptr, "-0.5f * u * u", "u * u", "u", "- 0.91893853320467274178f"},
        {"const float psi = u > 0.0f ? 1.0f : (u < 0.0f ? -1.0f : 0.0f);", "-fabsf(u)", "fabsf(u)", "psi", "+ -0.69314718055994530942f"},
        // (the hardware logarithm, as the static kernel's bnn_loc_scale_term)
        {"const float q = 1.0f + u * u, psi = 2.0f * u / q;", "-__logf(q)", "u * psi", "psi", "+ -1.14472988584940017414f"}};
    Family f = table[family == BSVI_DIST_LAPLACE ? 1 : (family == BSVI_DIST_CAUCHY ? 2 : 0)];
    // BSVI_BNN_CAUCHY_LOG=log1p: the library's log1pf in the place of the hardware logarithm (tools/bnn_likelihoods_timing.py measures both)
    if (family == BSVI_DIST_CAUCHY && cauchy_log1p) { f.psi_line = "const float uu = u * u, q = 1.0f + uu, psi = 2.0f * u / q;"; f.value = "-log1pf(uu)"; }
    return f;
}

// the loc-scale likelihood of a (sample, row): targets [B_pad][C] in A.lab; sigma from the table behind them — sigma [C] and
// -log sigma + the family's constant [C], as bnn_head_body leaves them: the values of the uniform table, never a host copy — or from a
// scale head, y[yl + c] the loc and y[yl + C + c] the raw scale, the transform and its two constants as literals (their bits: no
// decimal round trip), the second half's delta carrying d f / d sigma through the transform.
// sig_terms (bnn_upper_gen with a learnable sigma): wgt (u psi - 1) / sigma per (c, b, n) leaves for bnn_sig_rows
inline std::string loc_scale_epilogue(const Net& N, uint32_t yl, bool sig_terms) {
    const Family f = family_text(N.family, N.cauchy_log1p);
    const uint32_t C = N.C;
    std::string s = "        {\n";
    s += fmt("            const float* const yb = A.lab + (size_t)b * %uu;\n", C);
    if (N.heads) s += fmt("            const float ha = __uint_as_float(0x%08xu), hb = __uint_as_float(0x%08xu);\n", N.head_a_bits, N.head_b_bits);
    else s += fmt("            const float* const sg = A.lab + (size_t)A.B_pad * %uu;\n", C);
    s += "            float sn = 0.0f;\n#pragma unroll\n";
    s += fmt("            for (uint32_t c = 0; c < %uu; ++c) {\n", C);
    if (N.heads) {
        s += fmt("                const float raw = y[%uu + c];\n", yl + C);
        s += N.heads == BSVI_UT_EXP ? "                const float g = expf(raw), dg = g;\n"
           : N.heads == BSVI_UT_SIGMOID ? "                const float g = sigmoidf_(raw), dg = g * (1.0f - g);\n"
           : "                const float g = raw > 20.0f ? raw : log1pf(expf(raw)), dg = raw > 20.0f ? 1.0f : sigmoidf_(raw);\n";
        s += fmt("                const float sigma = ha + hb * g, u = (yb[c] - y[%uu + c]) / sigma;\n", yl);
    } else {
        s += fmt("                const float sigma = sg[c], u = (yb[c] - y[%uu + c]) / sigma;\n", yl);
    }
    if (f.psi_line) s += fmt("                %s\n", f.psi_line);
    if (N.heads) s += fmt("                sn += %s - logf(sigma) %s;\n", f.value, f.log_const);
    else s += fmt("                sn += %s + sg[%uu + c];\n", f.value, C);
    s += fmt("                d[%uu + c] = wgt * %s / sigma;\n", yl, f.score);
    if (N.heads) s += fmt("                d[%uu + c] = wgt * (%s - 1.0f) / sigma * (hb * dg);\n", yl + C, f.upsi);
    if (sig_terms) s += fmt("                A.sigt[((size_t)c * A.B_pad + b) * A.n_pad + n] = wgt * (%s - 1.0f) / sigma;\n", f.upsi);
    s += "            }\n            lik = wgt * sn;\n        }\n";
    return s;
}

// the likelihood of a (sample, row) and d f / d (last layer): wgt, lik and d[yl ..] (distributions.py:294-311 / 561-592 / 137 through torch)
inline std::string likelihood(const Net& N, bool sig_terms) {
    const uint32_t yl = N.act_off[N.n_layers - 1];
    std::string s = std::string("        const float wgt = live ? A.lik_weight * (A.f_weight ? A.f_weight[n] : 1.0f) : 0.0f") +
                    (N.likelihood == BSVI_LIK_NORMAL ? ";\n" : ", label = A.lab[b];\n") + "        float lik = 0.0f;\n";
    if (N.likelihood == BSVI_LIK_NORMAL) s += loc_scale_epilogue(N, yl, sig_terms);
    else s += classifier_epilogue(N.likelihood, N.layer[N.n_layers - 1].rows, yl);
    return s;
}

// ---- bnn_upper as generated source.  The static kernel walks the network with run-time loop bounds: every weight of the sample's
// small tensors and every activation is an LDS read in front of the FMA that needs it (~2 200 of them per (sample, row) of the
// 784-20-10 network), from ONE wave per SIMD: 434 of the 941 us of an iteration at config 4's scale.  A model is compiled once and
// iterated thousands of times, so — as specialize.cpp does for the scalar programs — the library writes the kernel for THIS network:
// the sample's small tensors (230 floats for 784-20-10) and the activations in REGISTERS (staged through LDS once per workgroup,
// transposed, as the static kernel stages them).
inline std::string upper_source(const Net& N) {
    const uint32_t NL = N.n_layers, RS = N.Rs ? N.Rs : 1, AW = N.act_floats;
    std::string s = preamble();
    s += "struct BnnUpperArgs { const float* Wsm; const float* a1T; const float* lab; float* acts; float* deltas; float* liknb; float* da1T; uint16_t* dlogp;\n"
         "    uint32_t n_local, n_pad, B, B_pad, NC, rows_per_wave, exact; float lik_weight; const float* f_weight;";
    s += N.scale_learn ? " float* sigt; };\n" : " };\n";
    s += GEN_BF16;
    s += fmt("#define RS %uu\n#define AW %uu\n", RS, AW);
    s += "extern \"C\" __global__ void __launch_bounds__(256) bnn_upper_gen(const BnnUpperArgs A) {\n"
         "    extern __shared__ float wl[];                       // [RS][65]: the small tensors of the workgroup's 64 samples, transposed\n"
         "    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, n = blockIdx.x * 64u + lane;\n"
         "    for (uint32_t i = threadIdx.x; i < 64u * RS; i += 256u) {\n"
         "        const uint32_t sn = i / RS, r = i - sn * RS;\n"
         "        wl[r * 65u + sn] = A.Wsm[(size_t)(blockIdx.x * 64u + sn) * RS + r];\n"
         "    }\n"
         "    __syncthreads();\n"
         "    float w[RS];\n"
         "#pragma unroll\n"
         "    for (uint32_t r = 0; r < RS; ++r) w[r] = wl[r * 65u + lane];\n"
         "    for (uint32_t bi = 0; bi < A.rows_per_wave; ++bi) {\n"
         "        const uint32_t b = (blockIdx.y * 4u + wave) * A.rows_per_wave + bi;\n"
         "        if (b >= A.B_pad) break;\n"
         "        const bool live = n < A.n_local && b < A.B;\n"
         "        float y[AW], d[AW];\n";
    s += forward_sweep(N, "w", "A.a1T[(size_t)b * A.NC + (size_t)h * A.n_pad + n]");
    s += likelihood(N, N.scale_learn);
    s += "        A.liknb[(size_t)b * A.n_pad + n] = lik;\n";
    s += reverse_sweep(N, "w");
    // what bnn_small reads
    for (uint32_t l = 0; l < NL; ++l) {
        s += "#pragma unroll\n";
        s += fmt("        for (uint32_t u = 0; u < %uu; ++u) {\n            const size_t at = ((size_t)(%uu + u) * A.B_pad + b) * A.n_pad + n;\n", N.layer[l].rows, N.act_off[l]);
        if (l + 1 < NL) s += fmt("            A.acts[at] = y[%uu + u];\n", N.act_off[l]);
        s += fmt("            A.deltas[at] = d[%uu + u];\n        }\n", N.act_off[l]);
    }
    // d f / d a1 as the operand of the second product, [(h, n)][b]
    s += "#pragma unroll\n";
    s += fmt("        for (uint32_t h = 0; h < %uu; ++h) {\n", N.layer[0].rows);
    s += "            const size_t at = ((size_t)h * A.n_pad + n) * A.B_pad + b;\n";
    s += fmt("            const float g = live ? d[%uu + h] : 0.0f;\n", N.act_off[0]);
    s += "            if (A.exact) {\n";
    s += SPLIT3;
    s += "                const size_t plane = (size_t)A.NC * A.B_pad;\n"
         "                A.dlogp[at] = hi; A.dlogp[plane + at] = mid; A.dlogp[2 * plane + at] = lo;\n"
         "            } else {\n"
         "                A.da1T[at] = g;\n"
         "            }\n"
         "        }\n"
         "    }\n"
         "}\n";
    return s;
}

// ---- the exact-data path's middle as ONE generated kernel, lanes along the MINIBATCH ROWS (round 5).  With lanes along the samples
// (bnn_upper, bnn_upper_gen) the operand of the second product — d f / d a1 as bf16 pieces [(h, n)][b] — leaves as 2-byte stores a
// kilobyte apart, 60 per (sample, row): most of what those kernels take.  Here a workgroup owns ONE sample: product 1 delivers a1
// transposed, [(h, n)][b] (bsvi_xgemm_nt_t), so loads and piece stores are contiguous along b; the sample's small tensors are 230
// floats of LDS read as broadcasts; activations and deltas of the sample's rows stay in an LDS tile [unit][b], from which the same
// workgroup then takes the gradients of the small tensors (one thread per element, rows in order: bnn_small's job) and the sample's
// likelihood — acts / deltas / liknb never reach memory, bnn_small and bnn_lik are not launched.
inline std::string mid_source(const Net& N) {
    const uint32_t NL = N.n_layers, RS = N.Rs ? N.Rs : 1, R1 = N.R1, AW = N.act_floats;
    const bsvi_bnn_layer& L0 = N.layer[0];
    const bsvi_bnn_layer& LL = N.layer[NL - 1];
    const uint32_t yl = N.act_off[NL - 1];
    // element r of the small tensors -> (unit of its delta row, unit of its input row in the tile, or "one" for a bias); the tile holds
    // the activations y at units [0, AW) and the deltas d at [AW, 2 AW)
    std::vector<uint32_t> du(RS, 0u), yu(RS, 0xFFFFu);
    for (uint32_t l = 0; l < NL; ++l) {
        const bsvi_bnn_layer& L = N.layer[l];
        if (L.bias_row0 != NO_BIAS)
            for (uint32_t i = 0; i < L.rows; ++i) du[L.bias_row0 - R1 + i] = AW + N.act_off[l] + i;
        if (l == 0) continue;
        for (uint32_t i = 0; i < L.rows; ++i)
            for (uint32_t j = 0; j < L.cols; ++j) {
                du[L.weight_row0 - R1 + i * L.cols + j] = AW + N.act_off[l] + i;
                yu[L.weight_row0 - R1 + i * L.cols + j] = N.act_off[l - 1] + j;
            }
    }
    std::string s = preamble();
    s += "struct BnnMidArgs { const float* Wsm; const float* a1; const float* lab; float* gsm; float* lik; uint16_t* dlogp;\n"
         "    uint32_t n_local, n_pad, B, B_pad, NC; float lik_weight; const float* f_weight;";
    s += N.scale_learn ? " float* gsig; };\n" : " };\n";
    s += "typedef float gen_f4 __attribute__((ext_vector_type(4)));\n";
    s += GEN_BF16;
    s += fmt("#define RS %uu\n#define RSP %uu\n#define AW %uu\n", RS, (RS + 3u) / 4u * 4u, AW);
    s += "__device__ const unsigned short GEN_DU[RS] = {";
    for (uint32_t r = 0; r < RS; ++r) s += fmt("%u%s", du[r], r + 1 < RS ? "," : "");
    s += "};\n__device__ const unsigned short GEN_YU[RS] = {";
    for (uint32_t r = 0; r < RS; ++r) s += fmt("%u%s", yu[r], r + 1 < RS ? "," : "");
    s += "};\n";
    s += "extern \"C\" __global__ void __launch_bounds__(256) bnn_mid_gen(const BnnMidArgs A) {\n"
         "    extern __shared__ __attribute__((aligned(16))) float lds[];      // small tensors [RSP] | tile [2 AW][BS]: y, then d, of every row b\n"
         "    __shared__ float red[4];\n"
         "    const uint32_t tid = threadIdx.x, n = blockIdx.x, BS = A.B_pad + 4u;\n"
         "    float* const wl = lds;\n"
         "    float* const T = lds + RSP;\n"
         "    for (uint32_t r = tid; r < RS; r += 256u) wl[r] = A.Wsm[(size_t)n * RS + r];\n"
         "    __syncthreads();\n"
         "    float lik_acc = 0.0f;\n";
    // (round 6: with 512 and more rows a thread takes PAIRS of neighbouring rows, so that the pieces of d f / d a1 leave as 4-byte
    //  stores — 106 -> 97 us at config 4's scale; the example's 32 rows keep one row per thread: half the threads would do twice the work)
    const bool pairs = N.B_pad >= 512u;
    if (pairs)
        s += "    for (uint32_t b2 = tid; b2 < A.B_pad / 2u; b2 += 256u) {\n"
             "      uint32_t pk[3][" + fmt("%u", L0.rows) + "];\n"
             "#pragma unroll\n"
             "      for (uint32_t bb = 0; bb < 2u; ++bb) {\n"
             "        const uint32_t b = 2u * b2 + bb;\n";
    else
        s += "    for (uint32_t b = tid; b < A.B_pad; b += 256u) {\n"
             "      {\n";
    s += "        const bool live = n < A.n_local && b < A.B;\n"
         "        float y[AW], d[AW];\n";
    s += forward_sweep(N, "wl", "A.a1[((size_t)h * A.n_pad + n) * A.B_pad + b]");
    s += likelihood(N, false);
    s += "        lik_acc += lik;\n";
    s += reverse_sweep(N, "wl");
    s += "#pragma unroll\n        for (uint32_t u = 0; u < AW; ++u) { T[(size_t)u * BS + b] = y[u]; T[(size_t)(AW + u) * BS + b] = d[u]; }\n";
    if (N.scale_learn)      // (the residuals where the last layer's outputs stood: what sigma's elements of the loop below read)
        s += fmt("#pragma unroll\n        for (uint32_t c = 0; c < %uu; ++c) T[(size_t)(%uu + c) * BS + b] = A.lab[(size_t)b * %uu + c] - y[%uu + c];\n",
                 LL.rows, yl, LL.rows, yl);
    s += "#pragma unroll\n";
    s += fmt("        for (uint32_t h = 0; h < %uu; ++h) {\n", L0.rows);
    s += fmt("            const float g = live ? d[%uu + h] : 0.0f;\n", N.act_off[0]);
    s += SPLIT3;
    if (pairs) {
        s += "            pk[0][h] = bb ? (pk[0][h] | ((uint32_t)hi << 16)) : (uint32_t)hi;\n"
             "            pk[1][h] = bb ? (pk[1][h] | ((uint32_t)mid << 16)) : (uint32_t)mid;\n"
             "            pk[2][h] = bb ? (pk[2][h] | ((uint32_t)lo << 16)) : (uint32_t)lo;\n"
             "        }\n"
             "      }\n"
             "#pragma unroll\n";
        s += fmt("      for (uint32_t h = 0; h < %uu; ++h) {\n", L0.rows);
        s += "          const size_t at = ((size_t)h * A.n_pad + n) * A.B_pad + 2u * b2, plane = (size_t)A.NC * A.B_pad;\n"
             "          *reinterpret_cast<uint32_t*>(A.dlogp + at) = pk[0][h];\n"
             "          *reinterpret_cast<uint32_t*>(A.dlogp + plane + at) = pk[1][h];\n"
             "          *reinterpret_cast<uint32_t*>(A.dlogp + 2 * plane + at) = pk[2][h];\n"
             "      }\n"
             "    }\n";
    } else {
        s += "            const size_t at = ((size_t)h * A.n_pad + n) * A.B_pad + b, plane = (size_t)A.NC * A.B_pad;\n"
             "            A.dlogp[at] = hi; A.dlogp[plane + at] = mid; A.dlogp[2 * plane + at] = lo;\n"
             "        }\n"
             "      }\n"
             "    }\n";
    }
    s += "    // the sample's likelihood: lanes, then the four waves, in order\n"
         "    {\n"
         "        const float ws = wave_sum(lik_acc);\n"
         "        if ((tid & 63u) == 0u) red[tid >> 6] = ws;\n"
         "    }\n"
         "    __syncthreads();                                   // (and the tile is complete)\n"
         "    if (tid == 0u) A.lik[n] = (red[0] + red[1]) + (red[2] + red[3]);\n"
         "    // gradients of the small tensors: element r = sum_b d[du(r)][b] * y[yu(r)][b] (a bias: y = 1), rows in order\n"
         "    for (uint32_t r = tid; r < RS; r += 256u) {\n"
         "        const uint32_t du = GEN_DU[r], yu = GEN_YU[r];\n"
         "        const gen_f4* const dr = reinterpret_cast<const gen_f4*>(T + (size_t)du * BS);\n"
         "        const gen_f4* const yr = reinterpret_cast<const gen_f4*>(T + (size_t)(yu == 0xFFFFu ? du : yu) * BS);\n"
         "        float sm = 0.0f;\n"
         "        if (yu == 0xFFFFu) {\n"
         "            for (uint32_t q = 0; q < A.B_pad / 4u; ++q) { const gen_f4 dv = dr[q]; sm += dv.x; sm += dv.y; sm += dv.z; sm += dv.w; }\n"
         "        } else {\n"
         "            for (uint32_t q = 0; q < A.B_pad / 4u; ++q) {\n"
         "                const gen_f4 dv = dr[q], yv = yr[q];\n"
         "                sm += dv.x * yv.x; sm += dv.y * yv.y; sm += dv.z * yv.z; sm += dv.w * yv.w;\n"
         "            }\n"
         "        }\n"
         "        A.gsm[(size_t)n * RS + r] = sm;\n"
         "    }\n";
    // a learnable sigma: its C per-sample sums are C more elements of this kind (a thread each, rows in order, 16-byte LDS reads, no LDS of
    // their own), taken from the LAST thread down — with Rs <= 192 a wave that has no element of the small tensors, so that no wave runs
    // both kinds one after the other.  The tile holds y_c - z_c (in the place of z_c, which no element reads) and d_c = wgt psi / sigma_c of
    // the last layer, and d_c (y_c - z_c) = wgt u psi: the loop of a weight element, instruction for instruction (four conditional
    // subtractions of wgt per iteration made this one 17 us of a 94 us launch at config 4's scale, profiles/r16); rows behind the
    // minibatch have d_c = 0, and sum_b wgt = wgt B leaves once, behind the loop
    if (N.scale_learn)
        s += fmt("    for (uint32_t c = 255u - tid; c < %uu; c += 256u) {\n"
                 "        const gen_f4* const dr = reinterpret_cast<const gen_f4*>(T + (size_t)(AW + %uu + c) * BS);\n"
                 "        const gen_f4* const rr = reinterpret_cast<const gen_f4*>(T + (size_t)(%uu + c) * BS);\n", LL.rows, yl, yl) +
             "        const float wv = n < A.n_local ? A.lik_weight * (A.f_weight ? A.f_weight[n] : 1.0f) : 0.0f;\n"
             "        float sm = 0.0f;\n"
             "        for (uint32_t q = 0; q < A.B_pad / 4u; ++q) {\n"
             "            const gen_f4 dv = dr[q], rv = rr[q];\n"
             "            sm += dv.x * rv.x; sm += dv.y * rv.y; sm += dv.z * rv.z; sm += dv.w * rv.w;\n"
             "        }\n" +
             fmt("        A.gsig[(size_t)c * A.n_pad + n] = (sm - wv * (float)A.B) / A.lab[(size_t)A.B_pad * %uu + c];\n"
                 "    }\n", LL.rows);
    s += "}\n";
    return s;
}

}  // namespace bsvi_bnn_source
