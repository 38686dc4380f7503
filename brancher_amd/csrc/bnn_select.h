// bnn_select.h — which kernel serves the middle of a Bayesian-neural-network iteration (upper layers, likelihood, reverse sweep), and the
// LDS each of them asks for: ONE pure function from the network's size to the kind.  Host only: no HIP, no getenv —
// bnn_kernel.inc fills the input (bnn_mid_ready, bnn_upper_ready, bnn_create); tests/c_abi/bnn_select_table.cpp walks the table without a GPU.
// A kernel that does not compile is not this header's business: the fallbacks stay where the compile is tried.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace bsvi_bnn_select {

// The values are public: bsvi_bnn_middle returns them.
enum BnnMiddle {
    MID_GEN = 0,            // bnn_mid_gen: generated, one workgroup per sample, lanes along the minibatch rows (exact-bf16 data only)
    UPPER_GEN = 1,          // bnn_upper_gen: generated, small tensors and activations in registers
    UPPER_LDS = 2,          // bnn_upper<true>: static, small tensors and activations in LDS
    UPPER_MEM = 3           // bnn_upper<false>: static, activations and deltas in global memory
};

constexpr size_t LDS_LIMIT = 150u * 1024u;          // what a workgroup may ask of a CU's 160 KiB
constexpr uint32_t MID_MAX_ACT = 96;                // units bnn_mid_gen keeps per thread (y and d: twice that many registers)
constexpr uint32_t GEN_MAX_FLOATS = 400;            // Rs + 2 act_floats floats per thread of bnn_upper_gen: the register file

struct Switches { bool mid_off = false, jit_off = false; };      // BSVI_BNN_MID=0, BSVI_BNN_JIT=0

// Rs: rows of the latent vector behind weights1 (every bias, every upper weight matrix; 0 is staged as 1); act_floats: the sum of all
// layer widths; B_pad: the minibatch rounded up to 32 rows
inline size_t rows(uint32_t Rs) { return Rs ? Rs : 1u; }
// bnn_mid_gen: the sample's small tensors [Rs4] | the tile [2 act_floats][B_pad + 4]
inline size_t mid_lds_bytes(uint32_t Rs, uint64_t act_floats, uint32_t B_pad) {
    return ((rows(Rs) + 3u) / 4u * 4u + 2u * (size_t)act_floats * ((size_t)B_pad + 4u)) * 4u;
}
// bnn_upper_gen: the staging tile [Rs][65] of the workgroup's 64 samples
inline size_t upper_gen_lds_bytes(uint32_t Rs) { return rows(Rs) * 65u * 4u; }
// bnn_upper<true>: that tile, then activations and deltas [2 act_floats][256]
inline size_t upper_lds_bytes(uint32_t Rs, uint64_t act_floats) { return (rows(Rs) * 65u + 2u * (size_t)act_floats * 256u) * 4u; }

inline BnnMiddle middle(uint32_t Rs, uint64_t act_floats, uint32_t B_pad, bool exact, Switches sw) {
    if (!sw.mid_off && exact && mid_lds_bytes(Rs, act_floats, B_pad) <= LDS_LIMIT && act_floats <= MID_MAX_ACT && B_pad % 4u == 0u) return MID_GEN;
    if (!sw.jit_off && (uint64_t)Rs + 2u * act_floats <= GEN_MAX_FLOATS && upper_gen_lds_bytes(Rs) <= LDS_LIMIT) return UPPER_GEN;
    return upper_lds_bytes(Rs, act_floats) <= LDS_LIMIT ? UPPER_LDS : UPPER_MEM;
}

inline const char* name(int kind) {
    switch (kind) {
    case MID_GEN: return "mid_gen";
    case UPPER_GEN: return "upper_gen";
    case UPPER_LDS: return "upper_lds";
    case UPPER_MEM: return "upper_mem";
    default: return "?";
    }
}

}  // namespace bsvi_bnn_select
