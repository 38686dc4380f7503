// bnn_source_text.cpp for a network whose activations carry parameters (bsvi_bnn_set_activation_params): the same description, every
// layer followed by the bits of its two parameters, as the library hands them to brancher_amd/csrc/bnn_source.h (bnn_source_net).
//     bnn_source_params upper|mid n_rows n_features batch_size likelihood family scale_learn heads head_a_bits head_b_bits cauchy_log1p
//                       n_layers  { rows cols weight_row0 bias_row0 activation p0_bits p1_bits } x n_layers
// tests/test_bnn_activations_cpu.py compiles this from the header alone and reads the text it prints.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "bnn_source.h"

int main(int argc, char** argv) {
    if (argc < 13) { fprintf(stderr, "usage: see the head of bnn_source_params.cpp\n"); return 2; }
    auto num = [&](int i) { return (uint32_t)strtoul(argv[i], nullptr, 10); };
    const bool mid = !strcmp(argv[1], "mid");
    if (!mid && strcmp(argv[1], "upper")) { fprintf(stderr, "upper or mid\n"); return 2; }
    const uint32_t n_rows = num(2), n_features = num(3), batch_size = num(4);
    bsvi_bnn_source::Net N;
    N.likelihood = num(5); N.family = num(6); N.scale_learn = num(7) != 0; N.heads = num(8); N.head_a_bits = num(9); N.head_b_bits = num(10);
    N.cauchy_log1p = num(11) != 0;
    N.n_layers = num(12);
    if (!N.n_layers || N.n_layers > bsvi_bnn_source::MAX_LAYERS || argc != 13 + 7 * (int)N.n_layers) { fprintf(stderr, "bad layer count\n"); return 2; }
    N.act_params_set = true;
    for (uint32_t l = 0; l < N.n_layers; ++l) {
        bsvi_bnn_layer& L = N.layer[l];
        L.rows = num(13 + 7 * l); L.cols = num(14 + 7 * l); L.weight_row0 = num(15 + 7 * l); L.bias_row0 = num(16 + 7 * l); L.activation = num(17 + 7 * l);
        for (int k = 0; k < 2; ++k) { const uint32_t bits = num(18 + 7 * l + k); memcpy(&N.act_p[l][k], &bits, 4); }
        N.act_off[l] = N.act_floats;
        N.act_floats += L.rows;
    }
    N.R1 = N.layer[0].rows * n_features; N.Rs = n_rows - N.R1;
    N.C = N.layer[N.n_layers - 1].rows / (N.heads ? 2u : 1u);
    N.B_pad = (batch_size + 31u) / 32u * 32u;
    const std::string s = mid ? bsvi_bnn_source::mid_source(N) : bsvi_bnn_source::upper_source(N);
    fputs(s.c_str(), stdout);
    return 0;
}
