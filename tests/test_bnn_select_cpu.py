"""Which kernel serves the middle of a Bayesian-neural-network iteration (brancher_amd/csrc/bnn_select.h: host only, no HIP, no
environment) against its table: tests/c_abi/bnn_select_table.cpp holds the rows that tests/test_gpu_bnn_middle.py runs on the device,
both sides of the three thresholds and a sweep over every realisable network — compiled here from the header alone, with the address
and undefined-behaviour sanitizers."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def table_output(tmp_path_factory):
    exe = tmp_path_factory.mktemp("bnn_select") / "bnn_select_table"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "brancher_amd", "csrc"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "c_abi", "bnn_select_table.cpp")])
    return subprocess.run([str(exe)], capture_output=True, text=True)


def test_selection_reproduces_the_table_rows_and_the_thresholds(table_output):
    assert table_output.returncode == 0, table_output.stdout + table_output.stderr


def test_no_realisable_network_selects_the_lds_kernel_with_both_generators_on(table_output):
    """with widths 1 .. 64 and one to eight layers, Rs <= act^2 / 4 + act; the generated register kernel declines from
    Rs + 2 act > 400 (act > 34) while the static kernel's LDS tile holds act < 33 — bnn_upper<true> is reached through BSVI_BNN_JIT=0 alone"""
    assert "upper_lds reachable with both switches on: no" in table_output.stdout, table_output.stdout


def test_widths_and_activations_build_any_depth_and_nine_layers_are_refused_with_the_limit_named():
    from brancher_amd import bnn, lowering, workloads as W
    api = W.native_api()
    acts = ["tanh", "relu", "sigmoid", "softplus", "tanh", "relu", "sigmoid"]
    for make, kw in ((W.build_bayesian_neural_network, dict(pixels="integers")), (W.build_bnn_regression, dict())):
        model = make(api, widths=[32, 6, 6, 6, 6, 6, 6, 6, 3], activations=acts, batch_size=17, dataset_size=40, **kw)
        p = bnn.lower_bnn(model, model.posterior_model, "pathwise")
        assert [(l["rows"], l["cols"]) for l in p.layers] == [(6, 32)] + [(6, 6)] * 6 + [(3, 6)]
        assert [l["activation"] for l in p.layers] == [bnn.ACTIVATIONS[a] for a in acts] + [0]
        assert p.n_rows == 6 * 32 + 279 and p.n_features == 32 and p.n_classes == 3
        nine = make(api, widths=[32] + [4] * 8 + [3], batch_size=17, dataset_size=40, **kw)
        with pytest.raises(lowering.LoweringError, match="the network has 9 layers, the kernels serve at most 8"):
            bnn.lower_bnn(nine, nine.posterior_model, "pathwise")
    # the keywords spelled as a list build the same model, draw for draw
    kw = dict(dataset_size=40, batch_size=17, q_scale1=3e-3, q_loc_scale=1.0)
    a = W.build_bayesian_neural_network(api, n_features=64, n_hidden=9, hidden2=6, n_classes=5, activation="relu", **kw)
    b = W.build_bayesian_neural_network(api, widths=[64, 9, 6, 5], activations=["relu", "relu"], **kw)
    pa, pb = (bnn.lower_bnn(m, m.posterior_model, "pathwise") for m in (a, b))
    assert np.array_equal(pa.dataset, pb.dataset) and np.array_equal(pa.labels, pb.labels) and np.array_equal(pa.row_uniform, pb.row_uniform)
    for (para, _, _, _), (parb, _, _, _) in zip(pa.parameters, pb.parameters):
        assert para.name == parb.name and np.array_equal(para.numpy(), parb.numpy())
    with pytest.raises(ValueError):
        W.build_bnn_regression(api, widths=[32, 6, 3], activations=["tanh", "relu"])


def test_the_python_names_follow_the_enum():
    from brancher_amd import bnn
    header = open(os.path.join(ROOT, "brancher_amd", "csrc", "bnn_select.h")).read()
    for value, (c_name, py_name) in enumerate(zip(("MID_GEN", "UPPER_GEN", "UPPER_LDS", "UPPER_MEM"), bnn.MIDDLE_PATHS)):
        assert "%s = %d," % (c_name, value) in header or "%s = %d " % (c_name, value) in header
        assert 'case %s: return "%s";' % (c_name, py_name) in header
    assert "BNN_MAX_LAYERS = %d;" % bnn.MAX_LAYERS in open(os.path.join(ROOT, "brancher_amd", "csrc", "bnn_kernel.inc")).read()
