"""The activations of the Bayesian-neural-network family behind tanh / relu / sigmoid / softplus (bnn._activation, bnn.lower_bnn,
bsvi_bnn_set_activation_params, csrc/bnn_source.h) as far as they go without a device: what every name lowers to, with
torch's defaults and with parameters given as keywords or as positional numbers; every refusal by its cause; the four old kinds left as
they were; the builders' `activations=`; the export; and the text bnn_source.h writes for such networks — compiled here from the header
alone (the existing driver for default parameters, tests/c_abi/bnn_source_params.cpp for given ones, both with the address and
undefined-behaviour sanitizers)."""
import importlib.util
import json
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from brancher_amd import bnn, native, workloads as W
from brancher_amd.lowering import LoweringError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("bnn_source_dump", os.path.join(ROOT, "tools", "bnn_source_dump.py"))
dump = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(dump)
DIGESTS = json.load(open(os.path.join(ROOT, "tests", "golden", "bnn_source", "digests.json")))
P, H, C_OUT, DS, B = 8, 3, 2, 12, 5
# name: (bsvi_bnn_activation, the two parameters with torch's defaults)
DEFAULTS = dict(leaky_relu=(5, (0.01, 0.0)), elu=(6, (1.0, 0.0)), selu=(7, (0.0, 0.0)), softsign=(8, (0.0, 0.0)), hardtanh=(9, (-1.0, 1.0)),
                relu6=(9, (0.0, 6.0)), silu=(10, (0.0, 0.0)), gelu=(11, (0.0, 0.0)))


def network(act):
    """P-H-C regression whose hidden layer is act(BF, pre-activation): the graph a user writes, not a builder's"""
    api = W.native_api()
    BF, rng = api.BF, np.random.RandomState(0)
    X = rng.randint(-3, 4, size=(DS, P, 1)).astype(np.float32)
    Y = rng.normal(size=(DS, C_OUT, 1)).astype(np.float32)
    indices = api.RandomIndices(dataset_size=DS, batch_size=B, name="indices", is_observed=True)
    x = api.EmpiricalVariable(X, indices=indices, name="x", is_observed=True)
    targets = api.EmpiricalVariable(Y, indices=indices, name="targets", is_observed=True)
    shapes = dict(weights1=(H, P), b1=(H, 1), weights2=(C_OUT, H), b2=(C_OUT, 1))
    t = {name: api.NormalVariable(np.zeros(s), np.ones(s), name) for name, s in shapes.items()}
    hidden = act(BF, BF.matmul(t["weights1"], x) + t["b1"])
    y = api.NormalVariable(BF.matmul(t["weights2"], hidden) + t["b2"], 0.5, "y")
    model = api.ProbabilisticModel([y])
    y.observe(targets)
    model.set_posterior_model(api.ProbabilisticModel([api.NormalVariable(0.1 * rng.normal(size=s), 0.1 * np.ones(s), name, learnable=True)
                                                      for name, s in shapes.items()]))
    return model


def lower(act):
    m = network(act)
    return bnn.lower_bnn(m, m.posterior_model, "pathwise")


@pytest.mark.parametrize("name", sorted(DEFAULTS))
def test_every_name_lowers_with_torchs_defaults(name):
    p = lower(lambda BF, h: getattr(BF, name)(h))
    kind, params = DEFAULTS[name]
    first, last = p.layers
    assert first["activation"] == kind == bnn.ACTIVATIONS[name] and first["activation_params"] == params and first["activation_name"] == name
    assert last["activation"] == 0 and "activation_params" not in last
    assert p.summary()["layers"] == [(H, P, kind), (C_OUT, H, 0)]


GIVEN = {
    "leaky_relu keyword": (lambda BF, h: BF.leaky_relu(h, negative_slope=0.2), 5, (0.2, 0.0), "leaky_relu(negative_slope=0.2)"),
    "leaky_relu positional": (lambda BF, h: BF.leaky_relu(h, 0.2), 5, (0.2, 0.0), "leaky_relu(negative_slope=0.2)"),
    "leaky_relu inplace=False": (lambda BF, h: BF.leaky_relu(h, 0.2, inplace=False), 5, (0.2, 0.0), "leaky_relu(negative_slope=0.2)"),
    "elu keyword": (lambda BF, h: BF.elu(h, alpha=0.7), 6, (0.7, 0.0), "elu(alpha=0.7)"),
    "elu positional integer": (lambda BF, h: BF.elu(h, 2), 6, (2.0, 0.0), "elu(alpha=2)"),
    "hardtanh positional": (lambda BF, h: BF.hardtanh(h, -0.5, 2.0), 9, (-0.5, 2.0), "hardtanh(min_val=-0.5, max_val=2)"),
    "hardtanh keywords": (lambda BF, h: BF.hardtanh(h, max_val=2.0, min_val=-0.5), 9, (-0.5, 2.0), "hardtanh(min_val=-0.5, max_val=2)"),
    "hardtanh mixed": (lambda BF, h: BF.hardtanh(h, -0.5, max_val=2.0), 9, (-0.5, 2.0), "hardtanh(min_val=-0.5, max_val=2)"),
    "hardtanh one limit": (lambda BF, h: BF.hardtanh(h, max_val=0.25), 9, (-1.0, 0.25), "hardtanh(min_val=-1, max_val=0.25)"),
    "relu6": (lambda BF, h: BF.relu6(h, inplace=False), 9, (0.0, 6.0), "relu6"),
    "gelu approximate none": (lambda BF, h: BF.gelu(h, approximate="none"), 11, (0.0, 0.0), "gelu"),
    "silu inplace=False": (lambda BF, h: BF.silu(h, inplace=False), 10, (0.0, 0.0), "silu"),
    "numpy scalar": (lambda BF, h: BF.leaky_relu(h, np.float32(0.25)), 5, (0.25, 0.0), "leaky_relu(negative_slope=0.25)"),
}


@pytest.mark.parametrize("case", sorted(GIVEN))
def test_parameters_as_keywords_and_as_positional_numbers(case):
    act, kind, params, text = GIVEN[case]
    p = lower(act)
    assert p.layers[0]["activation"] == kind and p.layers[0]["activation_params"] == params
    assert all(isinstance(v, float) for v in p.layers[0]["activation_params"])
    assert p.summary()["activations"] == [text]


def test_relu6_lowers_to_hardtanh_0_6():
    p = lower(lambda BF, h: BF.relu6(h))
    assert p.layers[0]["activation"] == bnn.ACTIVATIONS["hardtanh"] == 9 and p.layers[0]["activation_params"] == (0.0, 6.0)
    assert p.summary()["activations"] == ["relu6"]


def _a_variable(BF):
    return W.native_api().RootVariable(0.2, "slope")


REFUSALS = {
    "a variable as the slope": (lambda BF, h: BF.leaky_relu(h, negative_slope=_a_variable(BF)), r"BF\.leaky_relu .*negative_slope is not a number"),
    "a variable as a positional slope": (lambda BF, h: BF.leaky_relu(h, _a_variable(BF)), r"BF\.leaky_relu .*negative_slope is not a number"),
    "an array as alpha": (lambda BF, h: BF.elu(h, alpha=np.ones(3)), r"BF\.elu .*alpha is not a number"),
    "a boolean as alpha": (lambda BF, h: BF.elu(h, alpha=True), r"BF\.elu .*alpha is not a number"),
    "inplace": (lambda BF, h: BF.leaky_relu(h, 0.2, inplace=True), r"BF\.leaky_relu .*inplace=True is not served"),
    "inplace relu6": (lambda BF, h: BF.relu6(h, inplace=True), r"BF\.relu6 .*inplace=True is not served"),
    "inplace silu": (lambda BF, h: BF.silu(h, inplace=True), r"BF\.silu .*inplace=True is not served"),
    "tanh gelu": (lambda BF, h: BF.gelu(h, approximate="tanh"), r"BF\.gelu .*approximate='tanh' is not served \(only approximate='none'\)"),
    "slope zero": (lambda BF, h: BF.leaky_relu(h, 0.0), r"BF\.leaky_relu .*negative_slope > 0 in single precision \(got negative_slope=0\)"),
    # the library takes single precision: what is 0, infinite or equal there is refused here, by the function's name
    "slope zero in single precision": (lambda BF, h: BF.leaky_relu(h, 1e-50), r"BF\.leaky_relu .*negative_slope > 0 in single precision"),
    "alpha infinite in single precision": (lambda BF, h: BF.elu(h, alpha=1e39), r"BF\.elu .*finite parameters"),
    "limits equal in single precision": (lambda BF, h: BF.hardtanh(h, 1.0, 1.0 + 1e-9), r"BF\.hardtanh .*min_val < max_val in single precision"),
    "slope negative": (lambda BF, h: BF.leaky_relu(h, negative_slope=-0.1), r"BF\.leaky_relu .*negative_slope > 0"),
    "slope not finite": (lambda BF, h: BF.leaky_relu(h, float("inf")), r"BF\.leaky_relu .*finite parameters"),
    "alpha zero": (lambda BF, h: BF.elu(h, alpha=0.0), r"BF\.elu .*alpha > 0"),
    "limits equal": (lambda BF, h: BF.hardtanh(h, 1.0, 1.0), r"BF\.hardtanh .*min_val < max_val in single precision \(got min_val=1, max_val=1\)"),
    "limits swapped": (lambda BF, h: BF.hardtanh(h, min_val=2.0, max_val=-0.5), r"BF\.hardtanh .*min_val < max_val"),
    "unknown keyword": (lambda BF, h: BF.elu(h, beta=1.0), r"BF\.elu .*unknown keyword 'beta'"),
    "unknown keyword of a plain name": (lambda BF, h: BF.gelu(h, alpha=1.0), r"BF\.gelu .*unknown keyword 'alpha'"),
    "too many numbers": (lambda BF, h: BF.leaky_relu(h, 0.2, 0.3), r"BF\.leaky_relu .*2 positional arguments"),
    "a number for selu": (lambda BF, h: BF.selu(h, 1.0), r"BF\.selu .*1 positional arguments"),
    "a keyword twice": (lambda BF, h: BF.hardtanh(h, -0.5, min_val=-0.25), r"BF\.hardtanh .*min_val is given twice"),
    "softsign with a keyword": (lambda BF, h: BF.softsign(h, inplace=False), r"BF\.softsign takes the layer alone"),
    "another function": (lambda BF, h: BF.celu(h), r"between two layers stands one of BF\.tanh / BF\.relu / BF\.sigmoid / BF\.softplus / "
                         r"BF\.leaky_relu / BF\.elu / BF\.selu / BF\.softsign / BF\.hardtanh / BF\.relu6 / BF\.silu / BF\.gelu \(not BF\.celu\)"),
    "prelu": (lambda BF, h: BF.prelu(h, _a_variable(BF)), r"between two layers stands one of .*\(not BF\.prelu\)"),
    "tanh with a keyword": (lambda BF, h: BF.tanh(h, out=None), r"between two layers stands one of .*BF\.tanh takes the layer alone"),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_every_refusal_names_the_function_and_the_cause(case):
    act, cause = REFUSALS[case]
    with pytest.raises(LoweringError, match=cause):
        lower(act)


@pytest.mark.parametrize("name", ["tanh", "relu", "sigmoid", "softplus"])
def test_the_four_old_kinds_lower_to_the_layers_they_lowered_to(name):
    p = lower(lambda BF, h: getattr(BF, name)(h))
    kind = dict(tanh=1, relu=2, sigmoid=3, softplus=4)[name]
    assert p.layers == [dict(rows=H, cols=P, weight_row0=0, bias_row0=H * P, activation=kind, weights="weights1", bias="b1"),
                        dict(rows=C_OUT, cols=H, weight_row0=H * P + H, bias_row0=H * P + H + C_OUT * H, activation=0, weights="weights2", bias="b2")]
    assert "activations" not in p.summary() and p.summary()["layers"] == [(H, P, kind), (C_OUT, H, 0)]


def test_the_builders_take_a_name_or_a_name_with_keywords_per_hidden_layer():
    acts = [("leaky_relu", dict(negative_slope=0.2)), "selu", ("hardtanh", dict(min_val=-0.5, max_val=2.0)), "gelu"]
    want = [(5, (0.2, 0.0)), (7, (0.0, 0.0)), (9, (-0.5, 2.0)), (11, (0.0, 0.0))]
    for model in (W.build_bayesian_neural_network(W.native_api(), widths=[16, 5, 4, 4, 3, 2], activations=acts, batch_size=7, dataset_size=12, pixels="integers"),
                  W.build_bnn_regression(W.native_api(), widths=[16, 5, 4, 4, 3, 2], activations=acts, batch_size=7, dataset_size=12)):
        p = bnn.lower_bnn(model, model.posterior_model, "pathwise")
        assert [(l["activation"], l["activation_params"]) for l in p.layers[:-1]] == want
        assert p.summary()["activations"] == ["leaky_relu(negative_slope=0.2)", "selu", "hardtanh(min_val=-0.5, max_val=2)", "gelu"]
    one = W.build_bnn_regression(W.native_api(), n_features=16, n_hidden=5, activation="silu", batch_size=7, dataset_size=12)
    assert bnn.lower_bnn(one, one.posterior_model, "pathwise").layers[0]["activation"] == 10
    # the teacher of the regression builder applies the same functions: torch's values, in double
    import torch
    v = np.linspace(-3.0, 7.0, 41)
    F = torch.nn.functional
    for name, kw in (("leaky_relu", dict(negative_slope=0.2)), ("elu", dict(alpha=0.7)), ("selu", {}), ("softsign", {}), ("relu6", {}),
                     ("hardtanh", dict(min_val=-0.5, max_val=2.0)), ("silu", {}), ("gelu", {}), ("leaky_relu", {}), ("hardtanh", {})):
        assert np.allclose(W._np_activation(name, kw)(v), getattr(F, name)(torch.as_tensor(v), **kw).numpy(), rtol=1e-12, atol=1e-14), name


def test_the_abi_stays_11_with_one_more_export():
    header = open(os.path.join(ROOT, "include", "bsvi.h")).read()
    assert native.ABI_VERSION == 11 and re.search(r"#define\s+BSVI_ABI_VERSION\s+11\b", header)
    assert "int bsvi_bnn_set_activation_params(bsvi_bnn* b, const float* params /* [n_layers][2] */, uint32_t n_layers);" in header
    assert "BSVI_BNN_ACT_LEAKY_RELU = 5, BSVI_BNN_ACT_ELU = 6, BSVI_BNN_ACT_SELU = 7, BSVI_BNN_ACT_SOFTSIGN = 8, BSVI_BNN_ACT_HARDTANH = 9" in header
    assert "BSVI_BNN_ACT_SILU = 10, BSVI_BNN_ACT_GELU = 11" in header
    assert "bsvi_bnn_set_activation_params" in native.EXPORTS
    lib = native.load()
    assert lib.bsvi_abi_version() == 11 and hasattr(lib, "bsvi_bnn_set_activation_params")
    assert lib.bsvi_bnn_set_activation_params(None, None, 0) == -1 and b"bsvi_bnn_set_activation_params: null argument" in lib.bsvi_last_error()


# ---- the text of the generated kernels ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    out = {}
    for name in ("bnn_source_text", "bnn_source_params"):
        exe = tmp_path_factory.mktemp("bnn_activations") / name
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-I", os.path.join(ROOT, "brancher_amd", "csrc"), "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                               os.path.join(ROOT, "tests", "c_abi", name + ".cpp")])
        out[name] = str(exe)
    return out


def with_params(p, args):
    """the arguments of bnn_source_text.cpp -> those of bnn_source_params.cpp: every layer followed by the bits of its two parameters"""
    bits = lambda x: struct.unpack("<I", struct.pack("<f", x))[0]
    out = list(args[:11])
    for l, layer in enumerate(p.layers):
        out += args[11 + 5 * l:16 + 5 * l] + [str(bits(v)) for v in layer.get("activation_params", (0.0, 0.0))]
    return out


def text(exe, kind, args):
    run = subprocess.run([exe, kind] + args, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    return run.stdout


SEVEN = ["leaky_relu", "elu", "selu", "softsign", "hardtanh", "silu", "gelu"]
SEVEN_GIVEN = [("leaky_relu", dict(negative_slope=0.2)), ("elu", dict(alpha=0.7)), "selu", "softsign", ("hardtanh", dict(min_val=-0.5, max_val=2.0)),
               "silu", "gelu"]


def eight_layers(activations):
    m = W.build_bayesian_neural_network(W.native_api(), widths=[16, 4, 4, 4, 4, 4, 4, 4, 2], activations=activations, batch_size=17, dataset_size=40,
                                        pixels="integers")
    return bnn.lower_bnn(m, m.posterior_model, "pathwise")


@pytest.mark.parametrize("kind", ["upper", "mid"])
def test_default_parameters_through_the_existing_driver(programs, kind):
    """the driver that knows nothing of parameters: a Net without them writes torch's defaults, and the same text as one that was handed them"""
    p = eight_layers(SEVEN)
    args = dump.describe(p, {})
    t = text(programs["bnn_source_text"], kind, args)
    assert t == text(programs["bnn_source_params"], kind, with_params(p, args))
    for literal in ("v > 0.0f ? v : 0.00999999978f * v", "sm > 0.0f ? sm : 1.0f * expm1f(sm)", "1.05070102f * (sm > 0.0f ? sm : 1.67326319f * expm1f(sm))",
                    "sm / (1.0f + fabsf(sm))", "fminf(fmaxf(sm, -1.0f), 1.0f)", "y[20u + i] = sm * sg; d[20u + i] = sg * (1.0f + sm * (1.0f - sg));",
                    "y[24u + i] = sm * cdf; d[24u + i] = cdf + sm * (0.398942280f * expf(-0.5f * sm * sm));",
                    # the reverse sweep: the output-side derivatives, and the delta slot multiplied in place for silu and gelu
                    "d[0u + j] = sm * (y[0u + j] > 0.0f ? 1.0f : 0.00999999978f);", "d[4u + j] = sm * (y[4u + j] > 0.0f ? 1.0f : y[4u + j] + 1.0f);",
                    "d[8u + j] = sm * (y[8u + j] > 0.0f ? 1.05070102f : y[8u + j] + 1.75809932f);",
                    "d[12u + j] = sm * ((1.0f - fabsf(y[12u + j])) * (1.0f - fabsf(y[12u + j])));",
                    "d[16u + j] = sm * (y[16u + j] > -1.0f && y[16u + j] < 1.0f ? 1.0f : 0.0f);", "d[20u + j] = sm * d[20u + j];", "d[24u + j] = sm * d[24u + j];"):
        assert literal in t, literal


@pytest.mark.parametrize("kind", ["upper", "mid"])
def test_given_parameters_appear_as_float_literals(programs, kind):
    p = eight_layers(SEVEN_GIVEN)
    t = text(programs["bnn_source_params"], kind, with_params(p, dump.describe(p, {})))
    for literal in ("v > 0.0f ? v : 0.200000003f * v", "d[0u + j] = sm * (y[0u + j] > 0.0f ? 1.0f : 0.200000003f);",
                    "sm > 0.0f ? sm : 0.699999988f * expm1f(sm)", "y[4u + j] > 0.0f ? 1.0f : y[4u + j] + 0.699999988f",
                    "fminf(fmaxf(sm, -0.5f), 2.0f)", "y[16u + j] > -0.5f && y[16u + j] < 2.0f ? 1.0f : 0.0f"):
        assert literal in t, literal
    assert "0.00999999978f" not in t
    # relu6: the literals of hardtanh(0, 6)
    m = W.build_bnn_regression(W.native_api(), widths=[16, 5, 4, 3], activations=["relu6", "tanh"], batch_size=17, dataset_size=40)
    p6 = bnn.lower_bnn(m, m.posterior_model, "pathwise")
    t6 = text(programs["bnn_source_params"], kind, with_params(p6, dump.describe(p6, {})))
    assert "fminf(fmaxf(v, 0.0f), 6.0f)" in t6 and "y[0u + j] > 0.0f && y[0u + j] < 6.0f ? 1.0f : 0.0f" in t6


@pytest.mark.parametrize("name", ["16-4x7-2 eight layers", "16-5-4-3 head softplus normal", "784-20-10 B512 (bench bnn_cfg4scale)"])
def test_the_text_of_the_old_kinds_is_the_recorded_one_with_parameters_handed_in(programs, name):
    """a network of tanh / relu / sigmoid / softplus through the driver that sets the parameters, as the library does for every network:
    the recorded digests of tests/golden/bnn_source"""
    kw, env = dump.CASES[name]
    model = dump.build(W, kw)
    p = bnn.lower_bnn(model, model.posterior_model, "pathwise")
    assert not any("activation_params" in l for l in p.layers)
    for kind in dump.KINDS:
        assert dump.digest(text(programs["bnn_source_params"], kind, with_params(p, dump.describe(p, env)))) == DIGESTS[name][kind], (name, kind)
