"""The posterior-predictive pass of the Bayesian-neural-network family (`CompiledBnn.predict`, bsvi_bnn_predict): N weight
sets from the current posterior, the chain forward on rows the caller hands in, per-sample outputs, their mean over the samples (and the
Normal's variance), draws from the likelihood — and the reference's own call, `model._get_posterior_sample(N, input_values={x: rows})`.

The yardstick is the one of tests/test_gpu_bnn_middle.py: the chain written HERE in numpy, in float64 and in float32, on the parameters
and the noise the call REPORTS; per returned tensor  err <= max(4 |chain32 - chain64|, 1e-5 max |chain64|).  Shapes are the smallest that
cross each edge: N = 70 (a second block of 64 samples, ragged), M = 33 (a second block of 32 rows, ragged), P = 16.

Which arm of the forward kernel: predict_lds_bytes (csrc/bnn_select.h) = (Rs 65 + 2 max_width 256) 4 bytes against 150 KiB.  32-64-8 has
Rs = 584 and width 64: 282 912 bytes, the GLOBAL arm; 32-16-16-4 has Rs = 356 and width 16: 125 328 bytes, the LDS arm.

Draws: Categorical and Bernoulli draws must EQUAL the host rule applied in float32 to the device's own probabilities and the host
reference's u01 (tests written from the contract in csrc/philox.h); Normal draws are compared as (draw - loc) / sigma with the host's
single-precision Box-Muller under the Normal bound of tests/test_gpu_noise.py (16 x the host's single-against-double error, at most 1e-4).
"""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from brancher_amd import bnn, engine, lowering, native, workloads as W
from oracle import philox_ref as R

pytestmark = pytest.mark.gpu
TOL = 1e-5
N, M, P = 70, 33, 16
KEY_PREDICT = 0x2545F491
CYCLE = ["tanh", "relu", "sigmoid", "softplus", "tanh", "relu", "sigmoid"]
FIXTURES = ["bnn_predict_classifier_16_5_3", "bnn_predict_bernoulli_16_4_1", "bnn_predict_regression_16_5_2"]
NORMAL_TOL = min(16 * float(np.abs(R.normal_rows(0x1234567890ABC, 3, np.arange(1 << 16), np.arange(8), dtype=np.float32).astype(np.float64)
                                   - R.normal_rows(0x1234567890ABC, 3, np.arange(1 << 16), np.arange(8))).max()), 1e-4)


def classifier(widths, **kw):
    # (the scale of weights1 keeps the hidden units off saturation on integer features: 0.4 / sqrt(sum_p E x_p^2), E x^2 = 4)
    kw = dict(dict(widths=widths, batch_size=8, dataset_size=40, pixels="integers", q_scale1=0.4 / np.sqrt(widths[0] * 4.0), q_loc_scale=1.0), **kw)
    return W.build_bayesian_neural_network(W.native_api(), **kw)


def regression(widths, **kw):
    return W.build_bnn_regression(W.native_api(), **dict(dict(widths=widths, batch_size=8, dataset_size=40, q_scale=0.3), **kw))


MODELS = {
    "classifier": lambda: classifier([P, 5, 3]),
    "one_layer": lambda: regression([P, 3], bias=False, sigma=0.5),
    "bernoulli": lambda: classifier([P, 6, 1], activation="relu"),
    "normal_per_output": lambda: regression([P, 5, 2], sigma=[0.3, 0.6]),
    "normal_shared": lambda: regression([P, 5, 2], sigma=0.5),
    "eight_layers": lambda: classifier([P, 6, 6, 6, 6, 6, 6, 6, 3], activations=CYCLE, q_scale=0.5),
    "wide": lambda: classifier([32, 64, 8]),
    "deep": lambda: classifier([32, 16, 16, 4]),
}


def compiled(name):
    model = MODELS[name]()
    c = bnn.CompiledBnn(model, model.posterior_model, "pathwise")
    assert type(c).__name__ == "CompiledBnn"
    return c


def rows_for(c, kind, m=M, seed=3):
    rng = np.random.RandomState(seed)
    p = c.program.n_features
    return (rng.randint(-3, 4, size=(m, p)) if kind == "integers" else rng.normal(size=(m, p))).astype(np.float32)


def sigmas(p):
    out = []
    for c in range(p.n_classes):
        e = p.uniform[p.scale_uniform + c * p.scale_stride]
        x = float(p.consts[e["src"]])
        g = {lowering.UT["identity"]: x, lowering.UT["softplus"]: float(np.log1p(np.exp(x)))}[int(e["transform"])]
        out.append(float(e["a"]) + float(e["b"]) * g)
    return np.array(out)


ACT = {0: lambda v: v, 1: np.tanh, 2: lambda v: np.maximum(v, v.dtype.type(0)), 3: lambda v: v.dtype.type(1) / (v.dtype.type(1) + np.exp(-v)),
       4: lambda v: np.logaddexp(v, v.dtype.type(0))}


def chain(c, noise, rows, dtype):
    """the whole pass in numpy at `dtype`, on the current parameters and the reported noise [R, n] -> dict of the call's tensors"""
    p = c.program
    loc, scale = bnn.row_parameters(p, c.params.detach().cpu().numpy())
    w = (loc.astype(dtype)[None, :] + scale.astype(dtype)[None, :] * noise.T.astype(dtype)).astype(dtype)      # [n, R]
    h = np.broadcast_to(rows.astype(dtype)[None], (w.shape[0],) + rows.shape)
    for layer in p.layers:
        r, k, w0, b0 = layer["rows"], layer["cols"], layer["weight_row0"], layer["bias_row0"]
        h = np.einsum("nmc,nrc->nmr", h, w[:, w0:w0 + r * k].reshape(-1, r, k)).astype(dtype)
        if b0 != bnn.NO_BIAS:
            h = h + w[:, None, b0:b0 + r]
        h = ACT[layer["activation"]](h).astype(dtype)
    out = dict(outputs=h)
    if p.likelihood == bnn.LIK_CATEGORICAL:
        e = np.exp(h - h.max(axis=2, keepdims=True))
        out["probs"] = e / e.sum(axis=2, keepdims=True)
    elif p.likelihood == bnn.LIK_BERNOULLI:
        out["probs"] = dtype(1) / (dtype(1) + np.exp(-h))
    else:
        out["probs"] = h
        out["var"] = h.var(axis=0) + sigmas(p).astype(dtype)[None, :] ** 2
    out["mean"] = out["probs"].mean(axis=0)
    return {k: np.asarray(v, dtype=dtype) for k, v in out.items()}


def yardstick(c, res, rows, label=""):
    noise = res["noise"].cpu().numpy()
    c64, c32 = chain(c, noise, rows, np.float64), chain(c, noise, rows, np.float32)
    bad = []
    for key, e64 in c64.items():
        got = res[key].cpu().numpy().astype(np.float64)
        assert got.shape == e64.shape, (key, got.shape, e64.shape)
        err, yard, scale = np.abs(got - e64).max(), np.abs(c32[key].astype(np.float64) - e64).max(), np.abs(e64).max()
        bound = max(4 * yard, TOL * scale)
        print("%s %-8s err %.3g  chain32 %.3g  scale %.3g  err/bound %.3g" % (label, key, err, yard, scale, err / bound))
        if not err <= bound:
            bad.append((key, err, yard, scale))
    assert not bad, bad
    return c64


def predict_all(c, rows, n=N, **kw):
    return c.predict(rows, n, **dict(dict(seed=5, offset=9, want_outputs=True, want_draws=True, want_noise=True), **kw))


@pytest.mark.parametrize("name,data,path", [("classifier", "integers", "bf16x3"), ("classifier", "real", "f32"), ("one_layer", "integers", "bf16x3"),
                                            ("bernoulli", "real", "f32"), ("normal_per_output", "integers", "bf16x3"),
                                            ("normal_shared", "real", "f32"), ("eight_layers", "integers", "bf16x3")])
def test_the_pass_matches_the_chain_in_double_precision_on_the_reported_draws(name, data, path):
    c = compiled(name)
    rows = rows_for(c, data)
    res = predict_all(c, rows)
    assert res["data_path"] == path and res["n_rows"] == M
    assert ("var" in res) == (c.program.likelihood == bnn.LIK_NORMAL)
    assert all(bool(torch.isfinite(res[k]).all()) for k in ("probs", "mean", "outputs", "draws", "noise"))
    yardstick(c, res, rows, "%s %s" % (name, data))
    # the reference's layouts of the rows are the same call
    for shaped in (rows.reshape(M, -1, 1), rows.reshape(1, M, -1, 1)):
        again = predict_all(c, shaped)
        assert all(torch.equal(again[k], res[k]) for k in ("probs", "mean", "outputs", "draws", "noise"))


@pytest.mark.parametrize("name,arm", [("wide", "global"), ("deep", "lds")])
@pytest.mark.parametrize("data,path", [("integers", "bf16x3"), ("real", "f32")])
def test_both_arms_of_the_forward_kernel(name, arm, data, path):
    c = compiled(name)
    assert c.predict_path() == arm, c.predict_path()
    rows = rows_for(c, data)
    res = predict_all(c, rows)
    assert res["data_path"] == path and c.predict_path() == arm
    yardstick(c, res, rows, "%s %s" % (name, data))


@pytest.mark.parametrize("name,data", [("classifier", "integers"), ("classifier", "real"), ("normal_per_output", "real"), ("wide", "integers")])
def test_three_passes_of_32_rows_are_bit_equal_to_one_pass(name, data):
    c = compiled(name)
    rows = rows_for(c, data, m=70)
    one = predict_all(c, rows)
    three = predict_all(c, rows, rows_per_pass=32)
    assert one["rows_per_pass"] == 96 and three["rows_per_pass"] == 32
    for key in ("probs", "mean", "outputs", "draws", "noise") + (("var",) if "var" in one else ()):
        assert torch.equal(one[key], three[key]), key
    yardstick(c, three, rows, "%s %s three passes" % (name, data))
    with pytest.raises(ValueError, match="multiple of 32"):
        c.predict(rows, N, rows_per_pass=40)


def host_words(res, n, m, key1=0, base=0):
    """the four words of the predictive stream's call for every (sample, row): [4][n][m]"""
    (k0, k1), (o0, o1) = R.split64(res["seed"]), R.split64(res["offset"])
    s, r = np.arange(base, base + n, dtype=np.uint64)[:, None], np.arange(m, dtype=np.uint64)[None, :]
    return R.philox4x32(s, r, o0, o1, k0 ^ KEY_PREDICT, k1 ^ key1)


@pytest.mark.parametrize("name", ["classifier", "eight_layers", "wide"])
def test_categorical_draws_equal_the_host_rule_on_the_devices_probabilities(name):
    c = compiled(name)
    res = predict_all(c, rows_for(c, "integers"), seed=0x1234567890ABC, offset=(1 << 62) + 5)
    probs, draws = res["probs"].cpu().numpy(), res["draws"].cpu().numpy()
    u = R.u01(host_words(res, N, M)[0])
    cum = np.cumsum(probs, axis=2, dtype=np.float32)
    hit = cum >= u[:, :, None]
    pick = np.where(hit.any(axis=2), hit.argmax(axis=2), probs.shape[2] - 1)
    assert np.array_equal(draws, np.eye(probs.shape[2], dtype=np.float32)[pick])
    assert len(np.unique(pick)) == probs.shape[2]            # every class is drawn somewhere: the rule is exercised


def test_bernoulli_draws_equal_the_host_rule():
    c = compiled("bernoulli")
    res = predict_all(c, rows_for(c, "real"), seed=77, offset=3)
    u = R.u01(host_words(res, N, M)[0])
    draws = res["draws"].cpu().numpy()
    assert np.array_equal(draws[:, :, 0], (u < res["probs"].cpu().numpy()[:, :, 0]).astype(np.float32)) and 0 < draws.mean() < 1


@pytest.mark.parametrize("name,widths", [("normal_per_output", None), ("normal_six_outputs", [P, 5, 6])])
def test_normal_draws_follow_the_host_box_muller(name, widths):
    """six outputs: the second Philox call (key word k1 ^ 1) serves outputs 4 and 5"""
    if widths:
        model = regression(widths, sigma=[0.3, 0.6, 0.4, 0.5, 0.7, 0.2])
        c = bnn.CompiledBnn(model, model.posterior_model, "pathwise")
    else:
        c = compiled(name)
    res = predict_all(c, rows_for(c, "integers"), seed=0x1234567890ABC, offset=7)
    sg = sigmas(c.program)
    loc, draws = res["outputs"].cpu().numpy().astype(np.float64), res["draws"].cpu().numpy().astype(np.float64)
    e_dev = (draws - loc) / sg[None, None, :]
    worst = 0.0
    for c0 in range(0, len(sg), 4):
        x = host_words(res, N, M, key1=c0 >> 2)
        e = list(R.box_muller(x[0], x[1], dtype=np.float32)) + list(R.box_muller(x[2], x[3], dtype=np.float32))
        for j in range(min(4, len(sg) - c0)):
            worst = max(worst, float(np.abs(e_dev[:, :, c0 + j] - e[j].astype(np.float64)).max()))
    print("normal draws: |(draw - loc) / sigma - host box_muller32| %.3g, bound %.3g" % (worst, NORMAL_TOL))
    assert worst <= NORMAL_TOL


def test_noise_in_repeats_and_sample_base():
    c = compiled("classifier")
    rows = rows_for(c, "real")
    res = predict_all(c, rows)
    keys = ("probs", "mean", "outputs", "draws", "noise")
    again = predict_all(c, rows)
    assert all(torch.equal(res[k], again[k]) for k in keys)
    fed = predict_all(c, rows, noise=res["noise"])
    assert all(torch.equal(res[k], fed[k]) for k in keys)
    named = predict_all(c, rows, noise=c.named_noise(res["noise"].cpu().numpy(), N))
    assert all(torch.equal(res[k], named[k]) for k in keys)
    # the noise is the training stream's: what a launch of (seed, offset) reports
    assert torch.equal(res["noise"], c.evaluate(N, seed=5, offset=9, want_noise=True)["noise"])
    host = R.dense_noise(5, 9, 0, N, c.program.n_rows, dtype=np.float32)
    assert np.abs(res["noise"].cpu().numpy() - host).max() <= NORMAL_TOL
    tail = predict_all(c, rows, n=37, sample_base=33)
    assert torch.equal(tail["noise"], res["noise"][:, 33:])
    assert all(torch.equal(tail[k], res[k][33:]) for k in ("probs", "outputs", "draws"))
    other = predict_all(c, rows, offset=10)
    assert not torch.equal(other["noise"], res["noise"]) and not torch.equal(other["draws"], res["draws"])


def test_predict_leaves_the_training_state_alone_and_sees_stepped_parameters():
    c = compiled("classifier")
    rows = rows_for(c, "integers")
    c.evaluate(N, seed=1, offset=0)
    out, iteration, grads = c.out.clone(), c.iteration, c.read_grads(0, c.n_params).copy()
    first = predict_all(c, rows, offset=None)
    second = predict_all(c, rows, offset=None)
    assert first["offset"] >= (1 << 62) and second["offset"] == first["offset"] + 1
    assert torch.equal(c.out, out) and c.iteration == iteration and np.array_equal(c.read_grads(0, c.n_params), grads)
    before = c.params.clone()
    losses, finite = c.train(6, N, "Adam", seed=2, lr=0.01)
    assert bool(finite.all()) and not torch.equal(before, c.params)
    res = predict_all(c, rows)
    yardstick(c, res, rows, "after six Adam steps")
    stale = chain_with(c, before, res["noise"].cpu().numpy(), rows)
    assert np.abs(res["probs"].cpu().numpy() - stale).max() > 1e-4          # ... and not the parameters it was compiled with


def chain_with(c, params, noise, rows):
    keep = c.params
    try:
        c.params = params
        return chain(c, noise, rows, np.float64)["probs"]
    finally:
        c.params = keep


def test_the_argument_checks_that_need_a_model():
    c = compiled("wide")
    rows = torch.from_numpy(rows_for(c, "integers")).to(c.device)
    ws = torch.zeros(1024, dtype=torch.uint8, device=c.device)
    buf = torch.zeros(M * 8, device=c.device)
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def call(**kw):
        a = native.BnnPredictArgs(**dict(dict(params_dev=ptr(c.params), x_dev=ptr(rows), n_samples_local=4, n_rows=M, workspace_dev=ptr(ws)), **kw))
        return c.lib.bsvi_bnn_predict(c.handle, C.byref(a)), c.lib.bsvi_last_error()

    rc, msg = call(var_out=ptr(buf))
    assert rc == -1 and b"var_out is for the Normal likelihood" in msg
    rc, msg = call(n_samples_local=32768, rows_per_pass=1024)               # 64 hidden units x 32 768 samples x 1 024 rows = 2^31
    assert rc == -2 and b"32-bit index range" in msg
    rc, msg = call(rows_per_pass=48)
    assert rc == -1 and b"multiple of 32" in msg
    rc, msg = call(x_dev=None)
    assert rc == -1 and b"x_dev is null" in msg
    assert c.lib.bsvi_bnn_predict_workspace_bytes(c.handle, 4, M, 0) > c.lib.bsvi_bnn_predict_workspace_bytes(c.handle, 4, 1, 0) > 0
    assert c.lib.bsvi_bnn_predict_workspace_bytes(c.handle, 4, M, 48) == 0
    with pytest.raises(ValueError, match="17 features, the model was built on 32"):
        c.predict(np.zeros((3, 17), dtype=np.float32), 4)


# ---- through the public API, on the fixtures of the real reference (tools/gen_golden_bnn_predict.py) --------------------------------
@functools.lru_cache(maxsize=None)
def fixture(name):
    data = np.load(os.path.join(GOLDEN, "bnn_predict", name + ".npz"))
    return data, json.loads(str(data["meta"]))


def fixture_model(name):
    data, meta = fixture(name)
    model = getattr(W, meta["builder"])(W.native_api(), **meta["kwargs"])
    return model, next(v for v in model.flatten() if v.name == "x"), data, meta


@pytest.mark.parametrize("name", FIXTURES)
def test_get_posterior_sample_answers_with_the_references_keys_and_shapes(name):
    """On the commit before the predictive pass this raised LoweringError (the scalar sampler's: "no second half")."""
    model, x, data, meta = fixture_model(name)
    rows = torch.from_numpy(data["rows"])
    n = meta["n_shapes"]
    sample = model._get_posterior_sample(n, input_values={x: rows})
    assert {v.name: list(t.shape) for v, t in sample.items()} == meta["keys"]
    assert all(v in set(model.flatten()) for v in sample)                      # keyed by the JOINT model's variables
    lik = next(t for v, t in sample.items() if v.name == meta["likelihood"]).cpu().numpy()
    if meta["likelihood"] == "k":
        assert set(np.unique(lik)) <= {0.0, 1.0} and (lik.shape[2] == 1 or np.array_equal(lik.sum(axis=2), np.ones_like(lik.sum(axis=2))))
    # (the engine that answered: the model's own, or — 16-4-1 trains on the scalar engine — the one kept for prediction)
    c = engine._bnn_predictor(model, engine.compile_model(model, None, None))
    assert type(c).__name__ == "CompiledBnn"
    for pname, value in c.named_params().items():
        assert np.allclose(value.reshape(-1), data["param/" + pname].reshape(-1), rtol=1e-6, atol=1e-7), pname
    # a latent is what was drawn: loc + scale eps, inside five scales of its loc
    loc, scale = bnn.row_parameters(c.program, c.params.cpu().numpy())
    for t in c.program.tensors:
        w = next(v for k, v in sample.items() if k.name == t["name"]).cpu().numpy().reshape(n, -1)
        sl = slice(t["row0"], t["row0"] + t["size"])
        assert np.abs((w - loc[sl]) / scale[sl]).max() < 6.0 and np.abs(w[0] - w[1]).max() > 0
    frame = model.get_posterior_sample(3, input_values={x: rows})
    assert frame.shape[0] == 3 and meta["likelihood"] in frame.columns and "weights1" in frame.columns
    minibatch = model._get_posterior_sample(n)
    assert {v.name: list(t.shape) for v, t in minibatch.items()} == meta["keys_no_input"]
    idx = next(t for v, t in minibatch.items() if v.name == "indices").cpu().numpy()
    xs = next(t for v, t in minibatch.items() if v.name == "x").cpu().numpy()
    assert len(set(idx.tolist())) == meta["kwargs"]["batch_size"] and np.array_equal(xs[0, :, :, 0], c.program.dataset[idx]) and np.array_equal(xs[0], xs[-1])


@pytest.mark.parametrize("name", FIXTURES)
def test_the_predictive_agrees_with_the_real_reference_statistically(name):
    model, x, data, meta = fixture_model(name)
    c = bnn.CompiledBnn(model, model.posterior_model, "pathwise")
    n_dev, n_ref = 4000, meta["n_ref"]
    res = c.predict(data["rows"], n_dev, seed=2024, offset=1, want_draws=True)
    mean, draws = res["mean"].cpu().numpy().astype(np.float64), res["draws"].cpu().numpy().astype(np.float64)
    if meta["likelihood"] == "k":
        p = data["p"]
        bound = 5 * np.sqrt(p * (1 - p) * (1.0 / n_ref + 1.0 / n_dev))
        print(name, "mean - ref", np.abs(mean - data["ref_freq"]).max(), "draws - ref", np.abs(draws.mean(0) - data["ref_freq"]).max(), "bound", bound.min())
        assert (np.abs(mean - data["ref_freq"]) <= bound).all() and (np.abs(draws.mean(0) - data["ref_freq"]) <= bound).all()
    else:
        v, m4 = data["exact_var"], data["exact_m4"]
        b_mean = 5 * np.sqrt(v * (1.0 / n_ref + 1.0 / n_dev))
        b_var = 5 * np.sqrt((m4 - v ** 2) * (1.0 / n_ref + 1.0 / n_dev))
        var = res["var"].cpu().numpy().astype(np.float64)
        print(name, "mean", np.abs(mean - data["ref_mean"]).max(), b_mean.min(), "var", np.abs(var - data["ref_var"]).max(), b_var.min())
        assert (np.abs(mean - data["ref_mean"]) <= b_mean).all() and (np.abs(draws.mean(0) - data["ref_mean"]) <= b_mean).all()
        assert (np.abs(var - data["ref_var"]) <= b_var).all() and (np.abs(draws.var(0) - data["ref_var"]) <= b_var).all()
