"""The exact-data iteration of the dense-link path as two fused launches (csrc/dense_xfused.inc: dense_xfwd draws the
weights in LDS beside the logits product and takes the cross-entropy in its epilogue, dense_xbwd reduces the gradient
product against the redrawn normals) against
  (1) the round-3 sequence of six launches on the same Philox stream and minibatch (BSVI_DENSE_FUSED=0), and
  (2) the f32-input MFMA kernels (BSVI_DENSE_XGEMM=0),
over shapes that exercise every edge of the tiling: classes that do not divide the 64 weight rows of a workgroup, a
feature count that is not a multiple of the 128-feature chunk or of the 112-row tile of x^T, minibatches below and above
one 512-row tile, sample counts that leave ragged sample groups, a single output, both estimators, emitted and supplied noise.
(The `C = 1` shapes are Categorical models with ONE class: log-probability 0 and likelihood gradient 0 whatever the labels, NOT the
Bernoulli likelihood — they compare the prior, the entropy and the launch plan.  The Bernoulli / Binomial(1) likelihood on the same
shapes, against the oracle: tests/test_gpu_dense_models.py.)  Reference behaviour: examples/MNIST_logistic_regression.py:15-54 through
brancher/variables.py:843-870 (pinned against the reference itself by the `logreg_pixels_*` fixtures in test_gpu_parity)."""
import numpy as np
import pytest
import torch

from brancher_amd import engine, workloads as W

pytestmark = pytest.mark.gpu

SHAPES = [
    # (dataset, batch, features, classes, samples)
    (96, 40, 784, 10, 24),
    (300, 130, 100, 3, 70),       # two k chunks short of full, one 112-row tile of x^T, ragged sample block
    (700, 520, 64, 16, 33),       # two 512-row tiles of the minibatch, 16 classes (four samples per workgroup)
    (200, 64, 236, 7, 130),       # three tiles of x^T with a ragged last one, 130 samples
    (64, 32, 32, 1, 50),          # smallest feature count of the path
]


def build(api, shape, **kw):
    ds, b, p, c, _ = shape
    return W.build_logistic_regression(api, dataset_size=ds, batch_size=b, n_features=p, n_classes=c, pixels="uint8", q_scale=0.02, **kw)


def outputs(c, n, **kw):
    res = c.evaluate(n, seed=13, offset=2, want_fvalues=True, want_indices=True, **kw)
    torch.cuda.synchronize()
    return dict(loss=float(res["loss"].item()), f=res["f"].cpu().numpy().astype(np.float64),
                grads=res["grads"].cpu().numpy().astype(np.float64), idx=res["indices"].cpu().numpy(),
                noise=res["noise"].cpu().numpy() if "noise" in res and res["noise"] is not None else None)


@pytest.mark.parametrize("estimator", ["pathwise", "blackbox"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "DS%d_B%d_P%d_C%d_N%d" % s)
def test_fused_launches_equal_the_six_launch_sequence_and_the_f32_kernels(shape, estimator, monkeypatch):
    api = W.native_api()
    n = shape[4]
    fused = engine.compile_model(build(api, shape), None, estimator)
    assert fused.data_path() == "bf16x3"
    monkeypatch.setenv("BSVI_DENSE_FUSED", "0")
    six = engine.compile_model(build(api, shape), None, estimator)
    monkeypatch.setenv("BSVI_DENSE_XGEMM", "0")
    plain = engine.compile_model(build(api, shape), None, estimator)
    assert plain.data_path() == "f32"
    a, b, c = outputs(fused, n, want_noise=True), outputs(six, n, want_noise=True), outputs(plain, n)
    assert np.array_equal(a["idx"], b["idx"]) and np.array_equal(a["idx"], c["idx"])
    assert np.array_equal(a["noise"], b["noise"])                  # the same Philox counters
    fscale, gscale = np.abs(c["f"]).max(), max(np.abs(c["grads"]).max(), 1e-3)     # (one class: the likelihood's gradient is zero)
    bb = estimator == "blackbox"
    for other in (b, c):
        assert np.abs(a["f"] - other["f"]).max() <= 2e-5 * fscale
        assert abs(a["loss"] - other["loss"]) <= (2e-4 if bb else 2e-5) * abs(other["loss"])
        assert np.abs(a["grads"] - other["grads"]).max() <= (5e-4 if bb else 5e-5) * gscale + 1e-6
    # bit-reproducible call to call, with and without the diagnostic outputs
    again = outputs(fused, n, want_noise=True)
    assert again["loss"] == a["loss"] and np.array_equal(again["grads"], a["grads"]) and np.array_equal(again["f"], a["f"])
    # the emitted noise, fed back, reproduces the call (supplied-noise path of both launches)
    ds, bsz, p, ncls, _ = shape
    named = {"weights": a["noise"].T.reshape(n, 1, ncls, p)}
    replay = fused.evaluate(n, noise=named, minibatch={"indices": a["idx"].tolist()}, want_fvalues=True)
    torch.cuda.synchronize()
    assert np.abs(replay["f"].cpu().numpy() - a["f"]).max() <= 2e-6 * fscale
    assert np.abs(replay["grads"].cpu().numpy() - a["grads"]).max() <= 2e-6 * gscale


_HEAD, _TAIL = ("dense_head", "dense_wsplit"), ("dense_rows<sliced>", "dense_epilogue", "dense_param_kernel")
_F32 = ("dense_backward", "dense_rows", "dense_sample_sums", "dense_epilogue", "dense_param_kernel")
DENSE_PLAN_ROWS = [
    # (shape, environment at create, call, the launches in order): every branch of the launch plan (csrc/dense_select.h) that a small
    # shape reaches on 256 CUs; tests/c_abi/dense_select_table.cpp holds the same rows (tests/test_dense_select_cpu.py compares them)
    ((64, 32, 32, 1, 50), {}, "fvalues", _HEAD + ("dense_xfwd<0,1>", "dense_xbwd<0,2,7>") + _TAIL),                   # B_pad = 128
    ((256, 200, 32, 3, 24), {}, "fvalues", _HEAD + ("dense_xfwd<0,1>", "dense_xbwd<0,4,9>") + _TAIL),                 # B_pad = 256: nine-block tiles
    ((256, 200, 32, 3, 24), {"BSVI_XB_RB": "7"}, "fvalues", _HEAD + ("dense_xfwd<0,1>", "dense_xbwd<0,4,7>") + _TAIL),
    ((256, 200, 32, 3, 24), {}, "fvalues+noise", _HEAD + ("dense_xfwd<0,1>", "dense_xbwd<0,4,9,noise>") + _TAIL),
    ((96, 40, 784, 10, 24), {"BSVI_XF_NS": "4"}, "fvalues", _HEAD + ("dense_xfwd<0,2>", "dense_xbwd<0,2,7>") + _TAIL),   # config 4's forward kernel
    ((700, 650, 32, 1, 20), {}, "fvalues",                                                                             # B_pad = 768: x^T does not fit LDS
     _HEAD + ("xgemm_nt<logits>", "dense_ce", "xgemm_nt<grad>", "dense_xreduce", "dense_rows", "dense_epilogue", "dense_param_kernel")),
    ((64, 32, 30, 3, 20), {}, "fvalues", ("dense_prologue", "dense_gather", "dense_noise", "dense_forward<4>") + _F32),
    ((64, 32, 30, 3, 20), {}, "plain", ("dense_head", "dense_forward<4>", "dense_backward", "dense_rows", "dense_epilogue", "dense_param_kernel")),
    ((64, 32, 32, 16, 20), {"BSVI_DENSE_XGEMM": "0"}, "fvalues", ("dense_prologue", "dense_gather", "dense_noise", "dense_forward<16>") + _F32),
    ((96, 40, 784, 10, 24), {}, "plain", ("dense_head", "dense_xfwd<0,1>", "dense_xbwd<0,2,7>", "dense_rows<sliced>", "dense_param_fold_kernel")),
    ((96, 40, 784, 10, 24), {"BSVI_DENSE_FOLD": "0"}, "plain", ("dense_head", "dense_xfwd<0,1>", "dense_xbwd<0,2,7>") + _TAIL),
]
_f32_reference = {}


@pytest.mark.parametrize("row", DENSE_PLAN_ROWS, ids=lambda r: "DS%d_B%d_P%d_C%d_N%d" % r[0] + "".join("-%s=%s" % kv for kv in r[1].items()) + "-" + r[2])
def test_every_launch_plan_runs_what_it_says_and_equals_the_f32_kernels(row, monkeypatch):
    """The launches of each row are the ones the library reports (bsvi_dense_plan; the switches are read when the model is created),
    and loss, per-sample values and gradients equal those of the same model on the f32 kernels (BSVI_DENSE_XGEMM=0), within the
    tolerances of test_fused_launches_equal_the_six_launch_sequence_and_the_f32_kernels."""
    shape, env, call, names = row
    api = W.native_api()
    n, fvalues, supplied = shape[4], "fvalues" in call, "noise" in call
    for knob, value in env.items():
        monkeypatch.setenv(knob, value)
    model = engine.compile_model(build(api, shape), None, "pathwise")
    assert tuple(model.launch_plan(n, noise=supplied, want_fvalues=fvalues)) == names
    kw = {}
    if supplied:
        kw["noise"] = {"weights": np.random.RandomState(7).standard_normal((n, 1, shape[3], shape[2])).astype(np.float32)}
    if (shape, supplied) not in _f32_reference:
        monkeypatch.setenv("BSVI_DENSE_XGEMM", "0")
        plain = engine.compile_model(build(api, shape), None, "pathwise")
        assert plain.data_path() == "f32"
        _f32_reference[(shape, supplied)] = outputs(plain, n, **kw)
    ref = _f32_reference[(shape, supplied)]
    if fvalues:
        got = outputs(model, n, **kw)
    else:
        res = model.evaluate(n, seed=13, offset=2, want_indices=True, **kw)
        torch.cuda.synchronize()
        got = dict(loss=float(res["loss"].item()), grads=res["grads"].cpu().numpy().astype(np.float64), idx=res["indices"].cpu().numpy())
    assert np.array_equal(got["idx"], ref["idx"])
    fscale, gscale = np.abs(ref["f"]).max(), max(np.abs(ref["grads"]).max(), 1e-3)
    if fvalues:
        assert np.abs(got["f"] - ref["f"]).max() <= 2e-5 * fscale
    assert abs(got["loss"] - ref["loss"]) <= 2e-5 * abs(ref["loss"])
    assert np.abs(got["grads"] - ref["grads"]).max() <= 5e-5 * gscale + 1e-6


def test_fused_training_walks_the_trajectory_of_the_six_launch_sequence(monkeypatch):
    api = W.native_api()
    shape = (256, 64, 64, 10, 128)
    fused = engine.compile_model(build(api, shape), None, "pathwise")
    monkeypatch.setenv("BSVI_DENSE_FUSED", "0")
    six = engine.compile_model(build(api, shape), None, "pathwise")
    la, fa = fused.train(40, 128, "Adam", lr=5e-3, seed=3)
    lb, fb = six.train(40, 128, "Adam", lr=5e-3, seed=3)
    assert bool(fa.all()) and bool(fb.all())
    np.testing.assert_allclose(la.cpu().numpy(), lb.cpu().numpy(), rtol=2e-5)
    np.testing.assert_allclose(fused.params.cpu().numpy(), six.params.cpu().numpy(), rtol=0, atol=2e-5)


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[3]], ids=lambda s: "DS%d_B%d_P%d_C%d_N%d" % s)
def test_sample_sums_inside_the_parameter_kernel_equal_the_epilogue_launch(shape, monkeypatch):
    """dense_param_fold_kernel (every workgroup adds the value of the estimator itself) against dense_epilogue + dense_param_kernel
    (BSVI_DENSE_FOLD=0): the same gradients bit for bit — they never pass through the folded sums — and the same value up to the
    association of a 256- against a 1024-thread sum; the optimizer steps walk the same trajectory."""
    api = W.native_api()
    n = shape[4]
    folded = engine.compile_model(build(api, shape), None, "pathwise")
    monkeypatch.setenv("BSVI_DENSE_FOLD", "0")
    two = engine.compile_model(build(api, shape), None, "pathwise")
    ra, rb = folded.evaluate(n, seed=5, offset=1), two.evaluate(n, seed=5, offset=1)
    torch.cuda.synchronize()
    assert torch.equal(ra["grads"], rb["grads"])
    assert abs(float(ra["loss"]) - float(rb["loss"])) <= 1e-6 * abs(float(rb["loss"]))
    la, fa = folded.train(30, n, "Adam", lr=5e-3, seed=3)
    lb, fb = two.train(30, n, "Adam", lr=5e-3, seed=3)
    assert bool(fa.all()) and bool(fb.all())
    np.testing.assert_allclose(la.cpu().numpy(), lb.cpu().numpy(), rtol=1e-6)
    assert torch.equal(folded.params, two.params)
