"""Point-estimated tensors of the Bayesian-neural-network family on the device (bsvi_bnn_set_point_rows, bsvi_bnn_shared_first; DESIGN.md
4.7): a RootVariable of the posterior model named like a network tensor makes that tensor a point — w = the root's value for every
sample, no draw, no log q, no entropy, the prior as before; every tensor a point is `inference.MAP`.  The POINT instantiations of
bnn_draw / bnn_row_sums (any mixture of point and Normal tensors, quads that straddle the two), and — when weights1 is a point — the
shared first layer: one first product broadcast to the samples, d f / d a1 summed over the samples in a fixed order, one second product.

Every check is against `Oracle(..., dtype=float64)` on the draws and indices the kernels report, the single-precision oracle the
yardstick: conftest.yardstick_grad_check for every gradient, tests/test_gpu_bnn_priors.py's check_against for the loss and the per-sample
f.  Priors narrow and off centre (loc 0.1, scale 0.3), values half a posterior scale from zero: the prior is a visible share of every
gradient.  A point row with a Laplace prior takes the input condition of `laplace_draws_are_off_the_kink`, which for such a row (its
reported noise is 0) is |w - mu0| itself: a condition on the chosen seed, not a tolerance."""
import numpy as np
import pytest
import torch

from conftest import yardstick_grad_check
from brancher_amd import bnn, engine, inference, workloads as W
from brancher_amd.lowering import LoweringError
from oracle.svi_oracle import Oracle
from test_gpu_bnn_predict import yardstick as predict_yardstick
from test_gpu_bnn_priors import check_against, laplace_draws_are_off_the_kink
from test_gpu_bnn_sigma import SOFTMAX, weighted_pass

pytestmark = pytest.mark.gpu
TOL = 1e-5
NARROW = dict(prior_loc=0.1, prior_scale=0.3, q_loc_scale=0.5)
A = dict(dataset_size=40, batch_size=17, n_features=64, n_hidden=9, n_outputs=1, **NARROW)                               # 64-9-1, tanh, integers
B = dict(dataset_size=40, batch_size=33, n_features=36, n_hidden=5, hidden2=4, n_outputs=3, activation="relu", data="normal",
         sigma=[0.3, 0.5, 0.8], **NARROW)                                                                                # 36-5-4-3, relu
ONE_LAYER = dict(dataset_size=24, batch_size=8, n_features=32, n_hidden=0, n_outputs=2, bias=False, **NARROW)            # 32-2: Rs = 0
CLASSIFIER = dict(dataset_size=24, batch_size=8, widths=[32, 6, 3], pixels="integers", **NARROW)                         # 32-6-3, Categorical


def regression(**kw):
    return lambda: W.build_bnn_regression(W.native_api(), **kw)


def classifier(**kw):
    return lambda: W.build_bayesian_neural_network(W.native_api(), **kw)


MODELS = {
    "trunk": regression(point=("weights1", "b1"), **A),
    "head": regression(point=("weights2", "b2"), **A),
    "w1 only": regression(point=("weights1",), prior=dict(weights1="laplace", b1="cauchy"), **B),
    # weights1 Laplace and a point: whole 256-row chunks of point rows take their prior sum once on the shared path (R1 = 576)
    "trunk laplace": regression(point=("weights1", "b1"), prior=dict(weights1="laplace"), **A),
    # point rows beside a latent prior scale over the Normal tensors: the <MIXED, LATENT, POINT> instantiations
    "trunk latent": regression(point=("weights1", "b1"), scale_latent={"tau": ["weights2", "b2"]}, scale_latent_prior=(-0.5, 0.7),
                               scale_latent_q=(-0.8, 0.3), **A),
    "linear": regression(point="all", **ONE_LAYER),
    "classifier": classifier(point="all", **CLASSIFIER),
}
CASES = {
    # id: (model, N, middle kernel | None, data path | None, first layer, seed)
    "trunk": ("trunk", 70, "mid_gen", "bf16x3", "shared", 3),
    "trunk laplace": ("trunk laplace", 70, "mid_gen", "bf16x3", "shared", 3),
    "trunk latent": ("trunk latent", 70, "mid_gen", "bf16x3", "shared", 3),
    "head": ("head", 70, None, None, "per_sample", 3),
    "w1 only": ("w1 only", 130, "upper_gen", "f32", "shared", 3),
    "linear N=1": ("linear", 1, None, None, None, 3),
    "linear N=65": ("linear", 65, None, None, None, 3),
    "classifier": ("classifier", 1, None, None, None, 3),
}


def compile_bnn(model, estimator="pathwise"):
    m = MODELS[model]() if isinstance(model, str) else model()
    try:
        c = bnn.CompiledBnn(m, m.posterior_model, estimator)
    except LoweringError as err:
        pytest.fail("the bnn path refuses a posterior with point-estimated tensors: %s" % err)
    assert c.program.row_point.any()
    return c


def oracle_pair(model, n, estimator, named, mb):
    return (Oracle(MODELS[model](), dtype=torch.float64).loss_and_grads(n, estimator, named, mb),
            Oracle(MODELS[model]()).loss_and_grads(n, estimator, named, mb))


def reported_draws(c, res, n):
    noise = res["noise"].cpu().numpy()
    assert not noise[:c.program.n_rows][c.program.row_point != 0].any()   # point rows report 0 (a scale latent's draw lies behind the rows)
    return c.named_noise(noise, n), {c.program.indices_name: res["indices"].cpu().numpy().tolist()}


def evaluate_and_check(c, model, n, estimator, seed, label):
    res = c.evaluate(n, seed=seed, offset=5, want_noise=True, want_indices=True, want_fvalues=True)
    laplace_draws_are_off_the_kink(c.program, res["noise"].cpu().numpy(), label)
    named, mb = reported_draws(c, res, n)
    assert not any(t["name"] in named for t in c.program.tensors if t["point"])
    exact, ref32 = oracle_pair(model, n, estimator, named, mb)
    check_against(c, res, exact, ref32, label)
    grads = c.named_grads()
    # the same draws fed back in: the noise-in path of both kernels, and bit-equal repeat calls
    res2 = c.evaluate(n, noise=named, minibatch=mb, want_fvalues=True)
    check_against(c, res2, exact, ref32, label + " noise-in")
    g2 = c.named_grads()
    res3 = c.evaluate(n, noise=named, minibatch=mb, want_fvalues=True)
    assert torch.equal(res2["f"], res3["f"]) and all(np.array_equal(g2[k], v) for k, v in c.named_grads().items())
    return grads, exact, ref32


@pytest.mark.parametrize("estimator", ["pathwise", "blackbox"])
@pytest.mark.parametrize("case", list(CASES))
def test_each_case_matches_the_oracle_on_the_reported_draws(case, estimator, monkeypatch):
    model, n, middle, path, first, seed = CASES[case]
    c = compile_bnn(model, estimator)
    if middle:
        assert c.middle_path() == middle and c.data_path() == path, (c.middle_path(), c.data_path())
    if first:
        assert c.first_layer_path() == first
    grads, exact, ref32 = evaluate_and_check(c, model, n, estimator, seed, "%s %s" % (case, estimator))
    if first != "shared":
        return
    # the same model with both products per sample: the same bounds, and the two paths within 4 x the yardstick of each other
    monkeypatch.setenv("BSVI_BNN_SHARED1", "0")
    c0 = compile_bnn(model, estimator)
    assert c0.first_layer_path() == "per_sample" and c0.middle_path() == middle
    grads0, _, _ = evaluate_and_check(c0, model, n, estimator, seed, "%s %s per sample" % (case, estimator))
    scale = max(np.abs(v).max() for v in exact["grads"].values())
    for name, g64 in exact["grads"].items():
        yard = np.abs(ref32["grads"][name] - g64).max()
        assert np.abs(grads[name] - grads0[name]).max() <= max(4 * yard, TOL * scale), name


@pytest.mark.parametrize("model", ["trunk", "head"])
def test_the_normal_tensors_draw_what_they_drew_in_the_all_normal_model(model):
    """the Philox counters of the remaining rows do not move: row r draws from (sample, r >> 2) whatever its neighbours are"""
    n = 70
    c = compile_bnn(model)
    twin_model = regression(**A)()
    twin = bnn.CompiledBnn(twin_model, twin_model.posterior_model)
    assert not twin.program.row_point.any() and twin.first_layer_path() == "per_sample"
    a = c.evaluate(n, seed=11, offset=2, want_noise=True)["noise"].cpu().numpy()
    b = twin.evaluate(n, seed=11, offset=2, want_noise=True)["noise"].cpu().numpy()
    point = c.program.row_point != 0
    assert point.any() and not point.all() and np.array_equal(a[~point], b[~point]) and not a[point].any() and b[point].any()


def test_taylor1_on_the_head():
    n = 70
    c = compile_bnn("head", "taylor1")
    res = c.evaluate(n, seed=3, offset=5, want_noise=True, want_indices=True)
    named, mb = c.named_noise(res["noise"].cpu().numpy(), n), {c.program.indices_name: res["indices"].cpu().numpy().tolist()}
    exact, ref32 = oracle_pair("head", n, "taylor1", named, mb)
    loss = float(res["loss"].item())
    assert abs(loss - exact["loss"]) <= max(4 * abs(ref32["loss"] - exact["loss"]), TOL * abs(exact["loss"])), (loss, ref32["loss"], exact["loss"])
    yardstick_grad_check(c.named_grads(), exact["grads"], ref32["grads"])


def test_caller_weights_on_the_head():
    """`evaluate_weighted` under a softmax of f: a_n weights the point rows' prior terms through sum_n a_n alone"""
    n = 70
    c = compile_bnn("head", "blackbox")
    res = c.evaluate(n, seed=8, offset=3, want_noise=True, want_indices=True)
    named, mb = reported_draws(c, res, n)
    exact, ref32 = oracle_pair("head", n, SOFTMAX, named, mb)
    loss, grads, a = weighted_pass(c, SOFTMAX, n, named, mb)
    assert np.ptp(a) > 0.1 * np.abs(a).max()                      # the weights do differ
    assert abs(loss - exact["loss"]) <= max(4 * abs(ref32["loss"] - exact["loss"]), TOL * abs(exact["loss"])), (loss, ref32["loss"], exact["loss"])
    yardstick_grad_check(grads, exact["grads"], ref32["grads"])


def replayed_minibatches(model, iters, seed):
    """the minibatches of a training call that started at iteration 0 under `seed`: they depend on (seed, offset) alone"""
    c = compile_bnn(model)
    return [{c.program.indices_name: c.evaluate(1, seed=seed, offset=it, want_indices=True)["indices"].cpu().numpy().tolist()} for it in range(iters)]


def trajectory_check(c, got, model, iters, n, noise_seq, mb_seq, lr):
    o64, o32 = Oracle(MODELS[model](), dtype=torch.float64), Oracle(MODELS[model]())
    exact = o64.train(iters, n, "Adam", noise_seq=noise_seq, minibatch_seq=mb_seq, lr=lr).astype(np.float64)
    ref = o32.train(iters, n, "Adam", noise_seq=noise_seq, minibatch_seq=mb_seq, lr=lr).astype(np.float64)
    print("losses", got, exact, ref)
    assert np.abs(got - exact).max() <= max(4 * np.abs(ref - exact).max(), TOL * np.abs(exact).max())
    e64 = {k: t.detach().numpy() for k, t in o64.named_parameters().items()}
    e32 = {k: t.detach().numpy() for k, t in o32.named_parameters().items()}
    for pname, p in c.named_params().items():
        x = e64[pname].reshape(p.shape)
        assert np.abs(p - x).max() <= max(4 * np.abs(e32[pname].reshape(p.shape) - x).max(), 2e-5 * (1 + np.abs(x).max())), pname


def test_map_through_perform_inference_on_the_one_matrix_model_follows_the_oracle_whatever_engine_serves_it():
    """the user's call on "linear": `engine.compile_model` keeps its order, so the engine in front of this path may serve the one-matrix
    model; its loss curve and final root are held to Oracle.train all the same, on the minibatches that engine reports for (seed, offset)"""
    iters, lr = 6, 0.01
    torch.manual_seed(4321)
    seed = int(torch.initial_seed()) & 0x7FFFFFFFFFFFFFFF
    m, method = MODELS["linear"](), inference.MAP()
    inference.perform_inference(m, iters, optimizer="Adam", lr=lr, inference_method=method)
    c = method.last_compiled
    got = np.asarray(m.diagnostics["loss curve"], dtype=np.float64)
    probe = engine.compile_model(MODELS["linear"](), None, "pathwise")
    assert type(probe) is type(c)
    mb_seq = []
    for it in range(iters):
        idx = probe.evaluate(1, seed=seed, offset=it, want_indices=True)["indices"]
        idx = idx["indices"] if isinstance(idx, dict) else idx
        mb_seq.append({"indices": idx.cpu().numpy().tolist()})
    trajectory_check(c, got, "linear", iters, 1, None, mb_seq, lr)


def test_the_sharded_form_equals_the_fused_step_to_rounding_at_seventy_samples():
    """the general case beside the bit-equal one below: at N = 70 the fused launch's x / N and bsvi_finalize_step's x * (1 / N) differ in
    the last bit, the bound tests/test_gpu_bnn.py holds every model of the family to"""
    a, b = compile_bnn("trunk"), compile_bnn("trunk")
    la, _ = a.train(4, 70, "Adam", seed=2, lr=0.01)
    lb, _ = b.train(4, 70, "Adam", seed=2, lr=0.01, _force_sharded_path=True)
    assert a.first_layer_path() == "shared" and a.last_mode == "stepwise" and b.last_mode == "stepwise"
    np.testing.assert_allclose(lb.cpu().numpy(), la.cpu().numpy(), rtol=1e-6)
    np.testing.assert_allclose(b.params.cpu().numpy(), a.params.cpu().numpy(), rtol=1e-6, atol=1e-7)


def test_get_posterior_sample_hands_back_the_point_tensors_tiled():
    """the frame-level call of the reference on the trunk model: every tensor of the network is a key of the sample — the point
    estimates as the root's value for every sample (RootVariable._get_sample tiles it), the Normal tensors as drawn"""
    n = 3
    m = MODELS["trunk"]()
    c = engine.compile_model(m, None, "pathwise")
    x = next(v for v in m.flatten() if v.name == "x")
    rows = torch.from_numpy(np.random.RandomState(2).randint(-3, 4, size=(5, c.program.n_features, 1)).astype(np.float32))
    sample = m._get_posterior_sample(n, input_values={x: rows})
    by_name = {v.name: t.cpu().numpy() for v, t in sample.items()}
    params = c.named_params()
    for t in c.program.tensors:
        w = by_name[t["name"]]
        assert w.shape == (n, 1, t["rows"], t["cols"])
        if t["point"]:
            assert all(np.array_equal(w[k, 0], params[t["name"]].reshape(t["rows"], t["cols"])) for k in range(n))
        else:
            assert np.abs(w[0] - w[1]).max() > 0
    assert by_name["y"].shape == (n, 5, 1, 1)
    frame = m.get_posterior_sample(n, input_values={x: rows[:1]})      # (one row, as the reference's own prediction step hands in)
    assert frame.shape[0] == n and "weights1" in frame.columns and "b1" in frame.columns


@pytest.mark.parametrize("model", ["classifier", "linear"])
def test_six_adam_steps_of_map_through_perform_inference_follow_the_oracle(model):
    """the user's call: `inference.MAP()` on a network whose tensors are all points — one sample, no entropy, the loss -log p(theta, minibatch).
    (`engine.compile_model` keeps its order: the one-matrix model without a posterior draw is lowered by the scalar engine in front of this
    path, so for "linear" the call `MAP.run` makes — train on one sample — is made on the bnn engine directly.)"""
    iters, lr = 6, 0.01
    torch.manual_seed(4321)
    seed = int(torch.initial_seed()) & 0x7FFFFFFFFFFFFFFF
    m, method = MODELS[model](), inference.MAP()
    before = {v.name: np.array(v.parameter.numpy(), copy=True) for v in m.posterior_model.flatten()}
    if model == "linear":
        c = bnn.CompiledBnn(m, m.posterior_model, "pathwise")
        losses, finite = c.train(iters, 1, "Adam", seed=seed, lr=lr)
        assert finite.cpu().numpy().all()
        got = losses.cpu().numpy().astype(np.float64)
    else:
        inference.perform_inference(m, iters, optimizer="Adam", lr=lr, inference_method=method)
        c = method.last_compiled
        got = np.asarray(m.diagnostics["loss curve"], dtype=np.float64)
    assert type(c).__name__ == "CompiledBnn" and c.last_mode == "stepwise" and c.program.entropy_weight == 0.0 and c.program.row_point.all()
    assert len(got) == iters and all(np.abs(c.named_params()[k].reshape(-1) - v.reshape(-1)).max() > 0 for k, v in before.items())
    trajectory_check(c, got, model, iters, 1, None, replayed_minibatches(model, iters, seed), lr)


def test_four_adam_steps_on_the_trunk_follow_the_oracle_and_the_sharded_form_is_bit_equal():
    """ReverseKL on the trunk, fixed noise and minibatches, against Oracle.train; then the sequence a rank of the sharded path runs
    (bsvi_bnn_fwd_bwd + bsvi_finalize_step) against the fused step, bit for bit.  N = 128 — two segments of the sum over the samples —
    is a power of two on purpose: the fused launch divides the sums by N where bsvi_finalize_step multiplies by 1 / N (both older than
    this path, tests/test_gpu_bnn.py: "equal to rounding"), and the two are the same operation exactly when 1 / N is a binary number.
    Everything in front of that division is the same launches in both forms."""
    iters, n, lr = 4, 128, 0.01
    probe = compile_bnn("trunk")
    noise_seq, mb_seq = [], []
    for it in range(iters):
        res = probe.evaluate(n, seed=9, offset=it, want_noise=True, want_indices=True)
        named, mb = reported_draws(probe, res, n)
        noise_seq.append(named)
        mb_seq.append(mb)
    c = compile_bnn("trunk")
    assert c.first_layer_path() == "shared"
    losses, finite = c.train(iters, n, "Adam", noise_seq=noise_seq, minibatch_seq=mb_seq, lr=lr)
    assert c.last_mode == "stepwise" and finite.cpu().numpy().all()
    trajectory_check(c, losses.cpu().numpy().astype(np.float64), "trunk", iters, n, noise_seq, mb_seq, lr)
    c2 = compile_bnn("trunk")
    losses2, _ = c2.train(iters, n, "Adam", noise_seq=noise_seq, minibatch_seq=mb_seq, lr=lr, _force_sharded_path=True)
    assert torch.equal(losses, losses2) and all(np.array_equal(v, c2.named_params()[k]) for k, v in c.named_params().items())


@pytest.mark.parametrize("model", ["trunk", "classifier"])
@pytest.mark.parametrize("rows", [5, 40])
def test_predict_uses_the_value_for_the_point_tensors(model, rows):
    """against the chain in double precision on the reported noise (tests/test_gpu_bnn_predict.py's yardstick, whose weights are
    loc + scale eps with the scale of a point row 0); an all-point network gives N equal outputs, and the regression var is
    Var_n(loc) + sigma^2: the likelihood's own part alone where nothing is random"""
    n = 3
    c = compile_bnn(model)
    x = np.random.RandomState(rows).randint(-3, 4, size=(rows, c.program.n_features)).astype(np.float32)
    res = c.predict(x, n, seed=5, offset=9, want_outputs=True, want_noise=True)
    assert not res["noise"].cpu().numpy()[c.program.row_point != 0].any()
    predict_yardstick(c, res, x, "%s M=%d" % (model, rows))
    if model == "classifier":
        out = res["outputs"]
        assert torch.equal(out[0], out[1]) and torch.equal(out[0], out[2]) and torch.equal(res["probs"][0], res["probs"][2])


def test_an_all_point_regression_has_the_likelihoods_variance_alone():
    c = compile_bnn("linear")
    x = np.random.RandomState(1).randint(-3, 4, size=(5, c.program.n_features)).astype(np.float32)
    res = c.predict(x, 3, seed=5, offset=9, want_outputs=True)
    assert torch.equal(res["outputs"][0], res["outputs"][1]) and torch.equal(res["outputs"][0], res["outputs"][2])
    var = res["var"].cpu().numpy().astype(np.float64)
    assert np.abs(var / 0.5 ** 2 - 1.0).max() <= 1e-6                # (sigma = 0.5, the builder's default)


def test_the_setter_checks_its_arguments_and_its_moment():
    import ctypes as C
    m = regression(**A)()
    c = bnn.CompiledBnn(m, m.posterior_model)
    R, lib, INVALID = c.program.n_rows, c.lib, -1
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    none = np.zeros(R, dtype=np.uint8)
    assert lib.bsvi_bnn_set_point_rows(c.handle, ptr(none), R - 1) == INVALID and b"n_rows" in lib.bsvi_last_error()
    assert lib.bsvi_bnn_set_point_rows(c.handle, None, R) == INVALID
    bad = none.copy()
    bad[R // 2] = 2
    assert lib.bsvi_bnn_set_point_rows(c.handle, ptr(bad), R) == INVALID and b"0 (a random row) or 1" in lib.bsvi_last_error()
    bad[R // 2] = 1                                                  # (the q scale of that row is a learnable entry)
    assert lib.bsvi_bnn_set_point_rows(c.handle, ptr(bad), R) == INVALID and b"constant" in lib.bsvi_last_error()
    assert lib.bsvi_bnn_set_point_rows(c.handle, ptr(none), R) == 0 and c.first_layer_path() == "per_sample"
    # nothing stuck: the model is its all-Normal self
    first = c.evaluate(70, seed=3, offset=5)["loss"].clone()
    m2 = regression(**A)()
    assert torch.equal(first, bnn.CompiledBnn(m2, m2.posterior_model).evaluate(70, seed=3, offset=5)["loss"])
    assert lib.bsvi_bnn_set_point_rows(c.handle, ptr(none), R) == INVALID and b"launch" in lib.bsvi_last_error()


def test_the_public_route_serves_the_models():
    """`engine.compile_model` on a deterministic trunk under a Bayesian last layer and on the all-point classifier: before this feature
    the lowering refused both ("every latent of the network needs a Normal posterior", "the posterior must be mean-field Normal")"""
    for model, points in (("trunk", ["weights1", "b1"]), ("classifier", ["weights1", "b1", "weights2", "b2"])):
        try:
            c = engine.compile_model(MODELS[model](), None, "pathwise")
        except LoweringError as err:
            pytest.fail("the public route refuses point-estimated tensors: %s" % err)
        assert type(c).__name__ == "CompiledBnn" and c.program.summary()["point"] == points and c.first_layer_path() == "shared"
