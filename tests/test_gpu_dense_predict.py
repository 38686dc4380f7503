"""The posterior predictive of the dense-link path (csrc/dense_predict.inc): `CompiledDense.predict` (weight sets sampled
from the posterior), `predict_particles` (a table of particles read in place), `SteinVariationalGradientDescent.predict` and the
reference's own call `model._get_posterior_sample(N, input_values={x: rows})`, against plain torch in float64: W = mu + s noise | theta,
logits = W x, softmax | sigmoid, the mean over the sets.  The bound is the one of tests/test_gpu_svgd_dense_batched.py:
min(max(4 |ref32 - ref64|, 1e-5 scale), 1e-4 scale), ref32 the same code in float32; scale is the largest logit for the logits and 1 for
probabilities.  Every test fails on the commit before: CompiledDense had no predict, the two `_get_posterior_sample` calls raised
LoweringError."""
import numpy as np
import pytest
import torch

from brancher_amd import dense, engine, inference, workloads as W
from brancher_amd.variables import ProbabilisticModel, RootVariable

pytestmark = pytest.mark.gpu


def within(got, ref32, ref64, what, scale=None):
    got, ref32, ref64 = (np.asarray(torch.as_tensor(a).cpu(), dtype=np.float64) for a in (got, ref32, ref64))
    scale = np.abs(ref64).max() if scale is None else scale
    allowed = np.minimum(np.maximum(4 * np.abs(ref32 - ref64), 1e-5 * scale), 1e-4 * scale)
    excess = np.abs(got - ref64) - allowed
    print("%s: largest error %.3g, allowed there %.3g" % (what, np.abs(got - ref64).reshape(-1)[excess.argmax()], allowed.reshape(-1)[excess.argmax()]))
    assert got.shape == ref64.shape and np.isfinite(got).all() and excess.max() <= 0, what


def regression(c, p, point):
    """a model of the existing builders on c classes and p features; point: its posterior is a point estimate (what a particle is)"""
    api = W.native_api()
    if c == 1:
        model = W.build_binary_logistic_regression(api, dataset_size=8, batch_size=4, n_features=p)
        if point:
            model.set_posterior_model(api.ProbabilisticModel([api.RootVariable(0.5 * np.ones((1, p)), name="weights", learnable=True)]))
    elif point:
        model = W.build_map_logistic_regression(api, dataset_size=8, n_features=p, n_classes=c)
    else:
        model = W.build_logistic_regression(api, dataset_size=8, batch_size=4, n_features=p, n_classes=c)
    return model


def engine_of(c, p, point):
    model = regression(c, p, point)
    return dense.CompiledDense(model, model.posterior_model, particles=point)


def rows_of(m, p, seed=0):
    return torch.randn(m, p, generator=torch.Generator().manual_seed(seed + 31 * m + p)) * (2.0 / p ** 0.5)


def forward(weights, x, dtype):      # weights [N][C P] -> logits, probs [N][M][C], mean [M][C]
    c = weights.shape[1] // x.shape[1]
    logits = torch.einsum("ncp,mp->nmc", weights.to(dtype).reshape(weights.shape[0], c, -1), x.to(dtype))
    probs = torch.sigmoid(logits) if c == 1 else torch.softmax(logits, -1)
    return logits, probs, probs.mean(0)


def sampled_weights(compiled, noise, dtype):      # W = mu + s noise, noise [R][N]
    loc, scale = dense.row_parameters(compiled.program, compiled.params.cpu().numpy()[:compiled.program.n_params])
    return (torch.as_tensor(loc).to(dtype)[:, None] + torch.as_tensor(scale).to(dtype)[:, None] * noise.cpu().to(dtype)).T


def check(res, weights, x):
    (l64, p64, m64), (l32, p32, m32) = (forward(weights(dtype), x, dtype) for dtype in (torch.float64, torch.float32))
    within(res["outputs"], l32, l64, "logits")
    within(res["probs"], p32, p64, "probabilities", 1.0)
    within(res["mean"], m32, m64, "mean", 1.0)


def run(mode, n, c, p, m, ld_extra=0, sets_per_split=None, seed=3, **want):
    """one call of the path under test; returns (result, weights(dtype) -> [N][C P], rows)"""
    torch.manual_seed(n + c * p)
    x = rows_of(m, p)
    if mode == "table":
        compiled = engine_of(c, p, True)
        theta = 0.3 * torch.randn(n, c * p)
        table = torch.full((n, (c * p + 3) // 4 * 4 + ld_extra), float("nan"))      # (the pad columns are never read as weights)
        table[:, :c * p] = theta
        return compiled.predict_particles(table.cuda(), x, seed=seed, offset=5, sets_per_split=sets_per_split, **want), lambda dtype: theta, x
    compiled = engine_of(c, p, False)
    compiled.params.copy_(0.3 * torch.randn(compiled.params.numel()))
    noise = torch.randn(c * p, n) if mode == "noise" else None
    res = compiled.predict(x, n, seed=seed, offset=5, noise=None if noise is None else noise.cuda(), sets_per_split=sets_per_split,
                           want_noise=True, **want)
    return res, lambda dtype: sampled_weights(compiled, res["noise"], dtype), x


# (N, C, P, M): the scripts' one-row, one-set call; one block exactly with an odd P through the pad and a masked row tile; dead sets in the
# second block, two k chunks and a partial one, a second row tile that is partial; Bernoulli, 32 sets a block and one more; dead rows in the
# block and a single k step; no dead rows (32 classes: a table only); the long k loop; the join (13 blocks of 10 sets, 4 a split).
SHAPES = [(1, 3, 4, 1), (3, 10, 5, 16), (4, 10, 68, 130), (33, 1, 3, 130), (5, 7, 2, 5), (2, 32, 4, 129), (65, 16, 784, 40), (130, 3, 4, 300)]
CASES = [(mode,) + shape + (0, 40 if shape[0] == 130 else None) for mode in ("noise", "table") for shape in SHAPES
         if not (mode == "table" and shape[0] == 1) and not (mode == "noise" and shape[1] == 32)]
CASES.append(("table", 3, 10, 5, 16, 3, None))      # rows of the table that are not 16-byte aligned


@pytest.mark.parametrize("mode,n,c,p,m,ld_extra,sets_per_split", CASES)
def test_probabilities_logits_and_mean_against_torch_in_double(mode, n, c, p, m, ld_extra, sets_per_split):
    res, weights, x = run(mode, n, c, p, m, ld_extra, sets_per_split, want_outputs=True)
    check(res, weights, x)


@pytest.mark.parametrize("c,p", [(3, 5), (10, 68)])      # rows r = c P + p whose quads straddle the staging's four features, and aligned ones
def test_a_prediction_draws_the_noise_of_a_training_launch(c, p):
    res, weights, x = run("philox", 5, c, p, 16, seed=11, want_outputs=True)
    compiled = engine_of(c, p, False)
    trained = compiled.evaluate(5, seed=11, offset=5, want_noise=True)["noise"]
    assert torch.equal(res["noise"], trained) and float(trained.abs().max()) > 0
    check(res, weights, x)


@pytest.mark.parametrize("n,c,p,m,sets_per_split", [(4, 10, 68, 130, None), (130, 3, 4, 300, 40)])
def test_the_same_call_twice_gives_the_same_bits(n, c, p, m, sets_per_split):
    first, again = (run("philox", n, c, p, m, sets_per_split=sets_per_split, want_draws=True)[0] for _ in range(2))
    assert all(torch.equal(first[k], again[k]) for k in ("probs", "mean", "draws")) and float(first["draws"].sum()) == n * m


@pytest.mark.parametrize("c", [3, 1])
def test_draws_are_one_hot_and_follow_the_probabilities(c):
    """4000 sets of a point estimate share one probability vector a row; the rows keep every p inside [0.02, 0.98] (asserted on the
    float64 reference), so that five standard deviations of a frequency are a meaningful bound"""
    n, p, m = 4000, 4, 5
    compiled = engine_of(c, p, True)
    x = 0.25 * rows_of(m, p, seed=1)
    res = compiled.predict(x, n, seed=7, offset=2, want_draws=True)
    p64 = forward(sampled_weights(compiled, torch.zeros(c * p, 1), torch.float64), x, torch.float64)[1][0].numpy()
    cells = np.concatenate([p64, 1 - p64], 1) if c == 1 else p64
    assert cells.min() >= 0.02 and cells.max() <= 0.98
    draws = res["draws"].cpu().numpy().astype(np.float64)
    assert np.isin(draws, (0.0, 1.0)).all() and (c == 1 or (draws.sum(-1) == 1).all())
    assert (np.abs(draws.mean(0) - p64) <= 5 * np.sqrt(p64 * (1 - p64) / n)).all()


def rule_draw(probs, u):
    """the documented rule of the draw (include/bsvi.h, bsvi_dense_predict) on the float32 probabilities the call stored and the uniform
    of the stream's contract -> [N, M, C] one-hot | 0 / 1.  Categorical: the first class whose float32 partial sum, in class order, is
    >= u, the last class if none is; Bernoulli: u < p."""
    probs = np.asarray(probs, dtype=np.float32)
    if probs.shape[-1] == 1:
        return (u < probs[..., 0]).astype(np.float32)[..., None]
    cum = np.zeros(probs.shape[:-1], dtype=np.float32)
    pick = np.full(probs.shape[:-1], probs.shape[-1] - 1)
    found = np.zeros(probs.shape[:-1], dtype=bool)
    for c in range(probs.shape[-1]):
        cum = (cum + probs[..., c]).astype(np.float32)
        hit = (cum >= u) & ~found
        pick[hit] = c
        found |= hit
    return (pick[..., None] == np.arange(probs.shape[-1])).astype(np.float32)


@pytest.mark.parametrize("n,c,p,m", [(4, 10, 68, 130), (33, 1, 3, 130)])
@pytest.mark.parametrize("sample_base", [0, 5])
def test_the_draw_is_its_documented_rule_on_the_streams_uniform(n, c, p, m, sample_base):
    """u = u01(word m & 3) of Philox counter (sample_base + n, (m >> 2) | 0x20000000, offset) under the seed as it is (philox.h): rows
    m = 0 .. 129 read all four words of 33 counters.  The draw is the rule on the probabilities the same call returned, exactly."""
    from oracle import philox_ref as R
    torch.manual_seed(n + c * p)
    compiled = engine_of(c, p, False)
    compiled.params.copy_(0.3 * torch.randn(compiled.params.numel()))
    seed, offset = 0x1234567890ABC, (1 << 32) - 1
    res = compiled.predict(rows_of(m, p), n, seed=seed, offset=offset, sample_base=sample_base, want_draws=True)
    probs, draws = res["probs"].cpu().numpy(), res["draws"].cpu().numpy()
    u = R.dense_predict_uniform(seed, offset, sample_base, n, m)
    want = rule_draw(probs, u)
    assert draws.shape == want.shape == (n, m, c) and np.array_equal(draws, want), np.argwhere(draws != want)[:8]
    # the rule bites: another offset's uniforms, or the rows' words shifted by one, give other draws
    assert not np.array_equal(rule_draw(probs, R.dense_predict_uniform(seed, offset + 1, sample_base, n, m)), draws)
    assert not np.array_equal(rule_draw(probs, np.roll(u, 1, axis=1)), draws)


def test_the_ensemble_of_a_batched_svgd_run_is_predicted_from_its_table_in_place():
    model = regression(3, 4, True)
    start = 0.05 * np.random.RandomState(5).normal(size=(3, 12))
    parts = [ProbabilisticModel([RootVariable(row.reshape(3, 4), "weights", learnable=True)]) for row in start]
    method = inference.SteinVariationalGradientDescent(batched=True)
    inference.perform_inference(model, number_iterations=2, optimizer="SGD", lr=0.002, inference_method=method, posterior_model=parts)
    x = rows_of(16, 4)
    res = method.predict(model, parts, x, want_outputs=True)
    theta = torch.as_tensor(np.stack([next(iter(part.flatten())).parameter.numpy().reshape(-1) for part in parts]), dtype=torch.float32)
    assert np.abs(theta.numpy() - start).max() > 0
    direct = method.last_compiled.predict_particles(theta.cuda(), x, want_outputs=True)
    assert all(torch.equal(res[k], direct[k]) for k in ("probs", "mean", "outputs"))
    check(res, lambda dtype: theta, x)


@pytest.mark.parametrize("c,p", [(3, 5), (1, 2)])
def test_get_posterior_sample_answers_for_feature_counts_the_detour_refuses(c, p):
    model = regression(c, p, False)
    x = next(v for v in model.flatten() if v.name == "x")
    rows = rows_of(7, p).reshape(7, p, 1)
    sample = model._get_posterior_sample(6, input_values={x: rows})
    by_name = {v.name: t for v, t in sample.items()}
    assert all(v in set(model.flatten()) for v in sample)                      # keyed by the JOINT model's variables
    assert tuple(by_name["weights"].shape) == (6, 1, c, p) and tuple(by_name["k"].shape) == (6, 7, c, 1) and torch.equal(by_name["x"].cpu(), rows)
    # the call again: the same seed and the offset it took
    compiled = engine._dense_predictor(model, engine.compile_model(model, model.posterior_model, None))      # (two features train on the scalar engine)
    again = compiled.predict(rows, 6, seed=None, offset=(1 << 62) + engine._sample_tick[0], want_noise=True, want_draws=True)
    np.testing.assert_allclose(by_name["weights"].cpu().numpy().reshape(6, -1), sampled_weights(compiled, again["noise"], torch.float64).numpy(),
                               rtol=1e-6, atol=1e-7)
    assert torch.equal(by_name["k"].reshape(6, 7, c), again["draws"]) and float(again["noise"].std()) > 0.5
