"""The local reparameterisation estimator of the dense-link path (csrc/dense_local.inc) against its formulas in plain
torch double with autograd:  m = X mu^T, v = X^2 (s^2)^T, z_n = m + sqrt(v) zeta_n,
loss = -( (1 / N) sum_n sum_b log p(y_b | z_n[b]) + sum_r [-log s0 - log sqrt(2 pi) - ((mu - mu0)^2 + s^2) / (2 s0^2) + log sqrt(2 pi e) + log s] ).
The bound is the project's yardstick, max(4 |ref32 - ref64|, 1e-5 scale), ref32 the same code in float32.  Every test fails on the commit
before: lower_dense refused the estimator."""
import math

import numpy as np
import pytest
import torch

from conftest import yardstick_grad_check, yardstick_loss_check
from brancher_amd import dense, engine, inference, lowering, native, workloads as W
from brancher_amd.gradient_estimators import LocalReparameterizationEstimator, PathwiseDerivativeEstimator

pytestmark = pytest.mark.gpu


def build(c, p, b, learn_prior=False, zero_row=False, collide=False, spread=1.0):
    """a logistic regression on b + 3 rows.  The posterior's loc and log-scale are roots of their own names, so the prior (loc 0, scale 0.7
    or exp of a learnable scalar root) is not the posterior's; collide: the reference's own form, whose prior roots ARE the posterior's"""
    api, rng = W.native_api(), np.random.RandomState(7 * c + p)
    BF, ds = api.BF, b + 3
    X = (rng.standard_normal((ds, p, 1)) * spread / math.sqrt(p)).astype(np.float32)
    if zero_row:
        X[1] = 0.0
    labels = rng.randint(0, max(c, 2), (ds, 1)).astype(np.float32 if c == 1 else np.int32)
    indices = api.RandomIndices(dataset_size=ds, batch_size=b, name="indices", is_observed=True)
    x = api.EmpiricalVariable(X, indices=indices, name="x", is_observed=True)
    y = api.EmpiricalVariable(labels, indices=indices, name="labels", is_observed=True)
    prior_scale = BF.exp(api.RootVariable(math.log(0.7), "log_prior_scale", learnable=True)) if learn_prior else 0.7 * np.ones((c, p))
    weights = api.NormalVariable(np.zeros((c, p)), prior_scale, "weights")
    k = api.BinomialVariable(1, logits=BF.matmul(weights, x), name="k") if c == 1 else api.CategoricalVariable(logits=BF.matmul(weights, x), name="k")
    model = api.ProbabilisticModel([k])
    k.observe(y)
    loc, scale = 0.5 * rng.standard_normal((c, p)), 0.2 + 0.3 * rng.random_sample((c, p))
    if collide:
        q = api.NormalVariable(loc, scale, "weights", learnable=True)
    else:
        q = api.NormalVariable(api.RootVariable(loc, "q_loc", learnable=True), BF.exp(api.RootVariable(np.log(scale), "q_log_s", learnable=True)), "weights")
    model.set_posterior_model(api.ProbabilisticModel([q]))
    return model, X.reshape(ds, p), labels.reshape(ds)


def reference(p, theta, X, labels, idx, zeta, dtype):
    """the formulas of the module's docstring on the program's own uniform table -> (loss, {parameter name: gradient})"""
    th = torch.tensor(theta, dtype=dtype, requires_grad=True)
    uni, UT = p.uniform, lowering.UT
    src = torch.as_tensor(uni["src"].astype(np.int64))
    raw = torch.where(torch.as_tensor(uni["is_param"] != 0), th[src.clamp(max=len(theta) - 1)],
                      torch.as_tensor(np.append(p.consts, 0.0), dtype=dtype)[src.clamp(max=len(p.consts))])
    t = torch.as_tensor(uni["transform"].astype(np.int64))
    assert set(t.tolist()) <= {UT["identity"], UT["softplus"], UT["exp"]}
    val = torch.where(t == UT["exp"], raw.exp(), torch.where(t == UT["softplus"], torch.nn.functional.softplus(raw), raw))
    val = torch.as_tensor(uni["a"].copy(), dtype=dtype) + torch.as_tensor(uni["b"].copy(), dtype=dtype) * val
    C, P = p.n_classes, p.n_features
    mu, s, mu0, s0 = (val[base + stride * torch.arange(C * P)].reshape(C, P) for base, stride in (p.q_loc, p.q_scale, p.prior_loc, p.prior_scale))
    x, y, z0 = torch.as_tensor(X[idx], dtype=dtype), torch.as_tensor(labels[idx]), torch.as_tensor(zeta, dtype=dtype)
    m, v = x @ mu.T, (x * x) @ (s * s).T
    z = m + torch.sqrt(torch.where(v > 0, v, torch.ones_like(v))) * (v > 0) * z0            # [N, B, C]; v = 0: z = m
    if C == 1:
        lik = (y.to(dtype) * z[..., 0] - torch.nn.functional.softplus(z[..., 0])).sum()
    else:
        lik = torch.log_softmax(z, -1).gather(2, y.long().expand(z.shape[0], -1)[..., None]).sum()
    half_log_2pi = 0.5 * math.log(2 * math.pi)
    const = (-torch.log(s0) - half_log_2pi - ((mu - mu0) ** 2 + s * s) / (2 * s0 * s0) + (half_log_2pi + 0.5) + torch.log(s)).sum()
    loss = -(lik / z.shape[0] + const)
    loss.backward()
    g = th.grad.numpy().astype(np.float64)
    return float(loss.detach()), {par.name: g[off:off + size].reshape(par.shape) for par, off, size, _ in p.parameters}


CASES = {  # C, P, B, N, model form
    "bernoulli_ragged": (1, 3, 5, 3, dict(collide=True)),                 # one ragged tile of everything; the reference's own model form
    "two_row_tiles": (3, 5, 33, 9, dict(learn_prior=True)),               # a second tile of one row, ragged sample lanes, a shared entry
    "k_chunks_and_splits": (10, 70, 64, 40, dict()),                      # three K chunks, the last ragged; five sample splits
    "class_limit": (16, 130, 40, 17, dict()),                             # 16 classes; five column tiles, the last ragged
    "zero_row": (3, 5, 33, 9, dict(zero_row=True)),                       # v = 0 in one row
}


@pytest.fixture(scope="module", params=list(CASES))
def case(request):
    c, p_, b, n, form = CASES[request.param]
    model, X, labels = build(c, p_, b, **form)
    compiled = dense.CompiledDense(model, model.posterior_model, "local")
    rng = np.random.RandomState(3)
    idx = rng.permutation(b + 3)[:b].astype(np.int32)
    idx[4] = 1 if form.get("zero_row") and 1 not in idx else idx[4]
    return compiled, X, labels, idx, rng.standard_normal((n, b, c)).astype(np.float32)


def test_evaluate_matches_the_formulas(case):
    compiled, X, labels, idx, zeta = case
    p = compiled.program
    res = compiled.evaluate(zeta.shape[0], noise={p.likelihood_name: zeta}, minibatch=idx, seed=1, offset=0, want_indices=True)
    assert np.array_equal(res["indices"].cpu().numpy(), idx) and float(res["finite"]) == 1.0
    theta = compiled.params.cpu().numpy()[:p.n_params]
    loss64, g64 = reference(p, theta, X, labels, idx, zeta, torch.float64)
    loss32, g32 = reference(p, theta, X, labels, idx, zeta, torch.float32)
    named = compiled.named_grads()
    print("loss", float(res["loss"]), loss64, loss32, {k: (np.abs(named[k] - g64[k]).max(), np.abs(g32[k] - g64[k]).max()) for k in g64})
    yardstick_loss_check(float(res["loss"]), loss64, loss32)
    yardstick_grad_check(named, g64, g32)


def test_the_drawn_path_is_the_supplied_path():
    c, p_, b, n, form = CASES["k_chunks_and_splits"]
    model, _, _ = build(c, p_, b, **form)
    compiled = dense.CompiledDense(model, model.posterior_model, "local")
    drawn = compiled.evaluate(n, seed=11, offset=5, want_noise=True, want_indices=True)
    loss, grads, noise = drawn["loss"].clone(), drawn["grads"].clone(), drawn["noise"].clone()
    again = compiled.evaluate(n, seed=11, offset=5, want_noise=True)
    assert torch.equal(again["noise"], noise) and torch.equal(again["loss"], loss) and torch.equal(again["grads"], grads)
    supplied = compiled.evaluate(n, noise=noise, minibatch=drawn["indices"].cpu().numpy(), seed=11, offset=5)
    assert torch.equal(supplied["loss"], loss) and torch.equal(supplied["grads"], grads)
    other = compiled.evaluate(n, seed=11, offset=6, want_noise=True)
    assert not torch.equal(other["noise"], noise) and float((other["noise"] == noise).float().mean()) < 0.01
    z, n_values = noise.double().cpu(), noise.numel()      # standard normals: mean and variance within six of their standard errors
    assert tuple(noise.shape) == (n, b, c) and abs(float(z.mean())) < 6 / math.sqrt(n_values) and abs(float(z.var()) - 1) < 6 * math.sqrt(2 / n_values)
    # the minibatch of (seed, offset) is the one Pathwise gathers
    pathwise = dense.CompiledDense(*(lambda m: (m, m.posterior_model))(build(c, p_, b, **form)[0]), "pathwise")
    assert torch.equal(pathwise.evaluate(8, seed=11, offset=5, want_indices=True)["indices"], drawn["indices"])


def test_refusals_by_name():
    model, _, _ = build(3, 5, 33)
    compiled = dense.CompiledDense(model, model.posterior_model, "local")
    for call, words in ((lambda: compiled.evaluate(8, want_fvalues=True), "want_fvalues"),
                        (lambda: compiled.evaluate_weighted(8, None, None, 0, 0), "evaluate_weighted"),
                        (lambda: compiled.launch_plan(8), "sequence of its own"),
                        (lambda: compiled.evaluate(8, noise=np.zeros((8, 33, 2), np.float32)), r"noise must be \[8, 33, 3\]")):
        with pytest.raises(ValueError, match=words):
            call()
    lib = compiled.lib
    assert lib.bsvi_dense_local_workspace_bytes(compiled.handle, 0) == 0 and b"n_samples is 0" in lib.bsvi_last_error()
    args = native.DenseLocalArgs(n_samples=8, params_dev=compiled.params.data_ptr(), out_dev=compiled.out.data_ptr(), workspace_dev=compiled.out.data_ptr() + 4)
    assert lib.bsvi_dense_local_fwd_bwd(compiled.handle, args) == -1 and b"not 256-byte aligned" in lib.bsvi_last_error()
    point = W.build_map_logistic_regression(W.native_api())
    handle = dense.CompiledDense(point, point.posterior_model).handle
    assert lib.bsvi_dense_local_workspace_bytes(handle, 8) == 0 and b"point estimate" in lib.bsvi_last_error()
    wide = build(17, 5, 33)[0]
    handle = dense.CompiledDense(wide, wide.posterior_model, particles=True).handle      # (a handle of 17 classes exists for the particles)
    assert lib.bsvi_dense_local_workspace_bytes(handle, 8) == 0 and b"17 classes" in lib.bsvi_last_error()


def test_the_estimator_targets_the_elbo_of_pathwise():
    """Both estimators are unbiased for the same loss and the same gradient.  With N = 4096 drawn samples on one minibatch:
    loss — Pathwise reports its per-sample values f_n (want_fvalues), so its loss has the standard error se = std(f) / sqrt(N); the local
    estimator's value has no larger variance (its closed-form KL has none, its likelihood terms have Pathwise's marginals but are
    independent over the rows), so the difference of the two has at most sqrt(2) se: the bound is six of those.
    gradient — Pathwise reports no per-sample gradients, so its N samples are taken as 16 evaluations of 256 at offsets of their own: their
    mean is the N-sample gradient, and the spread of the 16 gives the standard error of that mean per component, std / sqrt(16); the
    local gradient's variance is no larger (Kingma et al. 2015, section 2.2), so again six times sqrt(2) se, per component."""
    c, p_, b = 3, 5, 33
    idx = np.random.RandomState(3).permutation(b + 3)[:b].astype(np.int32)
    models = {est: build(c, p_, b, spread=3.0)[0] for est in ("local", "pathwise")}
    engines = {est: dense.CompiledDense(m, m.posterior_model, est) for est, m in models.items()}
    local = engines["local"].evaluate(4096, minibatch=idx, seed=5, offset=0)
    loss_l, grad_l, losses, grads, fs = float(local["loss"]), local["grads"].double().cpu().numpy(), [], [], []
    for k in range(16):
        res = engines["pathwise"].evaluate(256, minibatch=idx, seed=5, offset=100 + k, want_fvalues=True)
        losses.append(float(res["loss"])); grads.append(res["grads"].double().cpu().numpy()); fs.append(res["f"].double().cpu().numpy())
    se_loss, grads = np.concatenate(fs).std(ddof=1) / math.sqrt(4096), np.stack(grads)
    se_grad = grads.std(0, ddof=1) / 4.0
    print("loss", loss_l, np.mean(losses), "se", se_loss, "worst gradient deviation in se", (np.abs(grad_l - grads.mean(0)) / se_grad).max())
    assert abs(loss_l - np.mean(losses)) <= 6 * math.sqrt(2) * se_loss
    assert (np.abs(grad_l - grads.mean(0)) <= 6 * math.sqrt(2) * se_grad).all()


def test_training_through_perform_inference():
    """200 Adam iterations (16 samples, lr 0.05) on two separable clouds: the loss falls, and the training accuracy of the posterior
    mean is at least Pathwise's of the same run minus the spread of Pathwise's accuracy over three seeds.
    Recorded on an MI355X: local 0.983; Pathwise 0.983, 0.983, 0.983 (spread 0)."""
    def run(estimator, seed):
        torch.manual_seed(seed)
        model = W.build_binary_logistic_regression(W.native_api(), dataset_size=60, batch_size=30, n_features=4)
        inference.perform_inference(model, 200, number_samples=16, optimizer="Adam", lr=0.05,
                                    inference_method=inference.ReverseKL(gradient_estimator=estimator))
        compiled = engine.compile_model(model, None, estimator)
        p, w = dense.lower_dense(model, model.posterior_model), compiled.named_params()["weights_loc"].reshape(-1)      # (p: the data)
        accuracy = float((((p.dataset @ w) > 0) == (p.labels > 0.5)).mean())
        return model.diagnostics["loss curve"], accuracy, compiled
    curve, acc_local, compiled = run(LocalReparameterizationEstimator, 0)
    assert compiled.last_mode == "local" and np.isfinite(curve).all() and curve[-20:].mean() < curve[:20].mean()
    acc_path = [run(PathwiseDerivativeEstimator, seed)[1] for seed in (0, 1, 2)]
    assert acc_local >= acc_path[0] - (max(acc_path) - min(acc_path))
