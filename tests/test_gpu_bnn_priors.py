"""Laplace and Cauchy priors of the Bayesian-neural-network family on the device (bsvi_bnn_set_row_priors): the
per-sample prior value of bnn_draw<true>, the per-sample sums T0 / T1 of bnn_row_sums<true> (T2 follows from the two) and the gradients
built from them, the constants in double precision, for every row kind and their mixtures — weights1 (uniform quads), the small tensors (quads
that straddle two tensors, a last quad of three rows), no small tensors at all.  Every check is against `Oracle(..., dtype=float64)` on
the draws and indices the kernels report, the single-precision oracle (or a fixture of the real reference) the yardstick:
conftest.yardstick_grad_check for every gradient, the bounds of tests/test_gpu_bnn_sigma.py's check_against for the loss and the
per-sample f.  The priors are narrow and off centre (scale 0.3, loc 0.1) and the posterior means lie half a posterior scale from zero:
the prior's gradient is a visible share of every gradient and sign(u) differs between the samples of a row.

sign(u) is discontinuous: a draw whose w - mu0 is within rounding of zero can have opposite signs in single and double precision, so
every Laplace test first asserts, from the reported noise and the row parameters in double precision, that no draw of a Laplace row
is that close (`laplace_draws_are_off_the_kink`) — a condition on the inputs, not a tolerance.  About 1e5 draws per case: a given seed
trips it with a probability of a few percent; the seeds below pass."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import Golden, yardstick_grad_check
from brancher_amd import bnn, distributions as D, engine, inference, native, workloads as W
from brancher_amd.lowering import LoweringError
from oracle.svi_oracle import Oracle
from test_bnn_priors_cpu import FIXTURES, MIXTURE, NARROW, prior_model
from test_gpu_bnn_sigma import SOFTMAX, weighted_pass

pytestmark = pytest.mark.gpu
TOL = 1e-5
A = dict(dataset_size=40, batch_size=17, n_features=64, n_hidden=9, n_outputs=1, **NARROW)                               # 64-9-1, tanh
ONE_LAYER = dict(dataset_size=24, batch_size=8, n_features=32, n_hidden=0, n_outputs=2, bias=False, **NARROW)            # 32-2: Rs = 0
B = dict(dataset_size=40, batch_size=33, n_features=36, n_hidden=5, hidden2=4, n_outputs=3, activation="relu", data="normal",
         sigma=[0.3, 0.5, 0.8], **NARROW)                                                                                # 36-5-4-3, relu
B_MIXTURE = dict(weights1="cauchy", b1="laplace", weights2="laplace", b2="cauchy", weights3="normal", b3="laplace")
INVALID, UNSUPPORTED = -1, -2


def build(kw):
    return kw() if callable(kw) else W.build_bnn_regression(W.native_api(), **kw)


def compile_bnn(kw, estimator="pathwise"):
    model = build(kw)
    c = bnn.CompiledBnn(model, model.posterior_model, estimator)
    assert (c.program.row_prior != D.DIST_NORMAL).any()
    return c


def prior_rows(p, theta=None):
    """(prior loc [R], prior scale [R]) in double precision: `bnn.row_parameters` on the program's prior entries"""
    q = copy.copy(p)
    q.row_uniform = p.row_uniform[[2, 3, 0, 1]]
    return bnn.row_parameters(q, theta)


def laplace_draws_are_off_the_kink(p, noise, label):
    """min |w - mu0| > 1e-6 max(|mu|, |s eps|, |mu0|) over the Laplace rows and the samples, from the reported eps [R, N]"""
    rows = np.flatnonzero(p.row_prior == D.DIST_LAPLACE)
    if not rows.size:
        return
    (mu, s), (mu0, _) = bnn.row_parameters(p), prior_rows(p)
    eps = np.asarray(noise, dtype=np.float64)[rows]
    mu, s, mu0 = mu[rows, None], s[rows, None], mu0[rows, None]
    margin = np.abs(mu + s * eps - mu0) - 1e-6 * np.maximum(np.maximum(np.abs(mu), np.abs(s * eps)), np.abs(mu0))
    print("%-30s %d Laplace draws, smallest margin %.3g" % (label, margin.size, margin.min()))
    assert margin.min() > 0, "%s: a Laplace draw lies within rounding of the prior's loc, where sign(u) is undefined between single " \
                             "and double precision: pick another seed" % label


def check_against(c, res, exact, yard, label, grads=None):
    """loss and per-sample f by the bounds of tests/test_gpu_bnn_sigma.py, every gradient by the suite's yardstick"""
    f64 = exact["f"].reshape(-1)
    floor = 1e-6 * (float(np.abs(f64).max()) + 0.5 * c.program.n_rows * 3.0)
    f_err, f_yard = np.abs(res["f"].cpu().numpy() - f64).max(), np.abs(np.asarray(yard["f"]).reshape(-1) - f64).max()
    loss = float(res["loss"].item())
    print(label, "f err %.3g yard %.3g floor %.3g | loss %.9g exact %.9g yard %.9g" % (f_err, f_yard, floor, loss, exact["loss"], yard["loss"]))
    assert float(res["finite"].item()) == 1.0 and f_err <= max(4 * f_yard, floor)
    assert abs(loss - exact["loss"]) <= max(4 * abs(yard["loss"] - exact["loss"]), TOL * abs(exact["loss"]), floor), (loss, exact["loss"], yard["loss"])
    yardstick_grad_check(c.named_grads() if grads is None else grads, exact["grads"], yard["grads"])


def oracle_pair(kw, n, estimator, named, mb):
    return (Oracle(build(kw), dtype=torch.float64).loss_and_grads(n, estimator, named, mb),
            Oracle(build(kw)).loss_and_grads(n, estimator, named, mb))


def reported_draws(c, res, n):
    idx = res["indices"].cpu().numpy()
    return c.named_noise(res["noise"].cpu().numpy(), n), {c.program.indices_name: idx.tolist()}


CASES = {
    # id: (builder keywords, N, middle kernel, data path, seed)
    "64-9-1 laplace": (dict(A, prior="laplace"), 70, "mid_gen", "bf16x3", 3),
    "64-9-1 cauchy": (dict(A, prior="cauchy"), 70, "mid_gen", "bf16x3", 3),
    "64-9-1 mixture": (dict(A, prior=MIXTURE), 70, "mid_gen", "bf16x3", 3),
    "32-2 Rs=0 laplace": (dict(ONE_LAYER, prior="laplace"), 65, "mid_gen", "bf16x3", 3),
    "36-5-4-3 mixture": (dict(B, prior=B_MIXTURE), 130, "upper_gen", "f32", 3),
}


@pytest.mark.parametrize("estimator", ["pathwise", "blackbox"])
@pytest.mark.parametrize("case", list(CASES))
def test_each_case_matches_the_oracle_on_the_reported_draws(case, estimator):
    kw, n, middle, path, seed = CASES[case]
    c = compile_bnn(kw, estimator)
    assert c.middle_path() == middle and c.data_path() == path, (c.middle_path(), c.data_path())
    res = c.evaluate(n, seed=seed, offset=5, want_noise=True, want_indices=True, want_fvalues=True)
    laplace_draws_are_off_the_kink(c.program, res["noise"].cpu().numpy(), case)
    named, mb = reported_draws(c, res, n)
    exact, ref32 = oracle_pair(kw, n, estimator, named, mb)
    check_against(c, res, exact, ref32, "%s %s" % (case, estimator))
    # the same draws fed back in: the noise-in path of both kernels, and bit-equal repeat calls
    res2 = c.evaluate(n, noise=named, minibatch=mb, want_fvalues=True)
    check_against(c, res2, exact, ref32, "%s %s noise-in" % (case, estimator))
    g2 = c.named_grads()
    res3 = c.evaluate(n, noise=named, minibatch=mb, want_fvalues=True)
    assert torch.equal(res2["f"], res3["f"]) and all(np.array_equal(g2[k], v) for k, v in c.named_grads().items())


def test_the_prior_is_a_visible_share_of_the_gradient():
    """the Normal-prior twin on the same draws: every posterior mean's gradient differs by far more than any bound above"""
    kw, n = dict(A, prior="laplace"), 70
    c = compile_bnn(kw)
    c.evaluate(n, seed=3, offset=5)
    g = c.named_grads()
    m = build(dict(A, prior="normal"))
    twin = bnn.CompiledBnn(m, m.posterior_model)
    assert (twin.program.row_prior == D.DIST_NORMAL).all()
    twin.evaluate(n, seed=3, offset=5)
    gt = twin.named_grads()
    for name in ("weights1_loc", "weights2_loc"):
        assert np.abs(g[name] - gt[name]).max() > 1e-2 * np.abs(g[name]).max(), name


@pytest.mark.parametrize("prior", ["laplace", "cauchy"])
def test_taylor1_runs_the_same_launches_on_zero_noise(prior):
    kw, n = dict(A, prior=prior), 70
    c = compile_bnn(kw, "taylor1")
    res = c.evaluate(n, seed=3, offset=5, want_noise=True, want_indices=True)
    laplace_draws_are_off_the_kink(c.program, np.zeros((c.program.n_rows, n)), "taylor1 " + prior)      # f at the posterior's means
    named, mb = reported_draws(c, res, n)
    exact, ref32 = oracle_pair(kw, n, "taylor1", named, mb)
    loss = float(res["loss"].item())
    print("taylor1", prior, loss, exact["loss"], ref32["loss"])
    assert abs(loss - exact["loss"]) <= max(4 * abs(ref32["loss"] - exact["loss"]), TOL * abs(exact["loss"])), (loss, ref32["loss"], exact["loss"])
    yardstick_grad_check(c.named_grads(), exact["grads"], ref32["grads"])


def test_a_learnable_prior_scale_takes_its_gradient_through_the_rows():
    """exp(log_tau), a learnable root of the joint model, as the scale of weights2's Laplace prior: rowg[s0] = prior_weight T2 through
    the chain rule of the entry.  Its bound: err <= max(4 |oracle32 - oracle64|, 1e-5 max |oracle64|, 1e-6 S), S the size of the
    summands, mean_n sum_r (|u| + 1) / s0 |d s0 / d theta| from the oracle's own draws (|u| - 1 cancels where the prior fits)"""
    kw, n = (lambda: prior_model("laplace", learnable_scale=True)), 70
    for estimator in ("pathwise", "blackbox"):
        c = compile_bnn(kw, estimator)
        res = c.evaluate(n, seed=4, offset=1, want_noise=True, want_indices=True, want_fvalues=True)
        laplace_draws_are_off_the_kink(c.program, res["noise"].cpu().numpy(), "learnable prior scale")
        named, mb = reported_draws(c, res, n)
        exact, ref32 = oracle_pair(kw, n, estimator, named, mb)
        grads = c.named_grads()
        others = lambda d: {k: v for k, v in d.items() if k != "log_tau"}
        check_against(c, res, dict(exact, grads=others(exact["grads"])), dict(ref32, grads=others(ref32["grads"])), "learnable prior scale " + estimator)
        s0 = 0.3                                                           # exp(log_tau) at the start; d s0 / d theta = s0
        u = (np.asarray(exact["samples"]["weights2"], dtype=np.float64).reshape(n, -1) - 0.1) / s0
        S = ((np.abs(u) + 1.0) / s0 * s0).sum() / n
        g64 = float(exact["grads"]["log_tau"].reshape(-1)[0])
        err = abs(float(grads["log_tau"].reshape(-1)[0]) - g64)
        bound = max(4 * abs(float(np.asarray(ref32["grads"]["log_tau"]).reshape(-1)[0]) - g64), TOL * abs(g64), 1e-6 * S)
        print("log_tau", estimator, grads["log_tau"].reshape(-1), g64, "err %.3g bound %.3g S %.3g" % (err, bound, S))
        assert abs(g64) > 10 * bound, "the case's gradient of the prior scale is all cancellation"
        assert err <= bound, (estimator, err, bound)


def test_a_user_defined_estimator_on_the_mixture():
    """engine.custom_estimator_loss under a softmax of f: a_n weights T0 / T1 (and N in T2) as it weights sum eps and sum eps^2"""
    from brancher_amd import gradient_estimators as ge
    kw, n = dict(A, prior=MIXTURE), 70
    model = build(kw)
    rng = np.random.RandomState(6)
    p = bnn.lower_bnn(model, model.posterior_model, "blackbox")
    named = {t["name"]: rng.normal(size=(n, 1, t["rows"], t["cols"])).astype(np.float32) for t in p.tensors}
    laplace_draws_are_off_the_kink(p, np.concatenate([named[t["name"]].reshape(n, -1).T for t in p.tensors]), "custom mixture")
    mb = {"indices": rng.permutation(A["dataset_size"])[:A["batch_size"]].tolist()}
    value = engine.custom_estimator_loss(model, model.posterior_model, W.custom_estimators(ge)["softmax"], n, noise=named, minibatch=mb)
    assert type(value.compiled).__name__ == "CompiledBnn" and value.compiled.program.summary()["priors"] == MIXTURE
    exact, ref32 = oracle_pair(kw, n, SOFTMAX, named, mb)
    loss = -float(value.detach().cpu())
    assert abs(loss - exact["loss"]) <= max(4 * abs(ref32["loss"] - exact["loss"]), TOL * abs(exact["loss"])), (loss, ref32["loss"], exact["loss"])
    yardstick_grad_check(value.compiled.named_grads(), exact["grads"], ref32["grads"])
    # ... and the weights do differ per sample
    c = compile_bnn(kw, "blackbox")
    _, grads, a = weighted_pass(c, SOFTMAX, n, named, mb)
    assert np.ptp(a) > 0.1 * np.abs(a).max()
    yardstick_grad_check(grads, exact["grads"], ref32["grads"])


@pytest.mark.parametrize("name", FIXTURES)
def test_the_reference_fixtures(name):
    """loss, per-sample terms and every gradient under Pathwise, BlackBox and Taylor1, and the Adam trajectory of the real reference: the
    double-precision oracle is the truth, the fixture the yardstick"""
    g = Golden(name)
    f_ref = (g.data["lp"] + g.data["H"]).reshape(-1)
    probe = compile_bnn(g.build)
    noise = probe.noise_from_named(g.noise, g.N)
    laplace_draws_are_off_the_kink(probe.program, noise, name[-14:])
    for estimator in ("pathwise", "blackbox"):
        c = compile_bnn(g.build, estimator)
        res = c.evaluate(g.N, noise=g.noise, minibatch=g.minibatch, want_fvalues=True)
        exact = Oracle(g.build(), dtype=torch.float64).loss_and_grads(g.N, estimator, g.noise, g.minibatch)
        fixture = dict(f=f_ref, loss=float(g.data["loss_" + estimator]), grads=g.group("grad_%s/" % estimator))
        check_against(c, res, exact, fixture, "%s %s" % (name[-14:], estimator))
        if estimator == "blackbox":
            lq64 = exact["lq"].reshape(-1)
            assert np.abs(res["lq"].cpu().numpy() - lq64).max() <= max(4 * np.abs(g.data["lq"].reshape(-1) - lq64).max(), TOL * np.abs(lq64).max())
    c = compile_bnn(g.build, "taylor1")
    laplace_draws_are_off_the_kink(c.program, np.zeros_like(noise), name[-14:] + " taylor1")
    exact = Oracle(g.build(), dtype=torch.float64).loss_and_grads(g.N, "taylor1", g.noise, g.minibatch)
    res = c.evaluate(g.N, noise=g.noise, minibatch=g.minibatch)
    loss, ref = float(res["loss"].item()), float(g.data["loss_taylor1"])
    assert abs(loss - exact["loss"]) <= max(4 * abs(ref - exact["loss"]), TOL * abs(exact["loss"])), (loss, ref, exact["loss"])
    yardstick_grad_check(c.named_grads(), exact["grads"], g.group("grad_taylor1/"))
    # the trajectory under Adam
    tr = g.meta["trajectory"]
    c = compile_bnn(g.build)
    laplace_draws_are_off_the_kink(c.program, c.noise_from_named(g.trajectory_noise()[0], tr["n"]), name[-14:] + " trajectory, iteration 0")
    losses, finite = c.train(tr["iters"], tr["n"], tr["optimizer"], noise_seq=g.trajectory_noise(),
                             minibatch_seq=g.trajectory_minibatch(), **g.opt_kwargs())
    assert c.last_mode == "stepwise" and finite.cpu().numpy().all()
    o = Oracle(g.build(), dtype=torch.float64)
    exact_losses = o.train(tr["iters"], tr["n"], tr["optimizer"], noise_seq=g.trajectory_noise(),
                           minibatch_seq=g.trajectory_minibatch(), **g.opt_kwargs()).astype(np.float64)
    got, ref_l = losses.cpu().numpy().astype(np.float64), g.data["traj/losses"].astype(np.float64)
    assert np.abs(got - exact_losses).max() <= max(4 * np.abs(ref_l - exact_losses).max(), TOL * np.abs(exact_losses).max())
    after = g.group("traj/param_after/")
    exact_after = {pname: t.detach().numpy() for pname, t in o.named_parameters().items()}
    for pname, p in c.named_params().items():
        e64 = exact_after[pname].reshape(p.shape)
        assert np.abs(p - e64).max() <= max(4 * np.abs(after[pname].reshape(p.shape) - e64).max(), 2e-5 * (1 + np.abs(e64).max())), pname


def test_predict_returns_what_the_normal_prior_twin_returns():
    """bnn_predict shares bnn_draw, whose prior partials it never reads: same posterior values, seed and offset, equal tensors"""
    c = compile_bnn(dict(A, prior="laplace"))
    m = build(dict(A, prior="normal"))
    twin = bnn.CompiledBnn(m, m.posterior_model)
    assert (twin.program.row_prior == D.DIST_NORMAL).all()
    assert all(np.array_equal(v, twin.named_params()[k]) for k, v in c.named_params().items())
    rows = c.program.dataset[:7]
    a = c.predict(rows, 70, seed=2, offset=9, want_outputs=True, want_draws=True, want_noise=True)
    b = twin.predict(rows, 70, seed=2, offset=9, want_outputs=True, want_draws=True, want_noise=True)
    for key in ("probs", "mean", "var", "outputs", "draws", "noise"):
        assert torch.equal(a[key], b[key]), key
    assert torch.isfinite(a["mean"]).all()


def test_the_setter_checks_its_arguments_and_its_moment():
    m = build(dict(A, prior="normal"))
    c = bnn.CompiledBnn(m, m.posterior_model)
    R = c.program.n_rows
    kinds = np.full(R, D.DIST_LAPLACE, dtype=np.uint8)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    lib = c.lib
    assert lib.bsvi_bnn_set_row_priors(c.handle, ptr(kinds), R - 1) == INVALID and b"n_rows" in lib.bsvi_last_error()
    assert lib.bsvi_bnn_set_row_priors(c.handle, None, R) == INVALID
    bad = kinds.copy()
    bad[R // 2] = D.DIST_LOGNORMAL
    assert lib.bsvi_bnn_set_row_priors(c.handle, ptr(bad), R) == UNSUPPORTED and b"Normal, Laplace or Cauchy" in lib.bsvi_last_error()
    bad[R // 2] = 0
    assert lib.bsvi_bnn_set_row_priors(c.handle, ptr(bad), R) == UNSUPPORTED
    # nothing of the refused calls stuck: the model is its all-Normal self, and equal to a model that was never asked
    first = c.evaluate(70, seed=3, offset=5)["loss"].clone()
    m2 = build(dict(A, prior="normal"))
    assert torch.equal(first, bnn.CompiledBnn(m2, m2.posterior_model).evaluate(70, seed=3, offset=5)["loss"])
    # after a launch the priors stay
    assert lib.bsvi_bnn_set_row_priors(c.handle, ptr(kinds), R) == INVALID and b"launch" in lib.bsvi_last_error()
    assert torch.equal(first, c.evaluate(70, seed=3, offset=5)["loss"])
    # before one, the call takes effect: the Laplace model's loss
    m3 = build(dict(A, prior="normal"))
    c3 = bnn.CompiledBnn(m3, m3.posterior_model)
    assert lib.bsvi_bnn_set_row_priors(c3.handle, ptr(kinds), R) == 0
    want = compile_bnn(dict(A, prior="laplace")).evaluate(70, seed=3, offset=5)["loss"]
    assert torch.equal(c3.evaluate(70, seed=3, offset=5)["loss"], want) and not torch.equal(want, first)


def test_the_public_route_serves_the_model_and_training_lowers_the_loss():
    """`engine.compile_model` on the 64-9-1 Laplace network: before this feature the lowering refused it ("weights and biases must be
    Normal variables") and every engine with it.  Then perform_inference: a finite loss curve that goes down."""
    kw = dict(A, prior="laplace")
    try:
        c = engine.compile_model(build(kw), None, "pathwise")
    except LoweringError as err:
        pytest.fail("the public route refuses a Laplace prior: %s" % err)
    assert type(c).__name__ == "CompiledBnn" and set(c.program.summary()["priors"].values()) == {"laplace"}
    assert c.middle_path() == "mid_gen"
    for prior in ("laplace", "cauchy"):
        model, method = build(dict(A, prior=prior)), inference.ReverseKL()
        torch.manual_seed(7)
        inference.perform_inference(model, number_iterations=60, number_samples=50, optimizer="Adam", lr=1e-2, inference_method=method)
        assert type(method.last_compiled).__name__ == "CompiledBnn"
        curve = np.asarray(model.diagnostics["loss curve"], dtype=np.float64)
        print(prior, "first ten %.6g last ten %.6g" % (curve[:10].mean(), curve[-10:].mean()))
        assert len(curve) == 60 and np.isfinite(curve).all() and curve[-10:].mean() < curve[:10].mean()
