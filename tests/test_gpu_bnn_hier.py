"""Latent prior scales of the Bayesian-neural-network family on the device (bsvi_bnn_set_scale_latents): a tensor's prior
scale b * tau with tau a LogNormal latent under a mean-field LogNormal posterior.  The latent blocks of bnn_head_gather (l, 1 / tau, the
draw), the per-latent sums of bnn_draw<true, true> (u psi - 1 over the rows under a latent, per chunk), T0 / T1 of
bnn_row_sums<true, true> with the per-sample scale inside the sum, bnn_latent_terms / bnn_latent_grads and the constants of bnn_epilogue.
Every check is against `Oracle(..., dtype=float64)` on the draws and indices the kernels report, the single-precision oracle the
yardstick: tests/test_gpu_bnn_priors.py's check_against and conftest.yardstick_grad_check as they stand.  Laplace rows first pass
`laplace_draws_are_off_the_kink` (sign(u) = sign(w - mu0) whatever the sample's scale is).

The shapes are the smallest at which the new code can go wrong: 64-9-1 (weights1 spans two chunks of 256 rows and part of a third, which
holds rows of both latents; quads straddle tensors; tau1 is shared by tensors in different chunks; the last sample block is partial),
32-2 without small tensors (T = 1), 36-5-4-3 with five latents over five of its six tensors (T > 4: a second Philox call for the
latents; differing multipliers; weights3 keeps its constant scale; a mixture of the three prior kinds) and a classifier on a static
middle kernel."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import yardstick_grad_check
from brancher_amd import bnn, engine, inference, native, workloads as W
from brancher_amd.lowering import LoweringError
from oracle import philox_ref
from oracle.svi_oracle import Oracle
from test_bnn_hier_cpu import A, B, B_LATENTS, CLASSIFIER, ONE_LAYER, hand_built
from test_gpu_bnn_priors import B_MIXTURE, TOL, check_against, laplace_draws_are_off_the_kink
from test_gpu_noise import NORMAL_TOL
from test_gpu_bnn_sigma import SOFTMAX, weighted_pass

pytestmark = pytest.mark.gpu
INVALID = -1


def build(kw):
    if callable(kw):
        return kw()
    kw = dict(kw)
    builder = W.build_bayesian_neural_network if kw.pop("classifier", False) else W.build_bnn_regression
    return builder(W.native_api(), **kw)


def compile_bnn(kw, estimator="pathwise"):
    model = build(kw)
    c = bnn.CompiledBnn(model, model.posterior_model, estimator)
    assert c.program.scale_latents and c.program.n_noise == c.program.n_rows + len(c.program.scale_latents)
    return c


def oracle_pair(kw, n, estimator, named, mb):
    return (Oracle(build(kw), dtype=torch.float64).loss_and_grads(n, estimator, named, mb),
            Oracle(build(kw)).loss_and_grads(n, estimator, named, mb))


def reported_draws(c, res, n):
    return c.named_noise(res["noise"].cpu().numpy(), n), {c.program.indices_name: res["indices"].cpu().numpy().tolist()}


CASES = {
    # id: (builder keywords, N, middle kernel, data path, seed, environment)
    "64-9-1 layer": (dict(A, scale_latent="layer"), 70, "mid_gen", "bf16x3", 3, {}),
    "32-2 Rs=0 one latent laplace": (dict(ONE_LAYER, scale_latent="global", prior="laplace"), 65, "mid_gen", "bf16x3", 3, {}),
    "36-5-4-3 five latents": (dict(B, prior=B_MIXTURE, scale_latent=B_LATENTS), 130, "upper_gen", "f32", 3, {}),
    "16-6-3 classifier global": (dict(CLASSIFIER, scale_latent="global"), 70, "upper_lds", "bf16x3", 3, dict(BSVI_BNN_MID="0", BSVI_BNN_JIT="0")),
    "32-2 learnable prior roots": (hand_built, 65, "mid_gen", "bf16x3", 3, {}),
}


@pytest.mark.parametrize("estimator", ["pathwise", "blackbox"])
@pytest.mark.parametrize("case", list(CASES))
def test_each_case_matches_the_oracle_on_the_reported_draws(case, estimator, monkeypatch):
    kw, n, middle, path, seed, env = CASES[case]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    c = compile_bnn(kw, estimator)
    assert c.middle_path() == middle and c.data_path() == path, (c.middle_path(), c.data_path())
    res = c.evaluate(n, seed=seed, offset=5, want_noise=True, want_indices=True, want_fvalues=True)
    assert tuple(res["noise"].shape) == (c.program.n_noise, n)
    laplace_draws_are_off_the_kink(c.program, res["noise"].cpu().numpy(), case)
    named, mb = reported_draws(c, res, n)
    assert all(named[l["name"]].shape == (n, 1, 1, 1) for l in c.program.scale_latents)
    exact, ref32 = oracle_pair(kw, n, estimator, named, mb)
    # (every learnable root: the latents' q loc / q scale, and in the hand-built case the roots of their prior)
    assert all(l["name"] + "_loc" in exact["grads"] and l["name"] + "_scale" in exact["grads"] for l in c.program.scale_latents)
    check_against(c, res, exact, ref32, "%s %s" % (case, estimator))
    if estimator == "blackbox":
        lq64 = exact["lq"].reshape(-1)
        lq_err, lq_yard = np.abs(res["lq"].cpu().numpy() - lq64).max(), np.abs(np.asarray(ref32["lq"]).reshape(-1) - lq64).max()
        print(case, "log q err %.3g yard %.3g" % (lq_err, lq_yard))
        assert lq_err <= max(4 * lq_yard, TOL * np.abs(lq64).max())
    # the same draws fed back in: the noise-in path of every kernel that draws, and bit-equal repeat calls
    res2 = c.evaluate(n, noise=named, minibatch=mb, want_fvalues=True)
    check_against(c, res2, exact, ref32, "%s %s noise-in" % (case, estimator))
    g2 = c.named_grads()
    res3 = c.evaluate(n, noise=named, minibatch=mb, want_fvalues=True)
    assert torch.equal(res2["f"], res3["f"]) and torch.equal(res2["loss"], res3["loss"])
    assert all(np.array_equal(g2[k], v) for k, v in c.named_grads().items())


def test_the_latents_randomness_is_in_the_result():
    """the twin whose scales are fixed at the posterior medians exp(m_t), on the same weight draws: the weights' gradients differ by far
    more than any bound above (a narrow, uncertain scale: E 1 / tau^2 is exp(2 s^2) = 1.65 times its value at the median)"""
    kw, n = dict(A, scale_latent="layer", scale_latent_q=(-1.5, 0.5)), 70
    c = compile_bnn(kw)
    res = c.evaluate(n, seed=3, offset=5, want_noise=True, want_indices=True)
    g = c.named_grads()
    named, mb = reported_draws(c, res, n)
    m = build(dict(A, prior_scale=float(np.exp(-1.5))))
    twin = bnn.CompiledBnn(m, m.posterior_model)
    assert not twin.program.scale_latents
    twin.evaluate(n, noise={k: v for k, v in named.items() if not k.startswith("tau")}, minibatch=mb)
    gt = twin.named_grads()
    for name in ("weights1_loc", "weights2_loc"):
        assert np.abs(g[name] - gt[name]).max() > 1e-2 * np.abs(g[name]).max(), name


def test_a_user_defined_estimator_through_the_weighted_second_pass():
    kw, n = dict(A, scale_latent="layer", prior="laplace"), 70
    c = compile_bnn(kw, "blackbox")
    res = c.evaluate(n, seed=8, offset=3, want_noise=True, want_indices=True)
    laplace_draws_are_off_the_kink(c.program, res["noise"].cpu().numpy(), "weighted pass")
    named, mb = reported_draws(c, res, n)
    exact, ref32 = oracle_pair(kw, n, SOFTMAX, named, mb)
    loss, grads, a = weighted_pass(c, SOFTMAX, n, named, mb)
    assert np.ptp(a) > 0.1 * np.abs(a).max()                      # the weights do differ
    assert abs(loss - exact["loss"]) <= max(4 * abs(ref32["loss"] - exact["loss"]), TOL * abs(exact["loss"])), (loss, ref32["loss"], exact["loss"])
    yardstick_grad_check(grads, exact["grads"], ref32["grads"])


def test_four_adam_steps_follow_the_oracle_and_the_two_step_paths_agree():
    """(64 samples: the fused step multiplies the sums by -1 / N where the step of the sharded path divides by N — the same value to the bit
    where 1 / N is exact, one rounding apart elsewhere, for every model of the family: tests/test_gpu_bnn_normal.py compares the two paths
    at N = 40 to 1e-6)"""
    kw, n, iters, lr = dict(A, scale_latent="layer"), 64, 4, 1e-2
    probe = compile_bnn(kw)
    noise_seq, mb_seq = [], []
    for it in range(iters):
        res = probe.evaluate(n, seed=11, offset=it, want_noise=True, want_indices=True)
        named, mb = reported_draws(probe, res, n)
        noise_seq.append(named)
        mb_seq.append(mb)
    a, b = compile_bnn(kw), compile_bnn(kw)
    la, fa = a.train(iters, n, "Adam", noise_seq=noise_seq, minibatch_seq=mb_seq, lr=lr)
    lb, _ = b.train(iters, n, "Adam", noise_seq=noise_seq, minibatch_seq=mb_seq, lr=lr, _force_sharded_path=True)
    assert a.last_mode == "stepwise" and fa.cpu().numpy().all()
    assert torch.equal(la, lb) and all(np.array_equal(v, b.named_params()[k]) for k, v in a.named_params().items())
    o64, o32 = Oracle(build(kw), dtype=torch.float64), Oracle(build(kw))
    exact_losses = o64.train(iters, n, "Adam", noise_seq=noise_seq, minibatch_seq=mb_seq, lr=lr).astype(np.float64)
    ref_losses = o32.train(iters, n, "Adam", noise_seq=noise_seq, minibatch_seq=mb_seq, lr=lr).astype(np.float64)
    got = la.cpu().numpy().astype(np.float64)
    print("losses", got, exact_losses, ref_losses)
    assert np.abs(got - exact_losses).max() <= max(4 * np.abs(ref_losses - exact_losses).max(), TOL * np.abs(exact_losses).max())
    e64 = {k: t.detach().numpy() for k, t in o64.named_parameters().items()}
    e32 = {k: t.detach().numpy() for k, t in o32.named_parameters().items()}
    params = a.named_params()
    assert abs(float(params["tau1_loc"].reshape(-1)[0])) > 0.5 * iters * lr * 0.5          # Adam steps of ~lr each, all one way at the start
    for pname, p in params.items():
        x = e64[pname].reshape(p.shape)
        assert np.abs(p - x).max() <= max(4 * np.abs(e32[pname].reshape(p.shape) - x).max(), 2e-5 * (1 + np.abs(x).max())), pname
    # predict on the trained model: the weights' posterior alone, its noise [n_rows, N]
    out = a.predict(a.program.dataset[:5], 33, seed=2, offset=9, want_noise=True)
    assert tuple(out["noise"].shape) == (a.program.n_rows, 33) and torch.isfinite(out["mean"]).all()
    again = a.predict(a.program.dataset[:5], 33, noise=out["noise"])
    assert torch.equal(out["mean"], again["mean"])


def test_the_latents_draws_are_the_stated_philox_words_and_equal_over_shards():
    """latent t: normal t & 3 of the row-quad call whose quad index is ceil(n_rows / 4) + (t >> 2), reported in row n_rows + t"""
    kw, n, seed, offset = dict(B, prior=B_MIXTURE, scale_latent=B_LATENTS), 130, 9, 6
    c = compile_bnn(kw)
    R, T = c.program.n_rows, len(c.program.scale_latents)
    whole = c.evaluate(n, seed=seed, offset=offset, want_noise=True)["noise"].cpu().numpy()
    quads = (R + 3) // 4
    rows = philox_ref.dense_noise(seed, offset, 0, n, 4 * quads + T)          # (row r: normal r & 3 of the call of quad r >> 2)
    want = np.stack([rows[4 * (quads + (t >> 2)) + (t & 3)] for t in range(T)])
    got = whole[R:]
    print("latent draws: max |device - host| %.3g (bound %.3g)" % (np.abs(got - want).max(), NORMAL_TOL))
    assert np.abs(got - want).max() <= NORMAL_TOL
    assert np.abs(whole[:R] - rows[:R]).max() <= NORMAL_TOL                    # (the weights' rows are where they were)
    parts = []
    for base, n_local in ((0, 33), (33, 97)):
        out = torch.empty((c.program.n_noise, n_local), device=c.device)
        args = c._args(n_local, n, base, seed=seed, offset=offset, noise_out=out)
        native.check(c.lib.bsvi_bnn_fwd_bwd(c.handle, C.byref(args)))
        parts.append(out.cpu().numpy())
    assert np.array_equal(np.concatenate(parts, axis=1), whole)


def test_taylor1_and_the_frame_level_sampler_are_refused_by_name():
    model = build(dict(A, scale_latent="layer"))
    with pytest.raises(LoweringError, match="Taylor1 estimator does not serve a model with scale latents"):
        bnn.CompiledBnn(model, model.posterior_model, "taylor1")
    model, method = build(dict(A, scale_latent="layer")), inference.ReverseKL()
    inference.perform_inference(model, number_iterations=3, number_samples=20, optimizer="Adam", lr=1e-2, inference_method=method)
    assert type(method.last_compiled).__name__ == "CompiledBnn" and np.isfinite(model.diagnostics["loss curve"]).all()
    with pytest.raises(NotImplementedError, match="scale latents"):
        model._get_posterior_sample(4)


def test_the_setter_checks_its_arguments_and_a_model_without_latents_is_what_it_was():
    """the guard that the old path reads none of the new tables: a constant-scale model whose handle was refused every call gives the
    arrays of one that was never asked; after a launch the call is refused"""
    m = build(dict(A))
    c = bnn.CompiledBnn(m, m.posterior_model)
    R, lib = c.program.n_rows, c.lib
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    rows = np.zeros(R, dtype=np.uint8)
    table = np.zeros(4, dtype=np.uint32)
    assert lib.bsvi_bnn_set_scale_latents(c.handle, 1, ptr(rows), R - 1, ptr(table)) == INVALID and b"n_rows" in lib.bsvi_last_error()
    assert lib.bsvi_bnn_set_scale_latents(c.handle, 0, ptr(rows), R, ptr(table)) == INVALID
    assert lib.bsvi_bnn_set_scale_latents(c.handle, 19, ptr(rows), R, ptr(np.zeros(76, dtype=np.uint32))) == INVALID
    assert lib.bsvi_bnn_set_scale_latents(c.handle, 1, None, R, ptr(table)) == INVALID
    bad = rows.copy()
    bad[R // 2] = 1
    assert lib.bsvi_bnn_set_scale_latents(c.handle, 1, ptr(bad), R, ptr(table)) == INVALID and b"past n_latents" in lib.bsvi_last_error()
    past = np.full(4, len(c.program.uniform), dtype=np.uint32)
    assert lib.bsvi_bnn_set_scale_latents(c.handle, 1, ptr(rows), R, ptr(past)) == INVALID and b"uniform table" in lib.bsvi_last_error()
    first = c.evaluate(70, seed=3, offset=5, want_fvalues=True)
    f, g = first["f"].clone(), c.named_grads()
    m2 = build(dict(A))
    c2 = bnn.CompiledBnn(m2, m2.posterior_model)
    assert int(lib.bsvi_bnn_workspace_bytes(c.handle, 70)) == int(lib.bsvi_bnn_workspace_bytes(c2.handle, 70))
    second = c2.evaluate(70, seed=3, offset=5, want_fvalues=True)
    assert torch.equal(f, second["f"]) and all(np.array_equal(g[k], v) for k, v in c2.named_grads().items())
    assert lib.bsvi_bnn_set_scale_latents(c.handle, 1, ptr(rows), R, ptr(table)) == INVALID and b"launch" in lib.bsvi_last_error()
    # ... and the workspace grows for a handle with latents only
    assert int(lib.bsvi_bnn_workspace_bytes(compile_bnn(dict(A, scale_latent="layer")).handle, 70)) > int(lib.bsvi_bnn_workspace_bytes(c.handle, 70))


def test_the_public_route_serves_the_model_and_training_lowers_the_loss():
    kw = dict(A, scale_latent="layer")
    try:
        c = engine.compile_model(build(kw), None, "pathwise")
    except LoweringError as err:
        pytest.fail("the public route refuses a hierarchical prior: %s" % err)
    assert type(c).__name__ == "CompiledBnn" and set(c.program.summary()["scale_latents"]) == {"tau1", "tau2"}
    model, method = build(kw), inference.ReverseKL()
    torch.manual_seed(7)
    inference.perform_inference(model, number_iterations=60, number_samples=50, optimizer="Adam", lr=1e-2, inference_method=method)
    curve = np.asarray(model.diagnostics["loss curve"], dtype=np.float64)
    print("first ten %.6g last ten %.6g" % (curve[:10].mean(), curve[-10:].mean()))
    assert len(curve) == 60 and np.isfinite(curve).all() and curve[-10:].mean() < curve[:10].mean()
