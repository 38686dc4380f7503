"""A learnable sigma of the Normal likelihood on the device (bsvi_bnn_create_normal_learnable): the gradient
G_c = sum_n sum_b wgt (u^2 - 1) / sigma_c at the three likelihood sites of csrc/bnn_kernel.inc (bnn_mid_gen, bnn_upper_gen, the static
bnn_upper with its activations in LDS and in memory), the reductions behind them, the add into the uniform entry, the step and the
predictive pass that follows it.  Every check is against `Oracle(..., dtype=float64)` on the draws and indices the kernels report, the
single-precision oracle (or a fixture of the real reference) the yardstick: conftest.yardstick_grad_check for every tensor, and for
sigma's root  err <= max(4 |oracle32 - oracle64|, 1e-5 max |oracle64|, 1e-6 S),  S = mean_n sum_b (u^2 + 1) / sigma_c |d sigma / d theta|
from the oracle's own draws: u^2 - 1 cancels near calibration, and S is the size of the summands — the floor check_against applies to f.
sigma starts at 0.5 against the data's 0.3 / 0.8, so that the gradient is not all cancellation.  Shapes: minibatches of 17 and 33 rows
(B_pad 32 / 64), N of 65, 70 and 130 (a partial last wave), 512 rows for the pairs-of-rows form of bnn_mid_gen."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import Golden, yardstick_grad_check
from brancher_amd import bnn, engine, inference, lowering, native, workloads as W
from brancher_amd.lowering import LoweringError
from oracle.svi_oracle import Oracle
from test_bnn_sigma_cpu import sigma_entries, sigma_model

pytestmark = pytest.mark.gpu
TOL = 1e-5
LEARN = dict(learnable_sigma=True, sigma=0.3, sigma_init=0.5)
A = dict(dataset_size=40, batch_size=17, n_features=64, n_hidden=9, n_outputs=1, **LEARN)                               # 64-9-1, tanh
ONE_LAYER = dict(dataset_size=24, batch_size=8, n_features=32, n_hidden=0, n_outputs=2, bias=False, **LEARN)            # 32-2: Rs = 0
PAIRS = dict(dataset_size=520, batch_size=512, n_features=16, n_hidden=4, n_outputs=2, **LEARN)                         # 16-4-2, B_pad 512
B = dict(dataset_size=40, batch_size=33, n_features=36, n_hidden=5, hidden2=4, n_outputs=3, activation="relu", data="normal",
         sigma=[0.3, 0.5, 0.8], learnable_sigma="exp", sigma_init=[0.5, 0.5, 0.5])                                      # 36-5-4-3, relu
MEM = dict(widths=[32, 18, 18, 3], batch_size=33, dataset_size=40, data="normal", q_scale=0.3, sigma=[0.3, 0.5, 0.8],
           learnable_sigma=True, sigma_init=[0.5, 0.5, 0.5])                                                            # 32-18-18-3
FIXTURES = ["bnn_sigma/bnn_sigma_tanh_P32_H6_C1_DS30_B12_N5", "bnn_sigma/bnn_sigma_linear_P16_C2_DS24_B10_N6"]
SOFTMAX = lambda f, lq: (torch.softmax(0.1 * f.detach().reshape(-1), dim=0).reshape(f.shape) * f).sum()
NP_ACT = {0: lambda v: v, 1: np.tanh, 2: lambda v: np.maximum(v, 0.0), 3: lambda v: 1.0 / (1.0 + np.exp(-v)), 4: lambda v: np.log1p(np.exp(v))}


def build(kw):
    return kw() if callable(kw) else W.build_bnn_regression(W.native_api(), **kw)


def compile_bnn(kw, estimator="pathwise"):
    model = build(kw)
    c = bnn.CompiledBnn(model, model.posterior_model, estimator)
    assert c.program.likelihood == bnn.LIK_NORMAL and c.program.scale_learnable
    return c


def summands(p, samples, idx, weights=None, theta=None):
    """S per element of sigma's root: sum_n |w_n| sum_b (u^2 + 1) / sigma_c |d sigma_c / d theta| (w_n = 1 / N unless the caller weights the
    samples), the chain forward in double precision on the weights the ORACLE drew"""
    n = next(iter(samples.values())).shape[0]
    h = np.broadcast_to(p.dataset[np.asarray(idx)].astype(np.float64), (n, len(idx), p.n_features))
    for l in p.layers:
        h = np.einsum("nij,nbj->nbi", np.asarray(samples[l["weights"]], dtype=np.float64).reshape(n, l["rows"], l["cols"]), h)
        if l["bias"] is not None:
            h = h + np.asarray(samples[l["bias"]], dtype=np.float64).reshape(n, 1, l["rows"])
        h = NP_ACT[l["activation"]](h)
    sig, dsig, name = sigma_entries(p, theta)
    u = (p.labels[np.asarray(idx)].astype(np.float64)[None] - h) / sig
    per = ((u * u + 1.0) / sig * np.abs(dsig)).sum(axis=1)                                       # [N, C]
    w = np.full(n, 1.0 / n) if weights is None else np.abs(np.asarray(weights, dtype=np.float64).reshape(-1))
    s = (w[:, None] * per).sum(axis=0)
    return name, (s if p.scale_stride else s.sum())


WORST = {}


def sigma_grad_check(p, grads, exact, yard_grads, idx, label, weights=None):
    """every tensor by the suite's yardstick, sigma's root by its own bound; prints err / bound before it asserts"""
    name, S = summands(p, exact["samples"], idx, weights)
    g64 = exact["grads"][name].reshape(-1)
    err = np.abs(grads[name].reshape(-1) - g64)
    bound = np.maximum(np.maximum(4 * np.abs(np.asarray(yard_grads[name]).reshape(-1) - g64), TOL * np.abs(g64).max()), 1e-6 * np.asarray(S).reshape(-1))
    ratio = float((err / bound).max())
    WORST[label] = ratio
    print("%-28s %s grad %s oracle64 %s err %s bound %s err/bound %.3g" % (label, name, grads[name].reshape(-1), g64, err, bound, ratio))
    assert np.abs(g64).min() > 10 * bound.max(), "the case's gradient of sigma is all cancellation"
    assert (err <= bound).all(), (label, name, err, bound)
    others = {k: v for k, v in exact["grads"].items() if k != name}
    yardstick_grad_check(grads, others, yard_grads)


def check_against(c, res, exact, yard, idx, label):
    """loss and per-sample f as tests/test_gpu_bnn_normal.py checks them, then the gradients"""
    f64 = exact["f"].reshape(-1)
    floor = 1e-6 * (float(np.abs(f64).max()) + 0.5 * c.program.n_rows * 3.0)
    f_err, f_yard = np.abs(res["f"].cpu().numpy() - f64).max(), np.abs(np.asarray(yard["f"]).reshape(-1) - f64).max()
    loss = float(res["loss"].item())
    print(label, "f err %.3g yard %.3g floor %.3g | loss %.9g exact %.9g yard %.9g" % (f_err, f_yard, floor, loss, exact["loss"], yard["loss"]))
    assert float(res["finite"].item()) == 1.0 and f_err <= max(4 * f_yard, floor)
    assert abs(loss - exact["loss"]) <= max(4 * abs(yard["loss"] - exact["loss"]), TOL * abs(exact["loss"]), floor), (loss, exact["loss"], yard["loss"])
    sigma_grad_check(c.program, c.named_grads(), exact, yard["grads"], idx, label)


def oracle_pair(kw, n, estimator, named, mb):
    return (Oracle(build(kw), dtype=torch.float64).loss_and_grads(n, estimator, named, mb),
            Oracle(build(kw)).loss_and_grads(n, estimator, named, mb))


SITES = {
    # id: (builder keywords, N, middle kernel, data path, environment)
    "mid_gen 64-9-1": (A, 70, "mid_gen", "bf16x3", {}),
    "mid_gen 32-2 Rs=0": (ONE_LAYER, 65, "mid_gen", "bf16x3", {}),
    "mid_gen 16-4-2 pairs": (PAIRS, 3, "mid_gen", "bf16x3", {}),
    "upper_gen 36-5-4-3": (B, 130, "upper_gen", "f32", {}),
    "upper_lds 36-5-4-3": (B, 130, "upper_lds", "f32", {"BSVI_BNN_JIT": "0"}),
    "upper_mem 32-18-18-3": (MEM, 70, "upper_mem", "f32", {}),
}


@pytest.mark.parametrize("estimator", ["pathwise", "blackbox"])
@pytest.mark.parametrize("site", list(SITES))
def test_each_site_matches_the_oracle_on_the_reported_draws(site, estimator, monkeypatch):
    kw, n, middle, path, env = SITES[site]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    c = compile_bnn(kw, estimator)
    assert c.middle_path() == middle and c.data_path() == path, (c.middle_path(), c.data_path())
    res = c.evaluate(n, seed=3, offset=5, want_noise=True, want_indices=True, want_fvalues=True)
    assert c.middle_path() == middle
    idx = res["indices"].cpu().numpy()
    named, mb = c.named_noise(res["noise"].cpu().numpy(), n), {c.program.indices_name: idx.tolist()}
    exact, ref32 = oracle_pair(kw, n, estimator, named, mb)
    check_against(c, res, exact, ref32, idx, "%s %s" % (site, estimator))
    # the same draws fed back in: the noise-in path of every kernel, and bit-equal repeat calls
    res2 = c.evaluate(n, noise=named, minibatch=mb, want_fvalues=True)
    check_against(c, res2, exact, ref32, idx, "%s %s noise-in" % (site, estimator))
    g2 = c.named_grads()
    res3 = c.evaluate(n, noise=named, minibatch=mb, want_fvalues=True)
    assert torch.equal(res2["f"], res3["f"]) and all(np.array_equal(g2[k], v) for k, v in c.named_grads().items())


@pytest.mark.parametrize("estimator", ["pathwise", "blackbox"])
def test_the_three_sites_agree_on_64_9_1(estimator, monkeypatch):
    """the bounds of test_gpu_bnn_normal.test_the_three_likelihood_sites_agree, sigma's gradient among the gradients"""
    def outputs(middle):
        c = compile_bnn(A, estimator)
        assert c.middle_path() == middle
        res = c.evaluate(70, seed=9, offset=2, want_fvalues=True)
        return float(res["loss"]), res["f"].cpu().numpy().astype(np.float64), res["grads"].cpu().numpy().astype(np.float64), c.named_grads()["y_scale"]

    gen = outputs("mid_gen")
    monkeypatch.setenv("BSVI_BNN_MID", "0")
    upper_gen = outputs("upper_gen")
    monkeypatch.setenv("BSVI_BNN_JIT", "0")
    generic = outputs("upper_lds")
    fscale, gscale = np.abs(generic[1]).max(), max(np.abs(generic[2]).max(), 1e-6)
    bb = estimator == "blackbox"
    for other in (gen, upper_gen):
        print(abs(other[0] - generic[0]) / abs(generic[0]), np.abs(other[1] - generic[1]).max() / fscale, np.abs(other[2] - generic[2]).max() / gscale,
              other[3], generic[3])
        assert abs(other[0] - generic[0]) <= (2e-4 if bb else 2e-6) * abs(generic[0])
        assert np.abs(other[1] - generic[1]).max() <= 2e-6 * fscale
        assert np.abs(other[2] - generic[2]).max() <= (2e-4 if bb else 5e-6) * gscale


def test_one_root_as_a_prior_scale_and_as_sigma_takes_both_contributions():
    """exp(log_s) is the prior scale of weights2 AND sigma: the entry's rows and the likelihood add up (an overwrite of either fails)"""
    kw = lambda: sigma_model("shared")
    n = 70
    c = compile_bnn(kw)
    res = c.evaluate(n, seed=4, offset=1, want_noise=True, want_indices=True, want_fvalues=True)
    idx = res["indices"].cpu().numpy()
    named, mb = c.named_noise(res["noise"].cpu().numpy(), n), {c.program.indices_name: idx.tolist()}
    exact, ref32 = oracle_pair(kw, n, "pathwise", named, mb)
    check_against(c, res, exact, ref32, idx, "shared root")
    # ... and neither part alone is the answer: the likelihood's share, from the summands' own formula, is far above the bound
    p = c.program
    name, S = summands(p, exact["samples"], idx)
    sig, dsig, _ = sigma_entries(p)
    lik_part = float(S) - 2.0 * p.batch_size * p.n_classes / sig[0] * dsig[0]        # mean_n sum (u^2 - 1) / sigma dsigma, from S
    g64 = float(exact["grads"][name].reshape(-1)[0])
    assert abs(lik_part) > 1e-2 * abs(g64) and abs(-g64 - lik_part) > 1e-2 * abs(g64), (lik_part, g64)


def test_sums_are_linear_over_sample_shards_with_a_base():
    """64-9-1 over 70 samples: the output block of the whole equals the sum of the blocks of samples 0..32 and 33..69 (the bounds of
    test_gpu_bnn_normal.test_sums_are_linear_over_sample_shards); sigma's entry among them"""
    from brancher_amd.native import OUT_HEADER
    for kw in (A, B):
        c = compile_bnn(kw)
        n = 70
        blocks = []
        for base, n_local in ((0, n), (0, 33), (33, 37)):
            args = c._args(n_local, n, base, seed=21, offset=4)
            native.check(c.lib.bsvi_bnn_fwd_bwd(c.handle, C.byref(args)))
            blocks.append(c.out.detach().cpu().numpy().copy())
            native.check(c.lib.bsvi_bnn_fwd_bwd(c.handle, C.byref(args)))
            assert np.array_equal(blocks[-1], c.out.detach().cpu().numpy())
        whole, a, b = blocks
        assert np.isfinite(whole).all() and whole[1] == 0.0
        scale = np.abs(whole[OUT_HEADER:]).max()
        assert scale > 0 and np.abs(a[OUT_HEADER:] + b[OUT_HEADER:] - whole[OUT_HEADER:]).max() <= 2e-5 * scale
        (par, off, size, _), = [t for t in c.program.parameters if t[0].name in ("y_scale", "y_log_scale")]
        sl = slice(OUT_HEADER + off, OUT_HEADER + off + size)
        assert np.abs(whole[sl]).min() > 0 and np.abs(a[sl] + b[sl] - whole[sl]).max() <= 2e-5 * np.abs(whole[sl]).max()
        assert abs(a[0] + b[0] - whole[0]) <= 2e-6 * (abs(whole[0]) + n * c.program.n_rows)


def weighted_pass(c, fn, n, named, mb):
    """the two passes of engine.custom_estimator_loss on THIS engine (the public function compiles through `compile_model`, which keeps a
    small model on the scalar path): f and log q per sample, the estimator's weights by autograd, the weighted launches"""
    first = c.evaluate(n, seed=5, offset=0, noise=named, minibatch=mb, want_fvalues=True)
    F, LQ = first["f"].detach().clone().reshape(-1, 1).requires_grad_(True), first["lq"].detach().clone().reshape(-1, 1).requires_grad_(True)
    value = fn(F, LQ)
    value.backward()
    a, b = F.grad, LQ.grad if LQ.grad is not None else torch.zeros_like(LQ)
    c.evaluate_weighted(n, a, b, 5, 0, noise=named, minibatch=mb)
    return -float(value.detach().cpu()), c.named_grads(), a.detach().cpu().numpy().reshape(-1)


@pytest.mark.parametrize("site", ["mid_gen 64-9-1", "upper_gen 36-5-4-3"])
def test_caller_weights_that_differ_per_sample(site):
    """`evaluate_weighted` under a softmax of f: a_n scales sigma's terms with the likelihood's seeds (q_weight plays no part)"""
    kw, n, middle, path, env = SITES[site]
    c = compile_bnn(kw, "blackbox")
    assert c.middle_path() == middle
    res = c.evaluate(n, seed=8, offset=3, want_noise=True, want_indices=True)
    idx = res["indices"].cpu().numpy()
    named, mb = c.named_noise(res["noise"].cpu().numpy(), n), {c.program.indices_name: idx.tolist()}
    exact, ref32 = oracle_pair(kw, n, SOFTMAX, named, mb)
    loss, grads, a = weighted_pass(c, SOFTMAX, n, named, mb)
    assert np.ptp(a) > 0.1 * np.abs(a).max()                      # the weights do differ
    assert abs(loss - exact["loss"]) <= max(4 * abs(ref32["loss"] - exact["loss"]), TOL * abs(exact["loss"])), (loss, ref32["loss"], exact["loss"])
    sigma_grad_check(c.program, grads, exact, ref32["grads"], idx, site + " softmax weights", weights=a)


def test_taylor1_runs_the_same_launches_on_zero_noise():
    n = 70
    c = compile_bnn(A, "taylor1")
    res = c.evaluate(n, seed=3, offset=5, want_noise=True, want_indices=True)
    idx = res["indices"].cpu().numpy()
    named, mb = c.named_noise(res["noise"].cpu().numpy(), n), {c.program.indices_name: idx.tolist()}
    exact, ref32 = oracle_pair(A, n, "taylor1", named, mb)
    loss = float(res["loss"].item())
    assert abs(loss - exact["loss"]) <= max(4 * abs(ref32["loss"] - exact["loss"]), TOL * abs(exact["loss"])), (loss, ref32["loss"], exact["loss"])
    # (f at the posterior's means: the oracle's samples are the draws, the summands are taken at the means the kernels evaluate)
    loc, _ = bnn.row_parameters(c.program)
    means = {t["name"]: np.broadcast_to(loc[t["row0"]:t["row0"] + t["size"]], (n, t["size"])) for t in c.program.tensors}
    sigma_grad_check(c.program, c.named_grads(), dict(exact, samples=means), ref32["grads"], idx, "taylor1 64-9-1")


@pytest.mark.parametrize("name", FIXTURES)
def test_the_reference_fixtures(name):
    """loss, per-sample terms, every gradient under the five estimator records and the Adam trajectory of the real reference: the
    double-precision oracle is the truth, the fixture the yardstick (tests/test_gpu_bnn_normal.py: test_the_reference_fixtures)"""
    g = Golden(name)
    idx = g.minibatch["indices"]
    f_ref = (g.data["lp"] + g.data["H"]).reshape(-1)
    for estimator in ("pathwise", "blackbox"):
        c = compile_bnn(g.build, estimator)
        res = c.evaluate(g.N, noise=g.noise, minibatch=g.minibatch, want_fvalues=True)
        exact = Oracle(g.build(), dtype=torch.float64).loss_and_grads(g.N, estimator, g.noise, g.minibatch)
        fixture = dict(f=f_ref, loss=float(g.data["loss_" + estimator]), grads=g.group("grad_%s/" % estimator))
        check_against(c, res, exact, fixture, idx, "%s %s" % (name[-14:], estimator))
        if estimator == "blackbox":
            lq64 = exact["lq"].reshape(-1)
            assert np.abs(res["lq"].cpu().numpy() - lq64).max() <= max(4 * np.abs(g.data["lq"].reshape(-1) - lq64).max(), TOL * np.abs(lq64).max())
    c = compile_bnn(g.build, "taylor1")
    exact = Oracle(g.build(), dtype=torch.float64).loss_and_grads(g.N, "taylor1", g.noise, g.minibatch)
    res = c.evaluate(g.N, noise=g.noise, minibatch=g.minibatch)
    loss, ref = float(res["loss"].item()), float(g.data["loss_taylor1"])
    assert abs(loss - exact["loss"]) <= max(4 * abs(ref - exact["loss"]), TOL * abs(exact["loss"])), (loss, ref, exact["loss"])
    loc, _ = bnn.row_parameters(c.program)
    means = {t["name"]: np.broadcast_to(loc[t["row0"]:t["row0"] + t["size"]], (g.N, t["size"])) for t in c.program.tensors}
    sigma_grad_check(c.program, c.named_grads(), dict(exact, samples=means), g.group("grad_taylor1/"), idx, name[-14:] + " taylor1")
    # the two user-defined estimators: caller weights (the softmax record's differ per sample)
    fns = {"baseline": lambda f, lq: (lq * (f - f.mean()).detach() + f).mean(), "softmax": SOFTMAX}
    for which, fn in fns.items():
        c = compile_bnn(g.build, "blackbox")
        exact = Oracle(g.build(), dtype=torch.float64).loss_and_grads(g.N, fn, g.noise, g.minibatch)
        loss, grads, a = weighted_pass(c, fn, g.N, g.noise, g.minibatch)
        ref = float(g.data["loss_custom_" + which])
        assert abs(loss - exact["loss"]) <= max(4 * abs(ref - exact["loss"]), TOL * abs(exact["loss"])), (which, loss, ref, exact["loss"])
        sigma_grad_check(c.program, grads, exact, g.group("grad_custom_%s/" % which), idx, "%s custom %s" % (name[-14:], which), weights=a)
    # the trajectory under Adam: y_scale stays on iteration 0 and moves afterwards
    tr = g.meta["trajectory"]
    c = compile_bnn(g.build)
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
    params = c.named_params()
    assert "y_scale" in params and np.abs(params["y_scale"].reshape(-1) - g.data["param/y_scale"].reshape(-1)).min() > 1e-3
    for pname, p in params.items():
        e64 = exact_after[pname].reshape(p.shape)
        assert np.abs(p - e64).max() <= max(4 * np.abs(after[pname].reshape(p.shape) - e64).max(), 2e-5 * (1 + np.abs(e64).max())), pname


def replayed_sequences(kw, n, iters, seed):
    """the draws and minibatches of a training call that started at iteration 0 under `seed`: they depend on (seed, offset) alone"""
    c = compile_bnn(kw)
    noise_seq, mb_seq = [], []
    for it in range(iters):
        res = c.evaluate(n, seed=seed, offset=it, want_noise=True, want_indices=True)
        noise_seq.append(c.named_noise(res["noise"].cpu().numpy(), n))
        mb_seq.append({c.program.indices_name: res["indices"].cpu().numpy().tolist()})
    return noise_seq, mb_seq


def test_six_adam_steps_through_perform_inference_follow_the_oracle():
    """pretraining_iterations = 0: the posterior's group is stepped from iteration 0, the joint model's — sigma — from iteration 1
    (inference.py:99-104); against Oracle.train on the same noise and minibatch sequences"""
    n, iters, lr = 40, 6, 1e-2
    torch.manual_seed(1234)
    seed = int(torch.initial_seed()) & 0x7FFFFFFFFFFFFFFF
    start = float(np.asarray(next(v for v in build(A).flatten() if v.name == "y_scale").parameter.numpy()).reshape(-1)[0])
    # one iteration: sigma is where it was, the posterior has moved
    model, method = build(A), inference.ReverseKL()
    before = {v.name: np.array(v.parameter.numpy(), copy=True) for v in model.posterior_model.flatten() if getattr(v, "learnable", False)}
    inference.perform_inference(model, number_iterations=1, number_samples=n, optimizer="Adam", lr=lr, pretraining_iterations=0,
                                inference_method=method)
    c = method.last_compiled
    assert type(c).__name__ == "CompiledBnn" and c.last_mode == "stepwise"
    params = c.named_params()
    assert float(params["y_scale"].reshape(-1)[0]) == np.float32(start)
    assert all(np.abs(params[k].reshape(-1) - v.reshape(-1)).max() > 0 for k, v in before.items())
    # six iterations
    model, method = build(A), inference.ReverseKL()
    inference.perform_inference(model, number_iterations=iters, number_samples=n, optimizer="Adam", lr=lr, pretraining_iterations=0,
                                inference_method=method)
    c = method.last_compiled
    got = np.asarray(model.diagnostics["loss curve"], dtype=np.float64)
    noise_seq, mb_seq = replayed_sequences(A, n, iters, seed)
    o64, o32 = Oracle(build(A), dtype=torch.float64), Oracle(build(A))
    exact_losses = o64.train(iters, n, "Adam", noise_seq=noise_seq, minibatch_seq=mb_seq, pretraining_iterations=0, lr=lr).astype(np.float64)
    ref_losses = o32.train(iters, n, "Adam", noise_seq=noise_seq, minibatch_seq=mb_seq, pretraining_iterations=0, lr=lr).astype(np.float64)
    print("losses", got, exact_losses, ref_losses)
    assert np.abs(got - exact_losses).max() <= max(4 * np.abs(ref_losses - exact_losses).max(), TOL * np.abs(exact_losses).max())
    params = c.named_params()
    e64 = {k: t.detach().numpy() for k, t in o64.named_parameters().items()}
    e32 = {k: t.detach().numpy() for k, t in o32.named_parameters().items()}
    for pname, p in params.items():
        x = e64[pname].reshape(p.shape)
        assert np.abs(p - x).max() <= max(4 * np.abs(e32[pname].reshape(p.shape) - x).max(), 2e-5 * (1 + np.abs(x).max())), pname
    moved = float(params["y_scale"].reshape(-1)[0]) - start
    assert abs(moved) > 0.5 * (iters - 1) * lr * 0.5, moved          # five Adam steps of ~lr each, all one way at the start


def test_a_reference_style_loop_with_two_optimizers_steps_sigma_from_iteration_one():
    """a user-defined gradient estimator keeps the loop of inference.py:95-108 on the host: one ProbabilisticOptimizer per model, the
    joint model's (sigma) updated when iteration > pretraining_iterations"""
    from brancher_amd import gradient_estimators as ge
    method = lambda: inference.ReverseKL(gradient_estimator=W.custom_estimators(ge)["baseline"])
    start = None
    for iters in (1, 4):
        model = build(A)
        start = float(np.asarray(next(v for v in model.flatten() if v.name == "y_scale").parameter.numpy()).reshape(-1)[0])
        inference.perform_inference(model, number_iterations=iters, number_samples=40, optimizer="Adam", lr=1e-2, inference_method=method())
        curve = np.asarray(model.diagnostics["loss curve"])
        now = float(np.asarray(next(v for v in model.flatten() if v.name == "y_scale").parameter.numpy()).reshape(-1)[0])
        assert len(curve) == iters and np.isfinite(curve).all()
        assert (now == start) if iters == 1 else abs(now - start) > 1e-2, (iters, start, now)


def test_predict_follows_the_trained_sigma():
    """var - Var_n(loc) is the CURRENT sigma^2 per output (to 1e-6), and the likelihood's draws scatter by it"""
    c = compile_bnn(B)
    n = 256
    rows = c.program.dataset[:5]
    for step in range(2):
        theta = c.named_params()
        sig, _, name = sigma_entries(c.program, theta)
        res = c.predict(rows, n, seed=2, offset=step, want_outputs=True, want_draws=True)
        loc = res["outputs"].cpu().numpy().astype(np.float64)                       # [N, M, C]
        var = res["var"].cpu().numpy().astype(np.float64)
        got = var - loc.var(axis=0)
        print("sigma", sig, "var - Var_n(loc)", got)
        assert np.abs(got / sig ** 2 - 1.0).max() <= 1e-6
        z = (res["draws"].cpu().numpy().astype(np.float64) - loc) / sig
        count = z.shape[0] * z.shape[1]
        assert np.abs(z.std(axis=(0, 1)) - 1.0).max() <= 5.0 / np.sqrt(2.0 * count)
        if step == 0:
            before = sig.copy()
            losses, finite = c.train(30, 64, "Adam", seed=3, lr=3e-2)
            assert finite.cpu().numpy().all()
    assert np.abs(sig - before).min() > 0.05                  # training did move every sigma


def test_the_public_route_serves_the_model():
    """`engine.compile_model` on the reference's idiom: before this feature the lowering refused it ("is learnable") and every engine
    with it — LoweringError.  The test of the suite that fails without the feature."""
    try:
        c = engine.compile_model(build(A), None, "pathwise")
    except LoweringError as err:
        pytest.fail("the public route refuses a learnable sigma: %s" % err)
    assert type(c).__name__ == "CompiledBnn" and c.program.scale_learnable and c.program.summary()["scale"] == "learnable"
    assert c.middle_path() == "mid_gen"
    # a constant sigma and a classifier next to it: the entry points they had
    k = engine.compile_model(W.build_bnn_regression(W.native_api(), **{k: v for k, v in A.items() if k not in LEARN}), None, "pathwise")
    assert type(k).__name__ == "CompiledBnn" and not k.program.scale_learnable
    assert k.lib.bsvi_bnn_workspace_bytes(k.handle, 70) < c.lib.bsvi_bnn_workspace_bytes(c.handle, 70)
    first = k.evaluate(70, seed=3, offset=5)["loss"].clone()
    assert torch.isfinite(first) and torch.equal(first, k.evaluate(70, seed=3, offset=5)["loss"])
