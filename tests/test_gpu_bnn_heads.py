"""A scale head on the Normal likelihood of the Bayesian-neural-network family on the device (bsvi_bnn_create_normal_heads; DESIGN.md
4.7): y ~ Normal(loc head, a + b g(scale head)), both heads latent and on one trunk, to the library ONE last layer of 2 C rows.  The
epilogue  d[c] = wgt u / sigma,  d[C + c] = wgt (u^2 - 1) / sigma b g'(raw)  at every site that has one (bnn_mid_gen with one row and
with pairs of rows per thread, its one-layer case, bnn_upper_gen, the static bnn_upper with its activations in LDS and in memory), the
reverse sweep and the reductions behind it, training, and the predictive pass (loc, sigma, total variance, draws).  Every check is
against `Oracle(..., dtype=float64)` on the draws and indices the kernels report, the single-precision oracle the yardstick:
conftest.yardstick_grad_check for every tensor (it holds for the scale head's too: measured, the worst err / bound 0.8), and for the
four parameters of the scale head ALSO the form of tests/test_gpu_bnn_sigma.py,  err <= max(4 |oracle32 - oracle64|, 1e-5 max |oracle64|
of the tensor, 1e-6 S),  S the sum of the absolute summands (u^2 + 1) / sigma |b g'(raw)| |input| from the oracle's own draws (u^2 - 1
changes sign inside the sum over the minibatch) — the bound that  max |oracle64| > 10 max bound  is asserted against, so that a case
that is all cancellation cannot pass.  The posterior starts away from the teacher, which keeps the gradients of the scale head large.  The three transforms are
spread over the sites (softplus + 0.05, exp + 0, sigmoid + 0.1, exp + 0.05, softplus + 0.05)."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import yardstick_grad_check
from brancher_amd import bnn, engine, inference, native, workloads as W
from brancher_amd.lowering import LoweringError
from oracle import philox_ref as R
from oracle.svi_oracle import Oracle
from test_gpu_bnn_predict import NORMAL_TOL, host_words

pytestmark = pytest.mark.gpu
TOL = 1e-5
A = dict(dataset_size=40, batch_size=17, n_features=64, n_hidden=9, n_outputs=1, scale_head="softplus", scale_floor=0.05)     # 64-9-(1+1), tanh
ONE_LAYER = dict(dataset_size=24, batch_size=8, n_features=32, n_hidden=0, n_outputs=2, bias=False, scale_head="exp", scale_floor=0.0)   # 32-(2+2): Rs = 0
PAIRS = dict(dataset_size=520, batch_size=512, n_features=16, n_hidden=4, n_outputs=2, scale_head="sigmoid", scale_floor=0.1)  # B_pad 512
B = dict(dataset_size=40, batch_size=33, n_features=36, n_hidden=5, hidden2=4, n_outputs=3, activation="relu", data="normal",
         scale_head="exp", scale_floor=0.05)                                                                                   # 36-5-4-(3+3), relu
MEM = dict(widths=[32, 18, 18, 3], batch_size=33, dataset_size=40, data="normal", q_scale=0.3, scale_head="softplus")         # 32-18-18-(3+3)
SOFTMAX = lambda f, lq: (torch.softmax(0.1 * f.detach().reshape(-1), dim=0).reshape(f.shape) * f).sum()
HEAD_TENSORS = ("weights_scale", "b_scale")


def np_act(code, v):
    one = v.dtype.type(1)
    return {0: lambda: v, 1: lambda: np.tanh(v), 2: lambda: np.maximum(v, v.dtype.type(0)), 3: lambda: one / (one + np.exp(-v)),
            4: lambda: np.logaddexp(v, v.dtype.type(0))}[code]()


def np_sigma(head, raw):
    """(sigma, |d sigma / d raw|) of (transform, a, b) at `raw`, in raw's precision; the softplus with its x > 20 branch"""
    g, a, b = head
    one = raw.dtype.type(1)
    if g == "exp":
        v = np.exp(raw)
        dv = v
    elif g == "sigmoid":
        v = one / (one + np.exp(-raw))
        dv = v * (one - v)
    else:
        v = np.where(raw > 20, raw, np.log1p(np.exp(np.minimum(raw, raw.dtype.type(20)))))
        dv = np.where(raw > 20, one, one / (one + np.exp(-raw)))
    return raw.dtype.type(a) + raw.dtype.type(b) * v, np.abs(raw.dtype.type(b) * dv)


def forward(p, tensor, rows, dtype):
    """the chain on `rows` [M, P] with `tensor(name)` -> [n, rows, cols] -> (input of the heads [n, M, cols], loc [n, M, C], sigma, |d sigma|)"""
    h = None
    for l in p.layers:
        last = l is p.layers[-1]
        x = np.broadcast_to(rows.astype(dtype)[None], (tensor(l["weights"]).shape[0],) + rows.shape) if h is None else h
        names = [(l["weights"], l["bias"])] + ([(l["weights_scale"], l["bias_scale"])] if last else [])
        outs = []
        for wn, bn in names:
            z = np.einsum("nij,nmj->nmi", tensor(wn).astype(dtype), x)
            outs.append(z + tensor(bn).astype(dtype).reshape(z.shape[0], 1, -1) if bn is not None else z)
        if last:
            sigma, dsigma = np_sigma(p.scale_head, outs[1].astype(dtype))
            return x, outs[0].astype(dtype), sigma.astype(dtype), dsigma.astype(dtype)
        h = np_act(l["activation"], outs[0].astype(dtype))


def build(kw):
    return kw() if callable(kw) else W.build_bnn_regression(W.native_api(), **kw)


def compile_bnn(kw, estimator="pathwise"):
    model = build(kw)
    c = bnn.CompiledBnn(model, model.posterior_model, estimator)
    p = c.program
    assert p.likelihood == bnn.LIK_NORMAL and p.scale_head and p.summary()["scale"] == "head"
    assert p.layers[-1]["rows"] == 2 * p.n_classes == 2 * p.labels.shape[1]
    return c


def head_summands(p, samples, noise, idx, weights=None):
    """S per element of the four parameters of the scale head: sum_n |w_n| sum_b (u^2 + 1) / sigma |d sigma / d raw| |input| — times
    |eps_n| |d s / d theta| for the posterior's scales — on the weights the ORACLE drew (w_n = 1 / N unless the caller weights the samples)"""
    n = next(iter(samples.values())).shape[0]
    by = {t["name"]: t for t in p.tensors}
    tensor = lambda name: np.asarray(samples[name], dtype=np.float64).reshape(n, by[name]["rows"], by[name]["cols"])
    x, loc, sigma, dsigma = forward(p, tensor, p.dataset[np.asarray(idx)], np.float64)
    u = (p.labels[np.asarray(idx)].astype(np.float64)[None] - loc) / sigma
    t = (u * u + 1.0) / sigma * dsigma                                                           # [n, B, C]
    w = np.full(n, 1.0 / n) if weights is None else np.abs(np.asarray(weights, dtype=np.float64).reshape(-1))
    theta = np.zeros(max(p.n_params, 1))
    for par, off, size, _ in p.parameters:
        theta[off:off + size] = par.numpy().reshape(-1)
    h = 1e-4
    ds = (bnn.row_parameters(p, theta + h)[1] - bnn.row_parameters(p, theta - h)[1]) / (2 * h)    # (one parameter per row: a diagonal)
    last, out = p.layers[-1], {}
    for name, per in ((last["weights_scale"], np.einsum("nbc,nbj->ncj", t, np.abs(x))), (last["bias_scale"], t.sum(axis=1)[:, :, None])):
        if name is None:
            continue
        per = per.reshape(n, -1)
        eps = np.abs(np.asarray(noise[name], dtype=np.float64).reshape(n, -1))
        out[name + "_loc"] = (w[:, None] * per).sum(axis=0)
        out[name + "_scale"] = (w[:, None] * per * eps).sum(axis=0) * np.abs(ds[by[name]["row0"]:by[name]["row0"] + by[name]["size"]])
    return out


def head_grad_check(p, grads, exact, yard_grads, noise, idx, label, weights=None, samples=None, locs_only=False):
    """the scale head's four parameters by their own bound (err / bound printed before it asserts), then every tensor by the suite's
    yardstick.  locs_only (Taylor1: f at the means does not depend on the posterior's scales, their gradient is exactly 0 on both sides)"""
    S = head_summands(p, exact["samples"] if samples is None else samples, noise, idx, weights)
    assert sorted(S) == sorted(k for k in exact["grads"] if k.startswith(HEAD_TENSORS))
    for name, s in S.items():
        g64 = exact["grads"][name].reshape(-1)
        err = np.abs(grads[name].reshape(-1) - g64)
        yard = 4 * np.abs(np.asarray(yard_grads[name]).reshape(-1) - g64)
        bound = np.maximum(np.maximum(yard, TOL * np.abs(g64).max()), 1e-6 * s)
        print("%-30s %-22s max|g64| %.3g err %.3g bound %.3g err/bound %.3g (4 yard %.3g, 1e-6 S %.3g)"
              % (label, name, np.abs(g64).max(), err.max(), bound.max(), (err / np.maximum(bound, 1e-300)).max(), yard.max(), 1e-6 * s.max()))
        if not (locs_only and name.endswith("_scale")):
            assert np.abs(g64).max() > 10 * bound.max(), "the case's gradient of %s is all cancellation" % name
        assert (err <= bound).all(), (label, name, err.max(), bound)
    yardstick_grad_check(grads, exact["grads"], yard_grads)


def check_against(c, res, exact, yard, named, idx, label):
    """loss and per-sample f as tests/test_gpu_bnn_sigma.py checks them, then the gradients"""
    f64 = exact["f"].reshape(-1)
    floor = 1e-6 * (float(np.abs(f64).max()) + 0.5 * c.program.n_rows * 3.0)
    f_err, f_yard = np.abs(res["f"].cpu().numpy() - f64).max(), np.abs(np.asarray(yard["f"]).reshape(-1) - f64).max()
    loss = float(res["loss"].item())
    print(label, "f err %.3g yard %.3g floor %.3g | loss %.9g exact %.9g yard %.9g" % (f_err, f_yard, floor, loss, exact["loss"], yard["loss"]))
    assert float(res["finite"].item()) == 1.0 and f_err <= max(4 * f_yard, floor)
    assert abs(loss - exact["loss"]) <= max(4 * abs(yard["loss"] - exact["loss"]), TOL * abs(exact["loss"]), floor), (loss, exact["loss"], yard["loss"])
    head_grad_check(c.program, c.named_grads(), exact, yard["grads"], named, idx, label)


def oracle_pair(kw, n, estimator, named, mb):
    return (Oracle(build(kw), dtype=torch.float64).loss_and_grads(n, estimator, named, mb),
            Oracle(build(kw)).loss_and_grads(n, estimator, named, mb))


SITES = {
    # id: (builder keywords, N, middle kernel, data path, environment)
    "mid_gen 64-9-(1+1)": (A, 70, "mid_gen", "bf16x3", {}),
    "mid_gen 32-(2+2) Rs=0": (ONE_LAYER, 65, "mid_gen", "bf16x3", {}),
    "mid_gen 16-4-(2+2) pairs": (PAIRS, 3, "mid_gen", "bf16x3", {}),
    "upper_gen 36-5-4-(3+3)": (B, 130, "upper_gen", "f32", {}),
    "upper_lds 36-5-4-(3+3)": (B, 130, "upper_lds", "f32", {"BSVI_BNN_JIT": "0"}),
    "upper_mem 32-18-18-(3+3)": (MEM, 70, "upper_mem", "f32", {}),
}


def drawn(c, res, n):
    idx = res["indices"].cpu().numpy()
    return idx, c.named_noise(res["noise"].cpu().numpy(), n), {c.program.indices_name: idx.tolist()}


@pytest.mark.parametrize("estimator", ["pathwise", "blackbox"])
@pytest.mark.parametrize("site", list(SITES))
def test_each_site_matches_the_oracle_on_the_reported_draws(site, estimator, monkeypatch):
    kw, n, middle, path, env = SITES[site]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    c = compile_bnn(kw, estimator)
    assert c.middle_path() == middle and c.data_path() == path, (c.middle_path(), c.data_path())
    if "pairs" in site:
        assert c.program.batch_size == 512
    if "Rs=0" in site:
        assert len(c.program.layers) == 1 and [t["name"] for t in c.program.tensors] == ["weights1", "weights_scale"]
    res = c.evaluate(n, seed=3, offset=5, want_noise=True, want_indices=True, want_fvalues=True)
    assert c.middle_path() == middle
    idx, named, mb = drawn(c, res, n)
    exact, ref32 = oracle_pair(kw, n, estimator, named, mb)
    check_against(c, res, exact, ref32, named, idx, "%s %s" % (site, estimator))
    # the same draws fed back in: the noise-in path of every kernel, and bit-equal repeat calls
    res2 = c.evaluate(n, noise=named, minibatch=mb, want_fvalues=True)
    check_against(c, res2, exact, ref32, named, idx, "%s %s noise-in" % (site, estimator))
    g2 = c.named_grads()
    res3 = c.evaluate(n, noise=named, minibatch=mb, want_fvalues=True)
    assert torch.equal(res2["f"], res3["f"]) and all(np.array_equal(g2[k], v) for k, v in c.named_grads().items())


@pytest.mark.parametrize("estimator", ["pathwise", "blackbox"])
def test_the_three_upper_sites_agree_on_one_network(estimator, monkeypatch):
    """36-5-4-(3+3) with exact data through bnn_mid_gen, bnn_upper_gen and the static bnn_upper: each within the yardstick of the oracle
    on the same draws (so within twice that of each other), and close to each other by test_gpu_bnn_sigma's bounds"""
    kw, n = dict(B, data="integers"), 70

    def outputs(middle):
        c = compile_bnn(kw, estimator)
        assert c.middle_path() == middle
        res = c.evaluate(n, seed=9, offset=2, want_noise=True, want_indices=True, want_fvalues=True)
        return c, res, (float(res["loss"]), res["f"].cpu().numpy().astype(np.float64), res["grads"].cpu().numpy().astype(np.float64))

    c, res, gen = outputs("mid_gen")
    idx, named, mb = drawn(c, res, n)
    exact, ref32 = oracle_pair(kw, n, estimator, named, mb)
    check_against(c, res, exact, ref32, named, idx, "agree mid_gen %s" % estimator)
    monkeypatch.setenv("BSVI_BNN_MID", "0")
    c, res, upper_gen = outputs("upper_gen")
    check_against(c, res, exact, ref32, named, idx, "agree upper_gen %s" % estimator)
    monkeypatch.setenv("BSVI_BNN_JIT", "0")
    c, res, generic = outputs("upper_lds")
    check_against(c, res, exact, ref32, named, idx, "agree upper_lds %s" % estimator)
    fscale, gscale = np.abs(generic[1]).max(), max(np.abs(generic[2]).max(), 1e-6)
    bb = estimator == "blackbox"
    for other in (gen, upper_gen):
        print(abs(other[0] - generic[0]) / abs(generic[0]), np.abs(other[1] - generic[1]).max() / fscale, np.abs(other[2] - generic[2]).max() / gscale)
        assert abs(other[0] - generic[0]) <= (2e-4 if bb else 2e-6) * abs(generic[0])
        assert np.abs(other[1] - generic[1]).max() <= 2e-6 * fscale
        assert np.abs(other[2] - generic[2]).max() <= (2e-4 if bb else 5e-6) * gscale


def test_sums_are_linear_over_sample_shards_with_a_base():
    """over 70 samples the output block of the whole equals the sum of the blocks of samples 0..32 and 33..69 (the bounds of
    test_gpu_bnn_sigma.test_sums_are_linear_over_sample_shards_with_a_base); the scale head's parameters among them"""
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
        for par, off, size, _ in c.program.parameters:
            if par.name in ("weights_scale_loc", "b_scale_loc"):
                sl = slice(OUT_HEADER + off, OUT_HEADER + off + size)
                assert np.abs(whole[sl]).max() > 0 and np.abs(a[sl] + b[sl] - whole[sl]).max() <= 2e-5 * np.abs(whole[sl]).max()
        assert abs(a[0] + b[0] - whole[0]) <= 2e-6 * (abs(whole[0]) + n * c.program.n_rows)


def weighted_pass(c, fn, n, named, mb):
    """the two passes of engine.custom_estimator_loss on THIS engine (tests/test_gpu_bnn_sigma.py: weighted_pass)"""
    first = c.evaluate(n, seed=5, offset=0, noise=named, minibatch=mb, want_fvalues=True)
    F, LQ = first["f"].detach().clone().reshape(-1, 1).requires_grad_(True), first["lq"].detach().clone().reshape(-1, 1).requires_grad_(True)
    value = fn(F, LQ)
    value.backward()
    a, b = F.grad, LQ.grad if LQ.grad is not None else torch.zeros_like(LQ)
    c.evaluate_weighted(n, a, b, 5, 0, noise=named, minibatch=mb)
    return -float(value.detach().cpu()), c.named_grads(), a.detach().cpu().numpy().reshape(-1)


@pytest.mark.parametrize("site", ["mid_gen 64-9-(1+1)", "upper_gen 36-5-4-(3+3)"])
def test_caller_weights_that_differ_per_sample(site):
    """`evaluate_weighted` under a softmax of f: a_n scales both deltas of the epilogue"""
    kw, n, middle, path, env = SITES[site]
    c = compile_bnn(kw, "blackbox")
    assert c.middle_path() == middle
    res = c.evaluate(n, seed=8, offset=3, want_noise=True, want_indices=True)
    idx, named, mb = drawn(c, res, n)
    exact, ref32 = oracle_pair(kw, n, SOFTMAX, named, mb)
    loss, grads, a = weighted_pass(c, SOFTMAX, n, named, mb)
    assert np.ptp(a) > 0.1 * np.abs(a).max()                      # the weights do differ
    assert abs(loss - exact["loss"]) <= max(4 * abs(ref32["loss"] - exact["loss"]), TOL * abs(exact["loss"])), (loss, ref32["loss"], exact["loss"])
    head_grad_check(c.program, grads, exact, ref32["grads"], named, idx, site + " softmax weights", weights=a)


def test_taylor1_runs_the_same_launches_on_zero_noise():
    n = 70
    c = compile_bnn(A, "taylor1")
    res = c.evaluate(n, seed=3, offset=5, want_noise=True, want_indices=True)
    idx, named, mb = drawn(c, res, n)
    exact, ref32 = oracle_pair(A, n, "taylor1", named, mb)
    loss = float(res["loss"].item())
    assert abs(loss - exact["loss"]) <= max(4 * abs(ref32["loss"] - exact["loss"]), TOL * abs(exact["loss"])), (loss, ref32["loss"], exact["loss"])
    # (f at the posterior's means: the summands are taken at the means the kernels evaluate, the draw eps = 0)
    loc, _ = bnn.row_parameters(c.program)
    means = {t["name"]: np.broadcast_to(loc[t["row0"]:t["row0"] + t["size"]], (n, t["size"])) for t in c.program.tensors}
    zeros = {k: np.zeros_like(v) for k, v in named.items()}
    head_grad_check(c.program, c.named_grads(), exact, ref32["grads"], zeros, idx, "taylor1 64-9-(1+1)", samples=means, locs_only=True)


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
    """the public route: `perform_inference` compiles the model onto CompiledBnn and steps all twelve posterior tensors; against
    Oracle.train on the same noise and minibatch sequences (tests/test_gpu_bnn_sigma.py's rule)"""
    n, iters, lr = 40, 6, 1e-2
    torch.manual_seed(1234)
    seed = int(torch.initial_seed()) & 0x7FFFFFFFFFFFFFFF
    model, method = build(A), inference.ReverseKL()
    before = {v.name: np.array(v.parameter.numpy(), copy=True) for v in model.posterior_model.flatten() if getattr(v, "learnable", False)}
    assert {"weights_scale_loc", "weights_scale_scale", "b_scale_loc", "b_scale_scale"} <= set(before)
    inference.perform_inference(model, number_iterations=iters, number_samples=n, optimizer="Adam", lr=lr, pretraining_iterations=0,
                                inference_method=method)
    c = method.last_compiled
    assert type(c).__name__ == "CompiledBnn" and c.last_mode == "stepwise" and c.program.scale_head
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
    for k in ("weights_scale_loc", "b_scale_loc"):      # six Adam steps of ~lr each
        assert np.abs(params[k].reshape(-1) - before[k].reshape(-1)).max() > 2 * lr, k


def test_a_reference_style_loop_with_two_optimizers_steps_the_head_tensors_from_iteration_one():
    """a user-defined gradient estimator keeps the loop of inference.py:95-108 on the host: the posterior's optimizer — the four head
    tensors are the posterior's — steps at the first iteration already"""
    from brancher_amd import gradient_estimators as ge
    model = build(A)
    value = lambda name: np.array(next(v for v in model.posterior_model.flatten() if v.name == name).parameter.numpy(), copy=True)
    names = ("weights_scale_loc", "b_scale_loc", "weights2_loc", "b2_loc")
    start = {k: value(k) for k in names}
    inference.perform_inference(model, number_iterations=1, number_samples=40, optimizer="Adam", lr=1e-2,
                                inference_method=inference.ReverseKL(gradient_estimator=W.custom_estimators(ge)["baseline"]))
    curve = np.asarray(model.diagnostics["loss curve"])
    assert len(curve) == 1 and np.isfinite(curve).all()
    for k in names:
        assert np.abs(value(k) - start[k]).max() > 1e-3, k


def predict_model(n_outputs, path):
    # (global arm: the small tensors and two buffers of the widest layer beyond LDS — test_gpu_bnn_predict's "wide" with two heads)
    widths = [32, 64, n_outputs] if path == "global" else [16, 5, n_outputs]
    head = {1: ("softplus", 0.05), 3: ("exp", 0.0), 5: ("sigmoid", 0.1)}[n_outputs]
    return dict(widths=widths, batch_size=8, dataset_size=40, q_scale=0.3, scale_head=head[0], scale_floor=head[1])


@pytest.mark.parametrize("path", ["lds", "global"])
@pytest.mark.parametrize("n_outputs", [1, 3, 5])
def test_predict_returns_loc_scale_total_variance_and_draws(n_outputs, path):
    """C = 5 crosses the four-outputs-per-Philox-call boundary; 33 rows in passes of 32 and in one pass"""
    N, M = 70, 33
    c = compile_bnn(predict_model(n_outputs, path))
    p = c.program
    assert c.predict_path() == path, c.predict_path()
    rows = np.random.RandomState(3).randint(-3, 4, size=(M, p.n_features)).astype(np.float32)
    kw = dict(seed=0x1234567890ABC, offset=7, want_outputs=True, want_draws=True, want_noise=True)
    res = c.predict(rows, N, rows_per_pass=32, **kw)
    assert c.predict_path() == path and res["rows_per_pass"] == 32
    Cn = n_outputs
    assert {k: tuple(res[k].shape) for k in ("probs", "outputs", "scale", "draws", "mean", "var")} == dict(
        probs=(N, M, Cn), outputs=(N, M, Cn), scale=(N, M, Cn), draws=(N, M, Cn), mean=(M, Cn), var=(M, Cn))
    assert torch.equal(res["probs"], res["outputs"])
    noise = res["noise"].cpu().numpy()
    loc_q, scale_q = bnn.row_parameters(p, c.params.detach().cpu().numpy())
    expect = {}
    for dtype in (np.float64, np.float32):
        w = loc_q.astype(dtype)[None, :] + scale_q.astype(dtype)[None, :] * noise.T.astype(dtype)
        by = {t["name"]: t for t in p.tensors}
        tensor = lambda name: w[:, by[name]["row0"]:by[name]["row0"] + by[name]["size"]].reshape(N, by[name]["rows"], by[name]["cols"])
        _, loc, sigma, _ = forward(p, tensor, rows, dtype)
        expect[dtype] = dict(outputs=loc, scale=sigma, mean=loc.mean(axis=0), var=loc.var(axis=0) + (sigma * sigma).mean(axis=0))
    for key, e64 in expect[np.float64].items():
        got = res[key].cpu().numpy().astype(np.float64)
        err, yard, scale = np.abs(got - e64).max(), np.abs(expect[np.float32][key].astype(np.float64) - e64).max(), np.abs(e64).max()
        print("C %d %-7s %-8s err %.3g chain32 %.3g scale %.3g err/bound %.3g" % (Cn, path, key, err, yard, scale, err / max(4 * yard, TOL * scale)))
        assert err <= max(4 * yard, TOL * scale), (key, err, yard, scale)
    # "var" is the total-variance formula on the device's own loc and sigma, accumulated in double
    loc, sigma = res["outputs"].cpu().numpy().astype(np.float64), res["scale"].cpu().numpy().astype(np.float64)
    total = loc.var(axis=0) + (sigma ** 2).mean(axis=0)
    assert np.abs(res["var"].cpu().numpy() - total).max() <= 2e-7 * np.abs(total).max()
    assert sigma.min() > p.scale_head[1] and np.ptp(sigma, axis=1).min() > 0            # the scale does depend on the row
    # the draws: loc + sigma e with e from the predictive stream (tests/test_gpu_bnn_predict.py's bound for its Normal draws)
    e_dev = (res["draws"].cpu().numpy().astype(np.float64) - loc) / sigma
    worst = 0.0
    for c0 in range(0, Cn, 4):
        x = host_words(res, N, M, key1=c0 >> 2)
        e = list(R.box_muller(x[0], x[1], dtype=np.float32)) + list(R.box_muller(x[2], x[3], dtype=np.float32))
        for j in range(min(4, Cn - c0)):
            worst = max(worst, float(np.abs(e_dev[:, :, c0 + j] - e[j].astype(np.float64)).max()))
    print("draws: |(draw - loc) / scale - host box_muller32| %.3g, bound %.3g" % (worst, NORMAL_TOL))
    assert worst <= NORMAL_TOL
    # independent of rows_per_pass
    one = c.predict(rows, N, **kw)
    assert one["rows_per_pass"] == 64
    for key in ("probs", "mean", "var", "outputs", "scale", "draws", "noise"):
        assert torch.equal(one[key], res[key]), key


def test_get_posterior_sample_answers_from_the_same_pass():
    model = build(predict_model(3, "lds"))
    by_name = {v.name: v for v in model.flatten()}
    rows = np.random.RandomState(5).randint(-3, 4, size=(33, 16)).astype(np.float32)
    sample = model._get_posterior_sample(12, input_values={by_name["x"]: torch.from_numpy(rows)})
    assert tuple(sample[by_name["y"]].shape) == (12, 33, 3, 1) and bool(torch.isfinite(sample[by_name["y"]]).all())
    for name, shape in (("weights2", (3, 5)), ("weights_scale", (3, 5)), ("b2", (3, 1)), ("b_scale", (3, 1))):
        assert tuple(sample[by_name[name]].shape) == (12, 1) + shape, name


def test_a_laplace_prior_on_the_scale_head_goes_through_upper_gen():
    kw, n = dict(B, prior={"weights_scale": "laplace"}), 130
    c = compile_bnn(kw)
    assert c.middle_path() == "upper_gen" and c.program.summary()["priors"]["weights_scale"] == "laplace"
    res = c.evaluate(n, seed=6, offset=1, want_noise=True, want_indices=True, want_fvalues=True)
    idx, named, mb = drawn(c, res, n)
    exact, ref32 = oracle_pair(kw, n, "pathwise", named, mb)
    check_against(c, res, exact, ref32, named, idx, "laplace weights_scale")


def test_the_public_route_serves_the_model_and_a_constant_sigma_runs_what_it_ran():
    try:
        c = engine.compile_model(build(A), None, "pathwise")
    except LoweringError as err:
        pytest.fail("the public route refuses a scale head: %s" % err)
    assert type(c).__name__ == "CompiledBnn" and c.program.summary()["scale"] == "head" and c.middle_path() == "mid_gen"
    # the constant-sigma model of the same widths (the last layer as wide as the two heads): its entry point, its summary
    k = engine.compile_model(W.build_bnn_regression(W.native_api(), **dict({k: v for k, v in A.items() if not k.startswith("scale_")}, n_outputs=2)),
                             None, "pathwise")
    assert type(k).__name__ == "CompiledBnn" and k.program.summary()["scale"] == "constant" and not k.program.scale_head
    assert k.program.layers[-1]["rows"] == c.program.layers[-1]["rows"] == 2 and k.middle_path() == "mid_gen"
    first = k.evaluate(70, seed=3, offset=5)["loss"].clone()
    assert torch.isfinite(first) and torch.equal(first, k.evaluate(70, seed=3, offset=5)["loss"])
