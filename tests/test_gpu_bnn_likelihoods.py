"""Laplace and Cauchy regression likelihoods of the Bayesian-neural-network family on the device (bsvi_bnn_set_likelihood_family;
DESIGN.md 4.7): per (row, sample, output) with u = (y - z) / sigma the value -|u| - log(2 sigma) | -log(1 + u^2) - log(pi sigma), the seed
d f / d z = wgt psi(u) / sigma and d f / d sigma = wgt (u psi(u) - 1) / sigma (psi = sign(u) | 2 u / (1 + u^2)) at every site that holds a
likelihood (bnn_mid_gen with one row and with pairs of rows per thread, its one-layer case, bnn_upper_gen, the static bnn_upper with its
activations in LDS and in memory) under a constant scale, a learnable one and a scale head; training; the predictive pass.
Every check is against `Oracle(..., dtype=float64)` on the draws and indices the kernels report, the single-precision oracle (or a fixture
of the real reference) the yardstick: conftest.yardstick_grad_check for every tensor, tests/test_gpu_bnn_sigma.py's rule for f and the
loss, and for sigma's root and the scale head's parameters that file's bound with the floor generalised to the families,
    err <= max(4 |oracle32 - oracle64|, 1e-5 max |oracle64|, 1e-6 S),   S = mean_n sum_b (|u psi(u)| + 1) / sigma_c |d sigma_c / d theta|.
A CONDITION, not a tolerance, is asserted before every Laplace comparison: no residual of the double-precision forward pass lies within
1e-5 max(1, |y|, |z|) of zero — there sign(u) differs between single and double precision and neither is wrong.  Each case's (seed,
offset) was chosen on the host (oracle/philox_ref.dense_noise / minibatch_index and the chain in double precision) so that it holds."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import Golden, yardstick_grad_check
from brancher_amd import bnn, distributions as D, engine, inference, native, workloads as W
from brancher_amd.lowering import LoweringError
from oracle import philox_ref as R
from oracle.svi_oracle import Oracle
from test_bnn_sigma_cpu import sigma_entries
from test_gpu_bnn_heads import forward as heads_forward
from test_gpu_bnn_predict import NORMAL_TOL, host_words
from test_gpu_bnn_sigma import NP_ACT, SOFTMAX, weighted_pass

pytestmark = pytest.mark.gpu
TOL = 1e-5
FAMILIES = {"laplace": D.DIST_LAPLACE, "cauchy": D.DIST_CAUCHY}
LEARN = dict(learnable_sigma=True, sigma=0.3, sigma_init=0.5)
A = dict(dataset_size=40, batch_size=17, n_features=64, n_hidden=9, n_outputs=1, **LEARN)                               # 64-9-1, tanh
ONE_LAYER = dict(dataset_size=24, batch_size=8, n_features=32, n_hidden=0, n_outputs=2, bias=False, **LEARN)            # 32-2: Rs = 0
PAIRS = dict(dataset_size=520, batch_size=512, n_features=16, n_hidden=4, n_outputs=2, **LEARN)                         # 16-4-2, B_pad 512
B = dict(dataset_size=40, batch_size=33, n_features=36, n_hidden=5, hidden2=4, n_outputs=3, activation="relu", data="normal",
         sigma=[0.3, 0.5, 0.8], learnable_sigma="exp", sigma_init=[0.5, 0.5, 0.5])                                      # 36-5-4-3, relu
MEM = dict(widths=[32, 18, 18, 3], batch_size=33, dataset_size=40, data="normal", q_scale=0.3, sigma=[0.3, 0.5, 0.8],
           learnable_sigma=True, sigma_init=[0.5, 0.5, 0.5])                                                            # 32-18-18-3
CONSTANT = lambda kw: {k: v for k, v in kw.items() if k not in ("learnable_sigma", "sigma_init")}
HEAD = lambda kw, g, floor: dict({k: v for k, v in kw.items() if k not in ("learnable_sigma", "sigma_init", "sigma")}, scale_head=g, scale_floor=floor)
FIXTURES = ["bnn_lik/bnn_lik_laplace_tanh_P32_H6_C1_DS30_B12_N5", "bnn_lik/bnn_lik_cauchy_linear_P16_C2_DS24_B10_N6"]
SITES = {
    # id: (builder keywords, N, middle kernel, data path, environment)
    "mid_gen 64-9-1": (A, 70, "mid_gen", "bf16x3", {}),
    "mid_gen 32-2 Rs=0": (ONE_LAYER, 65, "mid_gen", "bf16x3", {}),
    "mid_gen 16-4-2 pairs": (PAIRS, 3, "mid_gen", "bf16x3", {}),
    "upper_gen 36-5-4-3": (B, 130, "upper_gen", "f32", {}),
    "upper_lds 36-5-4-3": (B, 130, "upper_lds", "f32", {"BSVI_BNN_JIT": "0"}),
    "upper_mem 32-18-18-3": (MEM, 70, "upper_mem", "f32", {}),
}
# the (seed, offset) of every evaluation of a Laplace model, by the label of the case: chosen on the host so that the condition above
# holds with a margin of ten (a Cauchy case takes the default: it has no condition)
DRAWS = {"upper_mem 32-18-18-3 laplace": (8, 3), "constant upper_mem 32-18-18-3 laplace": (8, 3)}
DEFAULT_DRAW = (3, 5)
WORST = {}


def draw_of(label):
    return DRAWS.get(label, DEFAULT_DRAW)


def build(kw):
    return kw() if callable(kw) else W.build_bnn_regression(W.native_api(), **kw)


def compile_bnn(kw, estimator="pathwise", family=None):
    model = build(kw)
    c = bnn.CompiledBnn(model, model.posterior_model, estimator)
    assert c.program.likelihood == bnn.LIK_NORMAL and (family is None or c.program.family == FAMILIES[family])
    return c


def upsi(family, u):
    """|u psi(u)| of the family: |u| (Laplace), 2 u^2 / (1 + u^2) (Cauchy), u^2 (Normal)"""
    return {D.DIST_LAPLACE: np.abs(u), D.DIST_CAUCHY: 2.0 * u * u / (1.0 + u * u), D.DIST_NORMAL: u * u}[family]


def chain(p, samples, idx):
    """the chain forward in double precision on the weights the ORACLE drew -> z [N, B, rows of the last layer]"""
    n = next(iter(samples.values())).shape[0]
    by = {t["name"]: t for t in p.tensors}
    tensor = lambda name: np.asarray(samples[name], dtype=np.float64).reshape(n, by[name]["rows"], by[name]["cols"])
    if p.scale_head:
        return heads_forward(p, tensor, p.dataset[np.asarray(idx)], np.float64)
    h = np.broadcast_to(p.dataset[np.asarray(idx)].astype(np.float64), (n, len(idx), p.n_features))
    for l in p.layers:
        h = np.einsum("nij,nbj->nbi", tensor(l["weights"]), h)
        if l["bias"] is not None:
            h = h + np.asarray(samples[l["bias"]], dtype=np.float64).reshape(n, 1, l["rows"])
        h = NP_ACT[l["activation"]](h)
    return None, h, None, None


def residual_margin(p, samples, idx):
    """min over (sample, row, output) of |y - z| / max(1, |y|, |z|), the forward pass in double precision"""
    _, z, _, _ = chain(p, samples, idx)
    y = p.labels[np.asarray(idx)].astype(np.float64)[None]
    return float((np.abs(y - z) / np.maximum(1.0, np.maximum(np.abs(y), np.abs(z)))).min())


def laplace_condition(p, samples, idx, label):
    if p.family != D.DIST_LAPLACE:
        return
    m = residual_margin(p, samples, idx)
    print("%-40s smallest residual / max(1, |y|, |z|) %.3g" % (label, m))
    assert m > 1e-5, "%s: a residual within 1e-5 of zero (choose another (seed, offset) for this case)" % label


def summands(p, samples, idx, weights=None, theta=None):
    """S per element of sigma's root: sum_n |w_n| sum_b (|u psi(u)| + 1) / sigma_c |d sigma_c / d theta| (tests/test_gpu_bnn_sigma.py:
    summands, with the family's u psi(u) in the place of u^2)"""
    _, z, _, _ = chain(p, samples, idx)
    n = z.shape[0]
    sig, dsig, name = sigma_entries(p, theta)
    u = (p.labels[np.asarray(idx)].astype(np.float64)[None] - z) / sig
    per = ((upsi(p.family, u) + 1.0) / sig * np.abs(dsig)).sum(axis=1)                           # [N, C]
    w = np.full(n, 1.0 / n) if weights is None else np.abs(np.asarray(weights, dtype=np.float64).reshape(-1))
    s = (w[:, None] * per).sum(axis=0)
    return name, (s if p.scale_stride else s.sum())


def head_summands(p, samples, noise, idx, weights=None):
    """S per element of the scale head's parameters (tests/test_gpu_bnn_heads.py: head_summands, with the family's u psi(u))"""
    x, loc, sigma, dsigma = chain(p, samples, idx)
    n = loc.shape[0]
    by = {t["name"]: t for t in p.tensors}
    u = (p.labels[np.asarray(idx)].astype(np.float64)[None] - loc) / sigma
    t = (upsi(p.family, u) + 1.0) / sigma * dsigma
    w = np.full(n, 1.0 / n) if weights is None else np.abs(np.asarray(weights, dtype=np.float64).reshape(-1))
    theta = np.zeros(max(p.n_params, 1))
    for par, off, size, _ in p.parameters:
        theta[off:off + size] = par.numpy().reshape(-1)
    h = 1e-4
    ds = (bnn.row_parameters(p, theta + h)[1] - bnn.row_parameters(p, theta - h)[1]) / (2 * h)
    last, out = p.layers[-1], {}
    for name, per in ((last["weights_scale"], np.einsum("nbc,nbj->ncj", t, np.abs(x))), (last["bias_scale"], t.sum(axis=1)[:, :, None])):
        if name is None:
            continue
        per = per.reshape(n, -1)
        eps = np.abs(np.asarray(noise[name], dtype=np.float64).reshape(n, -1))
        out[name + "_loc"] = (w[:, None] * per).sum(axis=0)
        out[name + "_scale"] = (w[:, None] * per * eps).sum(axis=0) * np.abs(ds[by[name]["row0"]:by[name]["row0"] + by[name]["size"]])
    return out


def scale_grad_check(p, grads, exact, yard_grads, idx, label, weights=None, samples=None, noise=None):
    """every tensor by the suite's yardstick; sigma's root (or the scale head's parameters) by test_gpu_bnn_sigma.sigma_grad_check's
    bound with the generalised floor; prints err / bound before it asserts"""
    samples = exact["samples"] if samples is None else samples
    if p.scale_head:
        S = head_summands(p, samples, noise, idx, weights)
    elif p.scale_learnable:
        name, s = summands(p, samples, idx, weights)
        S = {name: np.asarray(s).reshape(-1)}
    else:
        S = {}
    worst = 0.0
    for name, s in S.items():
        g64 = exact["grads"][name].reshape(-1)
        err = np.abs(grads[name].reshape(-1) - g64)
        bound = np.maximum(np.maximum(4 * np.abs(np.asarray(yard_grads[name]).reshape(-1) - g64), TOL * np.abs(g64).max()), 1e-6 * s)
        ratio = float((err / bound).max())
        worst = max(worst, ratio)
        print("%-40s %-20s max|g64| %.3g err %.3g bound %.3g err/bound %.3g" % (label, name, np.abs(g64).max(), err.max(), bound.max(), ratio))
        # (as the sibling files: a case whose gradient is all cancellation cannot pass for that reason)
        assert (np.abs(g64).max() if p.scale_head else np.abs(g64).min()) > 10 * bound.max(), "the case's gradient of %s is all cancellation" % name
        assert (err <= bound).all(), (label, name, err, bound)
    WORST[label] = worst
    yardstick_grad_check(grads, exact["grads"], yard_grads)


def check_against(c, res, exact, yard, idx, label, noise=None):
    """loss and per-sample f as tests/test_gpu_bnn_sigma.py checks them (its 1e-6 floor of the summands), then the gradients"""
    f64 = exact["f"].reshape(-1)
    floor = 1e-6 * (float(np.abs(f64).max()) + 0.5 * c.program.n_rows * 3.0)
    f_err, f_yard = np.abs(res["f"].cpu().numpy() - f64).max(), np.abs(np.asarray(yard["f"]).reshape(-1) - f64).max()
    loss = float(res["loss"].item())
    print(label, "f err %.3g yard %.3g floor %.3g | loss %.9g exact %.9g yard %.9g" % (f_err, f_yard, floor, loss, exact["loss"], yard["loss"]))
    assert float(res["finite"].item()) == 1.0 and f_err <= max(4 * f_yard, floor)
    assert abs(loss - exact["loss"]) <= max(4 * abs(yard["loss"] - exact["loss"]), TOL * abs(exact["loss"]), floor), (loss, exact["loss"], yard["loss"])
    scale_grad_check(c.program, c.named_grads(), exact, yard["grads"], idx, label, noise=noise)


def oracle_pair(kw, n, estimator, named, mb):
    return (Oracle(build(kw), dtype=torch.float64).loss_and_grads(n, estimator, named, mb),
            Oracle(build(kw)).loss_and_grads(n, estimator, named, mb))


def drawn(c, res, n):
    idx = res["indices"].cpu().numpy()
    return idx, c.named_noise(res["noise"].cpu().numpy(), n), {c.program.indices_name: idx.tolist()}


def site_case(kw, n, middle, path, estimator, label, family):
    c = compile_bnn(kw, estimator, family)
    assert c.middle_path() == middle and c.data_path() == path, (c.middle_path(), c.data_path())
    seed, offset = draw_of(label)
    res = c.evaluate(n, seed=seed, offset=offset, want_noise=True, want_indices=True, want_fvalues=True)
    assert c.middle_path() == middle
    idx, named, mb = drawn(c, res, n)
    exact, ref32 = oracle_pair(kw, n, estimator, named, mb)
    laplace_condition(c.program, exact["samples"], idx, label)
    check_against(c, res, exact, ref32, idx, "%s %s" % (label, estimator), noise=named)
    if estimator == "blackbox":
        lq64 = exact["lq"].reshape(-1)
        assert np.abs(res["lq"].cpu().numpy() - lq64).max() <= max(4 * np.abs(np.asarray(ref32["lq"]).reshape(-1) - lq64).max(), TOL * np.abs(lq64).max())
    # the same draws fed back in: the noise-in path of every kernel, and bit-equal repeat calls
    res2 = c.evaluate(n, noise=named, minibatch=mb, want_fvalues=True)
    check_against(c, res2, exact, ref32, idx, "%s %s noise-in" % (label, estimator), noise=named)
    g2 = c.named_grads()
    res3 = c.evaluate(n, noise=named, minibatch=mb, want_fvalues=True)
    assert torch.equal(res2["f"], res3["f"]) and all(np.array_equal(g2[k], v) for k, v in c.named_grads().items())
    return c


@pytest.mark.parametrize("estimator", ["pathwise", "blackbox"])
@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("site", list(SITES))
def test_each_site_with_a_learnable_scale_matches_the_oracle_on_the_reported_draws(site, family, estimator, monkeypatch):
    kw, n, middle, path, env = SITES[site]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    c = site_case(dict(kw, likelihood=family), n, middle, path, estimator, "%s %s" % (site, family), family)
    assert c.program.scale_learnable
    if "pairs" in site:
        assert c.program.batch_size == 512
    if "Rs=0" in site:
        assert len(c.program.layers) == 1


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("site", ["mid_gen 64-9-1", "upper_mem 32-18-18-3"])
def test_a_constant_scale(site, family):
    kw, n, middle, path, env = SITES[site]
    c = site_case(dict(CONSTANT(kw), likelihood=family), n, middle, path, "pathwise", "constant %s %s" % (site, family), family)
    assert not c.program.scale_learnable and not c.program.scale_head


HEAD_CASES = {
    "head mid_gen 64-9-(1+1) softplus laplace": (HEAD(A, "softplus", 0.05), 70, "mid_gen", "bf16x3", "laplace"),
    "head mid_gen 64-9-(1+1) softplus cauchy": (HEAD(A, "softplus", 0.05), 70, "mid_gen", "bf16x3", "cauchy"),
    "head upper_mem 32-18-18-(3+3) softplus laplace": (HEAD(MEM, "softplus", 0.05), 70, "upper_mem", "f32", "laplace"),
    "head upper_mem 32-18-18-(3+3) softplus cauchy": (HEAD(MEM, "softplus", 0.05), 70, "upper_mem", "f32", "cauchy"),
    "head mid_gen 32-(2+2) exp laplace": (HEAD(ONE_LAYER, "exp", 0.0), 65, "mid_gen", "bf16x3", "laplace"),
    "head mid_gen 16-4-(2+2) pairs sigmoid cauchy": (HEAD(PAIRS, "sigmoid", 0.1), 3, "mid_gen", "bf16x3", "cauchy"),
}


@pytest.mark.parametrize("case", list(HEAD_CASES))
def test_a_scale_head(case):
    kw, n, middle, path, family = HEAD_CASES[case]
    c = site_case(dict(kw, likelihood=family), n, middle, path, "pathwise", case, family)
    assert c.program.scale_head and c.program.layers[-1]["rows"] == 2 * c.program.n_classes


LINEAR = {"64-9-1 laplace": (dict(A, likelihood="laplace"), "mid_gen"), "32-18-18-3 cauchy": (dict(MEM, likelihood="cauchy"), "upper_mem")}


@pytest.mark.parametrize("case", list(LINEAR))
def test_sums_are_linear_over_sample_shards_with_a_base(case):
    """over 70 samples the output block of the whole equals the sum of the blocks of samples 0..32 and 33..69 (the bounds of
    test_gpu_bnn_sigma.test_sums_are_linear_over_sample_shards_with_a_base); sigma's entry among them"""
    from brancher_amd.native import OUT_HEADER
    kw, middle = LINEAR[case]
    c = compile_bnn(kw)
    assert c.middle_path() == middle
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
    (par, off, size, _), = [t for t in c.program.parameters if t[0].name == "y_scale"]
    sl = slice(OUT_HEADER + off, OUT_HEADER + off + size)
    assert np.abs(whole[sl]).min() > 0 and np.abs(a[sl] + b[sl] - whole[sl]).max() <= 2e-5 * np.abs(whole[sl]).max()
    assert abs(a[0] + b[0] - whole[0]) <= 2e-6 * (abs(whole[0]) + n * c.program.n_rows)


@pytest.mark.parametrize("case", list(LINEAR))
def test_caller_weights_that_differ_per_sample(case):
    """`evaluate_weighted` under a softmax of f: a_n scales sigma's terms with the likelihood's seeds"""
    kw, middle = LINEAR[case]
    n, label = 70, "weights " + case
    c = compile_bnn(kw, "blackbox")
    assert c.middle_path() == middle
    seed, offset = draw_of(label)
    res = c.evaluate(n, seed=seed, offset=offset, want_noise=True, want_indices=True)
    idx, named, mb = drawn(c, res, n)
    exact, ref32 = oracle_pair(kw, n, SOFTMAX, named, mb)
    laplace_condition(c.program, exact["samples"], idx, label)
    loss, grads, a = weighted_pass(c, SOFTMAX, n, named, mb)
    assert np.ptp(a) > 0.1 * np.abs(a).max()                      # the weights do differ
    assert abs(loss - exact["loss"]) <= max(4 * abs(ref32["loss"] - exact["loss"]), TOL * abs(exact["loss"])), (loss, ref32["loss"], exact["loss"])
    scale_grad_check(c.program, grads, exact, ref32["grads"], idx, label, weights=a)


@pytest.mark.parametrize("case", list(LINEAR))
def test_taylor1_runs_the_same_launches_on_zero_noise(case):
    kw, middle = LINEAR[case]
    n, label = 70, "taylor1 " + case
    c = compile_bnn(kw, "taylor1")
    seed, offset = draw_of(label)
    res = c.evaluate(n, seed=seed, offset=offset, want_noise=True, want_indices=True)
    idx, named, mb = drawn(c, res, n)
    exact, ref32 = oracle_pair(kw, n, "taylor1", named, mb)
    loss = float(res["loss"].item())
    # (f at the posterior's means: the condition and the summands are taken at the means the kernels evaluate)
    loc, _ = bnn.row_parameters(c.program)
    means = {t["name"]: np.broadcast_to(loc[t["row0"]:t["row0"] + t["size"]], (n, t["size"])) for t in c.program.tensors}
    laplace_condition(c.program, means, idx, label)
    assert abs(loss - exact["loss"]) <= max(4 * abs(ref32["loss"] - exact["loss"]), TOL * abs(exact["loss"])), (loss, ref32["loss"], exact["loss"])
    scale_grad_check(c.program, c.named_grads(), exact, ref32["grads"], idx, label, samples=means)


@pytest.mark.parametrize("name", FIXTURES)
def test_the_reference_fixtures(name):
    """loss, per-sample terms, every gradient under the five estimator records and the Adam trajectory of the real reference: the
    double-precision oracle is the truth, the fixture the yardstick (tests/test_gpu_bnn_sigma.py: test_the_reference_fixtures)"""
    g = Golden(name)
    idx = g.minibatch["indices"]
    f_ref = (g.data["lp"] + g.data["H"]).reshape(-1)
    short = name.split("bnn_lik_")[-1][:14]
    for estimator in ("pathwise", "blackbox"):
        c = compile_bnn(g.build, estimator)
        res = c.evaluate(g.N, noise=g.noise, minibatch=g.minibatch, want_fvalues=True)
        exact = Oracle(g.build(), dtype=torch.float64).loss_and_grads(g.N, estimator, g.noise, g.minibatch)
        laplace_condition(c.program, exact["samples"], idx, "fixture " + short)
        fixture = dict(f=f_ref, loss=float(g.data["loss_" + estimator]), grads=g.group("grad_%s/" % estimator))
        check_against(c, res, exact, fixture, idx, "fixture %s %s" % (short, estimator))
        if estimator == "blackbox":
            lq64 = exact["lq"].reshape(-1)
            assert np.abs(res["lq"].cpu().numpy() - lq64).max() <= max(4 * np.abs(g.data["lq"].reshape(-1) - lq64).max(), TOL * np.abs(lq64).max())
    c = compile_bnn(g.build, "taylor1")
    exact = Oracle(g.build(), dtype=torch.float64).loss_and_grads(g.N, "taylor1", g.noise, g.minibatch)
    res = c.evaluate(g.N, noise=g.noise, minibatch=g.minibatch)
    loss, ref = float(res["loss"].item()), float(g.data["loss_taylor1"])
    loc, _ = bnn.row_parameters(c.program)
    means = {t["name"]: np.broadcast_to(loc[t["row0"]:t["row0"] + t["size"]], (g.N, t["size"])) for t in c.program.tensors}
    laplace_condition(c.program, means, idx, "fixture %s taylor1" % short)
    assert abs(loss - exact["loss"]) <= max(4 * abs(ref - exact["loss"]), TOL * abs(exact["loss"])), (loss, ref, exact["loss"])
    scale_grad_check(c.program, c.named_grads(), exact, g.group("grad_taylor1/"), idx, "fixture %s taylor1" % short, samples=means)
    # the two user-defined estimators: caller weights (the softmax record's differ per sample)
    fns = {"baseline": lambda f, lq: (lq * (f - f.mean()).detach() + f).mean(), "softmax": SOFTMAX}
    for which, fn in fns.items():
        c = compile_bnn(g.build, "blackbox")
        exact = Oracle(g.build(), dtype=torch.float64).loss_and_grads(g.N, fn, g.noise, g.minibatch)
        loss, grads, a = weighted_pass(c, fn, g.N, g.noise, g.minibatch)
        ref = float(g.data["loss_custom_" + which])
        assert abs(loss - exact["loss"]) <= max(4 * abs(ref - exact["loss"]), TOL * abs(exact["loss"])), (which, loss, ref, exact["loss"])
        scale_grad_check(c.program, grads, exact, g.group("grad_custom_%s/" % which), idx, "fixture %s custom %s" % (short, which), weights=a)
    # the trajectory under Adam
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
    for pname, p in c.named_params().items():
        e64 = exact_after[pname].reshape(p.shape)
        assert np.abs(p - e64).max() <= max(4 * np.abs(after[pname].reshape(p.shape) - e64).max(), 2e-5 * (1 + np.abs(e64).max())), pname


def test_six_adam_steps_through_perform_inference_follow_the_oracle():
    """64-9-1 with a learnable Laplace scale: against Oracle.train on the replayed noise and minibatch sequences
    (tests/test_gpu_bnn_sigma.py's rule)"""
    kw = dict(A, likelihood="laplace")
    n, iters, lr = 40, 6, 1e-2
    torch.manual_seed(1234)
    seed = int(torch.initial_seed()) & 0x7FFFFFFFFFFFFFFF
    start = float(np.asarray(next(v for v in build(kw).flatten() if v.name == "y_scale").parameter.numpy()).reshape(-1)[0])
    model, method = build(kw), inference.ReverseKL()
    inference.perform_inference(model, number_iterations=iters, number_samples=n, optimizer="Adam", lr=lr, pretraining_iterations=0,
                                inference_method=method)
    c = method.last_compiled
    assert type(c).__name__ == "CompiledBnn" and c.last_mode == "stepwise" and c.program.family == D.DIST_LAPLACE
    got = np.asarray(model.diagnostics["loss curve"], dtype=np.float64)
    r = compile_bnn(kw)
    noise_seq, mb_seq = [], []
    for it in range(iters):
        res = r.evaluate(n, seed=seed, offset=it, want_noise=True, want_indices=True)
        noise_seq.append(r.named_noise(res["noise"].cpu().numpy(), n))
        mb_seq.append({r.program.indices_name: res["indices"].cpu().numpy().tolist()})
    o64, o32 = Oracle(build(kw), dtype=torch.float64), Oracle(build(kw))
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


def family_draws(family, res, n, m, n_outputs):
    """e of every (sample, row, output) by the rule of csrc/philox.h, in single precision: word c & 3 of the call whose k1 is xor-ed
    with c >> 2, through philox_ref.laplace_noise (then the Laplace draw -sign(v) log1p(-|v|) of that base noise) / cauchy_noise"""
    out = np.zeros((n, m, n_outputs))
    for c in range(n_outputs):
        word = host_words(res, n, m, key1=c >> 2)[c & 3]
        if family == "laplace":
            v = R.laplace_noise(word, dtype=np.float32).astype(np.float64)
            out[:, :, c] = -np.sign(v) * np.log1p(-np.abs(v))
        else:
            out[:, :, c] = R.cauchy_noise(word, dtype=np.float32).astype(np.float64)
    return out


@pytest.mark.parametrize("family", list(FAMILIES))
def test_predict_on_a_trained_network(family):
    """36-5-4-3 with a scale per output after thirty Adam steps: the draws are loc + sigma e on the predictive stream's words, Laplace
    adds 2 sigma^2 to the variance of the loc, a Cauchy model has no variance; the reference's route answers like the Normal twin's"""
    kw = dict(B, likelihood=family)
    c = compile_bnn(kw, family=family)
    before, _, _ = sigma_entries(c.program, c.named_params())
    losses, finite = c.train(30, 64, "Adam", seed=3, lr=3e-2)
    assert finite.cpu().numpy().all()
    sig, _, _ = sigma_entries(c.program, c.named_params())
    assert np.abs(sig - before).min() > 0.02                  # training did move every sigma
    N, M, Cn = 256, 9, 3
    rows = c.program.dataset[:M]
    res = c.predict(rows, N, seed=0x1234567890ABC, offset=7, want_outputs=True, want_draws=True)
    loc = res["outputs"].cpu().numpy().astype(np.float64)
    e_dev = (res["draws"].cpu().numpy().astype(np.float64) - loc) / sig
    e = family_draws(family, res, N, M, Cn)
    assert e.size >= 2000
    keep = np.abs(e) <= 100.0 if family == "cauchy" else np.ones(e.shape, dtype=bool)
    worst = float(np.abs(e_dev - e)[keep].max())
    print("%s draws: |(draw - loc) / sigma - host| %.3g, bound %.3g, left out %d of %d" % (family, worst, NORMAL_TOL, (~keep).sum(), e.size))
    assert (~keep).sum() <= 0.02 * e.size and worst <= NORMAL_TOL
    if family == "laplace":
        var = res["var"].cpu().numpy().astype(np.float64)
        got = var - loc.var(axis=0)
        print("sigma", sig, "var - Var_n(loc)", got)
        assert np.abs(got / (2.0 * sig ** 2) - 1.0).max() <= 1e-6
    else:
        assert "var" not in res
        ws = torch.zeros(int(c.lib.bsvi_bnn_predict_workspace_bytes(c.handle, N, M, 0)), dtype=torch.uint8, device=c.device)
        x = torch.as_tensor(rows).to(c.device).contiguous()
        var = torch.zeros(M, Cn, device=c.device)
        ptr = lambda t: C.c_void_p(t.data_ptr())
        args = native.BnnPredictArgs(params_dev=ptr(c.params), x_dev=ptr(x), seed=1, offset=0, n_samples_local=N, sample_base=0, n_rows=M,
                                     rows_per_pass=0, var_out=ptr(var), workspace_dev=ptr(ws), stream=c._stream())
        assert c.lib.bsvi_bnn_predict(c.handle, C.byref(args)) == -2 and b"the Cauchy likelihood has no variance" in c.lib.bsvi_last_error()
        assert float(var.abs().max()) == 0.0
    # the reference's route: the key set and shapes of the Normal twin
    def route(k):
        model = build(k)
        by_name = {v.name: v for v in model.flatten()}
        sample = model._get_posterior_sample(12, input_values={by_name["x"]: torch.from_numpy(rows)})
        return {v.name: tuple(t.shape) for v, t in sample.items()}
    mine, twin = route(kw), route(B)
    assert mine == twin and mine["y"] == (12, M, Cn, 1)


def test_set_likelihood_family_checks_its_arguments():
    INVALID, UNSUPPORTED = -1, -2
    lib = native.load()
    kw = CONSTANT(A)
    c = compile_bnn(kw)
    assert c.program.family == D.DIST_NORMAL
    assert lib.bsvi_bnn_set_likelihood_family(c.handle, D.DIST_LOGNORMAL) == UNSUPPORTED and b"Normal, Laplace or Cauchy" in lib.bsvi_last_error()
    assert lib.bsvi_bnn_set_likelihood_family(c.handle, 77) == UNSUPPORTED
    assert lib.bsvi_bnn_set_likelihood_family(c.handle, D.DIST_NORMAL) == 0
    plain = compile_bnn(kw)
    a, b = c.evaluate(70, seed=3, offset=5, want_fvalues=True), plain.evaluate(70, seed=3, offset=5, want_fvalues=True)
    assert torch.equal(a["f"], b["f"]) and torch.equal(a["loss"], b["loss"]) and torch.equal(a["grads"], b["grads"])
    # after a launch
    assert lib.bsvi_bnn_set_likelihood_family(c.handle, D.DIST_LAPLACE) == INVALID and b"launched already" in lib.bsvi_last_error()
    assert lib.bsvi_bnn_set_likelihood_family(c.handle, D.DIST_NORMAL) == INVALID
    # a classifier's handle
    model = W.build_bayesian_neural_network(W.native_api(), dataset_size=40, batch_size=17, n_features=64, n_hidden=9, n_classes=3)
    k = bnn.CompiledBnn(model, model.posterior_model)
    assert lib.bsvi_bnn_set_likelihood_family(k.handle, D.DIST_LAPLACE) == INVALID and b"classifier" in lib.bsvi_last_error()
    assert lib.bsvi_bnn_set_likelihood_family(k.handle, D.DIST_NORMAL) == INVALID


def test_the_public_route_serves_the_model():
    """`engine.compile_model` on an observed Laplace over the chain: before this feature the lowering refused it ("expected one matmul
    likelihood") and every engine with it.  The test of this file that fails without the feature."""
    try:
        c = engine.compile_model(build(dict(A, likelihood="laplace")), None, "pathwise")
    except LoweringError as err:
        pytest.fail("the public route refuses an observed Laplace: %s" % err)
    assert type(c).__name__ == "CompiledBnn" and c.program.family == D.DIST_LAPLACE and c.program.summary()["family"] == "laplace"
    assert c.middle_path() == "mid_gen"
    # the Normal twin and a classifier beside it: the entry points and the workspace sizes they had
    k = engine.compile_model(build(A), None, "pathwise")
    assert type(k).__name__ == "CompiledBnn" and k.program.family == D.DIST_NORMAL and "family" not in k.program.summary()
    assert k.middle_path() == "mid_gen" and k.lib.bsvi_bnn_workspace_bytes(k.handle, 70) == c.lib.bsvi_bnn_workspace_bytes(c.handle, 70)
    const = engine.compile_model(build(CONSTANT(A)), None, "pathwise")
    assert const.lib.bsvi_bnn_workspace_bytes(const.handle, 70) < k.lib.bsvi_bnn_workspace_bytes(k.handle, 70)
    first = k.evaluate(70, seed=3, offset=5)["loss"].clone()
    assert torch.isfinite(first) and torch.equal(first, k.evaluate(70, seed=3, offset=5)["loss"])
    model = W.build_bayesian_neural_network(W.native_api(), dataset_size=40, batch_size=17, n_features=64, n_hidden=9, n_classes=3)
    z = engine.compile_model(model, None, "pathwise")
    assert z.program.likelihood == bnn.LIK_CATEGORICAL and bool(torch.isfinite(z.evaluate(70, seed=3, offset=5)["loss"]))


def test_zz_the_worst_ratios(capsys):
    """prints err / bound of every case that ran before it (tools/bnn_likelihoods_timing.py copies the line into the profile)"""
    if WORST:
        worst = sorted(WORST.items(), key=lambda kv: -kv[1])[:8]
        with capsys.disabled():
            print("\nworst err/bound of sigma's root and the scale head's parameters: " + "; ".join("%s %.3g" % kv for kv in worst))
    assert all(v <= 1.0 for v in WORST.values())
