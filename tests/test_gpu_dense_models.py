"""The model forms of the dense-link path (csrc/dense_kernel.inc, dense_xfused.inc, dense_select.h, dense.py) that no other test
builds, against the oracle in DOUBLE precision on the draws and the minibatch the kernels report, each on the three launch sequences
(the two fused exact-data launches; the six launches, BSVI_DENSE_FUSED=0; the f32-input kernels, BSVI_DENSE_XGEMM=0):

  A  the Bernoulli / Binomial(1) likelihood (the third arm of dense_forward, dense_ce and dense_xfwd) — the `C = 1` shapes of
     tests/test_gpu_dense_fused.py are one-class Categorical models, whose likelihood and likelihood gradient are identically 0;
  B  row parameters shared by all rows (stride 0), a uniform-table transform a + b exp(theta) and a learnable prior root (parameter
     group 1): rowg, the shared-entry sums of dense_epilogue with the BlackBox q-scale term, the refusal of dense_param_fold_kernel;
  C  the point estimate (scale 0, no entropy) on the exact-data path, over more than one tile;
  D  caller weights that differ from sample to sample (`evaluate_weighted`) against the oracle's callable estimator — a kernel that
     hands a_n to another sample stays linear in the weights, so linearity (tests/test_gpu_parity.py) cannot see it;
  E  four Adam steps of B and A through `train()` against the oracle's trajectory.

Every case first asserts the launches it is on (`launch_plan`, by name): a case that lands elsewhere FAILS.  The shapes are the smallest
that cross each rule of csrc/dense_select.h; the datasets are uint8 pixel counts, so the exact-data path serves them wherever P % 4 == 0
and P >= 32.  tests/test_dense_models_cpu.py holds the conditions under which these comparisons say something: every gradient the
likelihood reaches depends on the labels, and the bound resolves four digits of it.

The bound is the suite's yardstick (conftest.yardstick_grad_check / yardstick_loss_check, unchanged), per named tensor with the floor
taken from THAT tensor (per_tensor_check of tests/test_gpu_bnn_middle.py): err <= max(4 |oracle32 - oracle64|, 1e-5 max |oracle64|);
the loss and the per-sample values under the same rule.  Every figure is printed before it is asserted ("dense-models ..." lines);
profiles/r22/dense_models.txt holds the worst err / bound per form, sequence and estimator as measured."""
import functools

import numpy as np
import pytest
import torch

from brancher_amd import dense, engine, workloads as W
from oracle.svi_oracle import Oracle

pytestmark = pytest.mark.gpu
TOL = 1e-5

SEQUENCES = {"fused": {}, "six": {"BSVI_DENSE_FUSED": "0"}, "f32": {"BSVI_DENSE_XGEMM": "0"}}
ESTIMATORS = ["pathwise", "blackbox"]


# ---- the models --------------------------------------------------------------------------------------------------------------------
def pixel_data(ds, p, n_classes, seed=0, label_seed=0):
    """uint8 pixel counts; the labels have a seed of their own (tests/test_dense_models_cpu.py redraws them alone).  Seven labels in ten
    are the class `label_seed % n_classes`, the rest uniform: pixel counts are positive, so the class sums of x — what the draws of a
    SHARED scale meet in its gradient — move with the class proportions, and so does the likelihood under a q loc with unequal row sums.
    (With balanced labels of either seed the gradient of one scale for all rows changes by 1 to 3 %: its expectation over the draws does
    not depend on the labels at all, E[logit of the label] being linear in the weights.)"""
    X = np.random.RandomState(seed).randint(0, 256, size=(ds, p, 1)).astype(np.float32)
    rng = np.random.RandomState(1000 + label_seed)
    labels = np.where(rng.uniform(size=ds) < 0.7, label_seed % n_classes, rng.randint(0, n_classes, size=ds))
    return X, labels


def _observed(api, ds, b, X, labels):
    indices = api.RandomIndices(dataset_size=ds, batch_size=b, name="indices", is_observed=True)
    return (api.EmpiricalVariable(X, indices=indices, name="x", is_observed=True),
            api.EmpiricalVariable(labels, indices=indices, name="labels", is_observed=True))


def build_bernoulli(ds, b, p, label_seed=0):
    """A: BinomialVariable(1, logits = matmul(weights, x)) on float labels 0 / 1 (examples/minibatch_logistic_regression.py:13-43), a
    learnable loc and scale per weight: loc 0.001 randn and scale 0.002 keep the logits around +-1 on pixel counts — nothing saturates"""
    api = W.native_api()
    X, labels = pixel_data(ds, p, 2, label_seed=label_seed)
    x, y = _observed(api, ds, b, X, labels.reshape(ds, 1).astype(np.float32))
    weights = api.NormalVariable(np.zeros((1, p)), 0.5 * np.ones((1, p)), "weights")
    k = api.BinomialVariable(1, logits=api.BF.matmul(weights, x), name="k")
    model = api.ProbabilisticModel([k])
    k.observe(y)
    loc = 0.001 * np.random.RandomState(1).standard_normal((1, p))
    model.set_posterior_model(api.ProbabilisticModel([api.NormalVariable(loc, 0.002 * np.ones((1, p)), "weights", learnable=True)]))
    return model


def build_per_element(ds, b, p, c, label_seed=0):
    """the standard form (workloads.build_logistic_regression: a learnable loc and scale per weight, the prior's parameters aliased to them
    by the name-collision rule) with the small q of the other forms, for D"""
    api = W.native_api()
    X, labels = pixel_data(ds, p, c, label_seed=label_seed)
    x, y = _observed(api, ds, b, X, labels)
    weights = api.NormalVariable(np.zeros((c, p)), 10.0 * np.ones((c, p)), "weights")
    k = api.CategoricalVariable(logits=api.BF.matmul(weights, x), name="k")
    model = api.ProbabilisticModel([k])
    k.observe(y)
    loc = 0.001 * np.random.RandomState(1).standard_normal((c, p))
    model.set_posterior_model(api.ProbabilisticModel([api.NormalVariable(loc, 0.002 * np.ones((c, p)), "weights", learnable=True)]))
    return model


PRIOR_SCALE = 0.05


def build_shared(ds, b, p, c=3, learnable_prior=False, label_seed=0):
    """B: q loc a learnable root of shape (C, P); ONE q scale for all rows, 0.5 exp(log_s) + 0.001 with log_s a learnable scalar root
    (stride 0, transform exp, a = 0.001, b = 0.5); the prior's scale a constant scalar or exp(log_prior_scale), a learnable root of the
    joint model (parameter group 1).  No name collides: the prior's parameters are its own."""
    api = W.native_api()
    BF = api.BF
    X, labels = pixel_data(ds, p, c, label_seed=label_seed)
    x, y = _observed(api, ds, b, X, labels)
    prior_scale = BF.exp(api.RootVariable(np.log(PRIOR_SCALE), "log_prior_scale", learnable=True)) if learnable_prior else PRIOR_SCALE
    weights = api.NormalVariable(np.zeros((c, p)), prior_scale, "weights")
    k = api.CategoricalVariable(logits=BF.matmul(weights, x), name="k")
    model = api.ProbabilisticModel([k])
    k.observe(y)
    q_loc = api.RootVariable(0.001 * np.random.RandomState(1).standard_normal((c, p)), "q_loc", learnable=True)
    log_s = api.RootVariable(np.log(0.002), "log_s", learnable=True)
    model.set_posterior_model(api.ProbabilisticModel([api.NormalVariable(q_loc, 0.5 * BF.exp(log_s) + 0.001, "weights")]))
    return model


def build_point(ds, b, p, c=3, label_seed=0):
    """C: the posterior is one learnable RootVariable named like the weight matrix (examples/MAP_logistic_regression.py:46-56)"""
    api = W.native_api()
    X, labels = pixel_data(ds, p, c, label_seed=label_seed)
    x, y = _observed(api, ds, b, X, labels)
    weights = api.NormalVariable(np.zeros((c, p)), 10.0 * np.ones((c, p)), "weights")
    k = api.CategoricalVariable(logits=api.BF.matmul(weights, x), name="k")
    model = api.ProbabilisticModel([k])
    k.observe(y)
    init = 0.01 * np.random.RandomState(1).standard_normal((c, p))
    model.set_posterior_model(api.ProbabilisticModel([api.RootVariable(init, name="weights", learnable=True)]))
    return model


BUILDERS = dict(bernoulli=build_bernoulli, per_element=build_per_element, shared=build_shared, point=build_point)


def make(form, **kw):
    return BUILDERS[form](**kw)


# ---- the cases: (form, builder keywords, classes, samples, dense_xbwd of the fused sequence or None where the LDS rule refuses it) ---
_HEAD, _TAIL = ("dense_head", "dense_wsplit"), ("dense_epilogue", "dense_param_kernel")
_SIX = _HEAD + ("xgemm_nt<logits>", "dense_ce", "xgemm_nt<grad>", "dense_xreduce", "dense_rows") + _TAIL


def plan_names(seq, n_classes, xbwd, weighted=False):
    """the launches of a call that asks for per-sample values (or runs under BlackBox, or carries caller weights), in order: the rows of
    DENSE_PLAN_ROWS (tests/test_gpu_dense_fused.py) for the shapes shared with it — the plan does not depend on the likelihood"""
    first = ("dense_weighted_sums",) if weighted else ()
    if seq == "f32":
        forward = "dense_forward<1>" if n_classes == 1 else "dense_forward<4>"
        return first + ("dense_prologue", "dense_gather", "dense_noise", forward, "dense_backward", "dense_rows", "dense_sample_sums") + _TAIL
    if seq == "six" or xbwd is None:
        return first + _SIX
    return first + _HEAD + ("dense_xfwd<0,1,w>" if weighted else "dense_xfwd<0,1>", xbwd, "dense_rows<sliced>") + _TAIL


BERNOULLI = {
    # id: (dataset, batch, features, samples, dense_xbwd, supplied noise)
    "DS64_B32_P32_N50": (64, 32, 32, 50, "dense_xbwd<0,2,7>", False),                 # B_pad 128
    "DS256_B200_P32_N24": (256, 200, 32, 24, "dense_xbwd<0,4,9>", False),             # B_pad 256: nine-block tiles
    "DS256_B200_P32_N24-noise": (256, 200, 32, 24, "dense_xbwd<0,4,9,noise>", True),
    "DS700_B520_P64_N33": (700, 520, 64, 33, "dense_xbwd<0,2,7>", False),             # two 512-row tiles of dense_xfwd; B_pad 640: the ring of two
    "DS700_B650_P32_N20": (700, 650, 32, 20, None, False),                            # B_pad 768: six launches by the LDS rule, no knob set
}
BERNOULLI_F32 = (300, 130, 30, 20)      # P % 4 != 0: dense_forward<1> over three minibatch tiles, the last one ragged
SHARED = {
    "DS64_B40_P32_N20": (64, 40, 32, 20, "dense_xbwd<0,2,7>"),
    "DS300_B130_P100_N70": (300, 130, 100, 70, "dense_xbwd<0,4,9>"),      # R = 300: two row blocks of dense_rows, five of dense_rows<sliced>
}
POINT = (200, 200, 64, 2, "dense_xbwd<0,4,9>")       # B_pad 256
WEIGHTED = (300, 130, 100, 3, 70, "dense_xbwd<0,4,9>")


# ---- the checks --------------------------------------------------------------------------------------------------------------------
def bound_check(label, name, got, g64, g32):
    """err <= max(4 |oracle32 - oracle64|, 1e-5 max |oracle64|) over one tensor (a scalar, a vector); prints, then returns the failure"""
    got, g64, g32 = (np.asarray(v, dtype=np.float64).reshape(-1) for v in (got, g64, g32))
    err, yard, scale = np.abs(got - g64).max(), np.abs(g32 - g64).max(), np.abs(g64).max()
    bound = max(4 * yard, TOL * scale)
    print("dense-models %s %-16s err %.3g  oracle32 %.3g  scale %.3g  err/bound %.3g" % (label, name, err, yard, scale, err / bound if bound else 0.0))
    return [] if err <= bound else [(name, err, yard, scale)]


def per_tensor_check(named, exact, ref32, label=""):
    """the yardstick with each tensor's own floor; prints every figure before it asserts"""
    worst = []
    for name, g64 in exact.items():
        if g64 is None:
            continue
        worst += bound_check(label, name, named[name], g64, ref32[name])
    assert not worst, worst


_oracles = {}


def oracle_pair(form, kw, n, estimator, named, mb):
    """the two oracles on one set of draws, computed once (the exact-data sequences report the same draws) and left unchanged"""
    key = (form, tuple(sorted(kw.items())), n, estimator if isinstance(estimator, str) else id(estimator),
           tuple(mb["indices"]), tuple((k, v.tobytes()) for k, v in sorted(named.items())))
    if key not in _oracles:
        _oracles[key] = (Oracle(make(form, **kw), dtype=torch.float64).loss_and_grads(n, estimator, named, mb),
                         Oracle(make(form, **kw)).loss_and_grads(n, estimator, named, mb))
    return _oracles[key]


def compile_on(form, kw, seq, estimator, monkeypatch, exact_shape=True):
    for knob, value in SEQUENCES[seq].items():
        monkeypatch.setenv(knob, value)
    # (the path itself, not engine.compile_model: the scalar path takes a single-output Bernoulli model of up to 4096 products first)
    model = make(form, **kw)
    c = dense.CompiledDense(model, model.posterior_model, estimator)
    assert c.data_path() == ("bf16x3" if exact_shape and seq != "f32" else "f32")
    return c


def named_noise(c, eps, n):
    p = c.program
    return {p.latent_name: np.ascontiguousarray(eps.T).reshape(n, 1, p.n_classes, p.n_features)}


def run_case(form, kw, n, seq, estimator, names, monkeypatch, label, supplied=False, exact_shape=True):
    """loss, per-sample f (and log q under BlackBox) and every gradient against the two oracles on the reported draws and minibatch"""
    c = compile_on(form, kw, seq, estimator, monkeypatch, exact_shape)
    p = c.program
    assert tuple(c.launch_plan(n, noise=supplied, want_fvalues=True)) == names
    call = dict(seed=13, offset=2, want_fvalues=True, want_indices=True)
    if supplied:
        named = {p.latent_name: np.random.RandomState(7).standard_normal((n, 1, p.n_classes, p.n_features)).astype(np.float32)}
        res = c.evaluate(n, noise=named, **call)
    else:
        res = c.evaluate(n, want_noise=True, **call)
    torch.cuda.synchronize()
    idx = res["indices"].cpu().numpy()
    assert len(set(idx.tolist())) == kw["b"] and idx.min() >= 0 and idx.max() < kw["ds"]
    if not supplied:
        named = {} if p.point_estimate else named_noise(c, res["noise"].cpu().numpy(), n)
    mb = {p.indices_name: idx.tolist()}
    exact, ref32 = oracle_pair(form, kw, n, estimator, named, mb)
    loss = float(res["loss"].item())
    assert np.isfinite(loss) and float(res["finite"].item()) == 1.0
    worst = bound_check(label, "loss", loss, exact["loss"], ref32["loss"])
    worst += bound_check(label, "f", res["f"].cpu().numpy(), exact["f"], ref32["f"])
    if estimator == "blackbox" and not p.point_estimate:
        worst += bound_check(label, "log_q", res["lq"].cpu().numpy(), exact["lq"], ref32["lq"])
    assert not worst, worst
    per_tensor_check(c.named_grads(), exact["grads"], ref32["grads"], label)
    return c, res, exact, ref32


# ---- A: Bernoulli -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("estimator", ESTIMATORS)
@pytest.mark.parametrize("seq", sorted(SEQUENCES))
@pytest.mark.parametrize("case", sorted(BERNOULLI))
def test_bernoulli_likelihood_matches_the_oracle(case, seq, estimator, monkeypatch):
    ds, b, p, n, xbwd, supplied = BERNOULLI[case]
    c, _, _, _ = run_case("bernoulli", dict(ds=ds, b=b, p=p), n, seq, estimator, plan_names(seq, 1, xbwd), monkeypatch,
                       "bernoulli %s %s %s" % (seq, estimator, case), supplied=supplied)
    assert c.program.likelihood == dense.LIK_BERNOULLI


@pytest.mark.parametrize("estimator", ESTIMATORS)
def test_bernoulli_likelihood_on_ragged_minibatch_tiles_of_the_f32_kernels(estimator, monkeypatch):
    ds, b, p, n = BERNOULLI_F32
    c, _, _, _ = run_case("bernoulli", dict(ds=ds, b=b, p=p), n, "fused", estimator, plan_names("f32", 1, None), monkeypatch,
                       "bernoulli f32 %s DS%d_B%d_P%d_N%d" % (estimator, ds, b, p, n), exact_shape=False)
    assert c.program.likelihood == dense.LIK_BERNOULLI


# ---- B: shared entries --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("estimator", ESTIMATORS)
@pytest.mark.parametrize("seq", sorted(SEQUENCES))
@pytest.mark.parametrize("prior", ["constant", "learnable"])
@pytest.mark.parametrize("case", sorted(SHARED))
def test_shared_row_parameters_match_the_oracle(case, prior, seq, estimator, monkeypatch):
    ds, b, p, n, xbwd = SHARED[case]
    kw = dict(ds=ds, b=b, p=p, learnable_prior=prior == "learnable")
    c, res, exact, ref32 = run_case("shared", kw, n, seq, estimator, plan_names(seq, 3, xbwd), monkeypatch,
                             "shared-%s %s %s %s" % (prior, seq, estimator, case))
    prog = c.program
    assert prog.q_scale[1] == 0 and prog.prior_scale[1] == 0 and prog.n_uniform_grad == 3 * p + (2 if prior == "learnable" else 1)
    assert set(exact["grads"]) == {"q_loc", "log_s"} | ({"log_prior_scale"} if prior == "learnable" else set())
    if seq == "fused":
        # a plain evaluation: the shared entries need the epilogue's sums, so the sample sums do not fold into the parameter kernel
        plain = tuple(c.launch_plan(n))
        assert plain[-2:] == _TAIL and "dense_param_fold_kernel" not in plain and "dense_rows<sliced>" in plain
        again = c.evaluate(n, seed=13, offset=2)
        torch.cuda.synchronize()
        label = "shared-%s fused-plain %s %s" % (prior, estimator, case)
        worst = bound_check(label, "loss", float(again["loss"].item()), exact["loss"], ref32["loss"])
        assert not worst, worst
        per_tensor_check(c.named_grads(), exact["grads"], ref32["grads"], label)


# ---- C: point estimate --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seq", sorted(SEQUENCES))
def test_point_estimate_on_the_exact_data_path_matches_the_oracle(seq, monkeypatch):
    ds, b, p, n, xbwd = POINT
    c, res, exact, _ = run_case("point", dict(ds=ds, b=b, p=p), n, seq, "pathwise", plan_names(seq, 3, xbwd), monkeypatch, "point %s pathwise DS%d_B%d_P%d_N%d" % (seq, ds, b, p, n))
    assert c.program.point_estimate and c.program.entropy_weight == 0.0
    f = res["f"].cpu().numpy()
    assert f.shape == (n,) and np.all(f == f[0])          # nothing is sampled: every sample computes the same value
    assert np.all(exact["f"].reshape(-1) == exact["f"].reshape(-1)[0])


# ---- D: caller weights per sample ---------------------------------------------------------------------------------------------------
def _weights(n):
    rng = np.random.RandomState(11)
    return rng.standard_normal(n), rng.standard_normal(n)


def _weighted_estimator(a, b):
    def g(f, lq):
        return (torch.as_tensor(a, dtype=f.dtype) * f.reshape(-1) + torch.as_tensor(b, dtype=lq.dtype) * lq.reshape(-1)).sum()
    return g


@functools.lru_cache(maxsize=None)
def _weighted_estimators(n):
    a, b = _weights(n)
    perm = np.roll(np.arange(n), 1)
    return dict(a=a, b=b, perm=perm, plain=_weighted_estimator(a, b), permuted=_weighted_estimator(a[perm], b))


def weighted_run(form, kw, seq, monkeypatch):
    """`evaluate_weighted` on a BlackBox-lowered model: -(sum_n a_n grad f_n + b_n grad log q_n) in the output block (finalize with a
    count of 1), which is the gradient of the oracle's loss -g(f, log q) for g = sum_n a_n f_n + b_n log q_n"""
    ds, b, p, ncls, n, xbwd = WEIGHTED
    c = compile_on(form, kw, seq, "blackbox", monkeypatch)
    assert tuple(c.launch_plan(n, weighted=True)) == plan_names(seq, ncls, xbwd, weighted=True)
    first = c.evaluate(n, seed=13, offset=2, want_noise=True, want_indices=True)
    named = named_noise(c, first["noise"].cpu().numpy(), n)
    mb = {"indices": first["indices"].cpu().numpy().tolist()}
    w = _weighted_estimators(n)
    dev = c.device
    on_device = lambda v: torch.as_tensor(v, dtype=torch.float32, device=dev)
    c.evaluate_weighted(n, on_device(w["a"]), on_device(w["b"]), seed=13, offset=2)       # the draw and the minibatch of (seed, offset) again
    torch.cuda.synchronize()
    return c, named, mb, w, on_device


@pytest.mark.parametrize("seq", sorted(SEQUENCES))
@pytest.mark.parametrize("form", ["per_element", "shared"])
def test_caller_weights_that_differ_per_sample_match_the_oracle(form, seq, monkeypatch):
    ds, b, p, ncls, n, _ = WEIGHTED
    kw = dict(ds=ds, b=b, p=p, c=ncls)
    c, named, mb, w, on_device = weighted_run(form, kw, seq, monkeypatch)
    exact, ref32 = oracle_pair(form, kw, n, w["plain"], named, mb)
    per_tensor_check(c.named_grads(), exact["grads"], ref32["grads"], "weighted-%s %s blackbox DS%d_B%d_P%d_N%d" % (form, seq, ds, b, p, n))


@pytest.mark.parametrize("form", ["per_element", "shared"])
def test_caller_weights_handed_to_other_samples_give_another_gradient(form, monkeypatch):
    """the guard of the test above: with a_n rolled by one sample the kernels follow the oracle of the ROLLED weights and leave the
    unrolled oracle by far more than the bound — a comparison that could not tell the two would be blind to the sample index.  (Both
    forms: where the prior sits on the posterior's own roots the weighted row sums of dense_weighted_sums cancel between the prior's
    and the posterior's entries, so only the shared form sees that kernel; the per-element form sees the likelihood's sites.)"""
    ds, b, p, ncls, n, _ = WEIGHTED
    kw = dict(ds=ds, b=b, p=p, c=ncls)
    c, named, mb, w, on_device = weighted_run(form, kw, "fused", monkeypatch)
    unrolled = c.named_grads()
    c.evaluate_weighted(n, on_device(w["a"][w["perm"]]), on_device(w["b"]), seed=13, offset=2)
    torch.cuda.synchronize()
    rolled = c.named_grads()
    exact, ref32 = oracle_pair(form, kw, n, w["permuted"], named, mb)
    per_tensor_check(rolled, exact["grads"], ref32["grads"], "weighted-rolled-%s fused blackbox" % form)
    plain64, plain32 = oracle_pair(form, kw, n, w["plain"], named, mb)
    for name, g64 in plain64["grads"].items():
        bound = max(4 * np.abs(plain32["grads"][name] - g64).max(), TOL * np.abs(g64).max())
        assert np.abs(rolled[name] - g64).max() > 100 * bound and np.abs(rolled[name] - unrolled[name]).max() > 100 * bound, name


# ---- E: training --------------------------------------------------------------------------------------------------------------------
TRAINED = {
    "shared-learnable": ("shared", dict(ds=64, b=40, p=32, learnable_prior=True), 3, 20, "dense_xbwd<0,2,7>"),
    "bernoulli": ("bernoulli", dict(ds=64, b=32, p=32), 1, 50, "dense_xbwd<0,2,7>"),
}


@pytest.mark.parametrize("case", sorted(TRAINED))
def test_four_adam_steps_on_the_fused_sequence_follow_the_oracle(case, monkeypatch):
    """`train()` with the draws and minibatches of a fixed sequence: losses and every parameter after four steps within the yardstick of
    the double-precision oracle's trajectory (the bounds of test_six_adam_steps_on_the_memory_kernel_follow_the_oracle)"""
    form, kw, ncls, n, xbwd = TRAINED[case]
    iters = 4
    c = compile_on(form, kw, "fused", "pathwise", monkeypatch)
    plain = tuple(c.launch_plan(n, noise=True))
    assert plain[:3] == ("dense_head", "dense_xfwd<0,1>", xbwd[:-1] + ",noise>") and plain[3] == "dense_rows<sliced>"
    assert plain[4:] == (_TAIL if form == "shared" else ("dense_param_fold_kernel",))
    rng = np.random.RandomState(5)
    noise_seq = [{"weights": rng.standard_normal((n, 1, ncls, kw["p"])).astype(np.float32)} for _ in range(iters)]
    mb_seq = [{"indices": rng.permutation(kw["ds"])[:kw["b"]].tolist()} for _ in range(iters)]
    losses, finite = c.train(iters, n, "Adam", noise_seq=noise_seq, minibatch_seq=mb_seq, lr=0.01)
    got = losses.cpu().numpy().astype(np.float64)
    assert c.last_mode == "stepwise" and np.isfinite(got).all() and finite.cpu().numpy().all()
    o64, o32 = Oracle(make(form, **kw), dtype=torch.float64), Oracle(make(form, **kw))
    l64 = o64.train(iters, n, "Adam", noise_seq=noise_seq, minibatch_seq=mb_seq, lr=0.01).astype(np.float64)
    l32 = o32.train(iters, n, "Adam", noise_seq=noise_seq, minibatch_seq=mb_seq, lr=0.01).astype(np.float64)
    label = "train-%s fused pathwise" % case
    # (Oracle.train returns its losses as float32: half an ulp of them is part of what the yardstick can resolve)
    worst = bound_check(label, "losses", got, l64, l32)
    assert not worst, worst
    p64 = {k: t.detach().numpy() for k, t in o64.named_parameters().items()}
    p32 = {k: t.detach().numpy() for k, t in o32.named_parameters().items()}
    params = c.named_params()
    assert set(params) == set(p64)
    for pname, value in params.items():
        e64 = p64[pname].reshape(value.shape)
        err, yard = np.abs(value - e64).max(), np.abs(p32[pname].reshape(value.shape) - e64).max()
        print("dense-models %s %-16s err %.3g  oracle32 %.3g  scale %.3g" % (label, pname, err, yard, np.abs(e64).max()))
        assert err <= max(4 * yard, 2e-5 * (1 + np.abs(e64).max())), pname
