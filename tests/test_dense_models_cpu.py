"""The conditions that keep tests/test_gpu_dense_models.py from being vacuous, checked without a GPU on the models and shapes that file
runs (its builders and case tables, imported from it), with the double- and single-precision oracle on seeded draws:

  - every builder lowers through dense.lower_dense to the likelihood, the point-estimate flag and the bases and strides its form is
    there for (the device tests construct dense.CompiledDense themselves: engine.compile_model offers a model to the scalar path first,
    which takes a single-output Bernoulli model of up to 4096 products — the small Bernoulli shapes never reached these kernels);
  - the gradient of every tensor the likelihood reaches changes by at least 5 % of that tensor's largest entry when the labels are drawn
    again with another seed.  The labels enter through the likelihood alone: a comparison that passes this cannot be satisfied by the
    prior and the entropy.  The `C = 1` Categorical shapes of tests/test_gpu_dense_fused.py — listed there as the Bernoulli likelihood
    until this file — FAIL it with a change of exactly 0, which is asserted here so that the reason stays on record;
  - the bound of the device tests, max(4 |oracle32 - oracle64|, 1e-5 scale) per tensor, is at most 1e-4 scale: it resolves at least four
    digits of every gradient.  An input that misses this is changed (q scale, seed), never the condition."""
import functools

import numpy as np
import pytest
import torch

import test_gpu_dense_models as G
from brancher_amd import dense, lowering, workloads as W
from oracle.svi_oracle import Oracle

PRIOR_ONLY = {"log_prior_scale"}      # reached by the prior alone: exempt from the label condition


def _cases():
    """(id, form, builder keywords, classes, samples, estimator) of every case of A to D"""
    out = []
    bern = sorted({v[:4] for v in G.BERNOULLI.values()} | {G.BERNOULLI_F32})
    for ds, b, p, n in bern:
        for est in G.ESTIMATORS:
            out.append(("bernoulli-DS%d_B%d_P%d_N%d-%s" % (ds, b, p, n, est), "bernoulli", dict(ds=ds, b=b, p=p), 1, n, est))
    for case, (ds, b, p, n, _) in sorted(G.SHARED.items()):
        for learnable in (False, True):
            for est in G.ESTIMATORS:
                out.append(("shared-%s-%s-%s" % ("learnable" if learnable else "constant", case, est), "shared",
                            dict(ds=ds, b=b, p=p, learnable_prior=learnable), 3, n, est))
    ds, b, p, n, _ = G.POINT
    out.append(("point-DS%d_B%d_P%d_N%d-pathwise" % (ds, b, p, n), "point", dict(ds=ds, b=b, p=p), 3, n, "pathwise"))
    ds, b, p, c, n, _ = G.WEIGHTED
    for form in ("per_element", "shared"):
        out.append(("weighted-%s-DS%d_B%d_P%d_N%d" % (form, ds, b, p, n), form, dict(ds=ds, b=b, p=p, c=c), c, n, "weighted"))
    return out


CASES = _cases()


def draws(kw, n_classes, n):
    rng = np.random.RandomState(3)
    return ({"weights": rng.standard_normal((n, 1, n_classes, kw["p"])).astype(np.float32)}, {"indices": rng.permutation(kw["ds"])[:kw["b"]].tolist()})


@functools.lru_cache(maxsize=None)
def oracles(case_id):
    """the double- and the single-precision oracle of a case on its seeded draws, and the double-precision one with the labels redrawn"""
    _, form, kw, n_classes, n, est = next(c for c in CASES if c[0] == case_id)
    estimator = G._weighted_estimators(n)["plain"] if est == "weighted" else est
    named, mb = draws(kw, n_classes, n)
    if form == "point":
        named = {}
    run = lambda dtype, **more: Oracle(G.make(form, **dict(kw, **more)), dtype=dtype).loss_and_grads(n, estimator, named, mb)
    return run(torch.float64), run(torch.float32), run(torch.float64, label_seed=1)


def label_change(exact, redrawn):
    return {name: np.abs(redrawn["grads"][name] - g).max() / np.abs(g).max() for name, g in exact["grads"].items() if g is not None and np.abs(g).max() > 0}


@pytest.mark.parametrize("case_id", [c[0] for c in CASES])
def test_every_gradient_the_likelihood_reaches_depends_on_the_labels(case_id):
    exact, _, redrawn = oracles(case_id)
    change = label_change(exact, redrawn)
    print(case_id, change)
    assert set(change) - PRIOR_ONLY and set(change) == {k for k, g in exact["grads"].items() if g is not None}
    for name, rel in change.items():
        assert name in PRIOR_ONLY or rel >= 0.05, (name, rel)


@pytest.mark.parametrize("shape", [(64, 32, 32, 1, 50), (700, 650, 32, 1, 20)], ids=lambda s: "DS%d_B%d_P%d_C%d_N%d" % s)
def test_the_one_class_categorical_shapes_of_the_fused_tests_do_not_depend_on_the_labels(shape):
    """why this file and tests/test_gpu_dense_models.py exist: the `C = 1` rows of tests/test_gpu_dense_fused.py (among them the only one
    that reaches the six launches through the LDS rule) build a Categorical with ONE class — log-probability 0, likelihood gradient 0"""
    import test_gpu_dense_fused as F
    assert shape in F.SHAPES or any(row[0] == shape for row in F.DENSE_PLAN_ROWS)
    ds, b, p, c, n = shape
    api = W.native_api()
    model = F.build(api, shape)
    assert dense.lower_dense(model, model.posterior_model).likelihood == dense.LIK_CATEGORICAL
    named, mb = draws(dict(ds=ds, b=b, p=p), c, n)
    grads = []
    for seed in (0, 1):
        model = F.build(api, shape, seed=seed)       # another seed: other labels AND other pixels
        grads.append(Oracle(model, dtype=torch.float64).loss_and_grads(n, "pathwise", named, mb)["grads"])
    assert set(grads[0]) == {"weights_loc", "weights_scale"}
    for name, g in grads[0].items():
        assert np.array_equal(g, grads[1][name]), name         # change = 0: neither the labels nor the data are looked at
    assert np.abs(grads[0]["weights_loc"]).max() == 0.0 and np.abs(grads[0]["weights_scale"]).max() <= 1e-12


@pytest.mark.parametrize("case_id", [c[0] for c in CASES])
def test_the_bound_resolves_four_digits_of_every_gradient(case_id):
    exact, ref32, _ = oracles(case_id)
    for name, g64 in exact["grads"].items():
        scale, yard = np.abs(g64).max(), np.abs(ref32["grads"][name] - g64).max()
        print("%s %-16s 4 |oracle32 - oracle64| / scale %.3g" % (case_id, name, 4 * yard / scale))
        assert max(4 * yard, G.TOL * scale) <= 1e-4 * scale, (name, yard, scale)


def lowered(form, estimator="pathwise", **kw):
    model = G.make(form, **kw)
    return dense.lower_dense(model, model.posterior_model, estimator)


@pytest.mark.parametrize("estimator", G.ESTIMATORS)
def test_the_bernoulli_builder_lowers_to_the_bernoulli_likelihood(estimator):
    for ds, b, p, n in sorted({v[:4] for v in G.BERNOULLI.values()} | {G.BERNOULLI_F32}):
        prog = lowered("bernoulli", estimator, ds=ds, b=b, p=p)
        assert prog.likelihood == dense.LIK_BERNOULLI and not prog.point_estimate
        assert (prog.n_classes, prog.n_features, prog.dataset_size, prog.batch_size) == (1, p, ds, b)
        # a loc and a scale per weight, and the prior on the posterior's own roots (the name-collision rule)
        assert prog.q_loc == prog.prior_loc and prog.q_scale == prog.prior_scale and prog.q_loc[1] == 1 and prog.q_scale[1] == 1
        assert prog.n_params == prog.n_uniform_grad == 2 * p
        assert set(np.unique(prog.labels)) == {0.0, 1.0} and prog.labels.dtype == np.float32
        assert np.array_equal(prog.dataset, np.round(prog.dataset)) and prog.dataset.min() >= 0 and prog.dataset.max() <= 255


def test_the_scalar_path_would_take_the_small_bernoulli_shapes():
    """why the device tests construct dense.CompiledDense themselves: engine.compile_model tries the scalar path first, which unrolls a
    single-output matmul link of up to 4096 products — through it the small Bernoulli shapes would not run a dense kernel at all"""
    ds, b, p = G.BERNOULLI["DS64_B32_P32_N50"][:3]
    model = G.make("bernoulli", ds=ds, b=b, p=p)
    assert type(lowering.lower(model, model.posterior_model, "pathwise")).__name__ == "Program"
    ds, b, p = G.BERNOULLI["DS700_B650_P32_N20"][:3]
    model = G.make("bernoulli", ds=ds, b=b, p=p)
    with pytest.raises(lowering.LoweringError, match="matmul link"):
        lowering.lower(model, model.posterior_model, "pathwise")


@pytest.mark.parametrize("estimator", G.ESTIMATORS)
@pytest.mark.parametrize("learnable", [False, True], ids=["constant", "learnable"])
def test_the_shared_builder_lowers_to_stride_zero_entries(learnable, estimator):
    for ds, b, p, n, _ in G.SHARED.values():
        c = 3
        prog = lowered("shared", estimator, ds=ds, b=b, p=p, learnable_prior=learnable)
        assert prog.likelihood == dense.LIK_CATEGORICAL and not prog.point_estimate
        names = [par.name for par, _, _, _ in prog.parameters]
        assert sorted(names) == sorted(["q_loc", "log_s"] + (["log_prior_scale"] if learnable else []))
        assert prog.q_loc[1] == 1 and prog.q_scale[1] == 0 and prog.prior_loc[1] == 1 and prog.prior_scale[1] == 0
        assert prog.n_uniform_grad == c * p + (2 if learnable else 1) == prog.n_params
        # the q scale's entry takes a gradient; the prior's only when its root is learnable; the prior's loc never
        assert prog.q_scale[0] < prog.n_uniform_grad and (prog.prior_scale[0] < prog.n_uniform_grad) == learnable
        assert prog.prior_loc[0] >= prog.n_uniform_grad
        groups = {par.name: int(prog.param_group[off]) for par, off, _, _ in prog.parameters}
        assert groups["q_loc"] == 0 and groups["log_s"] == 0 and (not learnable or groups["log_prior_scale"] == 1)
        # the transform a + b exp(theta) of the shared scale, at its value
        entry = prog.uniform[prog.q_scale[0]]
        assert (float(entry["a"]), float(entry["b"])) == (np.float32(0.001), np.float32(0.5))


def test_the_point_builder_lowers_to_a_point_estimate_on_the_exact_data_shape():
    ds, b, p, n, _ = G.POINT
    prog = lowered("point", ds=ds, b=b, p=p)
    assert prog.point_estimate and prog.entropy_weight == 0.0 and prog.likelihood == dense.LIK_CATEGORICAL
    assert prog.q_loc == (0, 1) and prog.q_scale[1] == 0 and prog.q_scale[0] >= prog.n_uniform_grad and prog.n_params == 3 * p
    assert p % 4 == 0 and p >= 32 and ds == b          # the exact-data scan wants it; the full batch, as inference.MAP is used


def test_the_per_element_builder_of_the_weighted_cases_lowers_like_the_standard_model():
    ds, b, p, c, n, _ = G.WEIGHTED
    prog = lowered("per_element", "blackbox", ds=ds, b=b, p=p, c=c)
    assert prog.likelihood == dense.LIK_CATEGORICAL and prog.q_loc == prog.prior_loc == (0, 1) and prog.q_scale == prog.prior_scale == (c * p, 1)


def test_rolled_caller_weights_are_other_weights():
    n = G.WEIGHTED[4]
    w = G._weighted_estimators(n)
    assert not np.array_equal(w["a"], w["a"][w["perm"]]) and sorted(w["a"]) == sorted(w["a"][w["perm"]])
    assert np.abs(w["a"]).min() > 0 and w["a"].std() > 0.5 and w["b"].std() > 0.5
