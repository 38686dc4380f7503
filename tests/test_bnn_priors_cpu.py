"""Laplace and Cauchy priors on the weights and biases of the Bayesian-neural-network family (workloads.build_bnn_regression(prior=...),
bnn.lower_bnn, bsvi_bnn_set_row_priors) as far as it goes without a device: what the lowering records per tensor and per
row, the mixture across tensors, what it keeps refusing and why, the new export and the argument checks it makes in front of any device
work, the two reference fixtures of tests/golden/bnn_priors/ under the oracle, and that the builders without their new keywords build
what they built."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, Golden, rel_err
from brancher_amd import bnn, distributions as D, lowering, native, workloads as W
from brancher_amd.lowering import LoweringError
from oracle.svi_oracle import Oracle

TOL = 1e-5
FIXTURES = ["bnn_priors/bnn_laplace_tanh_P32_H6_C1_DS30_B12_N5", "bnn_priors/bnn_cauchy_linear_P16_C2_DS24_B10_N6"]
KIND = dict(normal=D.DIST_NORMAL, laplace=D.DIST_LAPLACE, cauchy=D.DIST_CAUCHY)
NARROW = dict(prior_scale=0.3, prior_loc=0.1, q_loc_scale=0.5)
A = dict(dataset_size=40, batch_size=17, n_features=64, n_hidden=9, n_outputs=1, **NARROW)                               # 64-9-1, tanh
MIXTURE = dict(weights1="laplace", b1="normal", weights2="cauchy", b2="laplace")
CLASSIFIER = dict(dataset_size=40, batch_size=17, n_features=64, n_hidden=9, n_classes=3, pixels="integers")


def prior_model(prior="laplace", posterior="normal", learnable_scale=False):
    """a 16-4-2 tanh network without biases, built by hand (tests/test_bnn_sigma_cpu.py: sigma_model): the prior of weights2 of the given
    family, its scale 0.3 or — learnable_scale — `BF.exp` of a learnable root `log_tau` of the joint model; weights1 Normal; the
    posterior of weights2 of the family `posterior`"""
    api = W.native_api()
    BF = api.BF
    rng = np.random.RandomState(0)
    DS, Bs, P, H, Cn = 20, 6, 16, 4, 2
    X = rng.randint(-3, 4, size=(DS, P, 1)).astype(np.float32)
    Y = rng.normal(size=(DS, Cn, 1)).astype(np.float32)
    indices = api.RandomIndices(dataset_size=DS, batch_size=Bs, name="indices", is_observed=True)
    x = api.EmpiricalVariable(X, indices=indices, name="x", is_observed=True)
    targets = api.EmpiricalVariable(Y, indices=indices, name="targets", is_observed=True)
    make = dict(normal=api.NormalVariable, laplace=api.LaplaceVariable, cauchy=api.CauchyVariable, lognormal=api.LogNormalVariable)
    scale = BF.exp(api.RootVariable(np.log(0.3), "log_tau", learnable=True)) if learnable_scale else 0.3 * np.ones((Cn, H))
    w1 = api.NormalVariable(np.zeros((H, P)), np.ones((H, P)), "weights1")
    w2 = make[prior](0.1 + np.zeros((Cn, H)), scale, "weights2")
    y = api.NormalVariable(BF.matmul(w2, BF.tanh(BF.matmul(w1, x))), 0.5, "y")
    model = api.ProbabilisticModel([y])
    y.observe(targets)
    q = [api.NormalVariable(0.02 * rng.normal(size=(H, P)), 0.05 * np.ones((H, P)), "weights1", learnable=True),
         make[posterior](0.05 * rng.normal(size=(Cn, H)), 0.1 * np.ones((Cn, H)), "weights2", learnable=True)]
    model.set_posterior_model(api.ProbabilisticModel(q))
    return model


def rows_of(p, name):
    t = next(t for t in p.tensors if t["name"] == name)
    return slice(t["row0"], t["row0"] + t["size"])


@pytest.mark.parametrize("prior", ["laplace", "cauchy"])
def test_the_three_builders_lower_with_a_kind_per_tensor(prior):
    """before this feature: LoweringError("bnn path: weights and biases must be Normal variables")"""
    api = W.native_api()
    models = [W.build_bnn_regression(api, prior=prior, **A), W.build_bayesian_neural_network(api, prior=prior, prior_scale=0.3, **CLASSIFIER),
              W.build_minibatch_linear_regression(api, n_features=8, n_outputs=2, prior=prior)]
    for model, latents in zip(models, (4, 4, 1)):
        try:
            p = bnn.lower_bnn(model, model.posterior_model)
        except LoweringError as err:
            pytest.fail("the lowering refuses a %s prior: %s" % (prior, err))
        assert p.row_prior.dtype == np.uint8 and p.row_prior.shape == (p.n_rows,) and (p.row_prior == KIND[prior]).all()
        assert len(p.tensors) == latents and all(t["prior"] == prior for t in p.tensors)
        assert p.summary()["priors"] == {t["name"]: prior for t in p.tensors}
        assert p.row_uniform.shape == (4, p.n_rows)
    # loc and scale through the same route as the Normal's: the constants of the model
    p = bnn.lower_bnn(models[0], models[0].posterior_model)
    assert (p.row_uniform[2:] >= p.n_uniform_grad).all()
    for role, value in ((2, 0.1), (3, 0.3)):
        e = p.uniform[p.row_uniform[role]]
        assert (e["transform"] == lowering.UT["identity"]).all() and not e["is_param"].any()
        assert np.allclose(e["a"] + e["b"] * np.asarray(p.consts)[e["src"]], value)


def test_a_mixture_across_tensors_is_a_kind_per_row():
    model = W.build_bnn_regression(W.native_api(), prior=MIXTURE, **A)
    p = bnn.lower_bnn(model, model.posterior_model)
    assert p.n_rows == 595 and [t["name"] for t in p.tensors] == ["weights1", "b1", "weights2", "b2"]
    for name, kind in MIXTURE.items():
        assert (p.row_prior[rows_of(p, name)] == KIND[kind]).all(), name
    assert p.summary()["priors"] == MIXTURE
    # a quad of the small tensors straddles two of them: rows 584 .. 587 are b1's last and weights2's first three
    assert sorted(set(p.row_prior[584:588].tolist())) == sorted({D.DIST_NORMAL, D.DIST_CAUCHY})
    # tensors a dict leaves out are Normal
    model = W.build_bnn_regression(W.native_api(), prior=dict(weights2="cauchy"), **A)
    p = bnn.lower_bnn(model, model.posterior_model)
    assert p.summary()["priors"] == dict(weights1="normal", b1="normal", weights2="cauchy", b2="normal")


def test_a_learnable_prior_scale_is_a_parameter_entry_of_its_rows():
    model = prior_model("laplace", learnable_scale=True)
    p = bnn.lower_bnn(model, model.posterior_model)
    sl = rows_of(p, "weights2")
    entries = set(p.row_uniform[3, sl].tolist())
    assert len(entries) == 1 and entries.pop() < p.n_uniform_grad and (p.row_prior[sl] == D.DIST_LAPLACE).all()
    assert (p.row_prior[rows_of(p, "weights1")] == D.DIST_NORMAL).all()
    (par, off, size, group), = [t for t in p.parameters if t[0].name == "log_tau"]
    assert group == 1 and size == 1


def test_what_stays_refused_is_refused_by_name():
    model = prior_model("lognormal")
    with pytest.raises(LoweringError) as err:
        bnn.lower_bnn(model, model.posterior_model)
    assert str(err.value).startswith("bnn path: ") and "LogNormal" in str(err.value) and "weights2" in str(err.value)
    assert "Normal, Laplace or Cauchy" in str(err.value)
    for posterior in ("laplace", "cauchy"):
        model = prior_model("laplace", posterior=posterior)
        with pytest.raises(LoweringError) as err:
            bnn.lower_bnn(model, model.posterior_model)
        assert "the posterior must be mean-field Normal variables" in str(err.value)
    with pytest.raises(ValueError):
        W.build_bnn_regression(W.native_api(), prior="lognormal")
    with pytest.raises(ValueError):
        W.build_bayesian_neural_network(W.native_api(), prior=dict(weights1="student"))


def test_the_export_is_declared_bound_and_present_and_checks_its_arguments():
    header = open(os.path.join(ROOT, "include", "bsvi.h")).read()
    declared = set(re.findall(r"\b(bsvi_[a-z0-9_]+)\s*\(", header))
    lib = native.load()
    assert "bsvi_bnn_set_row_priors" in declared and "bsvi_bnn_set_row_priors" in native.EXPORTS and hasattr(lib, "bsvi_bnn_set_row_priors")
    assert native.ABI_VERSION == 11 and lib.bsvi_abi_version() == 11            # a new export only
    # what the library validates in front of any device work: a null handle, a null array (a handle needs a device: the other codes
    # are checked where there is one, tests/test_gpu_bnn_priors.py)
    INVALID = -1
    kinds = np.full(8, D.DIST_LAPLACE, dtype=np.uint8)
    assert lib.bsvi_bnn_set_row_priors(None, kinds.ctypes.data_as(C.c_void_p), 8) == INVALID
    assert b"bsvi_bnn_set_row_priors" in lib.bsvi_last_error()
    assert lib.bsvi_bnn_set_row_priors(None, None, 0) == INVALID
    # the kinds the lowering writes are the header's
    for name, value in (("NORMAL", D.DIST_NORMAL), ("LAPLACE", D.DIST_LAPLACE), ("CAUCHY", D.DIST_CAUCHY)):
        assert re.search(r"BSVI_DIST_%s = %d," % (name, value), header)


def test_the_builders_without_the_keywords_build_what_they_built():
    """program for program: the default is prior="normal", prior_loc=0; the parameters the constant-sigma fixtures recorded from
    this builder are the ones it yields today; a non-Normal prior changes the kinds alone"""
    api = W.native_api()
    plain = dict(dataset_size=40, batch_size=17, n_features=64, n_hidden=9, n_outputs=1)
    for build, kw in ((W.build_bnn_regression, plain), (W.build_bayesian_neural_network, CLASSIFIER)):
        m1, m2, m3 = build(api, **kw), build(api, prior="normal", prior_loc=0., **kw), build(api, prior="cauchy", **kw)
        p1, p2, p3 = (bnn.lower_bnn(m, m.posterior_model) for m in (m1, m2, m3))
        for name in ("uniform", "consts", "row_uniform", "dataset", "labels", "param_uniform_ptr", "param_uniform_idx", "row_prior"):
            assert np.array_equal(getattr(p1, name), getattr(p2, name)), name
        # (a prior that is asked for has parameters of its own: the rows' q entries stay, the prior's become constants of the model)
        assert np.array_equal(p1.dataset, p3.dataset) and np.array_equal(p1.labels, p3.labels) and p1.layers == p3.layers
        assert np.array_equal(p1.row_uniform[:2], p3.row_uniform[:2]) and (p3.row_uniform[2:] >= p3.n_uniform_grad).all()
        assert (p1.row_uniform[2:] == p1.row_uniform[:2]).all()                # the reference's name-collision rule, as ever
        assert (p1.row_prior == D.DIST_NORMAL).all() and (p3.row_prior == D.DIST_CAUCHY).all()
        assert set(p1.summary()["priors"].values()) == {"normal"}
        for a, b in zip(p1.parameters, p3.parameters):
            assert a[0].name == b[0].name and np.array_equal(a[0].numpy(), b[0].numpy())
    for name in ("bnn_normal/bnn_normal_tanh_P32_H6_C1_DS30_B12_N5", "bnn_normal/bnn_normal_linear_P16_C2_DS24_B10_N6"):
        g = Golden(name)
        for v in g.build().posterior_model.flatten():
            if getattr(v, "learnable", False) and "param/" + v.name in g.data.files:
                assert np.array_equal(np.asarray(v.parameter.numpy(), dtype=np.float32).reshape(-1), g.data["param/" + v.name].reshape(-1)), v.name


def reference_present():
    from oracle import gen_golden                      # (where the generator looks for the reference)
    return os.path.isdir(os.path.join(gen_golden.REF, "brancher"))


needs_reference = pytest.mark.skipif(not reference_present(), reason="the reference is only present in the build container")


@needs_reference
def test_the_fixtures_regenerate_bit_for_bit(tmp_path):
    env = dict(os.environ, BSVI_GOLDEN_OUT=str(tmp_path), PYTHONDONTWRITEBYTECODE="1", OMP_NUM_THREADS="1")
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_golden_bnn_priors.py")], check=True, env=env,
                   stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=600)
    for name in FIXTURES:
        new, old = np.load(os.path.join(str(tmp_path), os.path.basename(name) + ".npz")), np.load(os.path.join(GOLDEN, name + ".npz"))
        assert sorted(new.files) == sorted(old.files)
        for key in old.files:
            if key == "meta":
                assert json.loads(str(new[key])) == json.loads(str(old[key]))
            else:
                assert np.array_equal(new[key], old[key], equal_nan=True), (name, key)


@pytest.mark.parametrize("name", FIXTURES)
def test_the_oracle_reproduces_the_fixtures(name):
    """the double-precision oracle against the real reference's record, within the bounds of tests/test_oracle_golden.py: 1e-5 of the
    loss, of the largest gradient, of the per-sample terms and of the trajectory"""
    g = Golden(name)
    prior = g.meta["kwargs"]["prior"]
    assert g.meta["builder"] == "build_bnn_regression" and prior in ("laplace", "cauchy")
    p = bnn.lower_bnn(g.build(), g.build().posterior_model)
    assert len(p.tensors) == 2 and (p.row_prior == KIND[prior]).all()
    for estimator in ("pathwise", "blackbox", "taylor1"):
        res = Oracle(g.build(), dtype=torch.float64).loss_and_grads(g.N, estimator, g.noise, g.minibatch)
        ref = float(g.data["loss_" + estimator])
        assert abs(res["loss"] - ref) <= TOL * abs(ref), estimator
        ref_grads = g.group("grad_%s/" % estimator)
        scale = max(np.abs(v).max() for v in ref_grads.values())
        for pname, g_ref in ref_grads.items():
            assert np.abs(res["grads"][pname] - g_ref).max() <= TOL * scale, (estimator, pname)
    res = Oracle(g.build(), dtype=torch.float64).loss_and_grads(g.N, "blackbox", g.noise, g.minibatch)
    assert rel_err(res["f"], g.data["lp"] + g.data["H"]) <= TOL and rel_err(res["lq"], g.data["lq"]) <= TOL
    tr = g.meta["trajectory"]
    oracle = Oracle(g.build(), dtype=torch.float64)
    losses = oracle.train(tr["iters"], tr["n"], tr["optimizer"], "pathwise", g.trajectory_noise(),
                          minibatch_seq=g.trajectory_minibatch(), **g.opt_kwargs())
    assert tr["optimizer"] == "Adam" and rel_err(losses, g.data["traj/losses"]) <= TOL
    after = g.group("traj/param_after/")
    for pname, par in oracle.named_parameters().items():
        assert np.abs(par.detach().numpy() - after[pname]).max() <= 1e-5 * (1 + np.abs(after[pname]).max()), pname
    # the prior is a visible share of the recorded gradient: the Normal-prior twin's gradient of the posterior means differs from it
    twin = W.build_bnn_regression(W.native_api(), **dict(g.meta["kwargs"], prior="normal"))
    other = Oracle(twin, dtype=torch.float64).loss_and_grads(g.N, "pathwise", g.noise, g.minibatch)["grads"]
    ref_grads = g.group("grad_pathwise/")
    name_loc = next(k for k in ref_grads if k.startswith("weights1") and ("loc" in k or "mu" in k))
    assert np.abs(other[name_loc] - ref_grads[name_loc]).max() > 1e-2 * np.abs(ref_grads[name_loc]).max()
