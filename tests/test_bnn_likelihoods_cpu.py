"""Laplace and Cauchy regression likelihoods of the Bayesian-neural-network family (workloads.build_bnn_regression(likelihood=...),
bnn.lower_bnn, bsvi_bnn_set_likelihood_family) as far as they go without a device: what the lowering records for an
observed `LaplaceVariable` / `CauchyVariable` over the chain under every form of the scale, that the Normal twin's program is what it
was, what stays refused and that the refusal names the family, the new export's null-handle check and the export count, the two
reference fixtures of tests/golden/bnn_lik/, and the table of DESIGN 4.7 (d f / d sigma = (u psi(u) - 1) / sigma) against the
double-precision oracle's own finite differences."""
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
from brancher_amd import bnn, distributions as D, native, workloads as W
from brancher_amd.lowering import LoweringError
from oracle.svi_oracle import Oracle
from test_bnn_normal_cpu import reference_present

TOL = 1e-5
FIXTURES = ["bnn_lik/bnn_lik_laplace_tanh_P32_H6_C1_DS30_B12_N5", "bnn_lik/bnn_lik_cauchy_linear_P16_C2_DS24_B10_N6"]
FAMILIES = {"laplace": (D.DIST_LAPLACE, "Laplace"), "cauchy": (D.DIST_CAUCHY, "Cauchy")}
A = dict(dataset_size=40, batch_size=17, n_features=64, n_hidden=9, n_outputs=1)                                    # 64-9-1, tanh
PER_OUTPUT = dict(dataset_size=40, batch_size=33, n_features=36, n_hidden=5, hidden2=4, n_outputs=3, activation="relu", data="normal",
                  sigma=[0.3, 0.5, 0.8])


def lowered(**kw):
    model = W.build_bnn_regression(W.native_api(), **kw)
    return bnn.lower_bnn(model, model.posterior_model)


def family_model(form, family):
    """a 16-4-2 tanh network without biases under an observed variable of `family` whose scale has the given form
    (tests/test_bnn_sigma_cpu.py: sigma_model, with the observed variable's class a parameter)"""
    api = W.native_api()
    BF = api.BF
    rng = np.random.RandomState(0)
    DS, Bs, P, H, Cn = 20, 6, 16, 4, 2
    X = rng.randint(-3, 4, size=(DS, P, 1)).astype(np.float32)
    Y = rng.normal(size=(DS, Cn, 1)).astype(np.float32)
    indices = api.RandomIndices(dataset_size=DS, batch_size=Bs, name="indices", is_observed=True)
    x = api.EmpiricalVariable(X, indices=indices, name="x", is_observed=True)
    targets = api.EmpiricalVariable(Y, indices=indices, name="targets", is_observed=True)
    q, learnable = [], False
    if form == "latent":
        scale = api.LogNormalVariable(0., 0.3, "sigma")
        q.append(api.LogNormalVariable(0., 0.2, "sigma", learnable=True))
    elif form == "bare":
        scale = api.RootVariable(0.5, name="sigma", learnable=True)
    elif form == "shape":
        scale, learnable = np.array([[0.3], [0.5], [0.8]]), True
    else:
        scale = 0.5
    w1 = api.NormalVariable(np.zeros((H, P)), np.ones((H, P)), "weights1")
    w2 = api.NormalVariable(np.zeros((Cn, H)), np.ones((Cn, H)), "weights2")
    loc = BF.matmul(w2, BF.tanh(BF.matmul(w1, x)))
    q += [api.NormalVariable(0.02 * rng.normal(size=(H, P)), 0.05 * np.ones((H, P)), "weights1", learnable=True),
          api.NormalVariable(0.05 * rng.normal(size=(Cn, H)), 0.1 * np.ones((Cn, H)), "weights2", learnable=True)]
    make = dict(normal=api.NormalVariable, laplace=api.LaplaceVariable, cauchy=api.CauchyVariable, lognormal=api.LogNormalVariable)[family]
    y = make(loc, scale, "y", learnable=learnable)
    model = api.ProbabilisticModel([y])
    y.observe(targets)
    model.set_posterior_model(api.ProbabilisticModel(q))
    return model


@pytest.mark.parametrize("family", list(FAMILIES))
def test_an_observed_laplace_or_cauchy_lowers_as_the_normal_twin_does(family):
    """the test of this file that fails without the feature: "bnn path: expected one matmul likelihood\""""
    kind, _ = FAMILIES[family]
    try:
        p = lowered(likelihood=family, **A)
    except LoweringError as err:
        pytest.fail("the lowering refuses an observed %s: %s" % (family, err))
    twin = lowered(**A)
    assert p.likelihood == bnn.LIK_NORMAL and p.family == kind and twin.family == D.DIST_NORMAL
    assert p.layers == twin.layers and p.n_rows == twin.n_rows and p.n_params == twin.n_params
    assert np.array_equal(p.dataset, twin.dataset) and np.array_equal(p.row_uniform, twin.row_uniform)
    # a constant: one entry among the table's constants
    assert not p.scale_learnable and p.scale_head is None and p.scale_stride == 0 and p.scale_uniform == twin.scale_uniform >= p.n_uniform_grad
    s = p.summary()
    assert s["likelihood"] == "normal" and s["scale"] == "constant" and s["family"] == family
    # one constant per output
    p3, t3 = lowered(likelihood=family, **PER_OUTPUT), lowered(**PER_OUTPUT)
    assert p3.family == kind and not p3.scale_learnable and p3.scale_stride == 1 and p3.scale_uniform == t3.scale_uniform >= p3.n_uniform_grad
    assert p3.layers == t3.layers and p3.n_rows == t3.n_rows
    # the reference's learnable=True, and exp of a learnable root per output
    for kw, root in ((dict(A, learnable_sigma=True, sigma_init=0.6), "y_scale"),
                     (dict(PER_OUTPUT, learnable_sigma="exp", sigma_init=[0.5, 0.5, 0.5]), "y_log_scale")):
        pl, tl = lowered(likelihood=family, **kw), lowered(**kw)
        assert pl.family == kind and pl.scale_learnable and pl.summary()["scale"] == "learnable" and pl.summary()["family"] == family
        assert (pl.scale_uniform, pl.scale_stride) == (tl.scale_uniform, tl.scale_stride) and pl.scale_uniform < pl.n_uniform_grad
        assert root in {par.name for par, _, _, _ in pl.parameters} and pl.layers == tl.layers
    # a scale head
    ph, th = lowered(likelihood=family, scale_head="softplus", **A), lowered(scale_head="softplus", **A)
    assert ph.family == kind and ph.scale_head == th.scale_head and ph.scale_head[0] == "softplus" and ph.layers == th.layers
    assert ph.layers[-1]["rows"] == 2 and ph.n_classes == 1 and ph.summary()["scale"] == "head" and ph.summary()["family"] == family


def test_the_normal_twin_is_what_it_was():
    """the default is likelihood="normal": the same program field for field, and no "family" in a summary that had none"""
    for kw in (A, PER_OUTPUT, dict(A, learnable_sigma=True), dict(A, scale_head="exp")):
        p, p2 = lowered(**kw), lowered(likelihood="normal", **kw)
        assert p.family == p2.family == D.DIST_NORMAL and p.summary() == p2.summary() and "family" not in p.summary()
        assert set(p.summary()) == {"kind", "layers", "n_rows", "dataset_size", "batch_size", "n_params", "likelihood", "latents", "scale", "priors"}
        for name in ("uniform", "consts", "row_uniform", "dataset", "labels", "param_uniform_ptr", "param_uniform_idx", "row_prior"):
            assert np.array_equal(getattr(p, name), getattr(p2, name)), name
        # ... and the other families are built on the same features and posterior, draw for draw; the targets differ by the teacher's noise
        for family in FAMILIES:
            pf = lowered(likelihood=family, **kw)
            assert np.array_equal(pf.dataset, p.dataset) and not np.array_equal(pf.labels, p.labels)
            old = {par.name: par.numpy() for par, _, _, _ in p.parameters}
            assert all(np.array_equal(old[par.name], par.numpy()) for par, _, _, _ in pf.parameters)
    model = W.build_bayesian_neural_network(W.native_api(), dataset_size=40, batch_size=17, n_features=64, n_hidden=9, n_classes=3)
    s = bnn.lower_bnn(model, model.posterior_model).summary()
    assert "family" not in s and "scale" not in s
    with pytest.raises(ValueError):
        W.build_bnn_regression(W.native_api(), likelihood="student")


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("form,cause", [("latent", "is a latent variable or computed from one"), ("bare", "is learnable"),
                                        ("shape", "neither one value nor one per output")])
def test_the_refusals_of_the_scale_name_the_family(form, cause, family):
    model = family_model(form, family)
    with pytest.raises(LoweringError) as err:
        bnn.lower_bnn(model, model.posterior_model)
    msg = str(err.value)
    assert msg.startswith("bnn path: the scale of the %s likelihood 'y' " % FAMILIES[family][1]) and cause in msg
    # ... and the Normal's is word for word what it was
    normal = family_model(form, "normal")
    with pytest.raises(LoweringError) as err:
        bnn.lower_bnn(normal, normal.posterior_model)
    assert str(err.value) == msg.replace("the %s likelihood" % FAMILIES[family][1], "the Normal likelihood")


def test_another_observed_family_over_the_chain_stays_refused():
    model = family_model(None, "lognormal")
    with pytest.raises(LoweringError, match="expected one matmul likelihood"):
        bnn.lower_bnn(model, model.posterior_model)


def test_the_export_and_the_abi():
    lib = native.load()
    INVALID = -1
    assert lib.bsvi_bnn_set_likelihood_family(None, D.DIST_LAPLACE) == INVALID and b"null handle" in lib.bsvi_last_error()
    assert lib.bsvi_bnn_set_likelihood_family(None, D.DIST_NORMAL) == INVALID
    assert native.ABI_VERSION == 11 and lib.bsvi_abi_version() == 11
    header = open(os.path.join(ROOT, "include", "bsvi.h")).read()
    declared = set(re.findall(r"\b(bsvi_[a-z0-9_]+)\s*\(", header)) - {"bsvi_status", "bsvi_op"}      # (tests/test_lowering_abi.py)
    assert "bsvi_bnn_set_likelihood_family" in declared
    out = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if len(line.split()) >= 3 and line.split()[-2] in "TW" and line.split()[-1].startswith("bsvi_")}
    assert len(exported) == len(declared) and exported == declared, (exported ^ declared)


@pytest.mark.parametrize("name", FIXTURES)
def test_the_fixtures_load(name):
    g = Golden(name)
    kw = g.meta["kwargs"]
    assert g.meta["builder"] == "build_bnn_regression" and kw["likelihood"] in FAMILIES
    p = bnn.lower_bnn(g.build(), g.build().posterior_model)
    assert p.family == FAMILIES[kw["likelihood"]][0] and len(p.tensors) == 2 and sorted(g.noise) == sorted(t["name"] for t in p.tensors)
    assert (g.N, p.dataset_size, p.batch_size) == ((5, 30, 12) if kw["likelihood"] == "laplace" else (6, 24, 10))
    assert p.scale_learnable == (kw["likelihood"] == "cauchy")
    for estimator in ("pathwise", "blackbox", "taylor1", "custom_baseline", "custom_softmax"):
        assert np.isfinite(float(g.data["loss_" + estimator])) and g.group("grad_%s/" % estimator)
    assert g.meta["trajectory"]["iters"] == 4 and g.meta["trajectory"]["optimizer"] == "Adam"
    # the oracle reproduces the record (the bounds of tests/test_bnn_sigma_cpu.py for its fixtures)
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


@pytest.mark.skipif(not reference_present(), reason="the reference is only present in the build container")
def test_the_fixtures_regenerate_bit_for_bit(tmp_path):
    env = dict(os.environ, BSVI_GOLDEN_OUT=str(tmp_path), PYTHONDONTWRITEBYTECODE="1", OMP_NUM_THREADS="1")
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_golden_bnn_likelihoods.py")], check=True, env=env,
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
def test_the_oracles_gradient_of_sigmas_root_is_the_finite_difference_of_its_loss(name):
    """the table of DESIGN 4.7 against the oracle, not the kernel: on the fixture's draws and minibatch, the double-precision oracle's
    gradient of sigma's root (the Laplace fixture's constant scale made the reference's learnable=True for this) equals a central
    difference of the oracle's own loss to 1e-6 relative.  (Central differences of step h are off by h^2 f''' / 6 ~ 1e-8 relative at
    h = 1e-4; |u| has a kink where a residual crosses zero, which no step of 1e-4 in sigma's root moves a residual across.)"""
    g = Golden(name)
    kw = dict(g.meta["kwargs"], learnable_sigma=True)
    build = lambda: W.build_bnn_regression(W.native_api(), **kw)

    def loss_at(shift):
        o = Oracle(build(), dtype=torch.float64)
        root = o.named_parameters()["y_scale"].detach().numpy().astype(np.float64)
        o.set_parameters({"y_scale": root + shift})
        return o.loss_and_grads(g.N, "pathwise", g.noise, g.minibatch)

    grad = loss_at(0.0)["grads"]["y_scale"].reshape(-1)
    h = 1e-4
    for c in range(grad.size):
        e = np.zeros(grad.size)
        e[c] = h
        shift = e.reshape(loss_at(0.0)["grads"]["y_scale"].shape)
        fd = (loss_at(shift)["loss"] - loss_at(-shift)["loss"]) / (2 * h)
        print(name[-22:], "output", c, "grad", grad[c], "finite difference", fd)
        assert abs(grad[c]) > 1e-3 and abs(fd - grad[c]) <= 1e-6 * abs(grad[c])
