"""Latent prior scales of the Bayesian-neural-network family, without a GPU: what `bnn.lower_bnn` makes of a hierarchical prior — a
tensor's prior scale `b * tau` with tau a LogNormalVariable under a LogNormal posterior of the same name (`scale_latents`, `row_latent`,
`latent_uniform`, `n_noise`) —, every refusal by its text, the builders' keywords, the noise round trip, the declaration of
`bsvi_bnn_set_scale_latents`, and the two fixtures of the real reference (tools/gen_golden_bnn_hier.py) against the oracle.  The device
side is tests/test_gpu_bnn_hier.py."""
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
from test_bnn_priors_cpu import NARROW

TOL = 1e-5
A = dict(dataset_size=40, batch_size=17, n_features=64, n_hidden=9, n_outputs=1, **NARROW)                               # 64-9-1, tanh
ONE_LAYER = dict(dataset_size=24, batch_size=8, n_features=32, n_hidden=0, n_outputs=2, bias=False, **NARROW)            # 32-2: Rs = 0
B = dict(dataset_size=40, batch_size=33, n_features=36, n_hidden=5, hidden2=4, n_outputs=3, activation="relu", data="normal",
         sigma=[0.3, 0.5, 0.8], **NARROW)                                                                                # 36-5-4-3, relu
# five latents over five of the six tensors, differing multipliers; weights3 keeps its constant scale
B_LATENTS = dict(ta=[("weights1", 0.5)], tb=[("b1", 2.0)], tc=["weights2"], td=[("b2", 1.5)], te=[("b3", 0.25)])
CLASSIFIER = dict(classifier=True, dataset_size=40, batch_size=17, n_features=16, n_hidden=6, n_classes=3, pixels="integers",
                  prior_scale=0.3, prior_loc=0.1, q_scale=0.1, q_loc_scale=0.5)
FIXTURES = ["bnn_hier/bnn_hier_normal_linear_P16_C2_DS24_B10_N6", "bnn_hier/bnn_hier_laplace_linear_P32_C1_DS30_B12_N5"]


def hand_built(scale=lambda tau: tau * 2.0, prior="laplace", tau_prior=None, tau_q=None, learnable_prior=True, weights_q="normal", lik_scale=None):
    """a 32-2 layer without a bias, built by hand: weights1 ~ prior(0.1, scale(tau)), tau a LogNormal whose loc and scale are learnable
    roots of the joint model (`tau_prior_loc`, exp of `tau_prior_log_scale`) — or the reference's auto-created `tau_loc` / `tau_scale`,
    which collide with the posterior's by name (learnable_prior=False) —, q(tau) a learnable LogNormal"""
    api = W.native_api()
    BF = api.BF
    rng = np.random.RandomState(0)
    DS, Bs, P, Cn = 24, 8, 32, 2
    X = rng.randint(-3, 4, size=(DS, P, 1)).astype(np.float32)
    Y = rng.normal(size=(DS, Cn, 1)).astype(np.float32)
    indices = api.RandomIndices(dataset_size=DS, batch_size=Bs, name="indices", is_observed=True)
    x = api.EmpiricalVariable(X, indices=indices, name="x", is_observed=True)
    targets = api.EmpiricalVariable(Y, indices=indices, name="targets", is_observed=True)
    make = dict(normal=api.NormalVariable, laplace=api.LaplaceVariable, cauchy=api.CauchyVariable, lognormal=api.LogNormalVariable)
    if tau_prior is not None:
        tau = tau_prior(api)
    elif learnable_prior:
        tau = api.LogNormalVariable(api.RootVariable(-0.3, "tau_prior_loc", learnable=True),
                                    BF.exp(api.RootVariable(np.log(0.7), "tau_prior_log_scale", learnable=True)), "tau")
    else:
        tau = api.LogNormalVariable(-0.3, 0.7, "tau")
    w1 = make[prior](0.1 + np.zeros((Cn, P)), scale(tau), "weights1")
    y = api.NormalVariable(BF.matmul(w1, x), lik_scale(tau) if lik_scale else 0.5, "y")
    model = api.ProbabilisticModel([y])
    y.observe(targets)
    q = [make[weights_q](0.05 * rng.normal(size=(Cn, P)), 0.1 * np.ones((Cn, P)), "weights1", learnable=True),
         tau_q(api) if tau_q is not None else api.LogNormalVariable(-0.5, 0.3, "tau", learnable=True)]
    model.set_posterior_model(api.ProbabilisticModel([v for v in q if v is not None]))
    return model


def lowered(model, estimator="pathwise"):
    return bnn.lower_bnn(model, model.posterior_model, estimator)


def regression(**kw):
    return W.build_bnn_regression(W.native_api(), **kw)


def test_the_layer_pattern_lowers_to_a_latent_per_row_and_a_table_of_entries():
    p = lowered(regression(**dict(A, scale_latent="layer")))
    assert [l["name"] for l in p.scale_latents] == ["tau1", "tau2"]
    assert p.scale_latents[0]["tensors"] == [("weights1", 1.0), ("b1", 1.0)] and p.scale_latents[1]["tensors"] == [("weights2", 1.0), ("b2", 1.0)]
    assert p.n_rows == 595 and p.n_noise == 597 and p.row_latent.dtype == np.uint8 and p.row_latent.shape == (595,)
    by_name = {t["name"]: t for t in p.tensors}
    for name, want in (("weights1", 0), ("b1", 0), ("weights2", 1), ("b2", 1)):
        t = by_name[name]
        assert (p.row_latent[t["row0"]:t["row0"] + t["size"]] == want).all(), name
    assert p.summary()["scale_latents"] == {"tau1": [("weights1", 1.0), ("b1", 1.0)], "tau2": [("weights2", 1.0), ("b2", 1.0)]}
    # the table: q loc and q scale are parameter entries (the posterior's learnable roots), the prior's two are constants of their own names
    assert p.latent_uniform.shape == (4, 2) and p.latent_uniform.dtype == np.uint32
    assert (p.latent_uniform[:2] < p.n_uniform_grad).all() and (p.latent_uniform[2:] >= p.n_uniform_grad).all()
    names = {par.name: off for par, off, _, _ in p.parameters}
    for t, latent in enumerate(("tau1", "tau2")):
        loc, scale = p.uniform[p.latent_uniform[0, t]], p.uniform[p.latent_uniform[1, t]]
        assert loc["src"] == names[latent + "_loc"] and scale["src"] == names[latent + "_scale"]
        assert scale["transform"] == 1 or scale["transform"] != loc["transform"]          # (the softplus of the reference's learnable scale)
    # a row under a latent keeps its multiplier where its prior scale stood: a constant 1
    values = np.asarray(p.consts)[p.uniform["src"][p.row_uniform[3]]]
    assert (p.uniform["is_param"][p.row_uniform[3]] == 0).all() and (values == 1.0).all()


def test_a_program_without_a_scale_latent_is_what_it_was():
    p = lowered(regression(**A))
    assert p.scale_latents == () and "scale_latents" not in p.summary() and p.n_noise == p.n_rows
    assert not hasattr(p, "row_latent") and not hasattr(p, "latent_uniform")


@pytest.mark.parametrize("spelling,b", [(lambda tau: tau, 1.0), (lambda tau: 2.0 * tau, 2.0), (lambda tau: tau * 2.0, 2.0), (lambda tau: tau / 4.0, 0.25)])
def test_the_multiplier_in_its_four_spellings(spelling, b):
    p = lowered(hand_built(scale=spelling))
    assert p.scale_latents == [dict(name="tau", tensors=[("weights1", b)])] and (p.row_latent == 0).all() and p.n_noise == 65
    values = np.asarray(p.consts)[p.uniform["src"][p.row_uniform[3]]]
    assert (values == np.float32(b)).all() and (p.row_prior == D.DIST_LAPLACE).all()
    # the prior's learnable roots are parameter entries of the joint model's group
    assert (p.latent_uniform < p.n_uniform_grad).all()


def test_the_auto_created_roots_of_prior_and_posterior_share_their_entries():
    """`LogNormalVariable(-0.3, 0.7, "tau")` in the model and `LogNormalVariable(..., "tau", learnable=True)` in the posterior both create
    `tau_loc` / `tau_scale`: by the reference's name collision the posterior's parameters are the prior's"""
    p = lowered(hand_built(learnable_prior=False))
    assert (p.latent_uniform[0] == p.latent_uniform[2]).all() and (p.latent_uniform[1] == p.latent_uniform[3]).all()


def test_one_latent_may_scale_tensors_of_every_kind_and_tensors_may_stay_constant():
    from test_gpu_bnn_priors import B_MIXTURE
    p = lowered(regression(**dict(B, prior=B_MIXTURE, scale_latent=B_LATENTS)))
    assert [l["name"] for l in p.scale_latents] == ["ta", "tb", "tc", "td", "te"] and p.n_noise == p.n_rows + 5
    by_name = {t["name"]: t for t in p.tensors}
    t3 = by_name["weights3"]
    assert (p.row_latent[t3["row0"]:t3["row0"] + t3["size"]] == bnn.NO_LATENT).all()
    assert p.summary()["scale_latents"]["ta"] == [("weights1", 0.5)] and p.summary()["priors"] == B_MIXTURE
    shared = lowered(regression(**dict(A, scale_latent=dict(t=["weights1", ("b2", 3.0)]))))
    assert shared.scale_latents == [dict(name="t", tensors=[("weights1", 1.0), ("b2", 3.0)])]


REFUSALS = [
    (dict(tau_prior=lambda api: api.NormalVariable(0.5, 0.1, "tau")), "the scale latent 'tau' must be a LogNormal variable: it is Normal"),
    (dict(tau_q=lambda api: api.NormalVariable(0.5, 0.1, "tau", learnable=True)),
     "the posterior of the scale latent 'tau' must be a LogNormal variable of the same name: it is Normal"),
    (dict(tau_prior=lambda api: api.LogNormalVariable(np.zeros((3, 1)), np.ones((3, 1)), "tau"),
          tau_q=lambda api: api.LogNormalVariable(np.zeros((3, 1)), np.ones((3, 1)), "tau", learnable=True)), "the scale latent 'tau' has 3 values"),
    (dict(tau_prior=lambda api: api.LogNormalVariable(api.NormalVariable(0., 1., "hyper"), 0.7, "tau")),
     "the prior of the scale latent 'tau' depends on another latent variable"),
    (dict(scale=lambda tau: tau + 1.0), "the prior scale of 'weights1' must be its scale latent 'tau' times a number b > 0"),
    (dict(scale=lambda tau: tau * -2.0), "the prior scale of 'weights1' must be its scale latent 'tau' times a number b > 0"),
    (dict(scale=lambda tau: 2.0 / tau), "the prior scale of 'weights1' must be its scale latent 'tau' times a number b > 0"),
]


@pytest.mark.parametrize("kw,text", REFUSALS)
def test_every_new_refusal_names_the_variable_and_the_cause(kw, text):
    with pytest.raises(LoweringError, match=re.escape(text)):
        lowered(hand_built(**kw))


def test_a_tensor_scaled_by_two_latents_and_taylor1_are_refused():
    api = W.native_api()

    def two(tau):
        other = api.LogNormalVariable(0., 1., "tau_b")
        return tau * other
    with pytest.raises(LoweringError, match=re.escape("the prior scale of 'weights1' is computed from two latent variables ('tau', 'tau_b')")):
        lowered(hand_built(scale=two))
    with pytest.raises(LoweringError, match=re.escape("the Taylor1 estimator does not serve a model with scale latents ('tau')")):
        lowered(hand_built(), "taylor1")


def test_the_pinned_refusals_keep_their_text_and_fire_first():
    # a Laplace posterior on the weights, with a scale latent in the model
    with pytest.raises(LoweringError, match="the posterior must be mean-field Normal variables"):
        lowered(hand_built(weights_q="laplace"))
    # a latent that is also the likelihood's scale: today's text
    with pytest.raises(LoweringError, match=re.escape("the scale of the Normal likelihood 'y' is a latent variable or computed from one")):
        lowered(hand_built(lik_scale=lambda tau: tau))
    # a LogNormal in the posterior that scales nothing of the network is no scale latent
    with pytest.raises(LoweringError, match="the posterior must be mean-field Normal variables"):
        lowered(hand_built(scale=lambda tau: 0.3 * np.ones((2, 32))))
    # a scale latent without a posterior
    with pytest.raises(LoweringError, match=re.escape("the posterior of the scale latent 'tau' must be a LogNormal variable of the same name: it is missing")):
        lowered(hand_built(tau_q=lambda api: None))
    # another prior family
    with pytest.raises(LoweringError, match="weights and biases must be Normal, Laplace or Cauchy variables: the prior of 'weights1' is LogNormal"):
        lowered(hand_built(prior="lognormal", scale=lambda tau: 0.3 * np.ones((2, 32)), tau_q=lambda api: None))


def test_the_builders_keywords():
    api = W.native_api()
    g = lowered(W.build_bayesian_neural_network(api, **dict({k: v for k, v in CLASSIFIER.items() if k != "classifier"}, scale_latent="global")))
    assert g.summary()["scale_latents"] == {"tau": [("weights1", 1.0), ("b1", 1.0), ("weights2", 1.0), ("b2", 1.0)]} and (g.row_latent == 0).all()
    h = lowered(regression(**dict(A, scale_head="softplus", scale_latent="layer")))
    assert set(h.summary()["scale_latents"]) == {"tau1", "tau2", "tau_scale"}
    m = regression(**dict(A, scale_latent="layer", scale_latent_prior=(0.4, 0.6), scale_latent_q=(-0.2, 0.15)))
    roots = {v.name: v for v in m.flatten() if type(v).__name__ == "RootVariable"}
    assert float(np.asarray(roots["tau1_prior_loc"].value).reshape(-1)[0]) == np.float32(0.4)
    assert float(np.asarray(roots["tau2_prior_scale"].value).reshape(-1)[0]) == np.float32(0.6)
    q = {v.name: v for v in m.posterior_model.flatten()}
    assert float(np.asarray(q["tau1_loc"].parameter.numpy()).reshape(-1)[0]) == np.float32(-0.2) and q["tau1_loc"].learnable
    with pytest.raises(ValueError, match="scale_latent is None"):
        regression(**dict(A, scale_latent="column"))
    with pytest.raises(ValueError, match="names the tensor 'weights9'"):
        regression(**dict(A, scale_latent=dict(t=["weights9"])))
    # without the keywords: draw for draw what it was (the same parameters, the same data, no latent)
    a, b = lowered(regression(**A)), lowered(regression(**dict(A, scale_latent=None)))
    assert np.array_equal(a.dataset, b.dataset) and np.array_equal(a.labels, b.labels) and np.array_equal(a.row_uniform, b.row_uniform)
    assert all(np.array_equal(x[0].numpy(), y[0].numpy()) and x[0].name == y[0].name for x, y in zip(a.parameters, b.parameters))
    # ... and with them the weights' posterior starts where it started
    c = lowered(regression(**dict(A, scale_latent="layer")))
    pa, pc = {x[0].name: x[0].numpy() for x in a.parameters}, {x[0].name: x[0].numpy() for x in c.parameters}
    assert all(np.array_equal(pa[k], pc[k]) for k in ("weights1_loc", "weights1_scale", "b2_loc")) and np.array_equal(a.dataset, c.dataset)


def test_named_noise_round_trips_with_the_latents_behind_the_weights():
    p = lowered(regression(**dict(B, scale_latent=B_LATENTS)))
    shell = bnn.CompiledBnn.__new__(bnn.CompiledBnn)
    shell.program = p
    n = 7
    noise = np.random.RandomState(1).normal(size=(p.n_noise, n)).astype(np.float32)
    named = shell.named_noise(noise, n)
    assert all(named[l["name"]].shape == (n, 1, 1, 1) for l in p.scale_latents)
    assert np.array_equal(named["td"].reshape(-1), noise[p.n_rows + 3])
    assert np.array_equal(shell.noise_from_named(named, n), noise)
    # the weights' rows alone (what `predict` reports): no latent key
    assert set(shell.named_noise(noise[:p.n_rows], n)) == {t["name"] for t in p.tensors}


def test_the_export_is_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "bsvi.h")).read()
    assert "int bsvi_bnn_set_scale_latents(bsvi_bnn* b, uint32_t n_latents, const uint8_t* row_latent, uint32_t n_rows, const uint32_t* latent_uniform);" in header
    assert "[n_rows + n_latents][n_samples_local]" in header
    assert "bsvi_bnn_set_scale_latents" in native._SIGNATURES if hasattr(native, "_SIGNATURES") else "bsvi_bnn_set_scale_latents" in open(native.__file__).read()
    assert re.search(r"#define BSVI_ABI_VERSION\s+11", header) and native.ABI_VERSION == 11
    lib = os.path.join(os.path.dirname(native.__file__), "libbsvi.so")
    if os.path.exists(lib):
        import ctypes
        assert hasattr(ctypes.CDLL(lib), "bsvi_bnn_set_scale_latents")


def test_the_oracle_takes_the_model_as_written():
    """the truth of every device check: Oracle in double precision on a [N, 1, 1, 1] draw per latent; the gradient of the latent's q loc is
    the central difference of the loss at a step h = 2^-10, which a single-precision root holds exactly.  (The difference is off by
    h^2 / 6 = 1.6e-7 times the third derivative, a few times the first here — the loss reads l through exp(-l) and l itself: 1e-5
    relative.)"""
    n = 6
    rng = np.random.RandomState(3)
    p = lowered(hand_built())
    noise = {t["name"]: rng.normal(size=(n, 1, t["rows"], t["cols"])) for t in p.tensors}
    noise["tau"] = rng.normal(size=(n, 1, 1, 1))
    mb = {"indices": list(range(8))}
    exact = Oracle(hand_built(), dtype=torch.float64).loss_and_grads(n, "pathwise", noise, mb)
    assert {"tau_loc", "tau_scale", "tau_prior_loc", "tau_prior_log_scale"} <= set(exact["grads"])

    def loss_at(delta):
        m = hand_built(tau_q=lambda api: api.LogNormalVariable(-0.5 + delta, 0.3, "tau", learnable=True))
        return Oracle(m, dtype=torch.float64).loss_and_grads(n, "pathwise", noise, mb)["loss"]
    h = 2.0 ** -10
    fd = (loss_at(h) - loss_at(-h)) / (2 * h)
    print("tau_loc", float(np.asarray(exact["grads"]["tau_loc"]).reshape(-1)[0]), "central difference", fd)
    assert abs(fd - float(np.asarray(exact["grads"]["tau_loc"]).reshape(-1)[0])) <= 1e-5 * max(1.0, abs(fd))


@pytest.mark.parametrize("name", FIXTURES)
def test_the_oracle_reproduces_the_fixtures(name):
    """the real reference's record of a weight tensor under a LogNormal scale latent, and the oracle in double precision on its draws and
    minibatch within the bounds tests/test_bnn_likelihoods_cpu.py uses for its fixtures (TOL of the loss, of the largest gradient, of the
    per-sample terms); the single-precision oracle — the yardstick of the device tests — within the same bounds"""
    g = Golden(name)
    kw = g.meta["kwargs"]
    assert g.meta["builder"] == "build_bnn_regression" and kw["scale_latent"]
    p = lowered(g.build())
    assert len(p.tensors) == 1 and len(p.scale_latents) == 1 and sorted(g.noise) == sorted([p.tensors[0]["name"], p.scale_latents[0]["name"]])
    assert np.asarray(g.noise[p.scale_latents[0]["name"]]).shape == (g.N, 1, 1, 1)
    laplace = kw.get("prior") == "laplace"
    assert (g.N, p.dataset_size, p.batch_size, p.n_features) == ((5, 30, 12, 32) if laplace else (6, 24, 10, 16))
    assert p.scale_latents[0]["tensors"] == [("weights1", 2.0 if laplace else 1.0)]
    assert (p.row_prior == (D.DIST_LAPLACE if laplace else D.DIST_NORMAL)).all()
    assert (bool((p.dataset == np.round(p.dataset)).all())) == laplace                     # integer | normal features
    for estimator in ("pathwise", "blackbox", "custom_baseline", "custom_softmax"):
        assert np.isfinite(float(g.data["loss_" + estimator])) and g.group("grad_%s/" % estimator)
    assert g.meta["trajectory"]["iters"] == 4 and g.meta["trajectory"]["optimizer"] == "Adam"
    for dtype in (torch.float64, torch.float32):
        for estimator in ("pathwise", "blackbox"):
            res = Oracle(g.build(), dtype=dtype).loss_and_grads(g.N, estimator, g.noise, g.minibatch)
            ref = float(g.data["loss_" + estimator])
            assert abs(res["loss"] - ref) <= TOL * abs(ref), (dtype, estimator)
            ref_grads = g.group("grad_%s/" % estimator)
            assert {"tau_loc", "tau_scale", "weights1_loc", "weights1_scale"} <= set(ref_grads)
            scale = max(np.abs(v).max() for v in ref_grads.values())
            for pname, g_ref in ref_grads.items():
                assert np.abs(res["grads"][pname] - g_ref).max() <= TOL * scale, (dtype, estimator, pname)
        res = Oracle(g.build(), dtype=dtype).loss_and_grads(g.N, "blackbox", g.noise, g.minibatch)
        assert rel_err(res["f"], g.data["lp"] + g.data["H"]) <= TOL and rel_err(res["lq"], g.data["lq"]) <= TOL


@pytest.mark.skipif(not reference_present(), reason="the reference is only present in the build container")
def test_the_fixtures_regenerate_bit_for_bit(tmp_path):
    env = dict(os.environ, BSVI_GOLDEN_OUT=str(tmp_path), PYTHONDONTWRITEBYTECODE="1", OMP_NUM_THREADS="1")
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_golden_bnn_hier.py")], check=True, env=env,
                   stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=600)
    for name in FIXTURES:
        new, old = np.load(os.path.join(str(tmp_path), os.path.basename(name) + ".npz")), np.load(os.path.join(GOLDEN, name + ".npz"))
        assert sorted(new.files) == sorted(old.files)
        for key in old.files:
            if key == "meta":
                assert json.loads(str(new[key])) == json.loads(str(old[key]))
            else:
                assert np.array_equal(new[key], old[key], equal_nan=True), (name, key)
