"""The regression model of the Bayesian-neural-network family — an observed Normal whose loc is the matmul chain
(workloads.build_bnn_regression, bnn.lower_bnn, bsvi_bnn_create_normal) — as far as it goes without a device: what the lowering
extracts, what it refuses and why, the argument checks of the new entry point (all of them in front of the device query), and the
two reference fixtures of tests/golden/bnn_normal/ (they regenerate, and the oracle in single precision reproduces them)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, Golden, rel_err
from brancher_amd import bnn, lowering, native, workloads as W
from brancher_amd.lowering import LoweringError
from oracle.svi_oracle import Oracle

TOL = 1e-5
FIXTURES = ["bnn_normal/bnn_normal_tanh_P32_H6_C1_DS30_B12_N5", "bnn_normal/bnn_normal_linear_P16_C2_DS24_B10_N6"]
A = dict(dataset_size=40, batch_size=17, n_features=64, n_hidden=9, n_outputs=1)
B = dict(dataset_size=40, batch_size=33, n_features=36, n_hidden=5, hidden2=4, n_outputs=3, activation="relu", data="normal",
         sigma=[0.3, 0.5, 0.8])
ONE_LAYER = dict(dataset_size=24, batch_size=8, n_features=32, n_hidden=0, n_outputs=2, bias=False)
NO_BIAS = 0xFFFFFFFF


def lowered(**kw):
    model = W.build_bnn_regression(W.native_api(), **kw)
    return model, bnn.lower_bnn(model, model.posterior_model)


def sigma_of(p, c):
    """the value of sigma's uniform entry: a + b * g(constant) — a scale is stored through the inverse of its softplus"""
    e = p.uniform[p.scale_uniform + c * p.scale_stride]
    assert not e["is_param"]
    x = float(p.consts[e["src"]])
    g = {lowering.UT["identity"]: x, lowering.UT["softplus"]: float(np.log1p(np.exp(x)))}[int(e["transform"])]
    return float(e["a"]) + float(e["b"]) * g


def test_the_tanh_network_lowers_to_the_normal_likelihood_with_targets_per_row():
    model, p = lowered(**A)
    assert p.likelihood == bnn.LIK_NORMAL and p.summary()["likelihood"] == "normal"
    assert [(l["rows"], l["cols"], l["activation"]) for l in p.layers] == [(9, 64, bnn.ACTIVATIONS["tanh"]), (1, 9, 0)]
    assert all(l["bias_row0"] != NO_BIAS for l in p.layers) and p.n_rows == 9 * 64 + 9 + 9 + 1
    assert p.labels.dtype == np.float32 and p.labels.shape == (40, 1) and p.labels.flags["C_CONTIGUOUS"]
    # one sigma for every output: a constant entry (behind the entries with a gradient), stride 0
    assert p.scale_stride == 0 and p.n_uniform_grad <= p.scale_uniform < len(p.uniform)
    assert sigma_of(p, 0) == pytest.approx(0.5, rel=1e-6)
    assert p.batch_size == 17 and p.dataset_size == 40 and p.n_features == 64 and p.n_classes == 1


def test_targets_are_row_major_and_a_scale_per_output_has_stride_one():
    model, p = lowered(**B)
    assert [(l["rows"], l["cols"], l["activation"]) for l in p.layers] == [(5, 36, 2), (4, 5, 2), (3, 4, 0)]
    targets = next(v for v in model.flatten() if v.name == "y").dataset              # the EmpiricalVariable y is observed through
    Y = np.asarray(targets.link.expressions()["dataset"].expr.attr.value, dtype=np.float32).reshape(40, 3)
    assert p.labels.shape == (40, 3) and np.array_equal(p.labels.reshape(-1), Y.reshape(-1)) and p.labels.size == 40 * 3
    assert p.scale_stride == 1 and p.scale_uniform >= p.n_uniform_grad and p.scale_uniform + 2 < len(p.uniform)
    assert [sigma_of(p, c) for c in range(3)] == pytest.approx([0.3, 0.5, 0.8], rel=1e-6)


def test_one_layer_without_a_bias_is_bayesian_linear_regression():
    model, p = lowered(**ONE_LAYER)
    assert len(p.layers) == 1 and (p.layers[0]["rows"], p.layers[0]["cols"], p.layers[0]["activation"]) == (2, 32, 0)
    assert p.layers[0]["bias_row0"] == NO_BIAS and p.layers[0]["weight_row0"] == 0 and p.n_rows == 64
    assert [t["name"] for t in p.tensors] == ["weights1"] and p.labels.shape == (24, 2) and p.scale_stride == 0
    # ... and with biases the table holds them
    _, pb = lowered(**dict(ONE_LAYER, bias=True))
    assert pb.layers[0]["bias_row0"] == 64 and pb.n_rows == 66


@pytest.mark.parametrize("estimator", ["blackbox", "taylor1"])
def test_the_other_estimators_lower_too(estimator):
    model = W.build_bnn_regression(W.native_api(), **A)
    p = bnn.lower_bnn(model, model.posterior_model, estimator)
    assert p.estimator == estimator and p.likelihood == bnn.LIK_NORMAL


def refused_model(what):
    """a 16-4-2 tanh network with ONE thing the path does not serve"""
    api = W.native_api()
    BF = api.BF
    rng = np.random.RandomState(0)
    DS, Bs, P, H, Cn = 20, 6, 16, 4, 2
    X = rng.randint(-3, 4, size=(DS, P, 1)).astype(np.float32)
    Y = rng.normal(size=(DS, 3 if what == "target columns" else Cn, 1)).astype(np.float32)
    indices = api.RandomIndices(dataset_size=DS, batch_size=Bs, name="indices", is_observed=True)
    x = api.EmpiricalVariable(X, indices=indices, name="x", is_observed=True)
    targets = api.EmpiricalVariable(Y, indices=indices, name="targets", is_observed=True)
    w1 = api.NormalVariable(np.zeros((H, P)), np.ones((H, P)), "weights1")
    w2 = api.NormalVariable(np.zeros((Cn, H)), np.ones((Cn, H)), "weights2")
    loc = BF.matmul(w2, BF.tanh(BF.matmul(w1, x)))
    q = [api.NormalVariable(np.zeros((H, P)), 0.05 * np.ones((H, P)), "weights1", learnable=True),
         api.NormalVariable(np.zeros((Cn, H)), 0.1 * np.ones((Cn, H)), "weights2", learnable=True)]
    scale = 0.5
    if what == "learnable scale":
        scale = api.RootVariable(0.5, name="sigma", learnable=True)
    elif what == "latent scale":
        scale = api.LogNormalVariable(0., 0.3, "sigma")
        q.append(api.LogNormalVariable(0., 0.2, "sigma", learnable=True))
    elif what == "scale computed from a latent":
        tau = api.NormalVariable(0., 0.3, "tau")
        scale = BF.exp(tau)
        q.append(api.NormalVariable(0., 0.2, "tau", learnable=True))
    elif what == "scale shape":
        scale = np.array([[0.3], [0.5], [0.8]])
    elif what == "loc":
        loc = BF.exp(loc)
    y = api.NormalVariable(loc, scale, "y")
    model = api.ProbabilisticModel([y])
    y.observe(targets)
    model.set_posterior_model(api.ProbabilisticModel(q))
    return model


@pytest.mark.parametrize("what,cause", [("learnable scale", "is learnable"),
                                        ("latent scale", "is a latent variable or computed from one"),
                                        ("scale computed from a latent", "is a latent variable or computed from one"),
                                        ("scale shape", "neither one value nor one per output"),
                                        ("target columns", "the targets have 3 columns but the last layer has 2 rows"),
                                        ("loc", "is not a chain of matmul layers")])
def test_what_the_path_does_not_serve_is_refused_with_its_cause(what, cause):
    model = refused_model(what)
    with pytest.raises(LoweringError) as err:
        bnn.lower_bnn(model, model.posterior_model)
    assert str(err.value).startswith("bnn path: ") and cause in str(err.value)
    # ... and the same model with nothing wrong lowers
    ok = refused_model(None)
    assert bnn.lower_bnn(ok, ok.posterior_model).likelihood == bnn.LIK_NORMAL


def test_create_normal_checks_its_arguments_in_front_of_the_device_query():
    lib = native.load()
    _, p = lowered(**A)
    handle = C.c_void_p()

    def create(scale_uniform, scale_stride, **change):
        d, keep = bnn.make_desc(p)
        for k, v in change.items():
            setattr(d, k, v)
        rc = lib.bsvi_bnn_create_normal(C.byref(d), scale_uniform, scale_stride, C.byref(handle))
        return rc, lib.bsvi_last_error()

    rc, msg = create(p.scale_uniform, p.scale_stride, struct_size=C.sizeof(native.BnnDesc) - 8)
    assert rc == -1 and b"bsvi_bnn_desc" in msg and not handle.value                                   # BSVI_ERR_INVALID
    rc, msg = create(len(p.uniform), 0)
    assert rc == -1 and b"scale entry out of the uniform table" in msg and not handle.value
    rc, msg = create(0, 0)                                                                              # entry 0 is a parameter's
    assert p.n_uniform_grad > 0 and rc == -2 and b"constant" in msg and not handle.value               # BSVI_ERR_UNSUPPORTED
    rc, msg = create(p.scale_uniform, 2)
    assert rc == -1 and b"scale_stride" in msg
    rc, msg = create(p.scale_uniform, 0, likelihood=bnn.LIK_CATEGORICAL)
    assert rc == -1 and b"BSVI_LIK_NORMAL" in msg
    rc, msg = create(p.scale_uniform, 0, abi_version=native.ABI_VERSION + 1)
    assert rc == -1 and b"ABI" in msg
    assert lib.bsvi_bnn_create_normal(None, 0, 0, C.byref(handle)) == -1
    # a scale per output whose LAST entry lies beyond the table
    _, pb = lowered(**B)
    d, keep = bnn.make_desc(pb)
    assert lib.bsvi_bnn_create_normal(C.byref(d), len(pb.uniform) - 2, 1, C.byref(handle)) == -1
    assert b"scale entry out of the uniform table" in lib.bsvi_last_error()


def test_the_classifiers_entry_point_refuses_the_normal_likelihood_and_names_the_new_one():
    lib = native.load()
    _, p = lowered(**A)
    d, keep = bnn.make_desc(p)
    handle = C.c_void_p()
    assert d.likelihood == 2 and lib.bsvi_bnn_create(C.byref(d), C.byref(handle)) == -2 and not handle.value
    assert b"bsvi_bnn_create_normal" in lib.bsvi_last_error()
    assert native.ABI_VERSION == 11 and lib.bsvi_abi_version() == 11


def reference_present():
    from oracle import gen_golden                      # (where the generator looks for the reference)
    return os.path.isdir(os.path.join(gen_golden.REF, "brancher"))


needs_reference = pytest.mark.skipif(not reference_present(), reason="the reference is only present in the build container")


@needs_reference
def test_the_fixtures_regenerate_bit_for_bit(tmp_path):
    env = dict(os.environ, BSVI_GOLDEN_OUT=str(tmp_path), PYTHONDONTWRITEBYTECODE="1", OMP_NUM_THREADS="1")
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_golden_bnn_normal.py")], check=True, env=env,
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
def test_the_oracle_in_single_precision_reproduces_the_fixtures(name):
    g = Golden(name)
    assert g.meta["builder"] == "build_bnn_regression" and g.meta["posterior_order"] == "sorted by name"
    for estimator in ("pathwise", "blackbox", "taylor1"):
        res = Oracle(g.build()).loss_and_grads(g.N, estimator, g.noise, g.minibatch)
        ref = float(g.data["loss_" + estimator])
        assert abs(res["loss"] - ref) <= TOL * abs(ref), estimator
        ref_grads = g.group("grad_%s/" % estimator)
        scale = max(np.abs(v).max() for v in ref_grads.values())
        for pname, g_ref in ref_grads.items():
            assert np.abs(res["grads"][pname] - g_ref).max() <= TOL * scale, (estimator, pname)
    res = Oracle(g.build()).loss_and_grads(g.N, "blackbox", g.noise, g.minibatch)
    assert rel_err(res["f"], g.data["lp"] + g.data["H"]) <= TOL and rel_err(res["lq"], g.data["lq"]) <= TOL
    tr = g.meta["trajectory"]
    oracle = Oracle(g.build())
    losses = oracle.train(tr["iters"], tr["n"], tr["optimizer"], "pathwise", g.trajectory_noise(),
                          minibatch_seq=g.trajectory_minibatch(), **g.opt_kwargs())
    assert tr["optimizer"] == "Adam" and rel_err(losses, g.data["traj/losses"]) <= TOL
    after = g.group("traj/param_after/")
    for pname, par in oracle.named_parameters().items():
        assert np.abs(par.detach().numpy() - after[pname]).max() <= 1e-5 * (1 + np.abs(after[pname]).max()), pname
