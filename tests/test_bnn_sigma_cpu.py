"""A learnable sigma of the Normal likelihood of the Bayesian-neural-network family (workloads.build_bnn_regression(learnable_sigma=...),
bnn._normal_scale, bsvi_bnn_create_normal_learnable) as far as it goes without a device: the forms the lowering accepts and what it
records, what it keeps refusing and why, the argument checks of the new entry point (all of them in front of the device query), the
two reference fixtures of tests/golden/bnn_sigma/ under the oracle, and that the builder without its new keyword builds what it built."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, Golden, rel_err
from brancher_amd import bnn, lowering, native, workloads as W
from brancher_amd.lowering import LoweringError
from oracle.svi_oracle import Oracle

TOL = 1e-5
FIXTURES = ["bnn_sigma/bnn_sigma_tanh_P32_H6_C1_DS30_B12_N5", "bnn_sigma/bnn_sigma_linear_P16_C2_DS24_B10_N6"]
NORMAL_FIXTURES = ["bnn_normal/bnn_normal_tanh_P32_H6_C1_DS30_B12_N5", "bnn_normal/bnn_normal_linear_P16_C2_DS24_B10_N6"]
A = dict(dataset_size=40, batch_size=17, n_features=64, n_hidden=9, n_outputs=1)
B = dict(dataset_size=40, batch_size=33, n_features=36, n_hidden=5, hidden2=4, n_outputs=3, activation="relu", data="normal",
         sigma=[0.3, 0.5, 0.8])


def sigma_model(form, per_output=False, n_outputs=2):
    """a 16-4-2 tanh network without biases whose noise scale has the given form (tests/test_bnn_normal_cpu.py: refused_model)"""
    api = W.native_api()
    BF = api.BF
    rng = np.random.RandomState(0)
    DS, Bs, P, H, Cn = 20, 6, 16, 4, n_outputs
    X = rng.randint(-3, 4, size=(DS, P, 1)).astype(np.float32)
    Y = rng.normal(size=(DS, Cn, 1)).astype(np.float32)
    indices = api.RandomIndices(dataset_size=DS, batch_size=Bs, name="indices", is_observed=True)
    x = api.EmpiricalVariable(X, indices=indices, name="x", is_observed=True)
    targets = api.EmpiricalVariable(Y, indices=indices, name="targets", is_observed=True)
    start = np.linspace(0.5, 0.8, Cn).reshape(Cn, 1) if per_output else 0.5
    if form == "shape":
        start = np.array([[0.3], [0.5], [0.8]])
    learnable, w2_scale = False, np.ones((Cn, H))
    q = []
    if form == "flag":
        scale, learnable = start, True
    elif form == "shape":
        scale, learnable = start, True
    elif form == "exp":
        scale = BF.exp(api.RootVariable(np.log(start), "log_s", learnable=True))
    elif form == "offset softplus":
        scale = 0.1 + BF.softplus(api.RootVariable(np.log(np.expm1(np.asarray(start) - 0.1)), "s_raw", learnable=True))
    elif form == "sigmoid":
        scale = 2.0 * BF.sigmoid(api.RootVariable(np.zeros_like(np.asarray(start, dtype=np.float64)) - 1.0, "s_logit", learnable=True))
    elif form == "negative factor":
        scale = 1.5 - BF.sigmoid(api.RootVariable(0.0, "s_logit", learnable=True))
    elif form == "bare":
        scale = api.RootVariable(0.5, name="sigma", learnable=True)
    elif form == "shared":          # ONE root: the prior scale of weights2 and the noise scale
        scale = BF.exp(api.RootVariable(np.log(0.5), "log_s", learnable=True))
        w2_scale = scale
    elif form == "latent":
        scale = api.LogNormalVariable(0., 0.3, "sigma")
        q.append(api.LogNormalVariable(0., 0.2, "sigma", learnable=True))
    else:
        scale = 0.5
    w1 = api.NormalVariable(np.zeros((H, P)), np.ones((H, P)), "weights1")
    w2 = api.NormalVariable(np.zeros((Cn, H)), w2_scale, "weights2")
    loc = BF.matmul(w2, BF.tanh(BF.matmul(w1, x)))
    q += [api.NormalVariable(0.02 * rng.normal(size=(H, P)), 0.05 * np.ones((H, P)), "weights1", learnable=True),
          api.NormalVariable(0.05 * rng.normal(size=(Cn, H)), 0.1 * np.ones((Cn, H)), "weights2", learnable=True)]
    y = api.NormalVariable(loc, scale, "y", learnable=learnable)
    model = api.ProbabilisticModel([y])
    y.observe(targets)
    model.set_posterior_model(api.ProbabilisticModel(q))
    return model


def sigma_entries(p, theta=None):
    """(sigma [C], d sigma / d theta [C], the parameter's name) of a lowered program with a learnable scale, in double precision"""
    sig, dsig, name = [], [], None
    by_offset = {off + i: (par, i) for par, off, size, _ in p.parameters for i in range(size)}
    for c in range(p.n_classes):
        e = p.uniform[p.scale_uniform + c * p.scale_stride]
        assert e["is_param"]
        par, i = by_offset[int(e["src"])]
        x = float(par.numpy().reshape(-1)[i]) if theta is None else float(np.asarray(theta[par.name]).reshape(-1)[i])
        name = par.name
        t = int(e["transform"])
        g, dg = {lowering.UT["softplus"]: (np.log1p(np.exp(x)), 1.0 / (1.0 + np.exp(-x))), lowering.UT["exp"]: (np.exp(x), np.exp(x)),
                 lowering.UT["sigmoid"]: (1.0 / (1.0 + np.exp(-x)), np.exp(-x) / (1.0 + np.exp(-x)) ** 2)}[t]
        sig.append(float(e["a"]) + float(e["b"]) * g)
        dsig.append(float(e["b"]) * dg)
    return np.array(sig), np.array(dsig), name


@pytest.mark.parametrize("per_output", [False, True], ids=["one sigma", "a sigma per output"])
@pytest.mark.parametrize("form,root,transform,a", [("flag", "y_scale", "softplus", 0.0), ("exp", "log_s", "exp", 0.0),
                                                   ("offset softplus", "s_raw", "softplus", 0.1), ("sigmoid", "s_logit", "sigmoid", 0.0)])
def test_the_accepted_forms_lower_to_parameter_entries_of_the_joint_models_group(form, root, transform, a, per_output):
    model = sigma_model(form, per_output)
    p = bnn.lower_bnn(model, model.posterior_model)
    assert p.likelihood == bnn.LIK_NORMAL and p.scale_learnable and p.summary()["scale"] == "learnable"
    assert p.scale_stride == (1 if per_output else 0)
    last = p.scale_uniform + p.scale_stride * (p.n_classes - 1)
    assert 0 <= p.scale_uniform and last < p.n_uniform_grad
    for c in range(p.n_classes):
        e = p.uniform[p.scale_uniform + c * p.scale_stride]
        assert e["is_param"] and int(e["transform"]) == lowering.UT[transform] and float(e["a"]) == pytest.approx(a) and float(e["b"]) > 0
    (par, off, size, group), = [t for t in p.parameters if t[0].name == root]
    assert group == 1 and size == (p.n_classes if per_output else 1) and int(p.uniform[p.scale_uniform]["src"]) == off
    assert p.param_active[off:off + size].all() and (p.param_group[off:off + size] == 1).all()
    # ... every other parameter is the posterior's: group 0, stepped from iteration 0
    assert all(g == 0 for t in p.parameters if t[0].name != root for g in [t[3]])
    sig, dsig, name = sigma_entries(p)
    want = np.linspace(0.5, 0.8, p.n_classes) if per_output else np.full(p.n_classes, 0.5)
    if form == "sigmoid":
        want = np.full(p.n_classes, 2.0 / (1.0 + np.e))
    assert name == root and sig == pytest.approx(want, rel=1e-6) and (dsig > 0).all()


def test_a_constant_scale_says_so_and_lowers_as_before():
    model = sigma_model(None)
    p = bnn.lower_bnn(model, model.posterior_model)
    assert not p.scale_learnable and p.summary()["scale"] == "constant" and p.scale_uniform >= p.n_uniform_grad
    model = W.build_bayesian_neural_network(W.native_api(), dataset_size=40, batch_size=17, n_features=64, n_hidden=9, n_classes=3)
    assert "scale" not in bnn.lower_bnn(model, model.posterior_model).summary()


def test_one_root_as_a_prior_scale_and_as_sigma_is_one_entry():
    model = sigma_model("shared")
    p = bnn.lower_bnn(model, model.posterior_model)
    t = next(t for t in p.tensors if t["name"] == "weights2")
    prior_scale_entries = set(p.row_uniform[3, t["row0"]:t["row0"] + t["size"]].tolist())
    assert p.scale_learnable and prior_scale_entries == {p.scale_uniform}


@pytest.mark.parametrize("form,cause", [("bare", "is learnable"), ("negative factor", "is learnable"),
                                        ("latent", "is a latent variable or computed from one"),
                                        ("shape", "neither one value nor one per output")])
def test_what_stays_refused_is_refused_with_its_cause(form, cause):
    model = sigma_model(form)
    with pytest.raises(LoweringError) as err:
        bnn.lower_bnn(model, model.posterior_model)
    assert str(err.value).startswith("bnn path: ") and cause in str(err.value)
    if form == "bare":
        assert "softplus / exp / sigmoid" in str(err.value)          # the message names the accepted forms


def test_create_normal_learnable_checks_its_arguments_in_front_of_the_device_query():
    lib = native.load()
    model = sigma_model("flag", per_output=True)
    p = bnn.lower_bnn(model, model.posterior_model)
    handle = C.c_void_p()
    INVALID, UNSUPPORTED = -1, -2

    def create(scale_uniform, scale_stride, program=p, uniform=None, **change):
        d, keep = bnn.make_desc(program)
        if uniform is not None:
            keep["uniform"] = uniform
            d.uniform = uniform.ctypes.data_as(C.c_void_p)
        for k, v in change.items():
            setattr(d, k, v)
        rc = lib.bsvi_bnn_create_normal_learnable(C.byref(d), scale_uniform, scale_stride, C.byref(handle))
        return rc, lib.bsvi_last_error()

    assert p.n_classes == 2 and p.scale_stride == 1 and p.scale_uniform + 1 < p.n_uniform_grad
    rc, msg = create(p.scale_uniform, 1, struct_size=C.sizeof(native.BnnDesc) - 8)
    assert rc == INVALID and b"bsvi_bnn_desc" in msg and not handle.value
    # constants only — the 36-5-4-3 network with its three constant sigmas: that is the sibling's model
    mc = W.build_bnn_regression(W.native_api(), **B)
    pc = bnn.lower_bnn(mc, mc.posterior_model)
    assert pc.scale_uniform == pc.n_uniform_grad and pc.scale_uniform + 3 == len(pc.uniform)
    rc, msg = create(pc.scale_uniform, 1, program=pc)
    assert rc == INVALID and b"constants" in msg and b"bsvi_bnn_create_normal" in msg and not handle.value
    # the last parameter entry and the first two constants
    rc, msg = create(pc.n_uniform_grad - 1, 1, program=pc)
    assert rc == INVALID and b"mix of constants and parameters" in msg and not handle.value
    # a parameter behind the identity (entry 0 is a posterior loc)
    assert int(p.uniform[0]["transform"]) == lowering.UT["identity"] and p.uniform[0]["is_param"]
    rc, msg = create(0, 0)
    assert rc == UNSUPPORTED and b"softplus, exp or sigmoid" in msg and not handle.value
    uni = p.uniform.copy()
    uni["transform"][p.scale_uniform + 1] = lowering.UT["identity"]
    rc, msg = create(p.scale_uniform, 1, uniform=np.ascontiguousarray(uni))
    assert rc == UNSUPPORTED and b"softplus, exp or sigmoid" in msg
    rc, msg = create(p.scale_uniform, 2)
    assert rc == INVALID and b"scale_stride" in msg
    rc, msg = create(len(p.uniform) - 1, 1)                                 # a last entry beyond the table
    assert rc == INVALID and b"scale entry out of the uniform table" in msg
    rc, msg = create(len(p.uniform), 0)
    assert rc == INVALID and b"scale entry out of the uniform table" in msg
    rc, msg = create(p.scale_uniform, 1, likelihood=bnn.LIK_CATEGORICAL)
    assert rc == INVALID and b"bsvi_bnn_create_normal_learnable takes likelihood BSVI_LIK_NORMAL" in msg
    rc, msg = create(p.scale_uniform, 1, abi_version=native.ABI_VERSION + 1)
    assert rc == INVALID and b"ABI" in msg
    assert lib.bsvi_bnn_create_normal_learnable(None, 0, 0, C.byref(handle)) == INVALID
    # ... and the sibling refuses these entries as it did; no struct changed
    d, keep = bnn.make_desc(p)
    assert lib.bsvi_bnn_create_normal(C.byref(d), p.scale_uniform, 1, C.byref(handle)) == UNSUPPORTED and b"constant" in lib.bsvi_last_error()
    assert native.ABI_VERSION == 11 and lib.bsvi_abi_version() == 11


def test_the_builder_without_the_keyword_builds_what_it_built():
    """program for program: the default is learnable_sigma=False; the learnable model differs from it in sigma's entry alone — the same
    dataset, targets, row tables and posterior parameters, draw for draw; and the parameters the constant-sigma fixtures recorded
    from this builder are the ones it yields today"""
    for kw in (A, B):
        model = W.build_bnn_regression(W.native_api(), **kw)
        p = bnn.lower_bnn(model, model.posterior_model)
        m2 = W.build_bnn_regression(W.native_api(), learnable_sigma=False, **kw)
        p2 = bnn.lower_bnn(m2, m2.posterior_model)
        assert not p.scale_learnable and (p.scale_uniform, p.scale_stride) == (p2.scale_uniform, p2.scale_stride)
        for name in ("uniform", "consts", "row_uniform", "dataset", "labels", "param_uniform_ptr", "param_uniform_idx"):
            assert np.array_equal(getattr(p, name), getattr(p2, name)), name
        for form in (True, "exp"):
            m3 = W.build_bnn_regression(W.native_api(), learnable_sigma=form, **kw)
            p3 = bnn.lower_bnn(m3, m3.posterior_model)
            assert p3.scale_learnable and p3.n_params == p.n_params + (1 if np.ndim(kw.get("sigma", 0.5)) == 0 else p.n_classes)
            assert np.array_equal(p3.dataset, p.dataset) and np.array_equal(p3.labels, p.labels) and p3.layers == p.layers
            old = {par.name: par.numpy() for par, _, _, _ in p.parameters}
            new = {par.name: par.numpy() for par, _, _, _ in p3.parameters}
            assert set(new) - set(old) == {"y_scale" if form is True else "y_log_scale"}
            assert all(np.array_equal(old[k], new[k]) for k in old)
            sig, _, _ = sigma_entries(p3)
            assert sig == pytest.approx(np.broadcast_to(np.asarray(kw.get("sigma", 0.5), dtype=np.float64), (p.n_classes,)), rel=1e-6)
    for name in NORMAL_FIXTURES:
        g = Golden(name)
        model = g.build()
        for v in model.posterior_model.flatten():
            if getattr(v, "learnable", False) and "param/" + v.name in g.data.files:
                assert np.array_equal(np.asarray(v.parameter.numpy(), dtype=np.float32).reshape(-1), g.data["param/" + v.name].reshape(-1)), v.name
    with pytest.raises(ValueError):
        W.build_bnn_regression(W.native_api(), sigma_init=0.4)
    with pytest.raises(ValueError):
        W.build_bnn_regression(W.native_api(), learnable_sigma="log")


def reference_present():
    from oracle import gen_golden                      # (where the generator looks for the reference)
    return os.path.isdir(os.path.join(gen_golden.REF, "brancher"))


needs_reference = pytest.mark.skipif(not reference_present(), reason="the reference is only present in the build container")


@needs_reference
def test_the_fixtures_regenerate_bit_for_bit(tmp_path):
    env = dict(os.environ, BSVI_GOLDEN_OUT=str(tmp_path), PYTHONDONTWRITEBYTECODE="1", OMP_NUM_THREADS="1")
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_golden_bnn_sigma.py")], check=True, env=env,
                   stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=600)
    for name in FIXTURES:
        new, old = np.load(os.path.join(str(tmp_path), os.path.basename(name) + ".npz")), np.load(os.path.join(GOLDEN, name + ".npz"))
        assert sorted(new.files) == sorted(old.files)
        for key in old.files:
            if key == "meta":
                assert json.loads(str(new[key])) == json.loads(str(old[key]))
            else:
                assert np.array_equal(new[key], old[key], equal_nan=True), (name, key)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["single", "double"])
@pytest.mark.parametrize("name", FIXTURES)
def test_the_oracle_reproduces_the_fixtures(name, dtype):
    """the bounds of tests/test_bnn_normal_cpu.py for its own fixtures; `y_scale` is among the gradients and the parameters"""
    g = Golden(name)
    assert g.meta["builder"] == "build_bnn_regression" and g.meta["kwargs"]["learnable_sigma"] is True
    for estimator in ("pathwise", "blackbox", "taylor1"):
        res = Oracle(g.build(), dtype=dtype).loss_and_grads(g.N, estimator, g.noise, g.minibatch)
        ref = float(g.data["loss_" + estimator])
        assert abs(res["loss"] - ref) <= TOL * abs(ref), estimator
        ref_grads = g.group("grad_%s/" % estimator)
        assert "y_scale" in ref_grads and np.abs(ref_grads["y_scale"]).min() > 0
        scale = max(np.abs(v).max() for v in ref_grads.values())
        for pname, g_ref in ref_grads.items():
            assert np.abs(res["grads"][pname] - g_ref).max() <= TOL * scale, (estimator, pname)
    # log q does not depend on sigma: the two estimators' gradients of its root are one number
    assert np.array_equal(g.data["grad_pathwise/y_scale"], g.data["grad_blackbox/y_scale"])
    res = Oracle(g.build(), dtype=dtype).loss_and_grads(g.N, "blackbox", g.noise, g.minibatch)
    assert rel_err(res["f"], g.data["lp"] + g.data["H"]) <= TOL and rel_err(res["lq"], g.data["lq"]) <= TOL
    tr = g.meta["trajectory"]
    oracle = Oracle(g.build(), dtype=dtype)
    losses = oracle.train(tr["iters"], tr["n"], tr["optimizer"], "pathwise", g.trajectory_noise(),
                          minibatch_seq=g.trajectory_minibatch(), **g.opt_kwargs())
    assert tr["optimizer"] == "Adam" and rel_err(losses, g.data["traj/losses"]) <= TOL
    after = g.group("traj/param_after/")
    for pname, par in oracle.named_parameters().items():
        assert np.abs(par.detach().numpy() - after[pname]).max() <= 1e-5 * (1 + np.abs(after[pname]).max()), pname
    # the joint model's group is stepped from iteration 1 on: sigma's root has moved by the end
    assert np.abs(after["y_scale"] - g.data["param/y_scale"]).min() > 1e-3
