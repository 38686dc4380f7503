"""A scale head on the Normal likelihood of the Bayesian-neural-network family (workloads.build_bnn_regression(scale_head=...),
bnn.lower_bnn, bsvi_bnn_create_normal_heads) as far as it goes without a device: the forms the lowering accepts and the layout it
records (to the library the two heads are ONE last layer of 2 C rows), every new refusal with its cause and the three old "latent"
refusals with their text, the argument checks of the new entry point (all of them in front of the device query), the oracle on the
builder's model in single and double precision, and that the builder without its new keyword builds what it built."""
import ctypes as C

import numpy as np
import pytest
import torch

from brancher_amd import bnn, distributions as D, lowering, native, workloads as W
from brancher_amd.lowering import LoweringError
from oracle.svi_oracle import Oracle
from test_bnn_normal_cpu import refused_model
from test_bnn_sigma_cpu import sigma_model

KW = dict(dataset_size=24, batch_size=9, n_features=32, n_hidden=5, n_outputs=2)
OLD_TEXT = "is a latent variable or computed from one (it must be a constant of the model)"


def lower(**kw):
    model = W.build_bnn_regression(W.native_api(), **dict(KW, **kw))
    return bnn.lower_bnn(model, model.posterior_model)


def heads_model(what=None, transform="softplus", a=0.05, b=1.0, bias=True):
    """a 16-4-(2+2) tanh network with two heads, and ONE thing about them that the path does not serve"""
    api = W.native_api()
    BF = api.BF
    rng = np.random.RandomState(0)
    DS, Bs, P, H, Cn = 20, 6, 16, 4, 2
    X = rng.randint(-3, 4, size=(DS, P, 1)).astype(np.float32)
    Y = rng.normal(size=(DS, 3 if what == "target columns" else Cn, 1)).astype(np.float32)
    indices = api.RandomIndices(dataset_size=DS, batch_size=Bs, name="indices", is_observed=True)
    x = api.EmpiricalVariable(X, indices=indices, name="x", is_observed=True)
    targets = api.EmpiricalVariable(Y, indices=indices, name="targets", is_observed=True)
    shapes = dict(weights1=(H, P), b1=(H, 1), weights_loc=(Cn, H), b_loc=(Cn, 1), weights_scale=(3 if what == "scale rows" else Cn, H),
                  b_scale=(3 if what == "scale rows" else Cn, 1), weights1b=(H, P))
    if not bias:
        del shapes["b_loc"], shapes["b_scale"]
    prior = {k: api.NormalVariable(np.zeros(s), np.ones(s), k) for k, s in shapes.items()}
    hidden = BF.tanh(BF.matmul(prior["weights1"], x) + prior["b1"])
    other = BF.tanh(BF.matmul(prior["weights1b"], x) + prior["b1"]) if what == "trunks" else \
        BF.relu(BF.matmul(prior["weights1"], x) + prior["b1"]) if what == "trunk activation" else hidden
    loc = BF.matmul(prior["weights_loc"], hidden)
    raw = BF.matmul(prior["weights_loc" if what == "reused by both heads" else "weights_scale"], other)
    used = ["weights1", "b1", "weights_loc", "weights_scale"] + (["weights1b"] if what == "trunks" else [])
    if what == "reused by both heads":
        used.remove("weights_scale")
    if bias:
        loc = loc + prior["b1" if what == "reused in the trunk" else "b_loc"]
        if what != "reused in the trunk":
            used.append("b_loc")
        if what != "one bias":
            raw = raw + prior["b_scale"]
            used.append("b_scale")
    if what == "tanh":
        scale = a + b * BF.tanh(raw)
    elif what == "bare":
        scale = raw
    elif what == "square":
        scale = a + raw * raw
    else:
        scale = a + b * getattr(BF, transform)(raw) if (a, b) != (0.0, 1.0) else getattr(BF, transform)(raw)
    y = api.NormalVariable(loc, scale, "y")
    model = api.ProbabilisticModel([y])
    y.observe(targets)
    model.set_posterior_model(api.ProbabilisticModel(
        [api.NormalVariable(0.02 * rng.normal(size=shapes[k]), 0.05 * np.ones(shapes[k]), k, learnable=True) for k in used]))
    return model


@pytest.mark.parametrize("bias", [True, False], ids=["biases", "no biases"])
@pytest.mark.parametrize("transform,a,b", [("softplus", 0.05, 1.0), ("exp", 0.0, 1.0), ("sigmoid", 0.1, 2.0)])
def test_the_accepted_forms_lower_to_one_last_layer_of_2c_rows(transform, a, b, bias):
    model = heads_model(None, transform, a, b, bias)
    p = bnn.lower_bnn(model, model.posterior_model)
    assert p.likelihood == bnn.LIK_NORMAL and not p.scale_learnable and p.summary()["scale"] == "head"
    g, pa, pb = p.scale_head
    assert g == transform and pa == pytest.approx(a) and pb == pytest.approx(b)
    assert p.n_classes == 2 and p.labels.shape == (20, 2)
    last = p.layers[-1]
    assert (last["rows"], last["cols"]) == (4, 4) and p.summary()["layers"][-1] == (4, 4, 0)
    names = [t["name"] for t in p.tensors]
    assert names == ["weights1", "b1", "weights_loc", "weights_scale"] + (["b_loc", "b_scale"] if bias else [])
    by = {t["name"]: t for t in p.tensors}
    # adjacent in the latent vector: weights_loc | weights_scale is a row-major [2 C, cols] block, b_loc | b_scale the column behind it
    assert last["weight_row0"] == by["weights_loc"]["row0"] and by["weights_scale"]["row0"] == by["weights_loc"]["row0"] + 2 * 4
    assert (last["weights"], last["weights_scale"]) == ("weights_loc", "weights_scale")
    if bias:
        assert last["bias_row0"] == by["b_loc"]["row0"] and by["b_scale"]["row0"] == by["b_loc"]["row0"] + 2
        assert (last["bias"], last["bias_scale"]) == ("b_loc", "b_scale")
    else:
        assert last["bias_row0"] == bnn.NO_BIAS and last["bias"] is None and last["bias_scale"] is None
    assert p.n_rows == sum(t["size"] for t in p.tensors) and p.row_uniform.shape == (4, p.n_rows)
    # four posterior parameters of the heads' own names (group 0: stepped from the first iteration)
    par = {t[0].name: t for t in p.parameters}
    assert {"weights_scale_loc", "weights_scale_scale", "weights_loc_loc", "weights_loc_scale"} <= set(par)
    assert all(t[3] == 0 for t in p.parameters)


def test_the_builders_models_lower_with_a_row_prior_per_tensor():
    p = lower(scale_head="softplus", prior={"weights_scale": "laplace"})
    assert [t["name"] for t in p.tensors] == ["weights1", "b1", "weights2", "weights_scale", "b2", "b_scale"]
    assert p.scale_head == ("softplus", 0.05, 1.0) and p.n_classes == 2 and p.layers[-1]["rows"] == 4
    for t in p.tensors:
        kind = D.DIST_LAPLACE if t["name"] == "weights_scale" else D.DIST_NORMAL
        assert (p.row_prior[t["row0"]:t["row0"] + t["size"]] == kind).all() and t["prior"] == bnn.PRIOR_KINDS[kind]
    assert p.summary()["priors"]["weights_scale"] == "laplace"
    # the one-layer form: H is x itself, the heads are the first (and last) layer
    p1 = lower(n_hidden=0, bias=False, scale_head="exp", scale_floor=0.0)
    assert [t["name"] for t in p1.tensors] == ["weights1", "weights_scale"] and p1.scale_head == ("exp", 0.0, 1.0)
    assert len(p1.layers) == 1 and (p1.layers[0]["rows"], p1.layers[0]["cols"], p1.layers[0]["weight_row0"]) == (4, 32, 0) and p1.n_rows == 128
    p1b = lower(n_hidden=0, scale_head="sigmoid", scale_floor=0.1)
    assert [t["name"] for t in p1b.tensors] == ["weights1", "weights_scale", "b1", "b_scale"] and p1b.layers[0]["bias_row0"] == 128
    # three layers, and the named noise goes back and forth through the four tensors' own names
    p3 = lower(widths=[36, 5, 4, 3], scale_head="exp")
    assert p3.summary()["layers"] == [(5, 36, 1), (4, 5, 1), (6, 4, 0)] and p3.n_classes == 3
    eng = bnn.CompiledBnn.__new__(bnn.CompiledBnn)
    eng.program = p3
    noise = np.arange(p3.n_rows * 2, dtype=np.float32).reshape(p3.n_rows, 2)
    named = eng.named_noise(noise, 2)
    assert named["weights_scale"].shape == (2, 1, 3, 4) and named["b_scale"].shape == (2, 1, 3, 1)
    assert np.array_equal(eng.noise_from_named(named, 2), noise)


@pytest.mark.parametrize("what,cause", [
    ("trunks", "stand on different trunks"), ("trunk activation", "stand on different trunks"),
    ("one bias", "has a bias and the other has none"),
    ("tanh", "the transform of the scale head of the Normal likelihood 'y' is BF.tanh"),
    ("bare", "the transform of the scale head of the Normal likelihood 'y' is missing"),
    ("square", "the transform of the scale head"),
    ("negative a", "has a = -0.1, b = 1"), ("zero b", "has a = 0.05, b = 0"), ("negative b", "has a = 0.05, b = -1"),
    ("reused by both heads", "the head tensor 'weights_loc' of the Normal likelihood 'y' is used twice"),
    ("reused in the trunk", "the head tensor 'b1' of the Normal likelihood 'y' is used twice"),
    ("scale rows", "the targets have 2 columns but the heads of the Normal likelihood 'y' have 2 (loc) and 3 (scale) rows"),
    ("target columns", "the targets have 3 columns but the heads of the Normal likelihood 'y' have 2 (loc) and 2 (scale) rows")])
def test_every_new_refusal_names_its_cause(what, cause):
    ab = {"negative a": (-0.1, 1.0), "zero b": (0.05, 0.0), "negative b": (0.05, -1.0)}.get(what, (0.05, 1.0))
    model = heads_model(what, a=ab[0], b=ab[1])
    with pytest.raises(LoweringError) as err:
        bnn.lower_bnn(model, model.posterior_model)
    assert str(err.value).startswith("bnn path: ") and cause in str(err.value), str(err.value)
    if what in ("tanh", "negative a"):
        assert "softplus / exp / sigmoid" in str(err.value) and "a >= 0 and b > 0" in str(err.value)      # the accepted form is named


def test_the_three_old_latent_refusals_keep_their_text():
    for model in (refused_model("latent scale"), refused_model("scale computed from a latent"), sigma_model("latent")):
        with pytest.raises(LoweringError) as err:
            bnn.lower_bnn(model, model.posterior_model)
        assert str(err.value) == "bnn path: the scale of the Normal likelihood 'y' " + OLD_TEXT


def test_create_normal_heads_checks_its_arguments_in_front_of_the_device_query():
    lib = native.load()
    assert "bsvi_bnn_create_normal_heads" in native.EXPORTS and hasattr(lib, "bsvi_bnn_create_normal_heads")
    p = lower(scale_head="softplus")
    handle = C.c_void_p()
    INVALID, UNSUPPORTED = -1, -2
    SOFTPLUS = lowering.UT["softplus"]

    def create(transform=SOFTPLUS, a=0.05, b=1.0, program=p, rows=None, **change):
        d, keep = bnn.make_desc(program)
        if rows is not None:
            keep["layers"][len(program.layers) - 1].rows = rows
        for k, v in change.items():
            setattr(d, k, v)
        rc = lib.bsvi_bnn_create_normal_heads(C.byref(d), transform, a, b, C.byref(handle))
        return rc, lib.bsvi_last_error()

    rc, msg = create(struct_size=C.sizeof(native.BnnDesc) - 8)
    assert rc == INVALID and b"bsvi_bnn_desc" in msg and not handle.value
    for t in ("identity", "log", "tanh", "sqrt", "square"):
        rc, msg = create(transform=lowering.UT[t])
        assert rc == UNSUPPORTED and b"softplus, exp or sigmoid" in msg and b"bsvi_bnn_create_normal_heads" in msg and not handle.value
    rc, msg = create(transform=99)
    assert rc == UNSUPPORTED
    for a, b in ((-0.1, 1.0), (0.05, 0.0), (0.05, -1.0), (float("nan"), 1.0), (0.05, float("inf")), (float("inf"), 1.0), (0.05, float("nan"))):
        rc, msg = create(a=a, b=b)
        assert rc == INVALID and b"a >= 0 and b > 0" in msg and not handle.value, (a, b)
    rc, msg = create(rows=3)
    assert rc == INVALID and b"odd number of rows" in msg and not handle.value
    rc, msg = create(likelihood=bnn.LIK_CATEGORICAL)
    assert rc == INVALID and b"bsvi_bnn_create_normal_heads takes likelihood BSVI_LIK_NORMAL" in msg
    rc, msg = create(abi_version=native.ABI_VERSION + 1)
    assert rc == INVALID and b"ABI" in msg
    assert lib.bsvi_bnn_create_normal_heads(None, SOFTPLUS, 0.05, 1.0, C.byref(handle)) == INVALID
    # every check passed: what is left is the device query (or a handle, on a machine with a GPU)
    for t in ("softplus", "exp", "sigmoid"):
        rc, msg = create(transform=lowering.UT[t], a=0.0)
        assert rc in (0, -4), (rc, msg)
        if rc == 0:
            lib.bsvi_bnn_destroy(handle)
            handle = C.c_void_p()
    # ... and the siblings refuse a heads program's descriptor as they refuse any Normal one without its scale entries; no struct changed
    d, keep = bnn.make_desc(p)
    assert lib.bsvi_bnn_create(C.byref(d), C.byref(handle)) == UNSUPPORTED and b"bsvi_bnn_create_normal" in lib.bsvi_last_error()
    assert native.ABI_VERSION == 11 and lib.bsvi_abi_version() == 11


def test_the_builder_without_the_keyword_builds_what_it_built():
    """scale_head=None is the default: program for program the same tables; with it the trunk and the loc head keep their draws"""
    for kw in (dict(), dict(n_hidden=0, bias=False), dict(widths=[36, 5, 4, 3], activation="relu", data="normal", sigma=[0.3, 0.5, 0.8])):
        p, p2 = lower(**kw), lower(scale_head=None, **kw)
        assert p.scale_head is None and p.summary()["scale"] == "constant"
        for name in ("uniform", "consts", "row_uniform", "dataset", "labels", "param_uniform_ptr", "param_uniform_idx", "row_prior"):
            assert np.array_equal(getattr(p, name), getattr(p2, name)), name
        assert p.layers == p2.layers and p.tensors == p2.tensors
        p3 = lower(scale_head="softplus", **{k: v for k, v in kw.items() if k != "sigma"})
        assert np.array_equal(p3.dataset, p.dataset) and p3.labels.shape == p.labels.shape and not np.array_equal(p3.labels, p.labels)
        old = {par.name: par.numpy() for par, _, _, _ in p.parameters}
        new = {par.name: par.numpy() for par, _, _, _ in p3.parameters}
        extra = {"weights_scale_loc", "weights_scale_scale"} | (set() if kw.get("bias", True) is False else {"b_scale_loc", "b_scale_scale"})
        assert set(new) - set(old) == extra and all(np.array_equal(old[k], new[k]) for k in old)
    with pytest.raises(ValueError):
        lower(scale_head="tanh")
    with pytest.raises(ValueError):
        lower(scale_head="exp", learnable_sigma=True)


@pytest.mark.parametrize("estimator", ["pathwise", "blackbox"])
def test_the_oracle_runs_the_builders_model_in_single_and_double_precision(estimator):
    kw = dict(scale_head="softplus")
    p = lower(**kw)
    n = 6
    rng = np.random.RandomState(2)
    named = {t["name"]: rng.normal(size=(n, 1, t["rows"], t["cols"])).astype(np.float32) for t in p.tensors}
    mb = {p.indices_name: rng.permutation(24)[:9].tolist()}
    build = lambda: W.build_bnn_regression(W.native_api(), **dict(KW, **kw))
    r64 = Oracle(build(), dtype=torch.float64).loss_and_grads(n, estimator, named, mb)
    r32 = Oracle(build()).loss_and_grads(n, estimator, named, mb)
    assert len(r64["grads"]) == 12 and set(r64["grads"]) == set(r32["grads"])
    assert np.isfinite(r64["loss"]) and abs(r32["loss"] - r64["loss"]) <= 1e-5 * abs(r64["loss"])
    scale = max(np.abs(g).max() for g in r64["grads"].values())
    for name, g in r64["grads"].items():
        assert np.isfinite(g).all() and np.abs(g).max() > 0, name
        assert np.abs(r32["grads"][name] - g).max() <= (1e-5 if estimator == "pathwise" else 1e-3) * scale, name
    # the (u^2 - 1) terms do not cancel: the gradient of the scale head's bias is of the size of the largest
    assert np.abs(r64["grads"]["b_scale_loc"]).max() > 0.1 * scale
