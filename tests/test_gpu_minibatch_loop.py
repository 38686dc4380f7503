"""Minibatched observations inside the in-kernel training loop (spec_main.h, the gather phase; `CompiledELBO.train(...,
minibatch_loop=True)`; `bsvi_train_persistent_minibatch`): ONE launch against the launch-by-launch path of the same build
(`allow_persistent=False`: one `bsvi_minibatch_gather` launch per source and one step launch per iteration), whose rows
tests/test_gpu_noise.py pins to the host reference.  Both sides draw the same rows and the same normals; under plain SGD the
in-kernel loop and the launch-per-iteration step are the same arithmetic in the same order (tests/test_gpu_spec_tail.py holds
them to equality at 193, 256 and 300 samples), so curve, flags and parameters must be EQUAL there.  Every side compiles a
fresh model.

(This file was written without a GPU at hand: it has been collected and its host side exercised, its cases have not run on a
device yet.  Every bound is the one the issue sets; none was chosen from a result.)"""
import warnings

import numpy as np
import pytest

from conftest import rel_err
from brancher_amd import engine, native, workloads as W

pytestmark = pytest.mark.gpu

SGD = ("SGD", dict(lr=1e-3))
MODELS = {
    "normal_mean": ("build_minibatch_normal_mean", dict(dataset_size=40, batch_size=8)),
    "normal_mean_own_draw": ("build_minibatch_normal_mean", dict(dataset_size=40, batch_size=8, own_draw=True)),
    "linreg": ("build_minibatch_linear_regression", dict(dataset_size=40, batch_size=8, n_features=3)),
    "linreg_laplace": ("build_minibatch_linear_regression", dict(dataset_size=30, batch_size=6, n_features=4, n_outputs=2, prior="laplace")),
    "linreg_latent_scale": ("build_minibatch_linear_regression", dict(dataset_size=40, batch_size=8, n_features=3, latent_scale=True)),
}


def compiled(builder, kw, estimator="pathwise"):
    return engine.compile_model(getattr(W, builder)(W.native_api(), **kw), None, estimator)


def train(builder, kw, n, iterations=30, optimizer=SGD, seed=5, estimator="pathwise", calls=None, iteration0=None, **opts):
    """(curve, flags, parameters, last_mode) of a fresh model"""
    c = compiled(builder, kw, estimator)
    if iteration0 is not None:
        c.iteration = iteration0
    curves, flags = [], []
    for k in (calls or [iterations]):
        losses, finite = c.train(k, n, optimizer[0], seed=seed, **opts, **optimizer[1])
        curves.append(losses.cpu().numpy())
        flags.append(finite.cpu().numpy())
    return np.concatenate(curves), np.concatenate(flags), c.params.cpu().numpy().copy(), c.last_mode


def pair(builder, kw, n, **opts):
    loop = train(builder, kw, n, minibatch_loop=True, **opts)
    step = train(builder, kw, n, allow_persistent=False, **opts)
    assert loop[3] == "persistent" and step[3] == "stepwise", (loop[3], step[3])
    return loop, step


def equal(loop, step):
    for x, y, what in zip(loop[:3], step[:3], ("loss curve", "finite flags", "parameters")):
        diff = np.nanmax(np.abs(x.astype(np.float64) - y.astype(np.float64)))
        print("%s: largest difference %.3g over %d values" % (what, diff, x.size))
        assert np.array_equal(x, y), what
    assert bool(loop[1].all()) and np.isfinite(loop[0]).all()


def close(loop, step):
    """the project's bound between the in-kernel loop and the launch-per-iteration path
    (tests/test_gpu_parity.py::test_split_persistent_trainer_on_other_workloads)"""
    (l1, f1, p1, _), (l0, f0, p0, _) = loop, step
    print("loss curve: rel_err %.3g; parameters: largest difference %.3g; equal: %s" % (
        rel_err(l1, l0), np.abs(p1 - p0).max(), np.array_equal(l1, l0) and np.array_equal(p1, p0)))
    assert np.array_equal(f0, f1)
    ok = f0 != 0
    assert ok.any()
    assert rel_err(l1[ok], l0[ok]) <= 1e-5
    assert np.abs(p1 - p0).max() <= 1e-4 * (1 + np.abs(p0).max())


# ---- 1. SGD, bit for bit: four and five sample waves (the draw service, the owners on a draw wave) ---------------------------
@pytest.mark.parametrize("n", [193, 256, 300])
@pytest.mark.parametrize("model", sorted(MODELS))
def test_sgd_loop_equals_launch_per_iteration(model, n):
    builder, kw = MODELS[model]
    loop, step = pair(builder, kw, n)
    equal(loop, step)
    assert not np.array_equal(loop[0][:-1], loop[0][1:])         # (the rows change: no two neighbouring losses agree)


# ---- 2. the other loop shapes: one sample wave + the draw wave, and many workgroups ------------------------------------------
@pytest.mark.parametrize("n", [64, 1024])
@pytest.mark.parametrize("model", sorted(MODELS))
def test_other_loop_shapes(model, n):
    builder, kw = MODELS[model]
    loop, step = pair(builder, kw, n)
    # (the project's bound between the two paths; `close` prints whether the run was in fact equal)
    close(loop, step)


# ---- 3. geometry ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ds,b", [(5, 5), (64, 7), (65, 9), (17, 1)])
def test_normal_mean_geometries(ds, b):
    """the whole dataset (a permutation) | an exact power of four (no cycle walk) | a domain of 256 (long walks) | one row"""
    loop, step = pair("build_minibatch_normal_mean", dict(dataset_size=ds, batch_size=b), 193, iterations=12)
    equal(loop, step)


@pytest.mark.parametrize("ds,b,p", [(40, 24, 4), (300, 70, 4)])
def test_linear_regression_geometries(ds, b, p):
    """two sources sharing one index draw: a stretch above 64 floats (96) | above 256 floats (280), two rows per lane"""
    loop, step = pair("build_minibatch_linear_regression", dict(dataset_size=ds, batch_size=b, n_features=p), 193, iterations=12)
    equal(loop, step)


def test_register_cap_both_sides():
    """The gathering wave holds sum ceil(batch / 64) * row_floats registers of rows, 32 at the most (specialize.cpp,
    kMinibatchMaxRegs): 8 rows of 31 features + 1 target are 32 and train in the kernel; 32 features are 33, train launch by
    launch and say why."""
    loop, step = pair("build_minibatch_linear_regression", dict(dataset_size=40, batch_size=8, n_features=31), 193, iterations=4)
    equal(loop, step)
    kw = dict(dataset_size=40, batch_size=8, n_features=32)
    c = compiled("build_minibatch_linear_regression", kw)
    assert not c.native.minibatch_loop and "32 registers" in c.native.minibatch_loop_refusal
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        losses, finite = c.train(4, 193, "SGD", seed=5, minibatch_loop=True, lr=1e-3)
    assert c.last_mode == "stepwise"
    assert "32 registers" in c.last_error and any("minibatch loop declined" in str(w.message) for w in seen)
    step = train("build_minibatch_linear_regression", kw, 193, iterations=4)
    assert step[3] == "stepwise" and np.array_equal(losses.cpu().numpy(), step[0])


# ---- 4. keys ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("own_draw", [False, True])
@pytest.mark.parametrize("what", ["offset carry", "wide seed"])
def test_keys(what, own_draw):
    """the carry into the offset's high word within a call; a seed beyond 32 bits; with its own draw the source's group
    constant is xor-ed into the 64-bit key"""
    kw = dict(dataset_size=40, batch_size=8, own_draw=own_draw)
    opts = dict(iteration0=2 ** 32 - 5) if what == "offset carry" else dict(seed=0x123456789ABCDEF)
    loop, step = pair("build_minibatch_normal_mean", kw, 193, iterations=12, **opts)
    equal(loop, step)


def test_nonzero_key_group():
    """a source of key group 3 (as a model with several independent draws numbers them): the constant 3 * 0x9E3779B97F4A7C15 is
    xor-ed into both words of a 64-bit seed, on the host for the launch-by-launch gather and in the kernel for the loop"""
    from brancher_amd import lowering
    runs = []
    for opts in (dict(minibatch_loop=True), dict(allow_persistent=False)):
        model = W.build_minibatch_normal_mean(W.native_api(), dataset_size=40, batch_size=8, own_draw=True)
        program = lowering.lower(model, model.posterior_model, "pathwise")
        program.minibatches[0]["group"] = 3
        c = engine.CompiledELBO(model, model.posterior_model, "pathwise", program=program)
        losses, finite = c.train(12, 193, "SGD", seed=0x123456789ABCDEF, lr=1e-3, **opts)
        runs.append((losses.cpu().numpy(), finite.cpu().numpy(), c.params.cpu().numpy().copy(), c.last_mode))
    assert runs[0][3] == "persistent" and runs[1][3] == "stepwise"
    equal(*runs)
    group0 = train("build_minibatch_normal_mean", dict(dataset_size=40, batch_size=8, own_draw=True), 193, iterations=12,
                   seed=0x123456789ABCDEF, minibatch_loop=True)
    assert not np.array_equal(group0[0], runs[0][0])             # (the group reaches the key)


# ---- 5. calls ---------------------------------------------------------------------------------------------------------------
def test_two_calls_continue():
    builder, kw = MODELS["linreg"]
    loop = train(builder, kw, 193, calls=[7, 9], minibatch_loop=True)
    step = train(builder, kw, 193, iterations=16, allow_persistent=False)
    assert loop[3] == "persistent" and step[3] == "stepwise"
    equal(loop, step)


def test_pretraining_iterations():
    builder, kw = MODELS["linreg_latent_scale"]
    loop, step = pair(builder, kw, 193, iterations=12, pretraining_iterations=3)
    equal(loop, step)


def test_one_iteration():
    builder, kw = MODELS["linreg"]
    loop, step = pair(builder, kw, 193, iterations=1)
    equal(loop, step)


# ---- 6. Adam and BlackBox ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("optimizer,estimator", [(("Adam", dict(lr=1e-2)), "pathwise"), (SGD, "blackbox")])
def test_adam_and_blackbox(optimizer, estimator):
    builder, kw = MODELS["linreg"]
    loop, step = pair(builder, kw, 300, iterations=40, optimizer=optimizer, estimator=estimator)
    close(loop, step)


# ---- 7. declines ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["BSVI_JIT=0", "minibatch_seq", "BSVI_MINIBATCH_LOOP=0", "_force_sharded_path", "no keyword"])
def test_declines_train_launch_by_launch(how, monkeypatch):
    builder, kw = MODELS["linreg"]
    n, k = 193, 6
    opts, plain_opts = dict(minibatch_loop=True), {}
    if how == "minibatch_seq":
        probe = compiled(builder, kw)
        seq = []
        for it in range(k):
            rows = probe.evaluate(1, seed=5, offset=it, want_indices=True)["indices"]
            seq.append({name: v.cpu().numpy().tolist() for name, v in rows.items()})
        opts["minibatch_seq"] = plain_opts["minibatch_seq"] = seq
    elif how == "_force_sharded_path":
        opts["_force_sharded_path"] = plain_opts["_force_sharded_path"] = True
    elif how == "no keyword":
        opts = {}
    elif how == "BSVI_JIT=0":
        monkeypatch.setenv("BSVI_JIT", "0")
    else:
        monkeypatch.setenv("BSVI_MINIBATCH_LOOP", "0")
    asked = train(builder, kw, n, iterations=k, **opts)
    plain = train(builder, kw, n, iterations=k, **plain_opts)
    assert asked[3] == "stepwise" and plain[3] == "stepwise", (asked[3], plain[3])
    for x, y in zip(asked[:3], plain[:3]):
        assert np.array_equal(x, y)


# ---- the C ABI's refusals, on a live program ----------------------------------------------------------------------------------
def test_set_minibatches_refusals():
    import ctypes as C
    builder, kw = MODELS["linreg"]
    c = compiled(builder, kw)
    lib, handle = c.lib, c.native.handle
    geo = lambda rows: (C.c_uint32 * (5 * len(rows)))(*[w for row in rows for w in row])
    n_obs = c.program.obs.size
    assert lib.bsvi_program_set_minibatches(handle, 1, geo([(n_obs - 4, 8, 1, 40, 0)])) != 0
    assert b"leaves the observation table" in lib.bsvi_last_error()
    assert lib.bsvi_program_set_minibatches(handle, 1, geo([(0, 41, 1, 40, 0)])) != 0
    assert b"exceeds dataset_size" in lib.bsvi_last_error()
    # the refusals left the program's own geometry in place: it trains in the kernel, and then takes no other geometry
    losses, finite = c.train(3, 193, "SGD", seed=5, minibatch_loop=True, lr=1e-3)
    assert c.last_mode == "persistent" and bool(finite.all())
    own, n = native.minibatch_geometry(c.program)
    assert lib.bsvi_program_set_minibatches(handle, n, own) != 0
    assert b"already prepared" in lib.bsvi_last_error()


# ---- 8. the public API ------------------------------------------------------------------------------------------------------
def test_perform_inference_keeps_the_loop_in_one_launch():
    from brancher_amd import inference
    api = W.native_api()
    model = W.build_minibatch_linear_regression(api)
    method = inference.ReverseKL()
    inference.perform_inference(model, inference_method=method, number_iterations=200, number_samples=64, optimizer="Adam", lr=0.01)
    curve = np.asarray(model.diagnostics["loss curve"])
    assert curve.size == 200 and np.isfinite(curve).all()
    assert curve[-20:].mean() < curve[:20].mean()
    assert method.last_compiled.last_mode == "persistent"
