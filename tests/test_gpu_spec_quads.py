"""Two items of the specialised training loop against the kernels without them.

  SPEC_QUADS        the table values a Normal record reads, and four observations, are one 16-byte read (spec_prelude.h) —
                    against BSVI_SPEC_QUADS=0, read when the program is created: the compact tables, every source as it was
  SPEC_OPT_LITERAL  the owners' epilogue compiled for the launch's optimizer (spec_main.h; specialize.cpp opt_literal) —
                    against BSVI_SPEC_OPT_LITERAL=0, read at every launch: the generic code object always

The same values through the same arithmetic in the same order, so loss curve, finite flags, parameters, the optimizer's state planes
and out[0:4] must agree bit for bit (`equal_bits`: all 32 bits of every value; of a NaN, that the other side is a NaN).  Every side creates its own program and hands the loop a state buffer of its own
(bsvi_train_persistent2: CompiledELBO.train starts every call from a fresh optimizer and keeps no state).
Modelled on tests/test_gpu_spec_tail.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from brancher_amd import engine, native, workloads as W

pytestmark = pytest.mark.gpu

SWITCHES = ["BSVI_SPEC_QUADS", "BSVI_SPEC_OPT_LITERAL"]
OPTIMIZERS = {
    # name: (optimizer, options, the literal its launches of variant 6 take)
    "sgd": ("SGD", dict(lr=1e-3), 1),
    "sgd-momentum": ("SGD", dict(lr=1e-3, momentum=0.9), 0),      # (the generic object's SGD arm)
    "adam": ("Adam", dict(lr=1e-2), 2),
    "adamw": ("AdamW", dict(lr=1e-2), 0),
}
WHAT = ("loss curve", "finite flags", "parameters", "optimizer state", "out[0:4]")
WHAT4 = ("loss curve", "finite flags", "parameters", "out[0:4]")


def readme_ar(estimator="pathwise"):
    return engine.compile_model(W.build_readme_ar(W.native_api(), T=20), None, estimator)


def loop(c, n, optimizer, kw, calls=(30,), pretraining=0, prepare=None):
    """(curve, flags, parameters, state, out[0:4], variant, literal) of the in-kernel loop on program `c`, the calls one after
    the other on one state buffer"""
    if prepare is not None:
        prepare(c)
    cfg = native.make_opt_cfg(optimizer, **kw)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    c.native.ensure_shares(n)
    state = torch.zeros(4 * c.n_params, device=c.device)
    curves, flags, offset = [], [], 0
    for iters in calls:
        loss, finite = torch.zeros(iters, device=c.device), torch.zeros(iters, device=c.device)
        args = c._elbo_args(n, n, 0, None, 4, offset)
        native.check(c.lib.bsvi_train_persistent2(c.native.handle, C.byref(args), C.byref(cfg), ptr(c.params), ptr(state),
                                                  ptr(c.mask_all), ptr(c.mask_first), pretraining, iters, ptr(loss), ptr(finite)))
        torch.cuda.synchronize()
        curves.append(loss.cpu().numpy())
        flags.append(finite.cpu().numpy())
        offset += iters
    lib = native.load()
    return (np.concatenate(curves), np.concatenate(flags), c.params.cpu().numpy().copy(), state.cpu().numpy().copy(),
            c.out.cpu().numpy()[:4].copy(), lib.bsvi_spec_last_variant(), lib.bsvi_spec_last_opt_literal())


def equal_bits(x, y):
    """the same 32 bits in every element — a zero's sign included — and a NaN where the other side has a NaN.  A NaN's own sign is
    left out: no IEEE operation defines it, and it follows the compiler's choice between v_fmac and a v_fma with a negated operand.
    Measured (README AR, parameter 0 set to NaN): every loss of the curve 0x7fc00000 with the grouped table, 0xffc00000 with
    BSVI_SPEC_QUADS=0 — NaN on both sides, as tests/test_gpu_spec_tail.py and tests/test_gpu_spec_trim.py compare (equal_nan)."""
    nan = np.isnan(x)
    return x.shape == y.shape and np.array_equal(nan, np.isnan(y)) and np.array_equal(x.view(np.uint32)[~nan], y.view(np.uint32)[~nan])


def same(a, b, what=WHAT):
    for x, y, name in zip(a, b, what):
        diff = np.nanmax(np.abs(x.astype(np.float64) - y.astype(np.float64))) if np.isfinite(x).any() else 0.0
        print("%s: largest difference %.3g over %d values" % (name, diff, x.size))
        assert equal_bits(x, y), name


def against_every_switch(monkeypatch, make, n, name, literal=None, **how):
    """the default against each switch at 0, one program per setting; returns the default's run"""
    optimizer, kw, expected = OPTIMIZERS[name]
    c = make()
    assert "#define SPEC_QUADS_MAP 1\n" in native.specialised_source(c.program, 6)
    new = loop(c, n, optimizer, kw, **how)
    print("variant %d, literal %d" % new[5:7])
    if new[5] == 6:
        assert new[6] == (expected if literal is None else literal)
    else:
        assert new[6] == 0                                # (only the owners' loop has a literal form)
    for switch in SWITCHES:
        monkeypatch.setenv(switch, "0")
        c = make()
        assert ("SPEC_QUADS_MAP" in native.specialised_source(c.program, 6)) == (switch != "BSVI_SPEC_QUADS")
        off = loop(c, n, optimizer, kw, **how)
        monkeypatch.delenv(switch)
        print("%s=0: variant %d, literal %d" % ((switch,) + off[5:7]))
        assert off[5] == new[5]
        if switch == "BSVI_SPEC_OPT_LITERAL":
            assert off[6] == 0
        same(new[:5], off[:5])
    return new


# one sample wave with and without idle lanes, two, four, five with one live lane, the headline's five
@pytest.mark.parametrize("n", [44, 64, 65, 193, 257, 300])
@pytest.mark.parametrize("name", sorted(OPTIMIZERS))
def test_sample_counts(n, name, monkeypatch):
    new = against_every_switch(monkeypatch, readme_ar, n, name)
    assert bool(new[1].all()) and np.isfinite(new[0]).all()
    if n >= 193:
        assert new[5] == 6
    assert new[3].reshape(4, -1)[3].max() == 30.0         # (the state was written back)


@pytest.mark.parametrize("calls", [(1,), (2,), (17, 17)])
@pytest.mark.parametrize("name", sorted(OPTIMIZERS))
def test_short_calls_and_a_second_call_on_the_same_state(calls, name, monkeypatch):
    new = against_every_switch(monkeypatch, readme_ar, 300, name, calls=calls)
    assert new[5] == 6 and new[0].size == sum(calls) and bool(new[1].all())
    assert new[3].reshape(4, -1)[3].max() == float(sum(calls))


@pytest.mark.parametrize("name", ["sgd", "adam"])
def test_pretraining_iterations(name, monkeypatch):
    new = against_every_switch(monkeypatch, readme_ar, 300, name, pretraining=7)
    steps = new[3].reshape(4, -1)[3]
    print("step counts:", sorted(set(steps.tolist())))
    assert new[5] == 6 and bool(new[1].all())


def test_non_finite_loss_skips_the_step_identically(monkeypatch):
    def prepare(c):
        with torch.no_grad():
            c.params[0] = float("nan")
    before = readme_ar().params.cpu().numpy()
    new = against_every_switch(monkeypatch, readme_ar, 300, "sgd", prepare=prepare)
    assert new[5] == 6 and not new[1].any() and not np.isfinite(new[0]).any()
    # out[1], the last iteration's non-finite count: every sample's value carries the NaN parameter; no step was taken
    assert new[4][1] == 300.0 and new[4][3] == 0.0
    assert np.array_equal(new[2][1:].view(np.uint32), before[1:].view(np.uint32)) and new[3].reshape(4, -1)[3].max() == 0.0


@pytest.mark.parametrize("name", ["sgd", "adam"])
def test_blackbox_program(name, monkeypatch):
    new = against_every_switch(monkeypatch, lambda: readme_ar("blackbox"), 300, name)
    assert new[5] == 6


def test_in_kernel_loop_equals_launch_per_iteration_bit_for_bit():
    """plain SGD, 300 samples, 30 iterations: the loop's literal object against one launch per iteration (the main loop's
    epilogue, optimizer_apply's dispatch)"""
    runs = {}
    for persistent in (True, False):
        c = readme_ar()
        losses, finite = c.train(30, 300, "SGD", seed=4, lr=1e-3, allow_persistent=persistent)
        runs[persistent] = (losses.cpu().numpy(), finite.cpu().numpy(), c.params.cpu().numpy().copy(), c.last_mode)
        if persistent:
            assert native.load().bsvi_spec_last_variant() == 6 and native.load().bsvi_spec_last_opt_literal() == 1
    assert runs[True][3] == "persistent" and runs[False][3] == "stepwise"
    same(runs[True][:3], runs[False][:3])


@pytest.mark.parametrize("name", ["sgd", "adam"])
def test_minibatched_linear_regression_in_the_gather_loop(name, monkeypatch):
    """tests/test_gpu_minibatch_loop.py's linear regression at 64 samples, the rows gathered by the kernel"""
    optimizer, kw, _ = OPTIMIZERS[name]
    runs = {}
    for setting in [None] + SWITCHES:
        if setting:
            monkeypatch.setenv(setting, "0")
        c = engine.compile_model(W.build_minibatch_linear_regression(W.native_api(), dataset_size=40, batch_size=8, n_features=3), None, "pathwise")
        losses, finite = c.train(30, 64, optimizer, seed=5, minibatch_loop=True, **kw)
        runs[setting] = (losses.cpu().numpy(), finite.cpu().numpy(), c.params.cpu().numpy().copy(), c.out.cpu().numpy()[:4].copy())
        assert c.last_mode == "persistent"
        print(setting, "variant", native.load().bsvi_spec_last_variant(), "literal", native.load().bsvi_spec_last_opt_literal())
        if setting:
            monkeypatch.delenv(setting)
    for setting in SWITCHES:
        same(runs[None], runs[setting], WHAT4)


@pytest.mark.parametrize("name", ["sgd", "adam"])
def test_many_workgroups_rebuild_the_grouped_table(name, monkeypatch):
    """4 096 samples, 5 iterations: every workgroup rebuilds its table from the new parameters in every iteration"""
    new = against_every_switch(monkeypatch, readme_ar, 4096, name, calls=(5,))
    assert new[5] == 2 and bool(new[1].all())


OTHER_MODELS = [
    ("build_readme_ar", dict(T=5), 300),
    ("build_readme_ar", dict(T=60), 128),               # more than 64 positions: DPP row sums
    ("build_beta_ar", dict(T=20), 300),
    ("build_lognormal_normal", dict(), 300),
    ("build_linear_predictor", dict(), 300),
    ("build_scale_from_latent", dict(), 2048),
]


@pytest.mark.parametrize("builder,kw,n", OTHER_MODELS)
def test_other_models_equal_the_compact_layout(builder, kw, n, monkeypatch):
    """the models of tests/test_gpu_spec_chain.py under Adam, 25 iterations, with and without the grouped table"""
    runs = {}
    for env in ("1", "0"):
        monkeypatch.setenv("BSVI_SPEC_QUADS", env)
        c = engine.compile_model(getattr(W, builder)(W.native_api(), **kw), None, "pathwise")
        losses, finite = c.train(25, n, "Adam", seed=3, lr=1e-2)
        launched = native.load().bsvi_spec_last_variant()
        src = (native.specialised_source(c.program, launched) if launched >= 0 else "") or ""
        print(builder, kw, n, "mode", c.last_mode, "variant", launched, "groups", (re.findall(r"#define SPEC_Q_GROUPS (\d+)", src) or ["none"])[0])
        assert env == "1" or "SPEC_QUADS_MAP" not in src
        runs[env] = (losses.cpu().numpy(), finite.cpu().numpy(), c.params.cpu().numpy().copy(), c.out.cpu().numpy()[:4].copy())
    same(runs["1"], runs["0"], WHAT4)


def test_lds_bytes_are_the_code_objects(tmp_path, monkeypatch):
    """bsvi_program_engine's lds_bytes of the headline launch is the static LDS of the variant's code object, with the grouped table
    and without; the grouped table is no larger"""
    readelf = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "llvm-readelf")
    sizes = {}
    for env in ("1", "0"):
        monkeypatch.setenv("BSVI_SPEC_QUADS", env)
        c = readme_ar()
        reported = c.native.engine(300, 2)
        dump = str(tmp_path / ("quads%s.co" % env))
        monkeypatch.setenv("BSVI_JIT_DUMP", dump)
        assert native.jit_compile(native.specialised_source(c.program, 6) + "\n// (not from the code cache) %s\n" % env) > 0
        monkeypatch.delenv("BSVI_JIT_DUMP")
        notes = subprocess.run([readelf, "--notes", dump], capture_output=True, text=True).stdout
        static = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", notes).group(1))
        print("BSVI_SPEC_QUADS=%s:" % env, reported, "static LDS of variant 6:", static)
        assert reported["engine"] == "specialised" and reported["lds_bytes"] == static
        sizes[env] = static
    assert sizes["1"] <= sizes["0"]
