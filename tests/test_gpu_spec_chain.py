"""The lean chain of the specialised training loop — the owners' epilogue with its argument words loaded beside the bodies,
one batch of LDS reads, the loss bookkeeping behind the new table, one table entry per parameter; the model's literal
1.0 / 0.0 folded in the body — against the kernel as it was (BSVI_SPEC_LEAN_CHAIN=0 launches the library's previous source
of the same program): the same draws and the same arithmetic in the same order, so loss curve, finite flags and parameters
must agree bit for bit.  The folded body alone is compared with the body as it was (BSVI_SPEC_LEAN_BODY=0) in the
many-workgroup kernels and on other models.  Modelled on tests/test_gpu_owner_wave.py."""
import numpy as np
import pytest
import torch

from brancher_amd import engine, native, workloads as W

pytestmark = pytest.mark.gpu

OPTIMIZERS = [
    ("SGD", dict(lr=1e-3)),
    ("Adam", dict(lr=1e-2)),
]


def run(n, optimizer, kw, estimator="pathwise", iterations=30, prepare=None, calls=1, T=20, **opts):
    c = engine.compile_model(W.build_readme_ar(W.native_api(), T=T), None, estimator)
    if prepare is not None:
        prepare(c)
    curves, flags = [], []
    for _ in range(calls):
        losses, finite = c.train(iterations, n, optimizer, seed=4, **opts, **kw)
        curves.append(losses.cpu().numpy())
        flags.append(finite.cpu().numpy())
    return np.concatenate(curves), np.concatenate(flags), c.params.cpu().numpy().copy(), c.last_mode


def both(monkeypatch, *args, **kwargs):
    runs = {}
    for env in ("1", "0"):
        monkeypatch.setenv("BSVI_SPEC_LEAN_CHAIN", env)
        runs[env] = run(*args, **kwargs)
        assert runs[env][3] == "persistent"
        # (the two runs are two kernels: 6 the owners' wave with the lean chain, 7 the library's previous source)
        assert native.load().bsvi_spec_last_variant() == (6 if env == "1" else 7)
    monkeypatch.setenv("BSVI_SPEC_LEAN_CHAIN", "1")
    return runs["1"], runs["0"]


def same(a, b):
    for x, y, what in zip(a[:3], b[:3], ("loss curve", "finite flags", "parameters")):
        diff = np.nanmax(np.abs(x.astype(np.float64) - y.astype(np.float64))) if np.isfinite(x).any() else 0.0
        print("%s: largest difference %.3g over %d values" % (what, diff, x.size))
        assert np.array_equal(x, y, equal_nan=True), what


@pytest.mark.parametrize("n", [193, 256, 300])      # four and five sample waves, with and without idle lanes
@pytest.mark.parametrize("optimizer,kw", OPTIMIZERS)
def test_lean_chain_equals_previous_arrangement(n, optimizer, kw, monkeypatch):
    lean, prev = both(monkeypatch, n, optimizer, kw)
    assert bool(lean[1].all())
    same(lean, prev)


@pytest.mark.parametrize("optimizer,kw", OPTIMIZERS)
def test_two_calls_continue(optimizer, kw, monkeypatch):
    """a second call goes on from the first one's parameters (and reads the table they give in its prologue)"""
    lean, prev = both(monkeypatch, 300, optimizer, kw, iterations=17, calls=2)
    assert bool(lean[1].all())
    same(lean, prev)


@pytest.mark.parametrize("optimizer,kw", OPTIMIZERS)
def test_pretraining_iterations(optimizer, kw, monkeypatch):
    lean, prev = both(monkeypatch, 300, optimizer, kw, pretraining_iterations=7)
    assert bool(lean[1].all())
    same(lean, prev)


@pytest.mark.parametrize("how", ["nan", "huge"])
def test_non_finite_loss_skips_the_step_identically(how, monkeypatch):
    """a loss that is not finite: no step, flag 0 (a NaN parameter: in every iteration, the parameters come back as they went in)"""
    def prepare(c):
        with torch.no_grad():
            if how == "nan":
                c.params[0] = float("nan")
            else:
                c.params.mul_(1e19)
    lean, prev = both(monkeypatch, 300, "SGD", dict(lr=1e-3), prepare=prepare)
    print("finite iterations:", int(lean[1].sum()), "of", lean[1].size)
    same(lean, prev)
    if how == "nan":
        assert not lean[1].any() and not np.isfinite(lean[0]).any()
        c = engine.compile_model(W.build_readme_ar(W.native_api(), T=20), None, "pathwise")
        prepare(c)
        assert np.array_equal(lean[2], c.params.cpu().numpy(), equal_nan=True)


def test_diverging_run_stops_stepping_identically(monkeypatch):
    """a step size that blows the parameters up within the call: finite iterations first, then skipped ones"""
    lean, prev = both(monkeypatch, 300, "SGD", dict(lr=1e3), iterations=40)
    print("finite iterations:", int(lean[1].sum()), "of", lean[1].size)
    same(lean, prev)


@pytest.mark.parametrize("n", [256, 300])
def test_blackbox_program(n, monkeypatch):
    lean, prev = both(monkeypatch, n, "Adam", dict(lr=1e-2), estimator="blackbox")
    same(lean, prev)


def test_in_kernel_loop_equals_launch_per_iteration_bit_for_bit(monkeypatch):
    """SGD, everything switched on: the loop kernel (owners on a draw wave, lean chain, folded constants) against one launch
    per iteration (the main loop's epilogue on the same generated body): the same arithmetic in the same order"""
    monkeypatch.setenv("BSVI_SPEC_LEAN_CHAIN", "1")
    loop = run(300, "SGD", dict(lr=1e-3))
    step = run(300, "SGD", dict(lr=1e-3), allow_persistent=False)
    assert loop[3] == "persistent" and step[3] == "stepwise"
    same(loop, step)


BODY_CASES = [
    # builder, keyword arguments, samples, the kernel variant the last launch must have used (None: whichever serves it)
    ("build_readme_ar", dict(T=20), 4096, 2),           # many workgroups, several chunks of samples each: cfg 2's geometry
    ("build_readme_ar", dict(T=20), 128, None),         # two sample waves and the single draw wave
    ("build_readme_ar", dict(T=5), 300, None),
    ("build_beta_ar", dict(T=20), 300, None),
    ("build_lognormal_normal", dict(), 300, None),
    ("build_linear_predictor", dict(), 300, None),
    ("build_scale_from_latent", dict(), 2048, None),
]


@pytest.mark.parametrize("builder,kw,n,variant", BODY_CASES)
@pytest.mark.parametrize("estimator", ["pathwise", "blackbox"])
def test_folded_constants_equal_table_reads(builder, kw, n, variant, estimator, monkeypatch):
    """the body with the literal 1.0 / 0.0 folded — x * 1 + 0 as x, a * b + 0 as fma(a, b, 0.0f), x * 1 + c and acc + g * 1 as
    adds that do not fuse — against the body that reads them from the uniform table (BSVI_SPEC_LEAN_BODY=0, read when the
    program is created): every rounding point kept, so the same bits, in other kernel variants and on other models"""
    runs = {}
    for env in ("1", "0"):
        monkeypatch.setenv("BSVI_SPEC_LEAN_BODY", env)
        c = engine.compile_model(getattr(W, builder)(W.native_api(), **kw), None, estimator)
        losses, finite = c.train(25, n, "Adam", seed=3, lr=1e-2)
        runs[env] = (losses.cpu().numpy(), finite.cpu().numpy(), c.params.cpu().numpy().copy())
        launched = native.load().bsvi_spec_last_variant()
        print(builder, n, estimator, "mode", c.last_mode, "variant", launched)
        if variant is not None:
            assert launched == variant
    same(runs["1"], runs["0"])
