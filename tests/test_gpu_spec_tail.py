"""The tail of the lean chain of the specialised training loop — the owners' loss bookkeeping beside the next bodies, plain
SGD as a step of its own (spec_main.h SPEC_LEAN_TAIL) — against the kernel as it was: BSVI_SPEC_TAIL=0, read when the program is
created, generates variant 6 in its previous form.  The same draws and the same arithmetic in the same order, so loss curve,
finite flags, parameters and the output block must agree bit for bit.  Modelled on tests/test_gpu_spec_chain.py."""
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
    return (np.concatenate(curves), np.concatenate(flags), c.params.cpu().numpy().copy(), c.out.cpu().numpy().copy(),
            c.last_mode, native.specialised_source(c.program, 6))


def both(monkeypatch, *args, **kwargs):
    runs = {}
    for env in ("1", "0"):
        monkeypatch.setenv("BSVI_SPEC_TAIL", env)
        runs[env] = run(*args, **kwargs)
        assert runs[env][4] == "persistent"
        assert native.load().bsvi_spec_last_variant() == 6
        assert ("#define SPEC_LEAN_TAIL 1\n" in runs[env][5]) == (env == "1")
    monkeypatch.delenv("BSVI_SPEC_TAIL")
    # (two kernels: variant 6 with the tail, and variant 6 as it was)
    assert runs["1"][5] != runs["0"][5]
    return runs["1"], runs["0"]


def same(a, b, n=4):
    for x, y, what in zip(a[:n], b[:n], ("loss curve", "finite flags", "parameters", "output block")):
        diff = np.nanmax(np.abs(x.astype(np.float64) - y.astype(np.float64))) if np.isfinite(x).any() else 0.0
        print("%s: largest difference %.3g over %d values" % (what, diff, x.size))
        assert np.array_equal(x, y, equal_nan=True), what


@pytest.mark.parametrize("n", [193, 256, 300])      # four and five sample waves, with and without idle lanes
@pytest.mark.parametrize("optimizer,kw", OPTIMIZERS)
def test_tail_equals_previous_arrangement(n, optimizer, kw, monkeypatch):
    new, prev = both(monkeypatch, n, optimizer, kw)
    assert bool(new[1].all())
    same(new, prev)


@pytest.mark.parametrize("kw", [dict(lr=1e-3, momentum=0.9), dict(lr=1e-3, weight_decay=1e-2),
                                dict(lr=1e-3, momentum=0.9, nesterov=True, weight_decay=1e-2)])
def test_sgd_with_momentum_weight_decay_nesterov(kw, monkeypatch):
    new, prev = both(monkeypatch, 300, "SGD", kw)
    assert bool(new[1].all())
    same(new, prev)
    plain = run(300, "SGD", dict(lr=1e-3))
    assert not np.array_equal(new[2], plain[2])              # (the options reached the step)


@pytest.mark.parametrize("iterations", [1, 2, 30])
@pytest.mark.parametrize("optimizer,kw", OPTIMIZERS)
def test_short_calls(iterations, optimizer, kw, monkeypatch):
    """one iteration: nothing is deferred; two: one deferred entry, then the last one's at once"""
    new, prev = both(monkeypatch, 300, optimizer, kw, iterations=iterations)
    assert new[0].size == iterations and bool(new[1].all()) and np.isfinite(new[0]).all()
    same(new, prev)


@pytest.mark.parametrize("optimizer,kw", OPTIMIZERS)
def test_two_calls_continue(optimizer, kw, monkeypatch):
    new, prev = both(monkeypatch, 300, optimizer, kw, iterations=17, calls=2)
    assert bool(new[1].all())
    same(new, prev)


@pytest.mark.parametrize("optimizer,kw", OPTIMIZERS)
def test_pretraining_iterations(optimizer, kw, monkeypatch):
    new, prev = both(monkeypatch, 300, optimizer, kw, pretraining_iterations=7)
    assert bool(new[1].all())
    same(new, prev)


@pytest.mark.parametrize("how", ["nan", "huge"])
def test_non_finite_loss_skips_the_step_identically(how, monkeypatch):
    def prepare(c):
        with torch.no_grad():
            if how == "nan":
                c.params[0] = float("nan")
            else:
                c.params.mul_(1e19)
    new, prev = both(monkeypatch, 300, "SGD", dict(lr=1e-3), prepare=prepare)
    print("finite iterations:", int(new[1].sum()), "of", new[1].size, "non-finite count of the last iteration:", new[3][1])
    same(new, prev)
    if how == "nan":
        assert not new[1].any() and not np.isfinite(new[0]).any()
        # out[1], the last iteration's non-finite count: every sample's value carries the NaN parameter
        assert new[3][1] == 300.0 and new[3][3] == 0.0


def test_non_finite_count_of_a_finite_call_is_zero(monkeypatch):
    new, prev = both(monkeypatch, 300, "SGD", dict(lr=1e-3), iterations=5)
    assert new[3][1] == 0.0 and new[3][3] == 1.0
    same(new, prev)


def test_diverging_run_stops_stepping_identically(monkeypatch):
    new, prev = both(monkeypatch, 300, "SGD", dict(lr=1e3), iterations=40)
    print("finite iterations:", int(new[1].sum()), "of", new[1].size, "non-finite count of the last iteration:", new[3][1])
    same(new, prev)


@pytest.mark.parametrize("n", [256, 300])
def test_blackbox_program(n, monkeypatch):
    new, prev = both(monkeypatch, n, "Adam", dict(lr=1e-2), estimator="blackbox")
    same(new, prev)


def test_in_kernel_loop_equals_launch_per_iteration_bit_for_bit():
    """SGD: the loop kernel with the tail against one launch per iteration (the main loop's epilogue, bookkeeping in every
    iteration, optimizer_apply's dispatch): the same arithmetic in the same order"""
    loop = run(300, "SGD", dict(lr=1e-3))
    step = run(300, "SGD", dict(lr=1e-3), allow_persistent=False)
    assert loop[4] == "persistent" and step[4] == "stepwise"
    assert "#define SPEC_LEAN_TAIL 1\n" in loop[5]
    same(loop, step, n=3)


BODY_CASES = [
    # builder, keyword arguments, samples, the kernel variant the last launch must have used (None: whichever serves it)
    ("build_readme_ar", dict(T=20), 4096, 2),           # many workgroups, several chunks of samples each: cfg 2's geometry
    ("build_readme_ar", dict(T=20), 128, None),         # two sample waves and the single draw wave
    ("build_readme_ar", dict(T=20), 300, 6),            # the draw service: the kernel with the tail
    ("build_readme_ar", dict(T=5), 300, None),
    ("build_beta_ar", dict(T=20), 300, None),
    ("build_lognormal_normal", dict(), 300, None),
    ("build_linear_predictor", dict(), 300, None),
    ("build_scale_from_latent", dict(), 2048, None),
]


@pytest.mark.parametrize("builder,kw,n,variant", BODY_CASES)
@pytest.mark.parametrize("estimator", ["pathwise", "blackbox"])
def test_new_body_equals_body_as_it_was(builder, kw, n, variant, estimator, monkeypatch):
    """the default body against the body as it was (BSVI_SPEC_LEAN_BODY=0, read when the program is created) on the models and
    sizes of tests/test_gpu_spec_chain.py, and in the kernel with the tail; no variant reads an entropy column (measured and
    dropped)"""
    runs = {}
    for env in ("1", "0"):
        monkeypatch.setenv("BSVI_SPEC_LEAN_BODY", env)
        c = engine.compile_model(getattr(W, builder)(W.native_api(), **kw), None, estimator)
        losses, finite = c.train(25, n, "Adam", seed=3, lr=1e-2)
        runs[env] = (losses.cpu().numpy(), finite.cpu().numpy(), c.params.cpu().numpy().copy(), c.out.cpu().numpy().copy())
        launched = native.load().bsvi_spec_last_variant()
        src = native.specialised_source(c.program, launched) if launched >= 0 else ""
        print(builder, n, estimator, "mode", c.last_mode, "variant", launched, "SPEC_UE reads", (src or "").count("SPEC_UE("))
        if variant is not None:
            assert launched == variant
        assert "SPEC_UE(" not in (src or "")
    same(runs["1"], runs["0"])
