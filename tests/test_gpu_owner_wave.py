"""The draw service's owners' epilogue on a draw wave (spec_main.h, SPEC_DRAW_OWNERS) against the owners on sample wave 1
(BSVI_SPEC_OWNER_WAVE=0): who draws which rows and which wave steps the parameters does not change a bit — the draws are
functions of (seed, offset, sample, row) and the owner arithmetic is the same — and against launch-per-iteration."""
import numpy as np
import pytest

from brancher_amd import engine, workloads as W

pytestmark = pytest.mark.gpu

OPTIMIZERS = [
    ("SGD", dict(lr=1e-3)),
    ("SGD", dict(lr=1e-3, momentum=0.9, nesterov=True)),
    ("Adam", dict(lr=1e-2)),
]


def rel_err(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def train(n, optimizer, kw, **opts):
    c = engine.compile_model(W.build_readme_ar(W.native_api(), T=20), None, "pathwise")
    losses, finite = c.train(30, n, optimizer, seed=4, **opts, **kw)
    assert bool(finite.all())
    return losses.cpu().numpy(), c.params.cpu().numpy().copy(), c.last_mode


@pytest.mark.parametrize("n", [193, 256, 257, 300, 320])      # four and five sample waves: the draw service
@pytest.mark.parametrize("optimizer,kw", OPTIMIZERS)
def test_owner_wave_loop_equals_sample_wave_owners(n, optimizer, kw, monkeypatch):
    runs = {}
    for env in ("1", "0"):
        monkeypatch.setenv("BSVI_SPEC_OWNER_WAVE", env)
        runs[env] = train(n, optimizer, kw)
        assert runs[env][2] == "persistent"
    assert np.array_equal(runs["1"][0], runs["0"][0])
    assert np.array_equal(runs["1"][1], runs["0"][1])
    monkeypatch.setenv("BSVI_SPEC_OWNER_WAVE", "1")
    step_curve, step_params, mode = train(n, optimizer, kw, allow_persistent=False)
    assert mode == "stepwise"
    # (the bounds of test_in_kernel_loop_equals_launch_per_iteration)
    assert rel_err(step_curve, runs["1"][0]) <= 2e-6
    assert np.abs(step_params - runs["1"][1]).max() <= 2e-5


def test_owner_wave_two_calls_continue(monkeypatch):
    """a second call goes on from the first one's parameters, optimizer state and Adam step count"""
    curves = {}
    for env in ("1", "0"):
        monkeypatch.setenv("BSVI_SPEC_OWNER_WAVE", env)
        c = engine.compile_model(W.build_readme_ar(W.native_api(), T=20), None, "pathwise")
        a, fa = c.train(17, 300, "Adam", seed=2, lr=1e-2)
        b, fb = c.train(9, 300, "Adam", seed=2, lr=1e-2)
        assert bool(fa.all()) and bool(fb.all())
        curves[env] = (np.concatenate([a.cpu().numpy(), b.cpu().numpy()]), c.params.cpu().numpy().copy())
    assert np.array_equal(curves["1"][0], curves["0"][0])
    assert np.array_equal(curves["1"][1], curves["0"][1])
