"""The trimmed specialised kernels (specialize.cpp BSVI_SPEC_TRIM; spec_prelude.h SPEC_SAME, SPEC_ENT_NOISE, SPEC_FLUSH_MASK)
against the kernels as they were: BSVI_SPEC_TRIM=0, read when the program is created, generates every variant's source in its
previous form.  The same draws and the same arithmetic in the same order — a skipped `+ 0.0f` can change the sign of an exact
zero at most, which compares equal — so loss curve, finite flags and parameters must agree bit for bit.  Modelled on
tests/test_gpu_spec_tail.py.

The sample counts: 44 a lone partial wave, 64 a full wave, 65 one live lane in the last wave, 193 the same with four waves, 257
a count that cuts a 16-byte piece of the tile's rows, 300 the headline's 44 live lanes in the last wave; 42, 46 and 47 cut a
piece after two and after three live lanes, behind an even and an odd number of whole pieces."""
import numpy as np
import pytest

from brancher_amd import engine, native, workloads as W

pytestmark = pytest.mark.gpu

OPTIMIZERS = [
    ("SGD", dict(lr=1e-3)),
    ("Adam", dict(lr=1e-2)),
]


def train(builder, bkw, n, optimizer, kw, estimator="pathwise", calls=(30,), seed=4, **opts):
    """(curve, flags, parameters, last mode, launched variant, that variant's source) of a fresh model"""
    c = engine.compile_model(getattr(W, builder)(W.native_api(), **bkw), None, estimator)
    curves, flags = [], []
    for k in calls:
        losses, finite = c.train(k, n, optimizer, seed=seed, **opts, **kw)
        curves.append(losses.cpu().numpy())
        flags.append(finite.cpu().numpy())
    launched = native.load().bsvi_spec_last_variant()
    return (np.concatenate(curves), np.concatenate(flags), c.params.cpu().numpy().copy(), c.last_mode, launched,
            native.specialised_source(c.program, launched) if launched >= 0 else "")


def both(monkeypatch, *args, **kwargs):
    runs = {}
    for env in ("1", "0"):
        monkeypatch.setenv("BSVI_SPEC_TRIM", env)
        runs[env] = train(*args, **kwargs)
        assert runs[env][4] >= 0                                     # (a specialised kernel ran, not the interpreter)
        assert ("#define SPEC_TRIM 1\n" in runs[env][5]) == (env == "1")
    monkeypatch.delenv("BSVI_SPEC_TRIM")
    assert runs["1"][3] == runs["0"][3] and runs["1"][4] == runs["0"][4]
    return runs["1"], runs["0"]


def same(a, b):
    for x, y, what in zip(a[:3], b[:3], ("loss curve", "finite flags", "parameters")):
        diff = np.nanmax(np.abs(x.astype(np.float64) - y.astype(np.float64))) if np.isfinite(x).any() else 0.0
        print("%s: largest difference %.3g over %d values" % (what, diff, x.size))
        assert np.array_equal(x, y), what


@pytest.mark.parametrize("calls", [(1,), (2,), (30,), (17, 17)], ids=["1", "2", "30", "17+17"])
@pytest.mark.parametrize("n", [42, 44, 46, 47, 64, 65, 193, 257, 300])
@pytest.mark.parametrize("optimizer,kw", OPTIMIZERS)
def test_headline_program(n, optimizer, kw, calls, monkeypatch):
    new, prev = both(monkeypatch, "build_readme_ar", dict(T=20), n, optimizer, kw, calls=calls)
    print("n", n, "mode", new[3], "variant", new[4])
    assert new[3] == "persistent"
    assert new[0].size == sum(calls) and bool(new[1].all()) and np.isfinite(new[0]).all()
    if n == 300:
        assert new[4] == 6                                           # (the kernel bench.py measures)
    same(new, prev)


def test_blackbox_program(monkeypatch):
    new, prev = both(monkeypatch, "build_readme_ar", dict(T=20), 300, "Adam", dict(lr=1e-2), estimator="blackbox")
    assert np.isfinite(new[0]).all()
    same(new, prev)


@pytest.mark.parametrize("n", [64, 300])
def test_minibatch_loop(n, monkeypatch):
    """the gather phase compiled into the loop variants (tests/test_gpu_minibatch_loop.py's linear regression)"""
    new, prev = both(monkeypatch, "build_minibatch_linear_regression", dict(dataset_size=40, batch_size=8, n_features=3), n,
                     "SGD", dict(lr=1e-3), seed=5, minibatch_loop=True)
    assert new[3] == "persistent" and bool(new[1].all()) and np.isfinite(new[0]).all()
    same(new, prev)


def test_many_workgroups(monkeypatch):
    """256-thread workgroups walking several chunks of samples: the flush takes each chunk's count"""
    new, prev = both(monkeypatch, "build_beta_binomial", dict(), 4096, "Adam", dict(lr=1e-2), calls=(20,))
    print("mode", new[3], "variant", new[4])
    assert new[4] == 2
    assert bool(new[1].all()) and np.isfinite(new[0]).all()
    same(new, prev)


@pytest.mark.parametrize("n", [257, 300])
def test_step_kernel_equals_loop(n):
    """SGD: one launch per iteration (variant 0's step kernel) and the in-kernel loop, both trimmed: the same arithmetic in
    the same order"""
    loop = train("build_readme_ar", dict(T=20), n, "SGD", dict(lr=1e-3))
    step = train("build_readme_ar", dict(T=20), n, "SGD", dict(lr=1e-3), allow_persistent=False)
    assert loop[3] == "persistent" and step[3] == "stepwise"
    assert "#define SPEC_TRIM 1\n" in loop[5] and "#define SPEC_TRIM 1\n" in step[5]
    same(loop, step)
