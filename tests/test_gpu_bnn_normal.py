"""The regression model of the Bayesian-neural-network family on the device: `NormalVariable(chain, sigma)` observed on a minibatch of
real targets (workloads.build_bnn_regression, bnn.lower_bnn, bsvi_bnn_create_normal; the likelihood BSVI_LIK_NORMAL at the three sites
of csrc/bnn_kernel.inc).  The bounds are the suite's yardstick as tests/test_gpu_bnn.py and test_gpu_parity.py use it: the truth is the
oracle in DOUBLE precision on the same draws, and the kernels must be as close to it as the reference arithmetic — the oracle in single
precision, or a fixture of the real reference — is (x4), or within 1e-5 of the scale; for the per-sample f, 1e-6 of its summands.
The shapes are the smallest that cross every boundary of the kernels: a padded minibatch (17 and 33 rows: B_pad 32 and 64), n_pad of
64 with a partial last wave (N 65, 70, 130), more than one output, both data paths and the generated and the generic middle."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import Golden, yardstick_grad_check
from brancher_amd import bnn, engine, native, workloads as W
from oracle.svi_oracle import Oracle

pytestmark = pytest.mark.gpu
TOL = 1e-5
A = dict(dataset_size=40, batch_size=17, n_features=64, n_hidden=9, n_outputs=1)                                     # 64-9-1, tanh
B = dict(dataset_size=40, batch_size=33, n_features=36, n_hidden=5, hidden2=4, n_outputs=3, activation="relu", data="normal",
         sigma=[0.3, 0.5, 0.8])                                                                                      # 36-5-4-3, relu
ONE_LAYER = dict(dataset_size=24, batch_size=8, n_features=32, n_hidden=0, n_outputs=2, bias=False)                  # 32-2
SMALL = dict(dataset_size=40, batch_size=17, n_features=16, n_hidden=5, n_outputs=2)                                 # 16-5-2: both engines
FIXTURES = ["bnn_normal/bnn_normal_tanh_P32_H6_C1_DS30_B12_N5", "bnn_normal/bnn_normal_linear_P16_C2_DS24_B10_N6"]
CUSTOM = {"baseline": lambda f, lq: (lq * (f - f.mean()).detach() + f).mean()}


def build(kw):
    return W.build_bnn_regression(W.native_api(), **kw)


def compile_bnn(kw, estimator="pathwise", direct=False):
    """through the public route — or, for a model small enough for the scalar path (which keeps it), straight to the family's engine"""
    model = build(kw)
    c = bnn.CompiledBnn(model, model.posterior_model, estimator) if direct else engine.compile_model(model, None, estimator)
    assert type(c).__name__ == "CompiledBnn" and c.program.likelihood == bnn.LIK_NORMAL
    return c


def check_against(c, res, exact, yard, label="", n_rows=None):
    """loss, per-sample f and every gradient: err <= max(4 |yardstick - oracle64|, 1e-5 scale); f: the 1e-6 summands floor"""
    f64 = exact["f"].reshape(-1)
    # f = lp + H cancels: measured against its summands, as tests/test_gpu_bnn.py does
    summands = float(np.abs(f64).max()) + 0.5 * (n_rows or c.program.n_rows) * 3.0
    f_err, f_yard = np.abs(res["f"].cpu().numpy() - f64).max(), np.abs(np.asarray(yard["f"]).reshape(-1) - f64).max()
    loss = float(res["loss"].item())
    print(label, "f err %.3g yard %.3g floor %.3g | loss %.9g exact %.9g yard %.9g" % (f_err, f_yard, 1e-6 * summands, loss, exact["loss"], yard["loss"]))
    assert f_err <= max(4 * f_yard, 1e-6 * summands)
    assert abs(loss - exact["loss"]) <= max(4 * abs(yard["loss"] - exact["loss"]), TOL * abs(exact["loss"]), 1e-6 * summands), \
        (loss, exact["loss"], yard["loss"])
    yardstick_grad_check(c.named_grads(), exact["grads"], yard["grads"])


@pytest.mark.parametrize("estimator", ["pathwise", "blackbox"])
@pytest.mark.parametrize("kw,n,path,direct", [(A, 70, "bf16x3", False), (B, 130, "f32", False), (ONE_LAYER, 65, "bf16x3", True)],
                         ids=["64-9-1", "36-5-4-3", "32-2"])
def test_philox_path_matches_the_oracle_on_the_reported_draws(kw, n, path, direct, estimator):
    c = compile_bnn(kw, estimator, direct)
    assert c.data_path() == path
    res = c.evaluate(n, seed=3, offset=5, want_noise=True, want_indices=True, want_fvalues=True)
    idx = res["indices"].cpu().numpy()
    assert len(set(idx.tolist())) == kw["batch_size"] and idx.min() >= 0 and idx.max() < kw["dataset_size"]
    named = c.named_noise(res["noise"].cpu().numpy(), n)
    mb = {c.program.indices_name: idx.tolist()}
    exact = Oracle(build(kw), dtype=torch.float64).loss_and_grads(n, estimator, named, mb)
    ref32 = Oracle(build(kw)).loss_and_grads(n, estimator, named, mb)
    check_against(c, res, exact, ref32, "%s %s" % (kw["n_features"], estimator))
    loss = float(res["loss"].item())
    # the same draws fed back in: the noise-in path of every kernel (and bit-equal repeat calls)
    res2 = c.evaluate(n, noise=named, minibatch=mb, want_fvalues=True)
    assert abs(float(res2["loss"].item()) - loss) <= 2e-6 * max(1.0, abs(loss))
    g2 = c.named_grads()
    res3 = c.evaluate(n, noise=named, minibatch=mb, want_fvalues=True)
    assert torch.equal(res2["f"], res3["f"]) and all(np.array_equal(g2[k], v) for k, v in c.named_grads().items())


@pytest.mark.parametrize("estimator", ["pathwise", "blackbox"])
@pytest.mark.parametrize("kw,n", [(A, 70), (B, 130)], ids=["64-9-1", "36-5-4-3"])
def test_the_three_likelihood_sites_agree(kw, n, estimator, monkeypatch):
    """the generated middle (bnn_mid_gen, exact data only), the generated upper kernel (bnn_upper_gen) and the static bnn_upper each
    compute the Normal likelihood and d f / d (last layer): the same arithmetic per (sample, row), sums over the minibatch in another
    association — the bounds of test_gpu_bnn.test_generated_middle_equals_the_separate_launches; each form bit-reproducible"""
    def outputs():
        c = compile_bnn(kw, estimator)
        res = c.evaluate(n, seed=9, offset=2, want_fvalues=True)
        torch.cuda.synchronize()
        again = c.evaluate(n, seed=9, offset=2, want_fvalues=True)
        torch.cuda.synchronize()
        assert torch.equal(res["f"], again["f"]) and torch.equal(res["grads"], again["grads"])
        return float(res["loss"]), res["f"].cpu().numpy().astype(np.float64), res["grads"].cpu().numpy().astype(np.float64)

    gen = outputs()                                    # bnn_mid_gen on exact data (else bnn_upper_gen)
    monkeypatch.setenv("BSVI_BNN_MID", "0")
    upper_gen = outputs()                              # bnn_upper_gen + bnn_small + bnn_lik
    monkeypatch.setenv("BSVI_BNN_JIT", "0")
    generic = outputs()                                # bnn_upper + bnn_small + bnn_lik
    fscale, gscale = np.abs(generic[1]).max(), max(np.abs(generic[2]).max(), 1e-6)
    bb = estimator == "blackbox"
    for other in (gen, upper_gen):
        print(abs(other[0] - generic[0]) / abs(generic[0]), np.abs(other[1] - generic[1]).max() / fscale, np.abs(other[2] - generic[2]).max() / gscale)
        assert abs(other[0] - generic[0]) <= (2e-4 if bb else 2e-6) * abs(generic[0])
        assert np.abs(other[1] - generic[1]).max() <= 2e-6 * fscale
        assert np.abs(other[2] - generic[2]).max() <= (2e-4 if bb else 5e-6) * gscale


@pytest.mark.parametrize("estimator", ["pathwise", "blackbox"])
def test_exact_piece_products_equal_the_f32_input_products(estimator, monkeypatch):
    """small integers are exactly bf16: three bf16 MFMAs on the exact pieces of the other operand; BSVI_DENSE_XGEMM=0 (at create
    time) sends the same model through the f32-input kernels — the bounds of the test of this name in test_gpu_bnn.py"""
    out = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("BSVI_DENSE_XGEMM", flag)
        c = compile_bnn(A, estimator)
        assert c.data_path() == ("bf16x3" if flag == "1" else "f32")
        res = c.evaluate(70, seed=9, offset=1, want_fvalues=True)
        out[flag] = (res["f"].cpu().numpy(), float(res["loss"].item()), c.named_grads())
    fa, la, ga = out["1"]
    fb, lb, gb = out["0"]
    assert np.abs(fa - fb).max() <= 2e-6 * (np.abs(fb).max() + 1500.0)
    assert abs(la - lb) <= (2e-5 if estimator == "pathwise" else 2e-4) * abs(lb)
    gscale = max(np.abs(v).max() for v in gb.values())
    for name in gb:
        assert np.abs(ga[name] - gb[name]).max() <= (5e-5 if estimator == "pathwise" else 5e-4) * gscale, name


@pytest.mark.parametrize("estimator", ["pathwise", "blackbox"])
def test_the_scalar_path_and_the_mfma_path_agree_on_a_model_both_run(estimator, monkeypatch):
    """16-5-2 at 17 rows is small enough for the scalar engine, which `compile_model` keeps it on; the same model through the family's
    engine on the same named noise and minibatch: each within the yardstick of the double-precision oracle.  (The scalar engine's
    interpreter kernels: compiling the specialised kernel of this program's 2 700 unrolled terms alone takes seven seconds.)"""
    monkeypatch.setenv("BSVI_JIT", "0")
    n = 12
    model = build(SMALL)
    scalar = engine.compile_model(model, None, estimator)
    assert type(scalar).__name__ == "CompiledELBO"
    m2 = build(SMALL)
    mfma = bnn.CompiledBnn(m2, m2.posterior_model, estimator, program=bnn.lower_bnn(m2, m2.posterior_model, estimator))
    rng = np.random.RandomState(4)
    named = {t["name"]: rng.normal(size=(n, 1, t["rows"], t["cols"])).astype(np.float32) for t in mfma.program.tensors}
    mb = {"indices": rng.permutation(SMALL["dataset_size"])[:SMALL["batch_size"]].tolist()}
    exact = Oracle(build(SMALL), dtype=torch.float64).loss_and_grads(n, estimator, named, mb)
    ref32 = Oracle(build(SMALL)).loss_and_grads(n, estimator, named, mb)
    for c in (scalar, mfma):
        res = c.evaluate(n, noise=named, minibatch=mb, want_fvalues=True)
        check_against(c, res, exact, ref32, type(c).__name__, n_rows=mfma.program.n_rows)


@pytest.mark.parametrize("name", FIXTURES)
def test_the_reference_fixtures(name):
    """loss, per-sample f and gradients of both estimators, Taylor1, and the Adam trajectory against the real reference's records: the
    double-precision oracle is the truth, the fixture the yardstick (the `bnn` branch of
    test_gpu_parity.test_training_trajectory_matches_reference_golden)"""
    g = Golden(name)
    f_ref = (g.data["lp"] + g.data["H"]).reshape(-1)
    for estimator in ("pathwise", "blackbox"):
        model = g.build()
        c = bnn.CompiledBnn(model, model.posterior_model, estimator)
        res = c.evaluate(g.N, noise=g.noise, minibatch=g.minibatch, want_fvalues=True)
        assert float(res["finite"].item()) == 1.0
        exact = Oracle(g.build(), dtype=torch.float64).loss_and_grads(g.N, estimator, g.noise, g.minibatch)
        fixture = dict(f=f_ref, loss=float(g.data["loss_" + estimator]), grads=g.group("grad_%s/" % estimator))
        check_against(c, res, exact, fixture, "%s %s" % (name[-12:], estimator))
    model = g.build()
    c = bnn.CompiledBnn(model, model.posterior_model, "taylor1")
    exact = Oracle(g.build(), dtype=torch.float64).loss_and_grads(g.N, "taylor1", g.noise, g.minibatch)
    ref = float(g.data["loss_taylor1"])
    for kwargs in (dict(want_fvalues=True), dict()):
        res = c.evaluate(g.N, noise=g.noise, minibatch=g.minibatch, **kwargs)
        loss = float(res["loss"].item())
        assert abs(loss - exact["loss"]) <= max(4 * abs(ref - exact["loss"]), TOL * abs(exact["loss"])), (loss, ref, exact["loss"])
        yardstick_grad_check(c.named_grads(), exact["grads"], g.group("grad_taylor1/"))
    # the trajectory under Adam
    tr = g.meta["trajectory"]
    model = g.build()
    c = bnn.CompiledBnn(model, model.posterior_model, "pathwise")
    losses, finite = c.train(tr["iters"], tr["n"], tr["optimizer"], noise_seq=g.trajectory_noise(),
                             minibatch_seq=g.trajectory_minibatch(), **g.opt_kwargs())
    assert c.last_mode == "stepwise" and finite.cpu().numpy().all()
    o = Oracle(g.build(), dtype=torch.float64)
    exact_losses = o.train(tr["iters"], tr["n"], tr["optimizer"], noise_seq=g.trajectory_noise(),
                           minibatch_seq=g.trajectory_minibatch(), **g.opt_kwargs()).astype(np.float64)
    got, ref_l = losses.cpu().numpy().astype(np.float64), g.data["traj/losses"].astype(np.float64)
    assert np.abs(got - exact_losses).max() <= max(4 * np.abs(ref_l - exact_losses).max(), TOL * np.abs(exact_losses).max())
    after = g.group("traj/param_after/")
    exact_after = {pname: t.detach().numpy() for pname, t in o.named_parameters().items()}
    for pname, p in c.named_params().items():
        e64 = exact_after[pname].reshape(p.shape)
        assert np.abs(p - e64).max() <= max(4 * np.abs(after[pname] - e64).max(), 2e-5 * (1 + np.abs(e64).max())), pname


def test_a_user_defined_estimator_through_the_two_weighted_passes():
    """the baseline estimator of workloads.custom_estimators (a GradientEstimator subclass) on 64-9-1: two passes of the launches
    around the user's torch code, the second with caller weights (f_weight_dev / q_weight_dev scale the Normal likelihood's
    deltas), against the oracle's restatement of the estimator"""
    from brancher_amd import gradient_estimators as ge
    n = 70
    model = build(A)
    rng = np.random.RandomState(6)
    tensors = bnn.lower_bnn(model, model.posterior_model, "blackbox").tensors
    named = {t["name"]: rng.normal(size=(n, 1, t["rows"], t["cols"])).astype(np.float32) for t in tensors}
    mb = {"indices": rng.permutation(A["dataset_size"])[:A["batch_size"]].tolist()}
    value = engine.custom_estimator_loss(model, model.posterior_model, W.custom_estimators(ge)["baseline"], n, noise=named, minibatch=mb)
    assert type(value.compiled).__name__ == "CompiledBnn" and value.compiled.data_path() == "bf16x3"
    exact = Oracle(build(A), dtype=torch.float64).loss_and_grads(n, CUSTOM["baseline"], named, mb)
    ref32 = Oracle(build(A)).loss_and_grads(n, CUSTOM["baseline"], named, mb)
    loss = -float(value.detach().cpu())
    assert abs(loss - exact["loss"]) <= max(4 * abs(ref32["loss"] - exact["loss"]), TOL * abs(exact["loss"])), (loss, ref32["loss"], exact["loss"])
    yardstick_grad_check(value.compiled.named_grads(), exact["grads"], ref32["grads"])


def test_sums_are_linear_over_sample_shards():
    """36-5-4-3 over 130 samples: the output block of the whole equals the sum of the blocks of the shards 0..64 and 65..129 (the Philox
    counters are GLOBAL sample indices), call after call bit-identical — the bounds of the shard test of test_gpu_bnn.py, the value's
    floor scaled to this network: per sample f adds ~n_rows terms of O(1)"""
    from brancher_amd.native import OUT_HEADER
    c = compile_bnn(B)
    n = 130
    blocks = []
    for base, n_local in ((0, n), (0, 65), (65, 65)):
        args = c._args(n_local, n, base, seed=21, offset=4)
        native.check(c.lib.bsvi_bnn_fwd_bwd(c.handle, C.byref(args)))
        blocks.append(c.out.detach().cpu().numpy().copy())
        native.check(c.lib.bsvi_bnn_fwd_bwd(c.handle, C.byref(args)))
        assert np.array_equal(blocks[-1], c.out.detach().cpu().numpy())
    whole, a, b = blocks
    assert np.isfinite(whole).all() and whole[1] == 0.0
    scale = np.abs(whole[OUT_HEADER:]).max()
    assert scale > 0 and np.abs(a[OUT_HEADER:] + b[OUT_HEADER:] - whole[OUT_HEADER:]).max() <= 2e-5 * scale
    assert abs(a[0] + b[0] - whole[0]) <= 2e-6 * (abs(whole[0]) + n * c.program.n_rows)


def test_two_rank_step_sequence_equals_the_fused_step():
    """bsvi_bnn_fwd_bwd + bsvi_finalize_step (what a rank of the sharded path runs around its all-reduce) against bsvi_bnn_step"""
    a, b = compile_bnn(A), compile_bnn(A)
    la, _ = a.train(6, 40, "Adam", seed=2, lr=1e-2)
    lb, _ = b.train(6, 40, "Adam", seed=2, lr=1e-2, _force_sharded_path=True)
    assert a.last_mode == "stepwise" and b.last_mode == "stepwise"
    np.testing.assert_allclose(lb.cpu().numpy(), la.cpu().numpy(), rtol=1e-6)
    np.testing.assert_allclose(b.params.cpu().numpy(), a.params.cpu().numpy(), rtol=1e-6, atol=1e-7)


def test_regression_trains_through_the_public_api_and_the_classifiers_are_served_as_before():
    from brancher_amd import inference
    model = build(A)
    inference.perform_inference(model, number_iterations=60, number_samples=50, optimizer="Adam", lr=0.01)
    curve = np.asarray(model.diagnostics["loss curve"])
    assert len(curve) == 60 and np.all(np.isfinite(curve)) and curve[-10:].mean() < curve[:10].mean()
    assert type(engine.compile_model(model)).__name__ == "CompiledBnn"
    # a 64-9-1 network of the classifier builder: the same engine class, and a loss bit-equal between two calls
    kw = dict(dataset_size=40, batch_size=17, n_features=64, n_hidden=9, n_classes=1, q_scale1=3e-3, q_loc_scale=1.0)
    c = engine.compile_model(W.build_bayesian_neural_network(W.native_api(), **kw), None, "pathwise")
    assert type(c).__name__ == "CompiledBnn" and c.program.likelihood == bnn.LIK_BERNOULLI
    first = c.evaluate(70, seed=3, offset=5)["loss"].clone()
    assert torch.isfinite(first) and torch.equal(first, c.evaluate(70, seed=3, offset=5)["loss"])
