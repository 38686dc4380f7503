"""Every middle kernel that the size of a Bayesian neural network selects (csrc/bnn_select.h) — bnn_mid_gen and
bnn_upper_gen at the limits of their own rules, bnn_upper<false> (activations and deltas in global memory), bnn_upper<true> — against
the oracle in DOUBLE precision on the draws the kernels report.  Each case first asserts the kernel it is on (`middle_path()`): a
case that lands elsewhere FAILS.  P = 32 features and N = 70 samples (n_pad 128, a ragged last wave) throughout; the widths are the
smallest that cross each rule (tests/c_abi/bnn_select_table.cpp holds the same rows for the selection function alone).

The bound is the suite's yardstick (conftest.yardstick_grad_check / yardstick_loss_check, unchanged) and, per named tensor, the same rule
with the floor taken from THAT tensor: err <= max(4 |oracle32 - oracle64|, 1e-5 max |oracle64|) over the tensor — the shared helper's
floor is the largest gradient of the whole model, under which a wrong bias gradient of an upper layer can hide."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from conftest import yardstick_grad_check, yardstick_loss_check
from brancher_amd import bnn, engine, lowering, native, workloads as W
from oracle.svi_oracle import Oracle

pytestmark = pytest.mark.gpu
TOL = 1e-5
N = 70
P = 32


def classifier(widths, batch_size, pixels, dataset_size=40, **kw):
    # the scale of weights1 keeps the hidden units off saturation: 0.4 / sqrt(sum_p E x_p^2), as build_bnn_regression chooses it
    ex2 = dict(integers=4.0, unit=1.0 / 3.0, normal=1.0)[pixels]
    return ("classifier", dict(dict(widths=widths, batch_size=batch_size, dataset_size=dataset_size, pixels=pixels,
                                    q_scale1=0.4 / np.sqrt(P * ex2), q_loc_scale=1.0), **kw))


def regression(widths, batch_size, data, dataset_size=40, **kw):
    return ("regression", dict(dict(widths=widths, batch_size=batch_size, dataset_size=dataset_size, data=data, q_scale=0.3), **kw))


CYCLE = ["tanh", "relu", "sigmoid", "softplus", "tanh", "relu", "sigmoid"]
CASES = {
    # id: (builder and keywords, data path, middle kernel)
    "a": (classifier([P, 48, 44, 4], 17, "integers"), "bf16x3", "mid_gen"),          # act 96, Rs 2384: the largest element tables
    "b": (classifier([P, 48, 44, 5], 17, "integers"), "bf16x3", "upper_mem"),        # act 97: exact data, three-piece dlogp stores
    "c": (classifier([P, 16, 16, 4], 17, "unit"), "f32", "upper_mem"),               # Rs 356, 428 floats: the da1T store
    "d": (classifier([P, 16, 14, 4], 17, "normal"), "f32", "upper_gen"),             # Rs 314, 382 floats: chosen by its own rule
    "e": (classifier([P, 32, 8], 448, "integers", dataset_size=460), "bf16x3", "mid_gen"),      # a tile of 145 824 bytes
    "f": (classifier([P, 32, 8], 449, "integers", dataset_size=460), "bf16x3", "upper_gen"),    # B_pad 480: 156 064 bytes refused
    "g": (classifier([P, 18, 18, 1], 33, "unit"), "f32", "upper_mem"),               # one logit: Bernoulli
    "h": (regression([P, 18, 18, 3], 33, "normal", sigma=[0.3, 0.5, 0.8]), "f32", "upper_mem"),      # Normal, a sigma per output
    "i": (classifier([P, 6, 6, 6, 6, 6, 6, 6, 3], 17, "integers", activations=CYCLE, q_scale=0.5), "bf16x3", "mid_gen"),      # eight layers
}


def build(spec):
    kind, kw = spec
    make = W.build_bayesian_neural_network if kind == "classifier" else W.build_bnn_regression
    return make(W.native_api(), **kw)


def compile_bnn(spec, estimator):
    model = build(spec)
    c = bnn.CompiledBnn(model, model.posterior_model, estimator)
    assert type(c).__name__ == "CompiledBnn"
    return c


def per_tensor_check(named, exact, ref32, label=""):
    """the yardstick with each tensor's own floor; prints every figure before it asserts"""
    worst = []
    for name, g64 in exact.items():
        if g64 is None:
            continue
        err, yard, scale = np.abs(named[name] - g64).max(), np.abs(ref32[name] - g64).max(), np.abs(g64).max()
        bound = max(4 * yard, TOL * scale)
        print("%s %-16s err %.3g  oracle32 %.3g  scale %.3g  err/bound %.3g" % (label, name, err, yard, scale, err / bound if bound else 0.0))
        if not err <= bound:
            worst.append((name, err, yard, scale))
    assert not worst, worst


def check_against(c, res, exact, ref32, label=""):
    """loss, per-sample f (floor: 1e-6 of its summands, as tests/test_gpu_bnn.py) and every gradient, the model's and each tensor's floor"""
    f64 = exact["f"].reshape(-1)
    summands = float(np.abs(f64).max()) + 0.5 * c.program.n_rows * 3.0
    f_err, f_yard = np.abs(res["f"].cpu().numpy() - f64).max(), np.abs(ref32["f"].reshape(-1) - f64).max()
    loss = float(res["loss"].item())
    print(label, "f err %.3g oracle32 %.3g floor %.3g | loss %.9g oracle64 %.9g oracle32 %.9g" % (f_err, f_yard, 1e-6 * summands, loss, exact["loss"], ref32["loss"]))
    assert np.isfinite(loss) and float(res["finite"].item()) == 1.0
    assert f_err <= max(4 * f_yard, 1e-6 * summands)
    assert abs(loss - exact["loss"]) <= max(4 * abs(ref32["loss"] - exact["loss"]), TOL * abs(exact["loss"]), 1e-6 * summands), \
        (loss, exact["loss"], ref32["loss"])
    grads = c.named_grads()
    yardstick_grad_check(grads, exact["grads"], ref32["grads"])
    per_tensor_check(grads, exact["grads"], ref32["grads"], label)


def oracle_pair(spec, estimator, named, mb, n=N):
    return (Oracle(build(spec), dtype=torch.float64).loss_and_grads(n, estimator, named, mb),
            Oracle(build(spec)).loss_and_grads(n, estimator, named, mb))


def run_case(spec, path, middle, estimator, label):
    c = compile_bnn(spec, estimator)
    assert c.middle_path() == middle and c.data_path() == path, (c.middle_path(), c.data_path())
    kw = spec[1]
    res = c.evaluate(N, seed=3, offset=5, want_noise=True, want_indices=True, want_fvalues=True)
    assert c.middle_path() == middle
    idx = res["indices"].cpu().numpy()
    assert len(set(idx.tolist())) == kw["batch_size"] and idx.min() >= 0 and idx.max() < kw["dataset_size"]
    named = c.named_noise(res["noise"].cpu().numpy(), N)
    mb = {c.program.indices_name: idx.tolist()}
    exact, ref32 = oracle_pair(spec, estimator, named, mb)
    check_against(c, res, exact, ref32, label)
    loss = float(res["loss"].item())
    # the same draws fed back in: the noise-in path of every kernel (and bit-equal repeat calls)
    res2 = c.evaluate(N, noise=named, minibatch=mb, want_fvalues=True)
    assert abs(float(res2["loss"].item()) - loss) <= 2e-6 * max(1.0, abs(loss))
    check_against(c, res2, exact, ref32, label + " noise-in")
    g2 = c.named_grads()
    res3 = c.evaluate(N, noise=named, minibatch=mb, want_fvalues=True)
    assert torch.equal(res2["f"], res3["f"]) and all(np.array_equal(g2[k], v) for k, v in c.named_grads().items())
    return c


@pytest.mark.parametrize("estimator", ["pathwise", "blackbox"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_every_selected_middle_matches_the_oracle_on_the_reported_draws(case, estimator):
    spec, path, middle = CASES[case]
    run_case(spec, path, middle, estimator, "%s %s" % (case, estimator))


@pytest.mark.parametrize("estimator", ["pathwise", "blackbox"])
@pytest.mark.parametrize("switches,kind", [(dict(BSVI_BNN_MID="0"), "upper_gen"), (dict(BSVI_BNN_MID="0", BSVI_BNN_JIT="0"), "static")])
def test_eight_layers_on_the_kernels_behind_the_switches(switches, kind, estimator, monkeypatch):
    """case i (mid_gen in the test above) on bnn_upper_gen and on the static kernel; which static kernel: what the selection gives for
    Rs 279 and 45 units — (279 * 65 + 90 * 256) * 4 = 164 700 bytes, beyond LDS: the memory kernel"""
    for k, v in switches.items():
        monkeypatch.setenv(k, v)
    spec, path, _ = CASES["i"]
    c = run_case(spec, path, "upper_gen" if kind == "upper_gen" else "upper_mem", estimator, "i %s %s" % (kind, estimator))
    assert len(c.program.layers) == 8


@functools.lru_cache(maxsize=None)
def case_c_draws(estimator, seed=21, offset=4):
    """case c once per estimator: the compiled model, its draws of (seed, offset) and the two oracles on them (left unchanged)"""
    spec, path, middle = CASES["c"]
    c = compile_bnn(spec, estimator)
    assert c.middle_path() == middle and c.data_path() == path
    res = c.evaluate(N, seed=seed, offset=offset, want_noise=True, want_indices=True, want_fvalues=True)
    named = c.named_noise(res["noise"].cpu().numpy(), N)
    mb = {c.program.indices_name: res["indices"].cpu().numpy().tolist()}
    exact, ref32 = oracle_pair(spec, estimator, named, mb)
    check_against(c, res, exact, ref32, "c %s (seed %d)" % (estimator, seed))
    return c, named, mb, exact, ref32


def test_sample_shards_with_a_base_sum_to_the_whole_on_the_memory_kernel():
    """case c split 33 + 37 (sample_base 33 in the second shard: other Philox counters, a partial wave in both): the output blocks add up
    to the whole's — the bounds of the shard tests of test_gpu_bnn.py / test_gpu_bnn_normal.py — and the whole agrees with the oracle"""
    from brancher_amd.native import OUT_HEADER
    c, named, mb, exact, ref32 = case_c_draws("pathwise")
    blocks = []
    for base, n_local in ((0, N), (0, 33), (33, 37)):
        args = c._args(n_local, N, base, seed=21, offset=4)
        native.check(c.lib.bsvi_bnn_fwd_bwd(c.handle, C.byref(args)))
        blocks.append(c.out.detach().cpu().numpy().copy())
        native.check(c.lib.bsvi_bnn_fwd_bwd(c.handle, C.byref(args)))
        assert np.array_equal(blocks[-1], c.out.detach().cpu().numpy())
    whole, a, b = blocks
    assert np.isfinite(whole).all() and whole[1] == 0.0
    scale = np.abs(whole[OUT_HEADER:]).max()
    assert scale > 0 and np.abs(a[OUT_HEADER:] + b[OUT_HEADER:] - whole[OUT_HEADER:]).max() <= 2e-5 * scale
    assert abs(a[0] + b[0] - whole[0]) <= 2e-6 * (abs(whole[0]) + N * c.program.n_rows)
    # the sums of the whole are the oracle's: loss = -(sum_n value_n) / N
    yardstick_loss_check(-whole[0] / N, exact["loss"], ref32["loss"])


def test_caller_weights_on_the_memory_kernel():
    """`evaluate_weighted` with weights that differ from sample to sample (what the second pass of engine.custom_estimator_loss hands
    down): the output block is -(sum_n a_n grad f_n + b_n grad log q_n) — the oracle differentiates that sum itself"""
    c, named, mb, _, _ = case_c_draws("blackbox")
    rng = np.random.RandomState(11)
    a, b = rng.uniform(0.2, 1.8, N) / N, rng.normal(0.0, 1.0, N) / N
    g = lambda f, lq: (torch.as_tensor(a, dtype=f.dtype) * f.reshape(-1)).sum() + (torch.as_tensor(b, dtype=lq.dtype) * lq.reshape(-1)).sum()
    exact, ref32 = oracle_pair(CASES["c"][0], g, named, mb)
    c.evaluate_weighted(N, torch.as_tensor(a, dtype=torch.float32, device=c.device), torch.as_tensor(b, dtype=torch.float32, device=c.device),
                        seed=0, offset=0, noise=named, minibatch=mb)
    grads = c.named_grads()
    yardstick_grad_check(grads, exact["grads"], ref32["grads"])
    per_tensor_check(grads, exact["grads"], ref32["grads"], "c weighted")


def test_six_adam_steps_on_the_memory_kernel_follow_the_oracle():
    """`train()` on case c with the draws and minibatches of a fixed sequence: every loss finite, losses and parameters after six steps
    within the yardstick of the double-precision oracle's trajectory (the bounds of the golden trajectory tests)"""
    spec, path, middle = CASES["c"]
    kw, iters = spec[1], 6
    c = compile_bnn(spec, "pathwise")
    assert c.middle_path() == middle
    rng = np.random.RandomState(5)
    noise_seq = [{t["name"]: rng.normal(size=(N, 1, t["rows"], t["cols"])).astype(np.float32) for t in c.program.tensors} for _ in range(iters)]
    mb_seq = [{c.program.indices_name: rng.permutation(kw["dataset_size"])[:kw["batch_size"]].tolist()} for _ in range(iters)]
    losses, finite = c.train(iters, N, "Adam", noise_seq=noise_seq, minibatch_seq=mb_seq, lr=0.01)
    got = losses.cpu().numpy().astype(np.float64)
    assert c.last_mode == "stepwise" and np.isfinite(got).all() and finite.cpu().numpy().all()
    o64, o32 = Oracle(build(spec), dtype=torch.float64), Oracle(build(spec))
    l64 = o64.train(iters, N, "Adam", noise_seq=noise_seq, minibatch_seq=mb_seq, lr=0.01).astype(np.float64)
    l32 = o32.train(iters, N, "Adam", noise_seq=noise_seq, minibatch_seq=mb_seq, lr=0.01).astype(np.float64)
    print("losses", got, l64, l32)
    # (Oracle.train returns its losses as float32: half an ulp of them is part of what the yardstick can resolve)
    assert np.abs(got - l64).max() <= max(4 * np.abs(l32 - l64).max(), TOL * np.abs(l64).max())
    p64 = {k: t.detach().numpy() for k, t in o64.named_parameters().items()}
    p32 = {k: t.detach().numpy() for k, t in o32.named_parameters().items()}
    for pname, p in c.named_params().items():
        e64 = p64[pname].reshape(p.shape)
        assert np.abs(p - e64).max() <= max(4 * np.abs(p32[pname].reshape(p.shape) - e64).max(), 2e-5 * (1 + np.abs(e64).max())), pname


def test_nine_layers_are_refused_by_the_lowering_with_the_limit_named():
    """by `lower_bnn` (tests/test_bnn_select_cpu.py asks it without a device), so that `engine.compile_model` names the limit among
    its four reasons; the layers are wide enough (4 800 products) that the scalar path does not take the model"""
    model = W.build_bayesian_neural_network(W.native_api(), widths=[P] + [24] * 8 + [3], batch_size=17, dataset_size=40, pixels="integers")
    with pytest.raises(lowering.LoweringError, match="at most 8"):
        bnn.lower_bnn(model, model.posterior_model, "pathwise")
    with pytest.raises(lowering.LoweringError, match="bnn path: the network has 9 layers, the kernels serve at most 8"):
        engine.compile_model(model, None, "pathwise")
