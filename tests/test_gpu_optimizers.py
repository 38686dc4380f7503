"""AdamW, RMSprop, Adagrad and Adamax in the fused device step (bsvi_device.h: optimizer_apply_more), at every site that steps.

  1  the step itself, per element, against torch.optim in double precision: bsvi_optimizer_step and bsvi_finalize_step on
     handed-in gradients, parameters AND state planes, the ownership mask, the finite flag
  2  the scalar path in its three launch modes (in-kernel loop, launch per iteration, graph replay) at the sample counts where
     the selection of the generated kernel changes (tests/test_gpu_spec_select.py), against the oracle on predicted noise
  3  state kept across two calls (the running products of the loop are rebuilt), a parameter first stepped after the
     pretraining iterations (Adagrad's sum starts then), a non-finite loss
  4  the dense, BNN and amortised paths and the in-kernel minibatch loop, one kind each, against their oracles
  5  perform_inference and a hand-written loop with ProbabilisticOptimizer.update()

Bounds.  (1): the project's yardstick rule per case, max(4 |torch_f32 - torch_f64|, 1e-5 max|value|), the value being the
parameters or one state plane.  (2), (3): those of tests/test_gpu_noise.py (train_all_modes_against_the_oracle, restated here).
(4): those of each path's own trajectory test (tests/test_gpu_parity.py, tests/test_gpu_amortized.py).  (5): those of
tests/test_gpu_specialised.py.

Every bound is the issue's or the named test's; none was chosen from a result.  Measured on an MI355X (`pytest -s` prints the
figures): (1) parameters within 2.5e-07 ... 7.5e-07 of torch in double precision at bounds of 3.0e-05 ... 3.2e-05 — for
RMSprop, Adagrad and Adamax the device's error equals torch's own in single precision to the printed digits."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import Golden, rel_err
from brancher_amd import distributions as D
from brancher_amd import engine, inference, native, workloads as W
from brancher_amd.optimizers import ProbabilisticOptimizer
from oracle import philox_ref as R

pytestmark = pytest.mark.gpu
TOL = 1e-5


# ---- 1. the step against torch.optim, per element ------------------------------------------------------------------------
P, STEPS = 70, 12                                         # one full wave and a partial one
MASKED = (3, 40, 64, 69)

# (kind, torch options, {torch state entry: plane}) — the planes of the table at bsvi_opt_cfg (include/bsvi.h)
STEP_CASES = {
    "AdamW": ("AdamW", dict(), dict(exp_avg=0, exp_avg_sq=1)),
    "AdamW-all": ("AdamW", dict(lr=3e-3, betas=(0.8, 0.95), eps=1e-6, weight_decay=0.1, amsgrad=True),
                  dict(exp_avg=0, exp_avg_sq=1, max_exp_avg_sq=2)),
    "RMSprop": ("RMSprop", dict(), dict(square_avg=1)),
    "RMSprop-all": ("RMSprop", dict(lr=3e-3, alpha=0.9, eps=1e-6, weight_decay=0.1, momentum=0.7, centered=True),
                    dict(momentum_buffer=0, square_avg=1, grad_avg=2)),
    "Adagrad": ("Adagrad", dict(), dict(sum=1)),
    "Adagrad-all": ("Adagrad", dict(lr=3e-2, lr_decay=0.05, initial_accumulator_value=0.3, weight_decay=0.1, eps=1e-6), dict(sum=1)),
    "Adamax": ("Adamax", dict(), dict(exp_avg=0, exp_inf=1)),
    "Adamax-all": ("Adamax", dict(lr=3e-3, betas=(0.8, 0.95), eps=1e-6, weight_decay=0.1), dict(exp_avg=0, exp_inf=1)),
    "Adamax-maximize": ("Adamax", dict(maximize=True), dict(exp_avg=0, exp_inf=1)),
}


def step_inputs():
    rng = np.random.RandomState(12)
    p0 = rng.normal(0, 1, P).astype(np.float32)
    grads = (rng.normal(0, 1, (STEPS, P)) * rng.choice([1e-3, 1.0, 30.0], (STEPS, P))).astype(np.float32)
    mask = np.ones(P, dtype=np.uint8)
    mask[list(MASKED)] = 0
    return p0, grads, mask


def torch_steps(name, kw, p0, grads, dtype):
    p = torch.tensor(p0, dtype=dtype, requires_grad=True)
    opt = getattr(torch.optim, name)([p], **kw)
    for g in grads:
        p.grad = torch.tensor(g, dtype=dtype)
        opt.step()
    (state,) = opt.state_dict()["state"].values()
    return p.detach().numpy().astype(np.float64), {k: np.asarray(v, dtype=np.float64) for k, v in state.items()}


def torch_options(name, cfg):
    """torch's options read back from the words of the configuration: bsvi_opt_cfg carries single-precision numbers, and the
    reference steps with the values the device is given (beta2 = 0.999 is 1.3e-5 of 1 - beta2 away from its float: the same
    arithmetic on two different configurations would differ by that much in exp_avg_sq)"""
    common = dict(lr=cfg.lr, eps=cfg.eps, weight_decay=cfg.weight_decay, maximize=bool(cfg.maximize))
    if name == "AdamW":
        return dict(common, betas=(cfg.beta1, cfg.beta2), amsgrad=bool(cfg.amsgrad))
    if name == "RMSprop":
        return dict(common, alpha=cfg.beta2, momentum=cfg.momentum, centered=bool(cfg.amsgrad))
    if name == "Adagrad":
        return dict(common, lr_decay=cfg.dampening, initial_accumulator_value=cfg.beta1)
    return dict(common, betas=(cfg.beta1, cfg.beta2))


_REFERENCE = {}


def reference(case):
    """torch in double precision (the truth) and in single precision (the yardstick), once per case"""
    if case not in _REFERENCE:
        name, kw, _ = STEP_CASES[case]
        kw = torch_options(name, native.make_opt_cfg(name, **kw))
        p0, grads, _ = step_inputs()
        _REFERENCE[case] = (torch_steps(name, kw, p0, grads, torch.float64), torch_steps(name, kw, p0, grads, torch.float32))
    return _REFERENCE[case]


def buffers(p0, mask):
    dev = torch.device("cuda:0")
    return (torch.from_numpy(p0.copy()).to(dev), torch.zeros(4 * P, device=dev), torch.from_numpy(mask).to(dev),
            torch.zeros(native.OUT_HEADER + P, device=dev))


def run_device(entry, cfg, p0, grads, mask, start=None, finite=True):
    """the gradients handed in through the output block, one launch each; -> (parameters, state [4 P]) after the last"""
    lib, ptr = native.load(), lambda t: C.c_void_p(t.data_ptr())
    params, state, m, out = buffers(p0, mask)
    if start is not None:
        params.copy_(start[0])
        state.copy_(start[1])
    for g in grads:
        block = np.zeros(native.OUT_HEADER + P, dtype=np.float32)
        if entry == "optimizer_step":
            block[3] = 1.0 if finite else 0.0
            block[native.OUT_HEADER:] = g
            out.copy_(torch.from_numpy(block))
            native.check(lib.bsvi_optimizer_step(C.byref(cfg), ptr(params), ptr(out), ptr(state), ptr(m), P, None))
        else:
            # one "sample": the launch scales the sums by -1 / 1, exactly
            block[0] = 1.0 if finite else np.nan
            block[native.OUT_HEADER:] = -g
            out.copy_(torch.from_numpy(block))
            native.check(lib.bsvi_finalize_step(C.byref(cfg), ptr(params), ptr(out), ptr(state), ptr(m), P, 1, None, None, None))
            torch.cuda.synchronize()
            assert float(out[3]) == (1.0 if finite else 0.0)
    torch.cuda.synchronize()
    return params, state


@pytest.mark.parametrize("entry", ["optimizer_step", "finalize_step"])
@pytest.mark.parametrize("case", sorted(STEP_CASES))
def test_step_equals_torch_optim_per_element(case, entry):
    name, kw, planes = STEP_CASES[case]
    p0, grads, mask = step_inputs()
    (p64, s64), (p32, s32) = reference(case)
    cfg = native.make_opt_cfg(name, **kw)
    params, state = run_device(entry, cfg, p0, grads, mask)
    got_p, got_s = params.cpu().numpy(), state.cpu().numpy().reshape(4, P)
    on = mask != 0
    bound = max(4 * np.abs(p32 - p64).max(), 1e-5 * np.abs(p64).max())
    err = np.abs(got_p[on] - p64[on]).max()
    print("%s %s: parameters |device - torch64| %.3g, |torch32 - torch64| %.3g, bound %.3g, max|p| %.3g" % (
        case, entry, err, np.abs(p32 - p64).max(), bound, np.abs(p64).max()))
    assert np.all(np.isfinite(got_p)) and err <= bound
    assert np.abs(got_p[on] - p0[on]).max() > 1e-3                   # (the steps moved them)
    for key, plane in planes.items():
        sbound = max(4 * np.abs(s32[key] - s64[key]).max(), 1e-5 * np.abs(s64[key]).max())
        serr = np.abs(got_s[plane][on] - s64[key][on]).max()
        print("  %s (plane %d): |device - torch64| %.3g, bound %.3g" % (key, plane, serr, sbound))
        assert serr <= sbound, key
    assert np.all(got_s[3][on] == float(STEPS)) and np.all(s64["step"] == float(STEPS))
    # a plane the kind does not use stays zero
    for plane in set(range(3)) - set(planes.values()):
        assert not got_s[plane].any(), plane
    # parameters the mask leaves out, and their state: untouched bit for bit
    assert np.array_equal(got_p[~on].view(np.uint32), p0[~on].view(np.uint32))
    assert not got_s[:, ~on].any()
    # the finite flag 0: nothing changes, the step counts included
    again_p, again_s = run_device(entry, cfg, p0, grads[:2], mask, start=(params, state), finite=False)
    assert np.array_equal(again_p.cpu().numpy().view(np.uint32), got_p.view(np.uint32))
    assert np.array_equal(again_s.cpu().numpy().view(np.uint32), got_s.reshape(-1).view(np.uint32))


def test_unknown_kind_is_refused():
    cfg = native.make_opt_cfg("Adamax")
    cfg.kind = 6
    p0, grads, mask = step_inputs()
    lib, ptr = native.load(), lambda t: C.c_void_p(t.data_ptr())
    params, state, m, out = buffers(p0, mask)
    assert lib.bsvi_optimizer_step(C.byref(cfg), ptr(params), ptr(out), ptr(state), ptr(m), P, None) != 0
    assert lib.bsvi_finalize_step(C.byref(cfg), ptr(params), ptr(out), ptr(state), ptr(m), P, 1, None, None, None) != 0


# ---- 2. every launch mode and loop variant of the scalar path (tests/test_gpu_noise.py's helper, restated) -----------------
MODES = (("persistent", dict()), ("stepwise", dict(allow_persistent=False)), ("graph", dict(_force_sharded_path=True)))
SEED = 1234


def softplus32(raw):
    raw = np.float32(raw)
    return float(raw if raw > 20 else np.log1p(np.exp(raw, dtype=np.float32), dtype=np.float32))


def named_noise(c, rows_by_index, n):
    noise = np.stack([rows_by_index[r] for r in range(c.program.n_noise)])
    return {name: noise[s.base:s.base + s.size].T.reshape((n,) + tuple(s.shape)) for name, s in c.program.slot_by_name.items()}


class PredictedNoise:
    """noise_seq of the oracle: iteration `it` draws at offset0 + it (oracle/philox_ref.py, the host reference of the stream)"""

    def __init__(self, c, oracle, seed, offset0, n):
        self.c, self.oracle, self.seed, self.offset0, self.n = c, oracle, seed, offset0, n

    def __getitem__(self, it):
        par = {k: v.detach().numpy().astype(np.float32).reshape(-1) for k, v in self.oracle.named_parameters().items()}
        rows = []
        for name, s in self.c.program.slot_by_name.items():
            for j in range(s.size):
                p0 = p1 = 0.0
                if s.dist == D.DIST_BETA:
                    p0, p1 = softplus32(par[name + "_concentration1"][j]), softplus32(par[name + "_concentration0"][j])
                rows.append((s.base + j, s.dist, p0, p1))
        return named_noise(self.c, R.scalar_noise(rows, self.seed, self.offset0 + it, 0, self.n), self.n)


def train_all_modes_against_the_oracle(n, iters, optimizer, opt_kw, variant=None, served="specialised", offset0=3,
                                       builder="build_readme_ar", kwargs=dict(T=20), **train_kw):
    from oracle.svi_oracle import Oracle
    api = W.native_api()
    build = lambda: getattr(W, builder)(api, **kwargs)
    runs = {}
    for mode, opts in MODES:
        c = engine.compile_model(build(), None, "pathwise")
        c.iteration = offset0
        losses, finite = c.train(iters, n, optimizer, seed=SEED, **opts, **train_kw, **opt_kw)
        # (no quiet fall-back: the mode, the engine, and in the in-kernel loop the generated kernel)
        assert c.last_mode == mode and bool(finite.all()) and c.iteration == offset0 + iters
        assert c.native.engine(n, 2)["engine"] == served
        if mode == "persistent" and variant is not None:
            assert native.load().bsvi_spec_last_variant() == variant
        runs[mode] = (losses.cpu().numpy(), c.named_params())
    o = Oracle(build())
    ref_losses = o.train(iters, n, optimizer, noise_seq=PredictedNoise(c, o, SEED, offset0, n), **train_kw, **opt_kw)
    ref_after = {k: v.detach().numpy() for k, v in o.named_parameters().items()}
    for mode, (losses, params) in runs.items():
        np.testing.assert_allclose(losses, runs["persistent"][0], rtol=2e-6, atol=1e-6)
        for name, p in params.items():
            np.testing.assert_allclose(p, runs["persistent"][1][name], rtol=2e-6, atol=1e-7)
        print(optimizer, n, mode, "loss curve rel. error %.3g" % rel_err(losses, ref_losses),
              "parameters %.3g" % max(np.abs(p - ref_after[k].reshape(p.shape)).max() for k, p in params.items()))
        assert rel_err(losses, ref_losses) <= TOL, mode
        for name, p in params.items():
            e = ref_after[name].reshape(p.shape)
            assert np.abs(p - e).max() <= 2e-5 * (1 + np.abs(e).max()), (mode, name)
    return c


# n -> variant of the in-kernel loop's launch (tests/test_gpu_spec_select.py): 4 the single draw wave, 6 the lean chain with the
# owners on a draw wave, 0 no extra wave, 2 three workgroups
LOOP_CASES = [
    (300, 6, "AdamW", dict(lr=5e-3, weight_decay=0.05, amsgrad=True)),
    (300, 6, "RMSprop", dict(lr=1e-3, momentum=0.5, centered=True)),
    (300, 6, "Adagrad", dict(lr=2e-2, lr_decay=0.02, initial_accumulator_value=0.1)),
    (300, 6, "Adamax", dict(lr=5e-3, betas=(0.8, 0.95))),
    (64, 4, "Adamax", dict(lr=5e-3)),
    (321, 0, "RMSprop", dict(lr=1e-3)),
    (513, 2, "Adagrad", dict(lr=2e-2)),
    (513, 2, "AdamW", dict(lr=5e-3)),
]


@pytest.mark.parametrize("n,variant,optimizer,opt_kw", LOOP_CASES, ids=["%s-%d" % (c[2], c[0]) for c in LOOP_CASES])
def test_every_launch_mode_and_loop_variant(n, variant, optimizer, opt_kw):
    train_all_modes_against_the_oracle(n, 10, optimizer, opt_kw, variant=variant)


def test_interpreter_loop(monkeypatch):
    monkeypatch.setenv("BSVI_JIT", "0")
    train_all_modes_against_the_oracle(300, 10, "RMSprop", dict(lr=1e-3, momentum=0.5), served="interpreter")


# ---- 3. state across calls, lazy state, a non-finite loss -------------------------------------------------------------------
def loop_call(c, cfg, n, iters, state, offset0):
    """bsvi_train_persistent2 with the caller's state buffer (CompiledELBO.train starts every call from a fresh optimizer)"""
    ptr = lambda t: C.c_void_p(t.data_ptr())
    c.native.ensure_shares(n)
    loss, finite = torch.zeros(iters, device=c.device), torch.zeros(iters, device=c.device)
    args = c._elbo_args(n, n, 0, None, SEED, offset0)
    native.check(c.lib.bsvi_train_persistent2(c.native.handle, C.byref(args), C.byref(cfg), ptr(c.params), ptr(state), ptr(c.mask_all),
                                              ptr(c.mask_first), 0, iters, ptr(loss), ptr(finite)))
    torch.cuda.synchronize()
    assert bool(finite.all())
    return loss.cpu().numpy()


@pytest.mark.parametrize("optimizer,opt_kw", [("RMSprop", dict(lr=1e-3, momentum=0.9)), ("Adamax", dict(lr=5e-3))])
def test_two_calls_with_the_state_kept_equal_one(optimizer, opt_kw):
    cfg = native.make_opt_cfg(optimizer, **opt_kw)
    n = 300
    build = lambda: engine.compile_model(W.build_readme_ar(W.native_api(), T=20), None, "pathwise")
    one = build()
    state_one = torch.zeros(4 * one.n_params, device=one.device)
    whole = loop_call(one, cfg, n, 12, state_one, 0)
    assert native.load().bsvi_spec_last_variant() == 6
    two = build()
    state_two = torch.zeros(4 * two.n_params, device=two.device)
    halves = np.concatenate([loop_call(two, cfg, n, 6, state_two, 0), loop_call(two, cfg, n, 6, state_two, 6)])
    assert native.load().bsvi_spec_last_variant() == 6
    # (the second call rebuilds beta^step by pow(), the single call carries running products: one ulp-scale bound)
    np.testing.assert_allclose(halves, whole, rtol=2e-6)
    np.testing.assert_allclose(two.params.cpu().numpy(), one.params.cpu().numpy(), rtol=2e-6, atol=1e-7)
    np.testing.assert_allclose(state_two.cpu().numpy(), state_one.cpu().numpy(), rtol=2e-6, atol=1e-7)
    steps = state_one.cpu().numpy().reshape(4, -1)[3]
    assert steps.max() == 12.0                                      # (the state was written back and continued)


def test_adagrad_sum_starts_at_a_parameters_own_first_step():
    """pretraining_iterations=3 on a model whose joint side owns parameters (a learnable prior location and likelihood scale): they
    are first stepped at iteration 4 and start their sum from initial_accumulator_value there (torch creates the sum with the
    optimizer; the device state arrives all zero)"""
    c = train_all_modes_against_the_oracle(60, 10, "Adagrad", dict(lr=2e-2, initial_accumulator_value=0.1),
                                           builder="build_learnable_model", kwargs=dict(), pretraining_iterations=3)
    first, every = c.mask_first.cpu().numpy(), c.mask_all.cpu().numpy()
    assert first.any() and (every != first).any()                  # (both groups exist in this model)


@pytest.mark.parametrize("optimizer,opt_kw", [("RMSprop", dict(lr=1e-3, momentum=0.5)), ("Adagrad", dict(lr=1e-2))])
def test_non_finite_loss_skips_the_step_as_under_adam(optimizer, opt_kw):
    """tests/test_gpu_spec_tail.py's set-up: a NaN parameter makes every iteration's loss non-finite"""
    def run(name, kw):
        c = engine.compile_model(W.build_readme_ar(W.native_api(), T=20), None, "pathwise")
        with torch.no_grad():
            c.params[0] = float("nan")
        before = c.params.cpu().numpy().copy()
        losses, finite = c.train(8, 300, name, seed=4, **kw)
        assert c.last_mode == "persistent" and native.load().bsvi_spec_last_variant() == 6
        return before, c.params.cpu().numpy(), losses.cpu().numpy(), finite.cpu().numpy(), c.out.cpu().numpy()
    before, after, losses, finite, out = run(optimizer, opt_kw)
    _, _, _, adam_finite, adam_out = run("Adam", dict(lr=1e-2))
    assert not finite.any() and not np.isfinite(losses).any()
    assert np.array_equal(after.view(np.uint32), before.view(np.uint32))          # no step was taken
    assert np.array_equal(finite, adam_finite)
    assert out[1] == adam_out[1] == 300.0 and out[3] == adam_out[3] == 0.0


# ---- 4. the other engines, one kind each: 8 iterations on handed-in noise and rows, against the oracle ------------------------
ITERS = 8


def handed_in(g, rng, per_sample_rows=False):
    """noise and minibatch rows in the shapes of the fixture's trajectory, for ITERS iterations"""
    ds = g.meta["kwargs"]["dataset_size"]
    noise = {k: rng.standard_normal((ITERS,) + v.shape[1:]).astype(np.float32) for k, v in g.group("traj/noise/").items()}
    rows = {}
    for k, v in g.group("traj/minibatch/").items():
        draw = lambda: rng.choice(ds, v.shape[-1], replace=False)
        rows[k] = np.stack([np.stack([draw() for _ in range(v.shape[1])]) if per_sample_rows else draw() for _ in range(ITERS)])
    return noise, rows


def sequences(noise, rows):
    return ([{k: v[it] for k, v in noise.items()} for it in range(ITERS)],
            [{k: [int(i) for i in v[it]] for k, v in rows.items()} for it in range(ITERS)])


def test_dense_path_rmsprop():
    from oracle.svi_oracle import Oracle
    g = Golden("logreg_C3_P6_DS20_B12_N5")
    n, kw = g.meta["trajectory"]["n"], dict(lr=5e-3, momentum=0.5)
    noise_seq, mb_seq = sequences(*handed_in(g, np.random.RandomState(1)))
    c = engine.compile_model(g.build(), None, "pathwise")
    assert type(c).__name__ == "CompiledDense"
    losses, finite = c.train(ITERS, n, "RMSprop", noise_seq=noise_seq, minibatch_seq=mb_seq, **kw)
    assert bool(finite.all())
    o = Oracle(g.build())
    ref = o.train(ITERS, n, "RMSprop", noise_seq=noise_seq, minibatch_seq=mb_seq, **kw)
    after = {k: v.detach().numpy() for k, v in o.named_parameters().items()}
    print("dense RMSprop: loss curve rel. error %.3g" % rel_err(losses.cpu().numpy(), ref))
    assert rel_err(losses.cpu().numpy(), ref) <= TOL
    for name, p in c.named_params().items():
        e = after[name].reshape(p.shape)
        assert np.abs(p - e).max() <= 2e-5 * (1 + np.abs(e).max()), name


def test_bnn_path_adamw():
    """the bound of the BNN's trajectory test: the oracle in double precision is the truth, in single precision the yardstick"""
    from oracle.svi_oracle import Oracle
    g = Golden("bnn_P48_H6_C4_DS30_B12_N5")
    n, kw = g.meta["trajectory"]["n"], dict(lr=5e-3, weight_decay=0.05)
    noise_seq, mb_seq = sequences(*handed_in(g, np.random.RandomState(2)))
    c = engine.compile_model(g.build(), None, "pathwise")
    assert type(c).__name__ == "CompiledBnn"
    losses, finite = c.train(ITERS, n, "AdamW", noise_seq=noise_seq, minibatch_seq=mb_seq, **kw)
    assert bool(finite.all())
    runs = {}
    for dtype in (torch.float64, torch.float32):
        o = Oracle(g.build(), dtype=dtype)
        curve = o.train(ITERS, n, "AdamW", noise_seq=noise_seq, minibatch_seq=mb_seq, **kw).astype(np.float64)
        runs[dtype] = (curve, {k: v.detach().numpy().astype(np.float64) for k, v in o.named_parameters().items()})
    (exact, exact_after), (single, single_after) = runs[torch.float64], runs[torch.float32]
    got = losses.cpu().numpy().astype(np.float64)
    print("BNN AdamW: |device - double| %.3g, |single - double| %.3g" % (np.abs(got - exact).max(), np.abs(single - exact).max()))
    assert np.abs(got - exact).max() <= max(4 * np.abs(single - exact).max(), TOL * np.abs(exact).max())
    for name, p in c.named_params().items():
        e64, e32 = exact_after[name].reshape(p.shape), single_after[name].reshape(p.shape)
        assert np.abs(p - e64).max() <= max(4 * np.abs(e32 - e64).max(), 2e-5 * (1 + np.abs(e64).max())), name


def test_amortised_path_adamax():
    """the bound of tests/test_gpu_amortized.py::test_vae_golden_trajectory.  Its allowance for Adam — 1 % of the largest distance
    the optimizer can move a parameter in these iterations — holds for Adamax for the reason given there: the step is
    lr * exp_avg / exp_inf, whose size does not depend on the size of the gradient, so an element whose gradient is rounding noise
    moves by its sign."""
    from oracle.vae_oracle import VaeOracle
    g = Golden("vae_P12_H8_H6_DS20_B5_N3")
    n, lr = g.meta["trajectory"]["n"], 0.01
    noise, rows = handed_in(g, np.random.RandomState(3), per_sample_rows=True)
    model = g.build()
    c = engine.compile_model(model, model.posterior_model, "pathwise")
    assert type(c).__name__ == "CompiledAmortized"
    losses, finite = c.train(ITERS, n, "Adamax", noise_seq=list(noise["z"]), minibatch_seq=list(rows["x"]), lr=lr)
    assert float(finite.min()) == 1.0
    o = VaeOracle(g.build(), dtype=torch.float32)
    ref = o.train(ITERS, list(rows["x"]), list(noise["z"]), "Adamax", lr=lr)
    print("amortised Adamax: loss curve rel. error %.3g" % rel_err(losses.cpu().numpy(), ref))
    assert rel_err(losses.cpu().numpy(), ref) <= TOL
    named = c.named_params()
    slack = 0.01 * lr * ITERS
    enc_link, dec_link = c.program.links
    for tag, link in (("enc", enc_link), ("dec", dec_link)):
        for pname, par in link.named.items():
            e = o.named_parameters()["%s/%s" % (tag, pname)].detach().numpy()
            assert np.abs(named[par.name].reshape(e.shape) - e).max() <= 1e-5 * (1 + np.abs(e).max()) + slack, (tag, pname)


def test_minibatch_loop_adagrad():
    """ONE launch that draws its noise and its rows itself; the oracle is handed what the stream contract predicts for them"""
    from oracle.svi_oracle import Oracle
    g = Golden("minibatch_linreg_P3_DS40_B8_N30")
    n, offset0, kw = 64, 5, dict(lr=5e-2, initial_accumulator_value=0.1)
    ds, batch = g.meta["kwargs"]["dataset_size"], g.meta["kwargs"]["batch_size"]
    (source,) = g.group("traj/minibatch/")
    c = engine.compile_model(g.build(), None, "pathwise")
    c.iteration = offset0
    losses, finite = c.train(ITERS, n, "Adagrad", seed=SEED, minibatch_loop=True, **kw)
    assert c.last_mode == "persistent"                             # (a declined loop trains launch by launch: "stepwise")
    assert bool(finite.all())
    o = Oracle(g.build())
    mb_seq = [{source: [int(i) for i in R.minibatch_index(SEED, offset0 + it, ds, np.arange(batch))]} for it in range(ITERS)]
    ref = o.train(ITERS, n, "Adagrad", noise_seq=PredictedNoise(c, o, SEED, offset0, n), minibatch_seq=mb_seq, **kw)
    after = {k: v.detach().numpy() for k, v in o.named_parameters().items()}
    print("minibatch loop Adagrad: loss curve rel. error %.3g" % rel_err(losses.cpu().numpy(), ref))
    assert rel_err(losses.cpu().numpy(), ref) <= TOL
    for name, p in c.named_params().items():
        e = after[name].reshape(p.shape)
        assert np.abs(p - e).max() <= 2e-5 * (1 + np.abs(e).max()), name


# ---- 5. the public API ---------------------------------------------------------------------------------------------------------
def test_perform_inference_with_rmsprop_walks_the_trajectory_of_train():
    torch.manual_seed(7)
    a = W.build_readme_ar(W.native_api(), T=20)
    inference.perform_inference(a, 25, number_samples=300, optimizer="RMSprop", lr=1e-3)
    la = np.asarray(a.diagnostics["loss curve"])
    b = engine.compile_model(W.build_readme_ar(W.native_api(), T=20), None, "pathwise")
    losses, finite = b.train(25, 300, "RMSprop", lr=1e-3)
    assert bool(finite.all()) and b.last_mode == "persistent"
    lb = losses.cpu().numpy()
    assert la.shape == lb.shape == (25,)
    assert rel_err(la, lb) <= 5e-6
    pa = engine.compile_model(a, None, "pathwise").params.cpu().numpy()
    assert np.abs(pa - b.params.cpu().numpy()).max() <= 2e-5


def test_hand_written_loop_with_adagrad_update():
    model = W.build_beta_binomial(W.native_api(), n_obs=30)
    opt = ProbabilisticOptimizer(model.posterior_model, "Adagrad", lr=0.05)
    values = []
    for _ in range(60):
        loss = -model.estimate_log_model_evidence(number_samples=512, for_gradient=True)
        opt.zero_grad()
        loss.backward()
        opt.update()
        values.append(float(loss))
    assert np.isfinite(values).all()
    assert np.mean(values[-10:]) < np.mean(values[:10])
