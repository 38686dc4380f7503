"""Every launch branch of the local reparameterisation estimator (csrc/dense_local.inc) that the five shapes of
tests/test_gpu_dense_local.py leave unrun, its noise stream against the host reference of the contract (oracle/philox_ref.py), and a
training trajectory against torch.optim in double precision.  `build` and `reference` are that module's; the bound of every comparison
with the formulas is the project's yardstick, max(4 |ref32 - ref64|, 1e-5 scale).  That each shape reaches the branch its comment
names is what tests/c_abi/dense_local_plan.cpp pins without a device (tests/test_dense_local_cpu.py compares its list with SHAPES)."""
import math

import numpy as np
import pytest
import torch

from conftest import rel_err, yardstick_grad_check, yardstick_loss_check
from brancher_amd import dense, native, workloads as W
from oracle import philox_ref as R
from test_gpu_dense_local import build, reference
from test_gpu_noise import NORMAL_TOL, OFFSETS, SEEDS, TOL

pytestmark = pytest.mark.gpu


def build_shared(c, p, b):
    """`build`'s data and posterior loc under three entries shared by all rows (stride 0): the posterior scale exp of ONE learnable scalar
    root, the prior loc a learnable scalar root, the prior scale exp of a learnable scalar root"""
    api, rng = W.native_api(), np.random.RandomState(7 * c + p)
    BF, ds = api.BF, b + 3
    X = (rng.standard_normal((ds, p, 1)) / math.sqrt(p)).astype(np.float32)
    labels = rng.randint(0, max(c, 2), (ds, 1)).astype(np.int32)
    indices = api.RandomIndices(dataset_size=ds, batch_size=b, name="indices", is_observed=True)
    x = api.EmpiricalVariable(X, indices=indices, name="x", is_observed=True)
    y = api.EmpiricalVariable(labels, indices=indices, name="labels", is_observed=True)
    weights = api.NormalVariable(api.RootVariable(0.1, "prior_loc", learnable=True),
                                 BF.exp(api.RootVariable(math.log(0.7), "log_prior_scale", learnable=True)), "weights")
    k = api.CategoricalVariable(logits=BF.matmul(weights, x), name="k")
    model = api.ProbabilisticModel([k])
    k.observe(y)
    q = api.NormalVariable(api.RootVariable(0.5 * rng.standard_normal((c, p)), "q_loc", learnable=True),
                           BF.exp(api.RootVariable(math.log(0.3), "q_log_s", learnable=True)), "weights")
    model.set_posterior_model(api.ProbabilisticModel([q]))
    return model, X.reshape(ds, p), labels.reshape(ds)


SHAPES = {  # C, P, B, N, model form — the branch each reaches (the plan of each: tests/c_abi/dense_local_plan.cpp)
    # one row tile, one K chunk, one split, one sample a lane, nothing ragged but the padding: tier 4 with two dead classes (C = 2),
    # P_pad = 64 > P
    "exact_two_dead_classes": (2, 32, 32, 8, dict()),
    # tier 4 and its Philox call exactly full (C = 4); P = P_pad, B = B_pad; two splits
    "tier4_full": (4, 64, 64, 16, dict()),
    # the lower edge of tier 10 (C = 5: the draw loop's guard 4 q < C drops the third call); exactly four K chunks, every wave of
    # dense_local_fwd live in one round, nothing ragged; three row tiles; three splits
    "tier10_edge_four_chunks": (5, 128, 96, 24, dict()),
    # the lower edge of tier 16 (C = 11: the fourth call dropped); nine K chunks = three rounds of dense_local_fwd, the last with wave 0
    # alone; five row tiles, so wave 0 of dense_local_bwd takes a second chunk and waves 1 .. 3 one; eleven splits, so dense_local_join
    # walks a second group of eight with five masked, and the last split holds one sample; nine column tiles, the last of four features
    "tier16_edge_three_rounds": (11, 260, 160, 81, dict()),
    # Bernoulli beyond one ragged tile: five row tiles, the last of two rows; two K chunks; three splits and the join
    "bernoulli_split_and_joined": (1, 40, 130, 20, dict()),
    # N = 1: one sample lane of one split works, seven contribute zeros
    "one_sample": (3, 5, 33, 1, dict()),
    # a stride-0 prior scale at R = 700: dense_local_tail's loop over the shared entry's rows makes three trips
    "shared_prior_scale_three_trips": (10, 70, 64, 40, dict(learn_prior=True)),
    # logits of tens: the fast exp, log and reciprocal of the categorical branch, the log1pf(expf(-|l|)) of the Bernoulli one
    "large_logits_categorical": (10, 70, 64, 40, dict(spread=20.0)),
    "large_logits_bernoulli": (1, 40, 130, 20, dict(spread=20.0)),
}
SHARED, DRAWN, DRAWN_BERNOULLI, TRAJECTORY = (10, 70, 64, 40), (11, 8, 40, 17), (1, 8, 40, 17), (3, 5, 33, 9)


def inputs(c, b, n, seed=3):
    rng = np.random.RandomState(seed)
    return rng.permutation(b + 3)[:b].astype(np.int32), rng.standard_normal((n, b, c)).astype(np.float32)


def check_against_the_formulas(compiled, X, labels, idx, zeta, res, what):
    p = compiled.program
    assert float(res["finite"]) == 1.0, what
    theta = compiled.params.cpu().numpy()[:p.n_params]
    loss64, g64 = reference(p, theta, X, labels, idx, zeta, torch.float64)
    loss32, g32 = reference(p, theta, X, labels, idx, zeta, torch.float32)
    named = compiled.named_grads()
    print(what, "loss", float(res["loss"]), loss64, loss32, {k: (np.abs(named[k] - g64[k]).max(), np.abs(g32[k] - g64[k]).max()) for k in g64})
    yardstick_loss_check(float(res["loss"]), loss64, loss32)
    yardstick_grad_check(named, g64, g32)


def evaluate_supplied(model, X, labels, c, b, n, what):
    compiled = dense.CompiledDense(model, model.posterior_model, "local")
    idx, zeta = inputs(c, b, n)
    res = compiled.evaluate(n, noise={compiled.program.likelihood_name: zeta}, minibatch=idx, seed=1, offset=0, want_indices=True)
    assert np.array_equal(res["indices"].cpu().numpy(), idx)
    check_against_the_formulas(compiled, X, labels, idx, zeta, res, what)
    return compiled


@pytest.mark.parametrize("name", list(SHAPES))
def test_branch_matches_the_formulas(name):
    c, p_, b, n, form = SHAPES[name]
    model, X, labels = build(c, p_, b, **form)
    compiled = evaluate_supplied(model, X, labels, c, b, n, name)
    prog = compiled.program
    if form.get("spread"):      # the case is about logits of tens: the mean logits of the dataset's rows reach them
        loc = dense.row_parameters(prog, compiled.params.cpu().numpy()[:prog.n_params])[0]
        assert np.abs(X.astype(np.float64) @ np.asarray(loc, dtype=np.float64).reshape(c, p_).T).max() > 10.0
    if form.get("learn_prior"):
        assert prog.prior_scale[1] == 0 and prog.n_classes * prog.n_features == 700 > 2 * 256


def test_three_shared_entries_go_through_the_tail_at_once():
    """the posterior scale, the prior loc and the prior scale each ONE uniform entry (stride 0) at R = 700: three of the four quadruples
    go through rowg and dense_local_tail's three-trip loop in one call, and only the posterior loc through the row step's stores"""
    c, p_, b, n = SHARED
    model, X, labels = build_shared(c, p_, b)
    prog = dense.lower_dense(model, model.posterior_model, "local")      # (lower_dense accepts all three forms)
    assert [q[1] for q in (prog.q_loc, prog.q_scale, prog.prior_loc, prog.prior_scale)] == [1, 0, 0, 0]
    compiled = evaluate_supplied(model, X, labels, c, b, n, "three shared entries")
    assert {k: v.size for k, v in compiled.named_grads().items()} == {"q_loc": 700, "q_log_s": 1, "prior_loc": 1, "log_prior_scale": 1}


def drawn(compiled, n, seed, offset):
    res = compiled.evaluate(n, seed=seed, offset=offset, want_noise=True, want_indices=True)
    return res, res["noise"].cpu().numpy(), res["indices"].cpu().numpy()


SPLITS = ("1", "3", "8", "9", None)      # of 81 samples: 1, 3, 6, 6 and (unset: the clamp) 11 splits


def test_the_number_of_splits_moves_neither_the_draw_nor_the_result(monkeypatch):
    """BSVI_LOCAL_SPLITS is read per call.  The drawn noise and minibatch are bit-identical over the split counts (a draw is a function of
    (seed, offset, sample, row, class), not of the split that makes it), and every run meets the formulas on the noise it reported."""
    c, p_, b, n, form = SHAPES["tier16_edge_three_rounds"]
    model, X, labels = build(c, p_, b, **form)
    runs = []
    for knob in SPLITS:
        if knob is None:
            monkeypatch.delenv("BSVI_LOCAL_SPLITS", raising=False)
        else:
            monkeypatch.setenv("BSVI_LOCAL_SPLITS", knob)
        compiled = dense.CompiledDense(model, model.posterior_model, "local")
        res, noise, idx = drawn(compiled, n, SEEDS[1], OFFSETS[3])
        runs.append((knob, noise, idx))
        assert noise.shape == (n, b, c) and np.array_equal(noise, runs[0][1]) and np.array_equal(idx, runs[0][2]), knob
        check_against_the_formulas(compiled, X, labels, idx, noise, res, "BSVI_LOCAL_SPLITS=%s" % knob)
    assert float(np.abs(runs[0][1]).max()) > 0 and len(set(runs[0][2].tolist())) == b


def test_more_splits_on_a_cached_workspace(monkeypatch):
    """ONE engine, the same N: a call of one split, then one of BSVI_LOCAL_SPLITS=9 (six splits of dM / dV).  `_local_args` asks the
    library for the size on every call and replaces a cached workspace that is too small."""
    c, p_, b, n, form = SHAPES["tier16_edge_three_rounds"]
    model, X, labels = build(c, p_, b, **form)
    compiled = dense.CompiledDense(model, model.posterior_model, "local")
    idx, zeta = inputs(c, b, n)
    sizes = []
    for knob in ("1", "9"):
        monkeypatch.setenv("BSVI_LOCAL_SPLITS", knob)
        res = compiled.evaluate(n, noise=zeta, minibatch=idx, seed=1, offset=0)
        need = int(compiled.lib.bsvi_dense_local_workspace_bytes(compiled.handle, n))
        assert compiled._workspaces[("local", n)].numel() >= need > 0
        sizes.append(need)
        check_against_the_formulas(compiled, X, labels, idx, zeta, res, "one engine, BSVI_LOCAL_SPLITS=%s" % knob)
    assert sizes[1] > sizes[0]


@pytest.mark.parametrize("shape", [DRAWN, DRAWN_BERNOULLI], ids=["categorical", "bernoulli"])
def test_the_drawn_normals_are_the_contracts(shape):
    """zeta[n][b][c] = normal c & 3 of Philox call (n, (4 b + (c >> 2)) | 0x10000000, offset) under the seed as it is (philox.h), over a
    seed with a high word and offsets 2^32 - 1, 2^32, 2^62 + 3: two row tiles, every q of a 16-tier row with classes 8 .. 10 in the third
    call, three splits; Bernoulli: normal 0 of call 0 of each row.  The minibatch is the dense path's keyed bijection, exactly.
    Measured on an MI355X, worst |reported - predicted| over seeds and offsets: categorical 6.19e-07, Bernoulli 3.93e-07 (bound
    NORMAL_TOL = 2.48e-05)."""
    c, p_, b, n = shape
    model, _, _ = build(c, p_, b)
    compiled = dense.CompiledDense(model, model.posterior_model, "local")
    worst = 0.0
    for seed in SEEDS:
        for offset in OFFSETS:
            _, noise, idx = drawn(compiled, n, seed, offset)
            want = R.local_noise(seed, offset, n, b, c)
            assert noise.shape == want.shape and np.isfinite(noise).all()
            err = float(np.abs(noise - want).max())
            worst = max(worst, err)
            assert err <= NORMAL_TOL, (hex(seed), hex(offset), err, NORMAL_TOL)
            assert np.array_equal(idx, R.minibatch_index(seed, offset, b + 3, np.arange(b))), (hex(seed), hex(offset))
    print("drawn normals of %r: worst |reported - predicted| %.3g, bound %.3g" % (shape, worst, NORMAL_TOL))


# ---- a training trajectory -----------------------------------------------------------------------------------------------------------
ITERS, LR = 5, 0.05


def trajectory(p, theta0, X, labels, idx_seq, noise_seq, optimizer, dtype):
    """the loss of `reference` stepped by torch.optim with the hyper-parameters native.make_opt_cfg hands the device (torch's own
    defaults: Adam betas (0.9, 0.999), eps 1e-8, no weight decay; SGD without momentum) -> (loss curve, final flat parameters)"""
    th = torch.tensor(theta0, dtype=dtype, requires_grad=True)
    opt = getattr(torch.optim, optimizer)([th], lr=LR)
    curve = []
    for idx, zeta in zip(idx_seq, noise_seq):
        loss, grads = reference(p, th.detach().numpy(), X, labels, idx, zeta, dtype)
        flat = np.zeros(len(theta0))
        for par, off, size, _ in p.parameters:
            flat[off:off + size] = grads[par.name].reshape(-1)
        th.grad = torch.tensor(flat, dtype=dtype)
        opt.step()
        curve.append(loss)
    return np.array(curve), th.detach().numpy().astype(np.float64)


def named(p, flat):
    return {par.name: flat[off:off + size].reshape(par.shape) for par, off, size, _ in p.parameters}


def trajectory_engine():
    c, p_, b, n = TRAJECTORY
    model, X, labels = build(c, p_, b, collide=True)
    compiled = dense.CompiledDense(model, model.posterior_model, "local")
    cfg = native.make_opt_cfg("Adam", lr=LR)
    assert (cfg.beta1, cfg.beta2, cfg.weight_decay, cfg.amsgrad) == (np.float32(0.9), np.float32(0.999), 0.0, 0) and abs(cfg.eps - 1e-8) < 1e-15
    assert torch.equal(compiled.mask_first, compiled.mask_all)      # every parameter is the posterior's: no iteration steps a subset
    return compiled, X, labels


@pytest.mark.parametrize("optimizer", ["Adam", "SGD"])
def test_training_on_handed_in_noise_follows_torch_optim_in_double(optimizer):
    """Five iterations on handed-in noise and minibatches: loss curve per iteration and final parameters within the yardstick,
    max(4 |traj32 - traj64|, 1e-5 scale), traj32 the same loop in float32; the finite curve is all ones.
    Measured on an MI355X, |device - traj64| (|traj32 - traj64|): Adam loss curve 3.45e-06 (2.46e-06) at losses of ~40, parameters
    1.85e-07 (1.47e-07); SGD loss curve 5.37e-06 (2.69e-06), parameters 1.39e-07 (1.39e-07)."""
    c, p_, b, n = TRAJECTORY
    compiled, X, labels = trajectory_engine()
    p = compiled.program
    theta0 = compiled.params.cpu().numpy()[:p.n_params].astype(np.float64)
    seq = [inputs(c, b, n, seed=20 + it) for it in range(ITERS)]
    idx_seq, noise_seq = [s[0] for s in seq], [s[1] for s in seq]
    losses, finite = compiled.train(ITERS, n, optimizer=optimizer, lr=LR, noise_seq=noise_seq, minibatch_seq=idx_seq)
    losses, finite = losses.cpu().numpy().astype(np.float64), finite.cpu().numpy()
    curve64, theta64 = trajectory(p, theta0, X, labels, idx_seq, noise_seq, optimizer, torch.float64)
    curve32, theta32 = trajectory(p, theta0, X, labels, idx_seq, noise_seq, optimizer, torch.float32)
    got, want, single = compiled.named_params(), named(p, theta64), named(p, theta32)
    print(optimizer, "loss curve |device - traj64| %.3g, |traj32 - traj64| %.3g; parameters %.3g, %.3g" % (
        np.abs(losses - curve64).max(), np.abs(curve32 - curve64).max(),
        max(np.abs(got[k] - want[k]).max() for k in want), max(np.abs(single[k] - want[k]).max() for k in want)))
    assert finite.shape == (ITERS,) and (finite == 1).all() and compiled.last_mode == "local"
    assert np.abs(theta64 - theta0).max() > 0.01                     # (the run moved)
    for it in range(ITERS):
        yardstick_loss_check(losses[it], curve64[it], curve32[it])
    yardstick_grad_check(got, want, single)


def test_training_on_drawn_noise_follows_the_predicted_stream():
    """`train` with a seed and no sequences: iteration `it` draws at offset0 + it.  The double-precision loop on R.local_noise and
    R.minibatch_index of those offsets, under the bounds tests/test_gpu_noise.py puts on the same comparison: loss curve within the
    relative 1e-5 (TOL), parameters within 2e-5 (1 + |e|).  A second call goes on from offset0 + 5.
    Measured on an MI355X: loss curve 1.74e-07 relative (bound 1e-5), parameters 1.41e-07; the second call's first loss 2.88e-07
    relative, and 9.1e-04 against the draw of offset0."""
    c, p_, b, n = TRAJECTORY
    compiled, X, labels = trajectory_engine()
    p, seed = compiled.program, SEEDS[1]
    compiled.iteration = (1 << 32) - 3                               # the low offset word wraps inside the run
    offset0 = compiled.iteration
    theta0 = compiled.params.cpu().numpy()[:p.n_params].astype(np.float64)
    predicted = lambda first, count: ([R.minibatch_index(seed, first + it, b + 3, np.arange(b)) for it in range(count)],
                                      [R.local_noise(seed, first + it, n, b, c) for it in range(count)])
    losses, finite = compiled.train(ITERS, n, optimizer="Adam", lr=LR, seed=seed)
    assert compiled.iteration == offset0 + ITERS and bool(finite.all())
    after = compiled.named_params()
    idx_seq, noise_seq = predicted(offset0, ITERS)
    curve64, theta64 = trajectory(p, theta0, X, labels, idx_seq, noise_seq, "Adam", torch.float64)
    want = named(p, theta64)
    err_curve = rel_err(losses.cpu().numpy(), curve64)
    err_par = max(np.abs(after[k] - want[k]).max() for k in want)
    print("drawn training: loss curve rel. error %.3g (bound %.3g), parameters %.3g" % (err_curve, TOL, err_par))
    assert err_curve <= TOL
    for k, e in want.items():
        assert np.abs(after[k] - e).max() <= 2e-5 * (1 + np.abs(e).max()), k
    # the next call: the offsets go on (its optimizer state is new: the reference's first step from the parameters reached)
    theta1 = compiled.params.cpu().numpy()[:p.n_params].astype(np.float64)
    losses2, _ = compiled.train(1, n, optimizer="Adam", lr=LR, seed=seed)
    idx_seq, noise_seq = predicted(offset0 + ITERS, 1)
    curve2, _ = trajectory(p, theta1, X, labels, idx_seq, noise_seq, "Adam", torch.float64)
    other, _ = trajectory(p, theta1, X, labels, *predicted(offset0, 1), "Adam", torch.float64)
    err2 = rel_err(losses2.cpu().numpy(), curve2)
    print("second call: first loss rel. error %.3g; against offset0's draw %.3g" % (err2, rel_err(losses2.cpu().numpy(), other)))
    assert compiled.iteration == offset0 + ITERS + 1 and err2 <= TOL
    assert rel_err(losses2.cpu().numpy(), other) > 10 * TOL            # (the comparison can tell the offsets apart)
