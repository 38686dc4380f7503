"""The activations behind tanh / relu / sigmoid / softplus on the device (bsvi_bnn_set_activation_params): leaky_relu, elu,
selu, softsign, hardtanh / relu6, silu and gelu in every middle kernel a size selects (bnn_mid_gen, bnn_upper_gen, bnn_upper<true>,
bnn_upper<false>), in an eight-layer network, under a scale head, a shared first layer, a scale latent and Taylor1, in `predict` on both of
its arms and through ten Adam steps.  tests/test_gpu_bnn_middle.py's rule throughout: each case asserts the kernel it is on, evaluates at
N = 70, P = 32, and is compared with `Oracle(..., dtype=float64)` on the draws and the minibatch the kernels report — loss, per-sample f,
every named gradient; conftest's yardstick and the per-tensor floor (check_against of that file) — then the same draws are fed back in.

leaky_relu, hardtanh and relu6 have kinks, where a kernel in single precision and an oracle may land on different sides.  Every case
recomputes the hidden pre-activations in double from the reported draws (`kink_margin`) and asserts that none lies within 1e-4 of a kink
BEFORE any gradient is compared: a condition on the chosen seeds (a violation says so itself), not a tolerance."""
import numpy as np
import pytest
import torch

from conftest import yardstick_grad_check
from brancher_amd import bnn, inference, workloads as W
from oracle.svi_oracle import Oracle
from test_gpu_bnn_middle import N, P, TOL, build, check_against, classifier, oracle_pair, regression

pytestmark = pytest.mark.gpu
F = torch.nn.functional
MARGIN = 1e-4
LEAKY, ELU, HARD = ("leaky_relu", dict(negative_slope=0.2)), ("elu", dict(alpha=0.7)), ("hardtanh", dict(min_val=-0.5, max_val=2.0))
SEVEN = [LEAKY, ELU, "selu", "softsign", HARD, "silu", "gelu"]
# two hidden layers each: the seven kinds and relu6 once per kernel, silu in the first layer (its own line in every kernel), gelu above it
NETS = {"n1": ["silu", LEAKY], "n2": [HARD, "gelu"], "n3": ["selu", "relu6"], "n4": ["softsign", ELU]}
MID0, STATIC = dict(BSVI_BNN_MID="0"), dict(BSVI_BNN_MID="0", BSVI_BNN_JIT="0")
# kernel: (widths, minibatch, pixels, switches, data path) — the widths of cases c and d of tests/test_gpu_bnn_middle.py; d's on exact data is
# bnn_mid_gen's, and behind both switches the static kernel with (314 * 65 + 68 * 256) * 4 = 151 272 bytes of LDS
KERNELS = {
    "mid_gen": ([P, 16, 14, 4], "integers", {}, "bf16x3"),
    "upper_gen": ([P, 16, 14, 4], "normal", MID0, "f32"),
    "upper_lds": ([P, 16, 14, 4], "integers", STATIC, "bf16x3"),
    "upper_mem": ([P, 16, 16, 4], "unit", STATIC, "f32"),
}


# the Philox seed of every (kernel, network) and of the eight-layer case: the first from 3 up whose draws (offset 5, N = 70; found on the
# host with oracle/philox_ref.py's normal_rows and minibatch_index) keep every pre-activation at least 1.3e-4 from a kink
SEEDS = {("mid_gen", "n1"): 99, ("mid_gen", "n2"): 77, ("mid_gen", "n3"): 10, ("mid_gen", "n4"): 3,
         ("upper_gen", "n1"): 56, ("upper_gen", "n2"): 109, ("upper_gen", "n3"): 172, ("upper_gen", "n4"): 3,
         ("upper_lds", "n1"): 99, ("upper_lds", "n2"): 77, ("upper_lds", "n3"): 10, ("upper_lds", "n4"): 3,
         ("upper_mem", "n1"): 37, ("upper_mem", "n2"): 12, ("upper_mem", "n3"): 202, ("upper_mem", "n4"): 3}
# SEED_STEPS: the first from 1234 up whose ten steps (offsets 0 .. 9, N = 40) keep at least 1.25e-4 along the double-precision oracle's trajectory
SEED_EIGHT, SEED_STEPS = 18, 4907


def compile_bnn(spec, estimator="pathwise"):
    model = build(spec)
    c = bnn.CompiledBnn(model, model.posterior_model, estimator)
    assert type(c).__name__ == "CompiledBnn"
    return c


def apply(layer, v):
    """the layer's activation through torch.nn.functional, with its parameters"""
    name = layer.get("activation_name") or {0: None, 1: "tanh", 2: "relu", 3: "sigmoid", 4: "softplus"}[layer["activation"]]
    if name is None:
        return v
    kw = {} if name == "relu6" else {k: p for (k, _), p in zip(bnn.ACTIVATION_PARAMS.get(name, ()), layer.get("activation_params", ()))}
    return getattr(F, name)(v, **kw)


def forward(c, noise, rows, dtype=torch.float64, theta=None):
    """the chain on the weights of the reported draws [n_rows, n] and the rows [M, P], a few lines of torch at `dtype` ->
    (the last layer's output [n, M, C], the hidden pre-activations of every layer); theta: the flat parameter vector (default: c's own)"""
    p = c.program
    loc, scale = bnn.row_parameters(p, c.params.detach().cpu().numpy() if theta is None else theta)
    w = torch.as_tensor(loc[:, None] + scale[:, None] * np.asarray(noise[:p.n_rows], dtype=np.float64)).to(dtype)      # [R, n]
    h = torch.as_tensor(np.asarray(rows, dtype=np.float64)).to(dtype)[None].expand(w.shape[1], -1, -1)
    pres = []
    for layer in p.layers:
        r, k, w0, b0 = layer["rows"], layer["cols"], layer["weight_row0"], layer["bias_row0"]
        pre = torch.einsum("nmk,nrk->nmr", h, w[w0:w0 + r * k].T.reshape(-1, r, k))
        if b0 != bnn.NO_BIAS:
            pre = pre + w[b0:b0 + r].T[:, None, :]
        pres.append(pre)
        h = apply(layer, pre)
    return h, pres[:-1]


def kink_margin(c, noise, idx, label="", theta=None):
    """the input condition of every comparison of gradients: no hidden pre-activation within MARGIN of a kink of its layer's function"""
    p = c.program
    _, pres = forward(c, noise, p.dataset[np.asarray(idx)], theta=theta)
    worst = np.inf
    for layer, pre in zip(p.layers, pres):
        name = layer.get("activation_name") or ("relu" if layer["activation"] == 2 else None)
        kinks = dict(relu=(0.0,), leaky_relu=(0.0,), relu6=(0.0, 6.0)).get(name, layer.get("activation_params", ()) if name == "hardtanh" else ())
        for k in kinks:
            worst = min(worst, float((pre - k).abs().min()))
    print(label, "kink margin %.3g" % worst)
    assert worst > MARGIN, "kink margin: a hidden pre-activation of %s lies %.3g from a kink of its activation (choose another seed)" % (label, worst)


def run_case(spec, path, middle, estimator, label, seed=3, first=None):
    c = compile_bnn(spec, estimator)
    assert c.middle_path() == middle and c.data_path() == path, (c.middle_path(), c.data_path())
    if first:
        assert c.first_layer_path() == first
    kw = spec[1]
    res = c.evaluate(N, seed=seed, offset=5, want_noise=True, want_indices=True, want_fvalues=True)
    assert c.middle_path() == middle
    idx = res["indices"].cpu().numpy()
    assert len(set(idx.tolist())) == kw["batch_size"] and idx.min() >= 0 and idx.max() < kw["dataset_size"]
    noise = res["noise"].cpu().numpy()
    kink_margin(c, noise, idx, label)
    named, mb = c.named_noise(noise, N), {c.program.indices_name: idx.tolist()}
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
@pytest.mark.parametrize("net", sorted(NETS))
@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_every_kind_in_every_middle_kernel(kernel, net, estimator, monkeypatch):
    """the four networks on the four kernels under both estimators (the draws of a seed, and so its kink margin, are the same under both)"""
    widths, pixels, switches, path = KERNELS[kernel]
    for k, v in switches.items():
        monkeypatch.setenv(k, v)
    c = run_case(classifier(widths, 17, pixels, activations=NETS[net]), path, kernel, estimator, "%s %s %s" % (kernel, net, estimator),
                 seed=SEEDS[kernel, net])
    assert [l["activation"] for l in c.program.layers] == [bnn.ACTIVATIONS[a if isinstance(a, str) else a[0]] for a in NETS[net]] + [0]


@pytest.mark.parametrize("estimator", ["pathwise", "blackbox"])
def test_the_seven_kinds_in_one_eight_layer_network(estimator):
    spec = classifier([P, 6, 6, 6, 6, 6, 6, 6, 3], 17, "integers", activations=SEVEN, q_scale=0.5)
    c = run_case(spec, "bf16x3", "mid_gen", estimator, "eight layers %s" % estimator, seed=SEED_EIGHT)
    assert [l["activation"] for l in c.program.layers] == [5, 6, 7, 8, 9, 10, 11, 0]
    assert c.program.layers[0]["activation_params"] == (0.2, 0.0) and c.program.layers[4]["activation_params"] == (-0.5, 2.0)


NARROW = dict(prior_loc=0.1, prior_scale=0.3, q_loc_scale=0.5)
TRUNKS = {
    # id: (spec, data path, middle kernel, first layer)
    "scale head": (regression([36, 5, 4, 3], 33, "normal", scale_head="softplus", activations=["silu", "gelu"]), "f32", "upper_gen", "per_sample"),
    "shared first layer": (regression([64, 9, 5, 1], 17, "integers", activations=["silu", "gelu"], point=("weights1", "b1"), **NARROW),
                           "bf16x3", "mid_gen", "shared"),
    "scale latent": (regression([64, 9, 5, 1], 17, "integers", activations=["silu", "gelu"], scale_latent={"tau": ["weights2", "b2"]},
                                scale_latent_prior=(-0.5, 0.7), scale_latent_q=(-0.8, 0.3), **NARROW), "bf16x3", "mid_gen", "per_sample"),
}


@pytest.mark.parametrize("estimator", ["pathwise", "blackbox"])
@pytest.mark.parametrize("case", sorted(TRUNKS))
def test_a_silu_gelu_trunk_under_the_other_features(case, estimator):
    spec, path, middle, first = TRUNKS[case]
    c = run_case(spec, path, middle, estimator, "%s %s" % (case, estimator), first=first)
    assert all(l["activation"] in (10, 11) for l in c.program.layers[:-1])


def test_taylor1_on_a_silu_gelu_trunk():
    spec = regression([P, 6, 5, 2], 17, "integers", activations=["silu", "gelu"])
    c = compile_bnn(spec, "taylor1")
    res = c.evaluate(N, seed=3, offset=5, want_noise=True, want_indices=True)
    named, mb = c.named_noise(res["noise"].cpu().numpy(), N), {c.program.indices_name: res["indices"].cpu().numpy().tolist()}
    exact, ref32 = oracle_pair(spec, "taylor1", named, mb)
    loss = float(res["loss"].item())
    print("taylor1 loss %.9g oracle64 %.9g oracle32 %.9g" % (loss, exact["loss"], ref32["loss"]))
    assert abs(loss - exact["loss"]) <= max(4 * abs(ref32["loss"] - exact["loss"]), TOL * abs(exact["loss"])), (loss, ref32["loss"], exact["loss"])
    yardstick_grad_check(c.named_grads(), exact["grads"], ref32["grads"])


@pytest.mark.parametrize("arm,widths,activations,q_scale", [("lds", [P, 6, 6, 6, 6, 6, 6, 6, 3], SEVEN, 0.5),
                                                            ("global", [P, 48, 44, 4], ["relu6", "gelu"], 0.2)])
def test_predict_on_both_arms_against_a_torch_forward_in_double(arm, widths, activations, q_scale):
    """33 held-out rows x 70 samples: logits, probabilities and their mean against the chain in torch (double; the same chain in single
    precision the yardstick, the bound of tests/test_gpu_bnn_predict.py) on the weight draws the call reports"""
    M = 33
    c = compile_bnn(classifier(widths, 17, "integers", activations=activations, q_scale=q_scale))
    assert c.predict_path() == arm, c.predict_path()
    rows = np.random.RandomState(3).normal(size=(M, P)).astype(np.float32)
    res = c.predict(rows, N, seed=5, offset=9, want_outputs=True, want_noise=True)
    noise = res["noise"].cpu().numpy()
    bad = []
    z64, z32 = forward(c, noise, rows)[0], forward(c, noise, rows, torch.float32)[0]
    for key, f in (("outputs", lambda z: z), ("probs", lambda z: torch.softmax(z, dim=2)), ("mean", lambda z: torch.softmax(z, dim=2).mean(dim=0))):
        e64, e32, got = f(z64).numpy(), f(z32).double().numpy(), res[key].cpu().numpy().astype(np.float64)
        assert got.shape == e64.shape, (key, got.shape, e64.shape)
        err, yard, scale = np.abs(got - e64).max(), np.abs(e32 - e64).max(), np.abs(e64).max()
        print("%s %-8s err %.3g  torch32 %.3g  scale %.3g" % (arm, key, err, yard, scale))
        if not err <= max(4 * yard, TOL * scale):
            bad.append((key, err, yard, scale))
    assert not bad, bad


def oracle_theta(program, oracle):
    """the flat parameter vector of `program` at the values an oracle holds now, in double"""
    held = {k: t.detach().numpy() for k, t in oracle.named_parameters().items()}
    theta = np.zeros(program.n_params, dtype=np.float64)
    for par, off, size, _ in program.parameters:
        theta[off:off + size] = held[par.name].reshape(-1)
    return theta


class DrawsWithMargin:
    """a noise sequence for Oracle.train that, when the oracle takes the draws of step `it` — it then holds the parameters that step is
    evaluated at —, first asserts the kink condition for these draws at THOSE parameters"""
    def __init__(self, c, oracle, noise_seq, raw):
        self.c, self.oracle, self.noise_seq, self.raw = c, oracle, noise_seq, raw

    def __getitem__(self, it):
        noise, idx = self.raw[it]
        kink_margin(self.c, noise, idx, "step %d at the double-precision oracle's parameters" % it, theta=oracle_theta(self.c.program, self.oracle))
        return self.noise_seq[it]


def test_ten_adam_steps_through_perform_inference_follow_the_oracle():
    """leaky_relu(0.2) and gelu, 32-6-5-2: `inference.perform_inference` against Oracle.train on the replayed draws and minibatches, the
    bounds of the family's other trajectory tests (losses: 4 x the single-precision oracle's distance from the double-precision one or 1e-5
    of the largest; parameters: that, or 2e-5 (1 + |value|)).  The kink condition is checked for every step inside the replay: on that
    step's draws at the parameters the double-precision oracle has stepped to (`DrawsWithMargin`; SEED_STEPS was chosen on the host so that
    all ten hold along that trajectory), before any loss of the trajectory is compared."""
    spec = regression([P, 6, 5, 2], 17, "integers", activations=[LEAKY, "gelu"])
    n, iters, lr = 40, 10, 1e-2
    torch.manual_seed(SEED_STEPS)
    seed = int(torch.initial_seed()) & 0x7FFFFFFFFFFFFFFF
    model, method = build(spec), inference.ReverseKL()
    inference.perform_inference(model, number_iterations=iters, number_samples=n, optimizer="Adam", lr=lr, pretraining_iterations=0,
                                inference_method=method)
    c = method.last_compiled
    assert type(c).__name__ == "CompiledBnn" and c.last_mode == "stepwise" and [l["activation"] for l in c.program.layers] == [5, 11, 0]
    got = np.asarray(model.diagnostics["loss curve"], dtype=np.float64)
    r = compile_bnn(spec)
    noise_seq, mb_seq, raw = [], [], []
    for it in range(iters):
        res = r.evaluate(n, seed=seed, offset=it, want_noise=True, want_indices=True)
        raw.append((res["noise"].cpu().numpy(), res["indices"].cpu().numpy()))
        noise_seq.append(r.named_noise(raw[-1][0], n))
        mb_seq.append({r.program.indices_name: raw[-1][1].tolist()})
    o64, o32 = Oracle(build(spec), dtype=torch.float64), Oracle(build(spec))
    exact_losses = o64.train(iters, n, "Adam", noise_seq=DrawsWithMargin(r, o64, noise_seq, raw), minibatch_seq=mb_seq, pretraining_iterations=0,
                             lr=lr).astype(np.float64)
    ref_losses = o32.train(iters, n, "Adam", noise_seq=noise_seq, minibatch_seq=mb_seq, pretraining_iterations=0, lr=lr).astype(np.float64)
    print("losses", got, exact_losses, ref_losses)
    assert np.isfinite(got).all() and got.shape == (iters,)
    assert np.abs(got - exact_losses).max() <= max(4 * np.abs(ref_losses - exact_losses).max(), TOL * np.abs(exact_losses).max())
    e64 = {k: t.detach().numpy() for k, t in o64.named_parameters().items()}
    e32 = {k: t.detach().numpy() for k, t in o32.named_parameters().items()}
    for pname, p in c.named_params().items():
        x = e64[pname].reshape(p.shape)
        assert np.abs(p - x).max() <= max(4 * np.abs(e32[pname].reshape(p.shape) - x).max(), 2e-5 * (1 + np.abs(x).max())), pname


def test_the_library_checks_the_parameters_itself():
    """bsvi_bnn_set_activation_params: every refusal by its message, kind 12 refused at create, and nothing accepted after a launch"""
    import ctypes as C
    from brancher_amd import native
    c = compile_bnn(classifier([P, 6, 5, 4, 3], 17, "integers", activations=[LEAKY, ELU, HARD]))
    lib, INVALID = c.lib, -1
    call = lambda values, n=4: (lib.bsvi_bnn_set_activation_params(c.handle, np.asarray(values, dtype=np.float32).ctypes.data_as(C.c_void_p), n),
                                lib.bsvi_last_error())
    good = [0.2, 0.0, 0.7, 0.0, -0.5, 2.0, 0.0, 0.0]
    for at, value, message in ((0, 0.0, b"negative_slope"), (0, -1.0, b"negative_slope"), (2, 0.0, b"alpha"), (4, 2.0, b"min_val < max_val"),
                               (5, -0.5, b"min_val < max_val"), (1, np.nan, b"not finite"), (6, np.inf, b"not finite")):
        bad = list(good)
        bad[at] = value
        status, err = call(bad)
        assert status == INVALID and message in err, (at, value, err)
    status, err = call(good, 3)
    assert status == INVALID and b"n_layers" in err
    assert lib.bsvi_bnn_set_activation_params(c.handle, None, 4) == INVALID
    assert call(good)[0] == 0
    c.evaluate(N, seed=1, offset=0)
    status, err = call(good)
    assert status == INVALID and b"launch" in err
    # kinds: 11 is the last
    d, keep = bnn.make_desc(c.program)
    keep["layers"][0].activation = 12
    handle = C.c_void_p()
    assert lib.bsvi_bnn_create(C.byref(d), C.byref(handle)) != 0 and b"unknown activation" in lib.bsvi_last_error()
    keep["layers"][0].activation = 11
    keep["layers"][3].activation = 11
    assert lib.bsvi_bnn_create(C.byref(d), C.byref(handle)) != 0 and b"the last layer yields the logits" in lib.bsvi_last_error()
    assert native.ABI_VERSION == 11
