"""Stein variational gradient descent on the device: `bsvi_svgd_direction` (csrc/svgd_kernel.hip) against the formulas of
include/bsvi.h written out in torch in double, and `inference.SteinVariationalGradientDescent` through `perform_inference` against a
float64 torch loop (autograd on the same log density, the same direction, plain SGD).

The bound everywhere is the project's yardstick, capped: min(max(4 |ref32 - ref64|, 1e-5 scale), 1e-4 scale) — ref32 the same torch code in
float32 with direct differences theta_i - theta_j, scale the largest magnitude of the expected output."""
import numpy as np
import pytest
import torch

from brancher_amd import bnn, inference, native, workloads as W
from brancher_amd.standard_variables import NormalVariable
from brancher_amd.variables import ProbabilisticModel, RootVariable

pytestmark = pytest.mark.gpu
DEV = "cuda"


def direction(theta, grad, bandwidth=None):
    """(out, bandwidth) in the dtype of theta"""
    n = theta.shape[0]
    d = ((theta[:, None, :] - theta[None, :, :]) ** 2).sum(-1)
    if bandwidth is None:
        rows, cols = torch.triu_indices(n, n, 1)
        bandwidth = 2 * np.median(d[rows, cols].sqrt().numpy()) ** 2 / np.log(theta.new_tensor(float(n)).numpy())
    k = torch.exp(-d / (2 * bandwidth))
    return k @ grad - (theta * k.sum(1, keepdim=True) - k @ theta) / bandwidth, bandwidth


def bound(ref32, ref64):
    ref32, ref64 = np.asarray(ref32, dtype=np.float64), np.asarray(ref64, dtype=np.float64)
    scale = np.abs(ref64).max()
    return np.minimum(np.maximum(4 * np.abs(ref32 - ref64), 1e-5 * scale), 1e-4 * scale)


def within(got, ref32, ref64, what):
    got, ref64 = np.asarray(got, dtype=np.float64), np.asarray(ref64, dtype=np.float64)
    excess = np.abs(got - ref64) - bound(ref32, ref64)
    assert np.isfinite(got).all() and excess.max() <= 0, "%s: off by %.3g where %.3g is allowed" % (
        what, np.abs(got - ref64).reshape(-1)[excess.argmax()], bound(ref32, ref64).reshape(-1)[excess.argmax()])


def particles(n, dim, ld, centre=0.0, spread=1.0, seed=0):
    g = torch.Generator().manual_seed(seed + 1000 * n + dim)
    theta, grad = torch.zeros(n, ld), torch.zeros(n, ld)
    theta[:, :dim] = centre + spread * torch.randn(n, dim, generator=g)
    grad[:, :dim] = torch.randn(n, dim, generator=g)
    return theta, grad


def run(theta, grad, dim, bandwidth, in_place=False):
    th, g = theta.to(DEV), grad.to(DEV)
    out = g if in_place else torch.full_like(g, 7.0)            # (7: what a column past dim must still hold)
    bw = torch.zeros(1, device=DEV)
    native.svgd_direction(th, g, out, dim=dim, bandwidth=bandwidth, bandwidth_out=bw)
    return out.cpu(), float(bw.item())


def check_direction(theta, grad, dim, bandwidth):
    out, bw = run(theta, grad, dim, bandwidth)
    r64, bw64 = direction(theta[:, :dim].double(), grad[:, :dim].double(), bandwidth)
    r32, bw32 = direction(theta[:, :dim], grad[:, :dim], bandwidth)
    within(bw, bw32, bw64, "bandwidth")
    within(out[:, :dim].numpy(), r32.numpy(), r64.numpy(), "out")
    assert (out[:, dim:] == 7.0).all()


SHAPES = [(2, 1, 1), (3, 5, 8), (4, 3, 3), (33, 70, 70), (64, 257, 260), (130, 1000, 1000)]


@pytest.mark.parametrize("bandwidth", [None, 0.7], ids=["median", "fixed"])
@pytest.mark.parametrize("n,dim,ld", SHAPES)
def test_direction_against_torch_in_double(n, dim, ld, bandwidth):
    check_direction(*particles(n, dim, ld), dim, bandwidth)


@pytest.mark.parametrize("bandwidth", [None, 0.7], ids=["median", "fixed"])
def test_particles_far_from_the_origin(bandwidth):
    check_direction(*particles(33, 70, 70, centre=100.0, spread=0.1), 70, bandwidth)


@pytest.mark.parametrize("n,dim,ld", [(33, 70, 70), (64, 257, 260)])
def test_in_place_and_twice_give_the_same_bits(n, dim, ld):
    theta, grad = particles(n, dim, ld)
    first, bw1 = run(theta, grad, dim, None)
    again, bw2 = run(theta, grad, dim, None)
    aliased, bw3 = run(theta, grad, dim, None, in_place=True)
    assert bw1 == bw2 == bw3 and torch.equal(first, again) and torch.equal(first[:, :dim], aliased[:, :dim])


def test_coincident_particles_are_refused_and_nothing_is_written():
    theta, grad = torch.ones(3, 5), particles(3, 5, 5)[1]
    th, g, out = theta.to(DEV), grad.to(DEV), torch.full((3, 5), 7.0, device=DEV)
    with pytest.raises(native.NativeError, match="all particles coincide"):
        native.svgd_direction(th, g, out)
    assert (out == 7.0).all()


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
def log_normal(x, loc, scale):
    return -0.5 * ((x - loc) / scale) ** 2 - np.log(scale) - 0.5 * np.log(2 * np.pi)


def scalar_case():
    y = np.array([0.3, -0.8, 1.9, 0.6, 1.1, -0.2], dtype=np.float32).reshape(-1, 1)
    mu = NormalVariable(0.0, 2.0, "mu")
    obs = NormalVariable(mu, 1.0, "y")
    model = ProbabilisticModel([obs])
    obs.observe(y)
    start = {"mu": np.linspace(-1.0, 2.0, 5).reshape(5, 1, 1)}

    def log_p(theta):           # theta [D] -> log p(theta, data)
        return log_normal(theta[0], 0.0, 2.0) + log_normal(theta.new_tensor(y.reshape(-1)), theta[0], 1.0).sum()
    return model, start, log_p, 5, 0.05


def bnn_case():
    # 64-4-1, tanh, the full batch of 16 rows: the smallest network the scalar engine in front of this path leaves to it (its unrolled sums
    # stop at 4096 terms); 265 numbers a particle
    model = W.build_bnn_regression(W.native_api(), point="all", prior_loc=0.1, prior_scale=0.3, dataset_size=16, batch_size=16,
                                   n_features=64, n_hidden=4, n_outputs=1)
    roots = {v.name: v.parameter.numpy().reshape(v.parameter.shape[-2:]) for v in model.posterior_model.flatten()}
    rng = np.random.RandomState(5)
    start = {k: np.stack([v + 0.05 * rng.normal(size=v.shape) for _ in range(3)]) for k, v in sorted(roots.items())}
    program = bnn.lower_bnn(model, model.posterior_model)
    assert program.lik_weight == 1.0 and program.prior_weight == 1.0

    def log_p(theta):
        x, y = theta.new_tensor(program.dataset), theta.new_tensor(program.labels)
        b1, b2, w1, w2 = theta[0:4], theta[4:5], theta[5:261].reshape(4, 64), theta[261:265].reshape(1, 4)
        net = torch.tanh(x @ w1.T + b1) @ w2.T + b2
        return log_normal(theta, 0.1, 0.3).sum() + log_normal(y, net, 0.5).sum()
    return model, start, log_p, 2, 0.002


def torch_loop(start, log_p, iterations, lr, dtype):
    theta = torch.tensor(np.concatenate([v.reshape(v.shape[0], -1) for v in start.values()], axis=1), dtype=dtype)
    curve = []
    for _ in range(iterations):
        theta.requires_grad_(True)
        losses = torch.stack([-log_p(row) for row in theta])
        grad, = torch.autograd.grad(losses.sum(), theta)
        theta = theta.detach()
        curve.append(float(losses.sum().detach()))
        theta = theta - lr * direction(theta, grad)[0]
    return theta.numpy(), np.array(curve)


@pytest.mark.parametrize("case,engine_name", [(scalar_case, "CompiledELBO"), (bnn_case, "CompiledBnn")], ids=["scalar", "bnn"])
def test_sgd_iterations_through_perform_inference_follow_the_torch_loop(case, engine_name):
    model, start, log_p, iterations, lr = case()
    n = len(next(iter(start.values())))
    parts = [ProbabilisticModel([RootVariable(v[i], k, learnable=True) for k, v in start.items()]) for i in range(n)]
    method = inference.SteinVariationalGradientDescent()
    inference.perform_inference(model, number_iterations=iterations, optimizer="SGD", lr=lr, inference_method=method, posterior_model=parts)
    assert {type(v.parameter._store).__name__ for p in parts for v in p.flatten()} == {engine_name}
    t64, c64 = torch_loop(start, log_p, iterations, lr, torch.float64)
    t32, c32 = torch_loop(start, log_p, iterations, lr, torch.float32)
    got = np.stack([np.concatenate([next(v for v in p.flatten() if v.name == k).parameter.numpy().reshape(-1) for k in start]) for p in parts])
    within(model.diagnostics["loss curve"], c32, c64, "loss curve")
    within(got, t32, t64, "particles")
    assert method.bandwidth > 0 and np.isfinite(method.bandwidth)
