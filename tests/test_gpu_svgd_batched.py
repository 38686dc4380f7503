"""All particles of a Bayesian neural network in one pass (csrc/bnn_particles.inc): `native.bnn_particles_fwd_bwd` against
-log p(theta_n, data) in torch and its autograd gradient in double, `SteinVariationalGradientDescent(batched=True)` against a float64 torch
loop.  The bound is the project's yardstick, capped: min(max(4 |ref32 - ref64|, 1e-5 scale), 1e-4 scale), ref32 the same code in float32."""
import numpy as np
import pytest
import torch

from brancher_amd import bnn, inference, native, workloads as W
from brancher_amd.variables import ProbabilisticModel, RootVariable

pytestmark = pytest.mark.gpu
PRIOR_LOC, PRIOR_SCALE, SIGMA = 0.1, 0.3, 0.5


def bound(ref32, ref64):
    ref32, ref64 = np.asarray(ref32, dtype=np.float64), np.asarray(ref64, dtype=np.float64)
    scale = np.abs(ref64).max()
    return np.minimum(np.maximum(4 * np.abs(ref32 - ref64), 1e-5 * scale), 1e-4 * scale)


def within(got, ref32, ref64, what):
    got, ref64 = np.asarray(got, dtype=np.float64), np.asarray(ref64, dtype=np.float64)
    excess = np.abs(got - ref64) - bound(ref32, ref64)
    print("%s: largest error %.3g, allowed there %.3g" % (what, np.abs(got - ref64).reshape(-1)[excess.argmax()], bound(ref32, ref64).reshape(-1)[excess.argmax()]))
    assert np.isfinite(got).all() and excess.max() <= 0, what


def network(n_features, hidden, outputs, exact, prior="normal"):      # every tensor a point; the full batch of 16 rows: the BNN path
    kw = dict(point="all", prior=prior, prior_loc=PRIOR_LOC, prior_scale=PRIOR_SCALE, dataset_size=16, batch_size=16,
              widths=[n_features, *hidden, outputs])
    if outputs == 1:
        model = W.build_bnn_regression(W.native_api(), sigma=SIGMA, data="integers" if exact else "normal", **kw)
    else:
        model = W.build_bayesian_neural_network(W.native_api(), pixels="integers" if exact else "normal", **kw)
    return model, bnn.lower_bnn(model, model.posterior_model)


def log_p(program, theta):      # theta [N][D] in the latent vector's row order -> log p(theta_n, data) [N]
    t = {s["name"]: theta[:, s["row0"]:s["row0"] + s["size"]].reshape(-1, s["rows"], s["cols"]) for s in program.tensors}
    total = 0.0
    for s in program.tensors:
        u = (t[s["name"]] - PRIOR_LOC) / PRIOR_SCALE
        value = {"normal": -0.5 * u ** 2 - np.log(PRIOR_SCALE) - 0.5 * np.log(2 * np.pi), "laplace": -u.abs() - np.log(2 * PRIOR_SCALE),
                 "cauchy": -torch.log1p(u ** 2) - np.log(np.pi * PRIOR_SCALE)}[s["prior"]]
        total = total + value.sum((1, 2))
    h = theta.new_tensor(program.dataset).expand(theta.shape[0], -1, -1)
    for i, layer in enumerate(program.layers):
        h = h @ t[layer["weights"]].transpose(1, 2) + t[layer["bias"]].transpose(1, 2)
        h = torch.tanh(h) if i + 1 < len(program.layers) else h
    if program.likelihood == bnn.LIK_NORMAL:
        y = theta.new_tensor(program.labels)
        return total + (-0.5 * ((y - h) / SIGMA) ** 2 - np.log(SIGMA) - 0.5 * np.log(2 * np.pi)).sum((1, 2))
    labels = torch.as_tensor(program.labels, dtype=torch.int64).expand(theta.shape[0], -1)
    return total + torch.log_softmax(h, -1).gather(2, labels[:, :, None]).sum((1, 2))


def loss_and_grad(program, theta, dtype):
    loss = -log_p(program, theta := theta.to(dtype).requires_grad_(True))
    return loss.detach().numpy(), torch.autograd.grad(loss.sum(), theta)[0].numpy()


def evaluate(model, program, theta, ld):
    compiled = bnn.CompiledBnn(model, model.posterior_model, program=program)
    table = torch.nn.functional.pad(theta, (0, ld - theta.shape[1]))
    grad, loss = torch.full((theta.shape[0], ld), 7.0, device="cuda"), torch.zeros(theta.shape[0], device="cuda")
    native.bnn_particles_fwd_bwd(compiled.handle, compiled.params, compiled.out, table.to("cuda"), grad, loss, seed=3)
    return loss.cpu().numpy(), grad.cpu().numpy(), compiled


def check(n, n_features, hidden, outputs, exact, prior="normal", ld_extra=0):
    model, program = network(n_features, hidden, outputs, exact, prior)
    dim = program.n_rows
    theta = PRIOR_LOC + 0.1 * torch.randn(n, dim, generator=torch.Generator().manual_seed(n + dim))
    loss, grad, compiled = evaluate(model, program, theta, (dim + 3) // 4 * 4 + ld_extra)
    assert compiled.data_path() == ("bf16x3" if exact else "f32") and compiled.first_layer_path() == "per_sample"
    (l64, g64), (l32, g32) = loss_and_grad(program, theta, torch.float64), loss_and_grad(program, theta, torch.float32)
    within(loss, l32, l64, "loss")
    within(grad[:, :dim], g32, g64, "gradient")
    assert (grad[:, dim:] == 7.0).all()


# N at the edges of 4 particles a workgroup, 64 lanes and n_pad; 68 features: a Kp pad and a partial LDS tile; (20, 4): a second product
# of the upper layers; exact or not: both GT layouts; ld_extra = 3: rows that are not 16-byte aligned (the scalar loads and stores)
@pytest.mark.parametrize("n,n_features,hidden,outputs,exact,ld_extra", [
    (2, 64, (4,), 1, True, 0), (3, 64, (4,), 1, False, 0), (3, 68, (4,), 3, True, 0), (65, 64, (20, 4), 1, True, 0),
    (65, 68, (4,), 3, False, 0), (130, 68, (20, 4), 3, True, 0), (130, 64, (4,), 1, False, 0), (2, 68, (20, 4), 1, False, 0),
    (3, 64, (20, 4), 3, True, 0), (65, 68, (20, 4), 1, True, 0), (130, 64, (4,), 3, True, 0), (2, 64, (4,), 3, False, 0),
    (3, 64, (4,), 1, True, 3), (65, 68, (4,), 1, False, 3)])
def test_particles_against_torch_autograd_in_double(n, n_features, hidden, outputs, exact, ld_extra):
    check(n, n_features, hidden, outputs, exact, ld_extra=ld_extra)


@pytest.mark.parametrize("prior", ["normal", "laplace", "cauchy", dict(weights1="laplace", b1="cauchy", weights2="normal", b2="laplace")],
                         ids=["normal", "laplace", "cauchy", "mixed"])
@pytest.mark.parametrize("exact", [True, False], ids=["bf16x3", "f32"])
def test_every_prior_kind(prior, exact):
    check(3, 64, (4,), 1, exact, prior)


@pytest.mark.parametrize("exact", [True, False], ids=["bf16x3", "f32"])
def test_the_same_call_twice_gives_the_same_bits(exact):
    model, program = network(68, (20, 4), 3, exact)
    theta = PRIOR_LOC + 0.1 * torch.randn(65, program.n_rows, generator=torch.Generator().manual_seed(1))
    first, again = (evaluate(model, program, theta, (program.n_rows + 3) // 4 * 4) for _ in range(2))
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])


def direction(theta, grad):
    d = ((theta[:, None, :] - theta[None, :, :]) ** 2).sum(-1)
    n = theta.shape[0]
    rows, cols = torch.triu_indices(n, n, 1)
    bandwidth = 2 * np.median(d[rows, cols].sqrt().numpy()) ** 2 / np.log(theta.new_tensor(float(n)).numpy())
    k = torch.exp(-d / (2 * bandwidth))
    return k @ grad - (theta * k.sum(1, keepdim=True) - k @ theta) / bandwidth


def torch_loop(program, start, iterations, optimizer, lr, dtype):
    theta = torch.tensor(start, dtype=dtype, requires_grad=True)
    opt = getattr(torch.optim, optimizer)([theta], lr=lr)
    curve = []
    for _ in range(iterations):
        losses = -log_p(program, theta)
        grad, = torch.autograd.grad(losses.sum(), theta)
        curve.append(float(losses.sum().detach()))
        theta.grad = direction(theta.detach(), grad)
        opt.step()
    return theta.detach().numpy(), np.array(curve)


@pytest.mark.parametrize("n,optimizer,lr", [(3, "SGD", 0.002), (65, "SGD", 0.002), (3, "Adam", 0.001)])
def test_iterations_through_perform_inference_follow_the_torch_loop(n, optimizer, lr):
    model, program = network(64, (4,), 1, True)
    start = PRIOR_LOC + 0.05 * np.random.RandomState(5).normal(size=(n, program.n_rows))
    parts = [ProbabilisticModel([RootVariable(row[t["row0"]:t["row0"] + t["size"]].reshape(t["rows"], t["cols"]), t["name"], learnable=True)
                                 for t in program.tensors]) for row in start]
    method = inference.SteinVariationalGradientDescent(batched=True)
    inference.perform_inference(model, number_iterations=2, optimizer=optimizer, lr=lr, inference_method=method, posterior_model=parts)
    assert {type(v.parameter._store).__name__ for p in parts for v in p.flatten()} == {"CompiledBnn"}
    got = np.stack([np.concatenate([next(v for v in p.flatten() if v.name == t["name"]).parameter.numpy().reshape(-1) for t in program.tensors])
                    for p in parts])
    (t64, c64), (t32, c32) = (torch_loop(program, start, 2, optimizer, lr, dtype) for dtype in (torch.float64, torch.float32))
    within(model.diagnostics["loss curve"], c32, c64, "loss curve")
    within(got, t32, t64, "particles")
    assert method.bandwidth > 0 and np.isfinite(method.bandwidth)
