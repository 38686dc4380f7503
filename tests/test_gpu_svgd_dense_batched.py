"""All particles of a logistic regression in one fused kernel (csrc/dense_particles.inc): `native.dense_particles_fwd_bwd`
against -log p(theta_n, data) in torch and its autograd gradient in double, `SteinVariationalGradientDescent(batched=True)` against a
float64 torch loop and against batched=False.  The bound is the one of tests/test_gpu_svgd_batched.py:
min(max(4 |ref32 - ref64|, 1e-5 scale), 1e-4 scale), ref32 the same code in float32."""
import numpy as np
import pytest
import torch

from brancher_amd import dense, inference, native, workloads as W
from brancher_amd.variables import ProbabilisticModel, RootVariable

pytestmark = pytest.mark.gpu


def within(got, ref32, ref64, what):
    got, ref32, ref64 = (np.asarray(a, dtype=np.float64) for a in (got, ref32, ref64))
    scale = np.abs(ref64).max()
    allowed = np.minimum(np.maximum(4 * np.abs(ref32 - ref64), 1e-5 * scale), 1e-4 * scale)
    excess = np.abs(got - ref64) - allowed
    print("%s: largest error %.3g, allowed there %.3g" % (what, np.abs(got - ref64).reshape(-1)[excess.argmax()], allowed.reshape(-1)[excess.argmax()]))
    assert np.isfinite(got).all() and excess.max() <= 0, what


def regression(c, p, b):      # the full batch of b rows: the minibatch is the dataset, whatever the order
    api = W.native_api()
    if c > 1:
        model = W.build_map_logistic_regression(api, dataset_size=b, n_features=p, n_classes=c)
    else:
        model = W.build_binary_logistic_regression(api, dataset_size=b, batch_size=b, n_features=p)
        model.set_posterior_model(api.ProbabilisticModel([api.RootVariable(np.zeros((1, p)), name="weights", learnable=True)]))
    program = dense.lower_dense(model, model.posterior_model)
    return model, program, (10.0 if c > 1 else 0.5)      # the builders' prior: Normal(0, scale)


def log_p(program, scale, theta):      # theta [N][C P] -> log p(theta_n, data) [N]
    prior = (-0.5 * (theta / scale) ** 2 - np.log(scale) - 0.5 * np.log(2 * np.pi)).sum(1)
    logits = theta.reshape(theta.shape[0], program.n_classes, program.n_features) @ theta.new_tensor(program.dataset).T      # [N][C][B]
    if program.likelihood == dense.LIK_BERNOULLI:
        k = theta.new_tensor(program.labels)
        return prior + (k * logits[:, 0] - torch.nn.functional.softplus(logits[:, 0])).sum(1)
    labels = torch.as_tensor(program.labels, dtype=torch.int64).expand(theta.shape[0], 1, -1)
    return prior + torch.log_softmax(logits, 1).gather(1, labels).sum((1, 2))


def loss_and_grad(program, scale, theta, dtype):
    loss = -log_p(program, scale, theta := theta.to(dtype).requires_grad_(True))
    return loss.detach().numpy(), torch.autograd.grad(loss.sum(), theta)[0].numpy()


def evaluate(model, program, theta, ld):
    compiled = dense.CompiledDense(model, model.posterior_model, program=program, particles=True)
    table = torch.nn.functional.pad(theta, (0, ld - theta.shape[1]))
    grad, loss = torch.full((theta.shape[0], ld), 7.0, device="cuda"), torch.zeros(theta.shape[0], device="cuda")
    native.dense_particles_fwd_bwd(compiled.handle, compiled.params, compiled.out, table.to("cuda"), grad, loss, seed=3)
    return loss.cpu().numpy(), grad.cpu().numpy()


# N: 2; one block exactly (3 x 10) and a second with dead particles (4 x 10); 32 Bernoulli particles a block and one more; 65, 130.
# C: 7 leaves dead rows in the block, 32 none.  P: 4 below a k chunk, 5 odd rows, 68 a partial 32-column block, 784 seven blocks a wave.
# B: 5 and 16 a masked tile, 130 a second pass with a partial tile.  Few workgroups deal the passes over grid.y, one pass a workgroup and
# the join launch; on the 256 compute units of the MI355X 256 workgroups (256 x 32 classes) keep both passes in one workgroup and its own
# epilogue, and 86 workgroups at 300 rows (256 x 10 classes) make two splits, the first of two passes, before the join.
# P: 200 and 400 select the variants of two and four 32-feature blocks a wave.  ld_extra = 3: rows that are not 16-byte aligned.
@pytest.mark.parametrize("n,c,p,b,ld_extra", [
    (2, 3, 4, 5, 0), (3, 10, 68, 16, 0), (4, 10, 5, 130, 0), (33, 1, 5, 16, 0), (65, 10, 68, 130, 0), (130, 3, 4, 5, 0),
    (5, 7, 68, 130, 0), (2, 16, 5, 16, 0), (3, 32, 68, 5, 0), (2, 1, 68, 130, 3), (65, 7, 5, 16, 3), (4, 10, 784, 130, 0),
    (256, 32, 4, 130, 0), (256, 10, 5, 300, 0), (2, 3, 200, 16, 0), (2, 3, 400, 16, 0)])
def test_particles_against_torch_autograd_in_double(n, c, p, b, ld_extra):
    model, program, scale = regression(c, p, b)
    dim = c * p
    theta = 0.1 * torch.randn(n, dim, generator=torch.Generator().manual_seed(n + dim))
    loss, grad = evaluate(model, program, theta, (dim + 3) // 4 * 4 + ld_extra)
    (l64, g64), (l32, g32) = loss_and_grad(program, scale, theta, torch.float64), loss_and_grad(program, scale, theta, torch.float32)
    within(loss, l32, l64, "loss")
    within(grad[:, :dim], g32, g64, "gradient")
    assert (grad[:, dim:] == 7.0).all()


@pytest.mark.parametrize("n,c,p,b", [(65, 10, 68, 130), (256, 32, 4, 130), (256, 10, 5, 300)])
def test_the_same_call_twice_gives_the_same_bits(n, c, p, b):
    model, program, _ = regression(c, p, b)
    theta = 0.1 * torch.randn(n, c * p, generator=torch.Generator().manual_seed(1))
    first, again = (evaluate(model, program, theta, (c * p + 3) // 4 * 4) for _ in range(2))
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])


def direction(theta, grad):
    d = ((theta[:, None, :] - theta[None, :, :]) ** 2).sum(-1)
    n = theta.shape[0]
    rows, cols = torch.triu_indices(n, n, 1)
    bandwidth = 2 * np.median(d[rows, cols].sqrt().numpy()) ** 2 / np.log(theta.new_tensor(float(n)).numpy())
    k = torch.exp(-d / (2 * bandwidth))
    return k @ grad - (theta * k.sum(1, keepdim=True) - k @ theta) / bandwidth


def torch_loop(program, scale, start, iterations, optimizer, lr, dtype):
    theta = torch.tensor(start, dtype=dtype, requires_grad=True)
    opt = getattr(torch.optim, optimizer)([theta], lr=lr)
    curve = []
    for _ in range(iterations):
        losses = -log_p(program, scale, theta)
        grad, = torch.autograd.grad(losses.sum(), theta)
        curve.append(float(losses.sum().detach()))
        theta.grad = direction(theta.detach(), grad)
        opt.step()
    return theta.detach().numpy(), np.array(curve)


@pytest.mark.parametrize("n,optimizer,lr", [(3, "SGD", 0.002), (65, "SGD", 0.002), (3, "Adam", 0.001)])
def test_iterations_through_perform_inference_follow_the_torch_loop(n, optimizer, lr):
    start = 0.05 * np.random.RandomState(5).normal(size=(n, 12))
    curves = {}
    for batched in (True, False):
        model, program, scale = regression(3, 4, 16)
        parts = [ProbabilisticModel([RootVariable(row.reshape(3, 4), "weights", learnable=True)]) for row in start]
        method = inference.SteinVariationalGradientDescent(batched=batched)
        inference.perform_inference(model, number_iterations=2, optimizer=optimizer, lr=lr, inference_method=method, posterior_model=parts)
        curves[batched] = np.asarray(model.diagnostics["loss curve"], dtype=np.float64)
        if batched:
            assert {type(v.parameter._store).__name__ for p in parts for v in p.flatten()} == {"CompiledDense"}
            got = np.stack([next(iter(p.flatten())).parameter.numpy().reshape(-1) for p in parts])
            assert method.bandwidth > 0 and np.isfinite(method.bandwidth)
    (t64, c64), (t32, c32) = (torch_loop(program, scale, start, 2, optimizer, lr, dtype) for dtype in (torch.float64, torch.float32))
    within(curves[True], c32, c64, "loss curve")
    within(curves[False], c32, c64, "loss curve of batched=False")
    within(got, t32, t64, "particles")
