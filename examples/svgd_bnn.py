"""Stein variational gradient descent on a small Bayesian neural network, all particles in one pass.

A 64-8-1 tanh regression network; sixteen particles, each a point estimate of all four tensors, start as small random networks.
`batched=True` evaluates every particle's loss and gradient in one call (the particles ride the sample axis of the network's kernels),
couples the gradients and steps one table that holds all particles.  The particles end as a sample of the posterior: the spread of their
predictions is the model's uncertainty about its mean, next to the noise scale it was given.

    python examples/svgd_bnn.py
"""
import numpy as np

from brancher_amd import inference, workloads as W
from brancher_amd.variables import ProbabilisticModel, RootVariable


def main(n_particles=16, iterations=300, lr=2e-4):
    model = W.build_bnn_regression(W.native_api(), point="all", dataset_size=48, batch_size=48, n_features=64, n_hidden=8, n_outputs=1,
                                   prior_loc=0.0, prior_scale=0.5, prior="normal", sigma=0.5)
    shapes = {v.name: v.parameter.shape[-2:] for v in model.posterior_model.flatten()}
    rng = np.random.RandomState(0)
    particles = [ProbabilisticModel([RootVariable(0.05 * rng.normal(size=shape), name, learnable=True) for name, shape in sorted(shapes.items())])
                 for _ in range(n_particles)]
    method = inference.SteinVariationalGradientDescent(batched=True)
    inference.perform_inference(model, number_iterations=iterations, optimizer="Adam", lr=lr, inference_method=method, posterior_model=particles)

    program = method.last_compiled.program
    x, y = program.dataset, program.labels                       # [rows, 64], [rows, 1]
    result = method.predict_network(model, particles, x)      # all particles on all rows in one fused kernel, their table read in place
    mean, spread = result["mean"].cpu().numpy(), result["probs"].std(0, unbiased=False).cpu().numpy()      # [rows, 1] each
    curve = model.diagnostics["loss curve"]
    print("loss (sum over %d particles): %.1f -> %.1f, last bandwidth %.3f" % (n_particles, curve[0], curve[-1], method.bandwidth))
    print("rmse of the particles' mean prediction: %.3f (noise scale 0.5)" % np.sqrt(((mean - y) ** 2).mean()))
    print("predictive spread over the particles, per row: mean %.3f, min %.3f, max %.3f" % (
        spread.mean(), spread.min(), spread.max()))


if __name__ == "__main__":
    main()
