"""Stein variational gradient descent on a target with two modes.

The model observes y = mu^2 with noise, so the posterior of mu has a mode near +sqrt(y) and one near -sqrt(y).  MAP finds one of them and
says nothing about its width.  Twelve particles started around zero fall into both modes, and the repulsion of SVGD keeps the particles of
a mode apart: they end as a sample of both modes with a spread, not as two points.  `bandwidth=None` is the reference's median rule.  The
direction carries no 1 / N (as in the reference), so the step size is chosen for the sum over the particles.

    python examples/svgd_two_modes.py
"""
import numpy as np

from brancher_amd import inference
from brancher_amd.standard_variables import NormalVariable
from brancher_amd.variables import ProbabilisticModel, RootVariable


def main(n_particles=12, iterations=600, lr=0.005):
    mu = NormalVariable(0.0, 2.0, "mu")
    y = NormalVariable(mu * mu, 1.0, "y")
    model = ProbabilisticModel([y])
    y.observe(np.full((2, 1), 1.5, dtype=np.float32))

    start = np.linspace(-0.55, 0.6, n_particles)
    roots = [RootVariable(np.array([[v]]), "mu", learnable=True) for v in start]
    particles = [ProbabilisticModel([root]) for root in roots]
    method = inference.SteinVariationalGradientDescent()
    inference.perform_inference(model, number_iterations=iterations, optimizer="SGD", lr=lr,
                                inference_method=method, posterior_model=particles)
    end = np.array([float(root.value.reshape(-1)[0]) for root in roots])
    print("start :", np.round(start, 2))
    print("end   :", np.round(np.sort(end), 2))
    print("modes : +-%.2f,  particles below zero: %d of %d,  last bandwidth %.3f" % (np.sqrt(1.5), (end < 0).sum(), n_particles, method.bandwidth))
    print("loss  : %.2f -> %.2f" % (model.diagnostics["loss curve"][0], model.diagnostics["loss curve"][-1]))


if __name__ == "__main__":
    main()
