"""Stein variational gradient descent on a multinomial logistic regression, all particles in one fused kernel.

Three classes, four features (iris-like magnitudes); the particles are point estimates of the weight matrix, as in the reference's SVGD
playground, and start as small random matrices.  `batched=True` evaluates every particle's loss and gradient in one call
(csrc/dense_particles.inc), couples the gradients and steps one table that holds all particles.  The ensemble predicts with the mean of
the particles' softmax, here on rows the particles never saw: one `predict` call (csrc/dense_predict.inc) reads the particles' table in
place and hands back every particle's probabilities and their mean — the playground's last step, without its loop over particles and rows.

    python examples/svgd_logistic_regression.py
"""
import numpy as np
import torch

from brancher_amd import inference, workloads as W
from brancher_amd.variables import ProbabilisticModel, RootVariable


def labelled_rows(n_rows, n_features, n_classes, seed):
    """features like the builder's (uniform, times six) with labels a fixed linear rule gives them, so that there is something to learn"""
    rng = np.random.RandomState(seed)
    x = (6.0 * rng.uniform(0.0, 1.0, size=(n_rows, n_features))).astype(np.float32)
    rule = np.random.RandomState(7).normal(size=(n_classes, n_features))
    return x, ((x - 3.0) @ rule.T).argmax(1)


def main(n_particles=5, iterations=400, lr=0.02, n_train=90, n_test=60, n_features=4, n_classes=3):
    x, y = labelled_rows(n_train + n_test, n_features, n_classes, seed=1)
    model = W.build_map_logistic_regression(W.native_api(), dataset_size=n_train, n_features=n_features, n_classes=n_classes,
                                            data=(x[:n_train], y[:n_train]))
    rng = np.random.RandomState(0)
    particles = [ProbabilisticModel([RootVariable(0.1 * rng.normal(size=(n_classes, n_features)), "weights", learnable=True)])
                 for _ in range(n_particles)]
    method = inference.SteinVariationalGradientDescent(batched=True)
    inference.perform_inference(model, number_iterations=iterations, optimizer="Adam", lr=lr, inference_method=method, posterior_model=particles)

    labels = torch.tensor(y[n_train:])
    predicted = method.predict(model, particles, x[n_train:])       # "probs" [particles][rows][classes], "mean" [rows][classes]
    ensemble = (predicted["mean"].argmax(1).cpu() == labels).float().mean()
    each = (predicted["probs"].argmax(2).cpu() == labels).float().mean(1)
    curve = model.diagnostics["loss curve"]
    print("loss (sum over %d particles): %.1f -> %.1f, last bandwidth %.3f" % (n_particles, curve[0], curve[-1], method.bandwidth))
    print("held-out accuracy of the ensemble (mean softmax of the particles): %.3f; of the particles alone: %.3f .. %.3f" % (
        ensemble, each.min(), each.max()))


if __name__ == "__main__":
    main()
