"""Bayesian logistic regression on minibatches with the local reparameterisation estimator (Kingma, Salimans and Welling, 2015).

The model of the reference's `examples/minibatch_logistic_regression.py`: two Gaussian clouds, a Normal posterior over the weights of the
linear link.  Under `LocalReparameterizationEstimator` the logits of a minibatch row are sampled directly from their Normal instead of a
weight matrix per Monte-Carlo sample (csrc/dense_local.inc): the same ELBO, a lower-variance gradient, a closed-form KL term.

    python examples/local_reparameterization.py [--estimator local|pathwise]
"""
import argparse

import numpy as np

from brancher_amd import engine, inference, workloads as W
from brancher_amd.gradient_estimators import LocalReparameterizationEstimator, PathwiseDerivativeEstimator


def main(estimator="local", iterations=400, number_samples=16, lr=0.05):
    cls = dict(local=LocalReparameterizationEstimator, pathwise=PathwiseDerivativeEstimator)[estimator]
    model = W.build_binary_logistic_regression(W.native_api(), dataset_size=200, batch_size=50, n_features=6)
    inference.perform_inference(model, number_iterations=iterations, number_samples=number_samples, optimizer="Adam", lr=lr,
                                inference_method=inference.ReverseKL(gradient_estimator=cls))
    compiled = engine.compile_model(model, None, cls)
    w = compiled.named_params()["weights_loc"].reshape(-1)
    curve = model.diagnostics["loss curve"]
    print("%s estimator (%s): loss %.1f -> %.1f (means of the first and last 20 iterations)" % (
        estimator, type(compiled).__name__, np.mean(curve[:20]), np.mean(curve[-20:])))
    print("posterior mean of the weights:", np.round(w, 3))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--estimator", choices=("local", "pathwise"), default="local")
    main(ap.parse_args().estimator)
