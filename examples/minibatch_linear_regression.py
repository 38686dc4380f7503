"""Minibatched Bayesian linear regression: the Normal-likelihood neighbour of the reference's `minibatch_*` examples.

`x` and the targets are two EmpiricalVariables that share a RandomIndices variable, so every iteration sees another
minibatch of the dataset.  The model is far too small for the dense (matrix-core) path: it runs on the scalar engine, and
`perform_inference` keeps the whole optimisation in ONE kernel launch — the generated kernel draws and gathers each
iteration's rows itself (`BSVI_MINIBATCH_LOOP=0` trains launch by launch instead: one gather launch per source and one step
launch per iteration).  Run on a machine with an MI355X:

    python examples/minibatch_linear_regression.py
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from brancher_amd import inference, workloads as W

model = W.build_minibatch_linear_regression(W.native_api(), dataset_size=40, batch_size=8, n_features=3)
method = inference.ReverseKL()
for attempt in ("first call (lowering, program upload, kernel compilation or code-object cache)", "second call"):
    t0 = time.time()
    inference.perform_inference(model, inference_method=method, number_iterations=2000, number_samples=64,
                                optimizer="Adam", lr=0.01)
    seconds = time.time() - t0
    loss = np.asarray(model.diagnostics["loss curve"])
    print("%s: 2000 iterations in %.3f s, mode %s; loss %.2f -> %.2f"
          % (attempt, seconds, method.last_compiled.last_mode, loss[:20].mean(), loss[-20:].mean()))
