"""The Normal likelihood of the Bayesian-neural-network family against the Bernoulli one -> profiles/r13/bnn_normal.txt:
us per fused step (CompiledBnn.train -> bsvi_bnn_step) of the 784-20-1 regression network and the Bernoulli network of the same
shape: warm-up, 300 ms spin-up on the timed path, then six timed regions of K steps; median (min .. max).
Usage:  python tools/bnn_normal_timing.py [file to write the lines to]"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from brancher_amd import engine, workloads as W

def timed(model, n, K=50, W_=20, spin_ms=300.0, reps=6):
    c = engine.compile_model(model, None, "pathwise")
    assert type(c).__name__ == "CompiledBnn"
    train = lambda k: c.train(k, n, "Adam", seed=0, lr=1e-3)
    train(W_); torch.cuda.synchronize()
    t = time.perf_counter()
    while (time.perf_counter() - t) * 1e3 < spin_ms:
        train(200); torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter(); train(K); torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e6 / K)
    return c.data_path(), out

api = W.native_api()
rows = []
for label, B, N, DS in (("config 4 scale", 512, 1024, 4096), ("example size", 30, 50, 512)):
    for rnd in range(2):          # (each pair twice, alternating, so that drift shows)
        for kind in ("normal", "bernoulli"):
            if kind == "normal":
                m = W.build_bnn_regression(api, dataset_size=DS, batch_size=B, n_features=784, n_hidden=20, n_outputs=1)
            else:
                m = W.build_bayesian_neural_network(api, dataset_size=DS, batch_size=B, n_features=784, n_hidden=20, n_classes=1, q_scale1=4e-4, q_loc_scale=1.0)
            path, us = timed(m, N)
            line = "%-15s B %4d N %5d  %-9s %s  median %8.1f us/step  (min %8.1f .. max %8.1f)  six: %s" % (
                label, B, N, kind, path, float(np.median(us)), min(us), max(us), " ".join("%.1f" % u for u in us))
            print(line, flush=True); rows.append(line)
if len(sys.argv) > 1:
    open(sys.argv[1], "w").write("\n".join(rows) + "\n")
