"""What latent prior scales cost per fused step (CompiledBnn.train -> bsvi_bnn_step) against the same 784-20-10 classifier with constant
prior scales, at BASELINE config 4's scale (minibatch 512, 1 024 samples), on the same build -> profiles/r21/bnn_scale_latents.txt.  The
constant model is built without the builder's keywords and launches bnn_draw<false> / bnn_row_sums<false>, the kernels of every model
before the feature; "laplace" (the precedent: profiles/r18/bnn_priors.txt) launches the MIXED instantiations; "layer" (one latent per
layer) and "global" (one for every tensor) launch the LATENT ones, bnn_latent_terms and bnn_latent_grads.  Device events around K steps
after warm-up and 300 ms of untimed steps (an idle MI355X takes that long to ramp); six timed regions per line, the models alternating
inside every round and each measured twice, so that drift and the constant line's own spread show: median (min .. max) us per step.
    python tools/bnn_hier_timing.py [file to write the lines to]
    python tools/bnn_hier_timing.py --only constant [file]       (the constant line alone: what also runs on a build without the feature)
    python tools/bnn_hier_timing.py --steps constant|laplace|layer|global K      (one model, K steps after warm-up: the run to put under
                                                                                 `rocprofv3 --kernel-trace --stats -- python ...`)"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from brancher_amd import bnn, workloads as W

B, N, DS, K = 512, 1024, 4096, 50
MODELS = dict(constant={}, laplace=dict(prior="laplace"), layer=dict(scale_latent="layer"), **{"global": dict(scale_latent="global")})


def compiled(model):
    m = W.build_bayesian_neural_network(W.native_api(), dataset_size=DS, batch_size=B, n_features=784, n_hidden=20, n_classes=10, **MODELS[model])
    c = bnn.CompiledBnn(m, m.posterior_model, "pathwise")
    assert len(c.program.summary().get("scale_latents", {})) == {"constant": 0, "laplace": 0, "layer": 2, "global": 1}[model]
    return c


def timed(c, reps=6, spin_ms=300.0):
    train = lambda k: c.train(k, N, "Adam", seed=0, lr=1e-3)
    train(20); torch.cuda.synchronize()
    t = time.perf_counter()
    while (time.perf_counter() - t) * 1e3 < spin_ms:
        train(K); torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); train(K); b.record(); b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / K)
    return out


def main(models, out_path):
    rows = []
    for rnd in range(2):
        for model in models:
            c = compiled(model)
            us = timed(c)
            line = "784-20-10  B %4d N %5d  scales %-8s %-8s %s  median %8.1f us/step  (min %8.1f .. max %8.1f)  six: %s" % (
                B, N, model, c.middle_path(), c.data_path(), float(np.median(us)), min(us), max(us), " ".join("%.1f" % u for u in us))
            print(line, flush=True); rows.append(line)
    if out_path:
        open(out_path, "w").write("\n".join(rows) + "\n")


if __name__ == "__main__":
    args = sys.argv[1:]
    if args[:1] == ["--steps"]:
        c = compiled(args[1])
        c.train(20, N, "Adam", seed=0, lr=1e-3); torch.cuda.synchronize()
        c.train(int(args[2]), N, "Adam", seed=0, lr=1e-3); torch.cuda.synchronize()
    elif args[:1] == ["--only"]:
        main([args[1]], args[2] if len(args) > 2 else None)
    else:
        main(["constant", "laplace", "layer", "global"], args[0] if args else None)
