"""What the activation between the layers costs per fused step (CompiledBnn.train -> bsvi_bnn_step) at the 784-20-10 classifier of BASELINE
config 4's scale (minibatch 512, 1 024 samples, Adam) -> profiles/r25/bnn_activations.txt: tanh (the kernel text of every commit before
the new kinds: the line that also runs on such a tree, --tree DIR --only tanh) beside leaky_relu, elu, silu and gelu.
Device events around K steps after warm-up and 300 ms of untimed steps (an idle MI355X takes that long to ramp); six timed regions per
line, the models alternating inside every round and each measured `rounds` times, so that drift and a line's own spread show: median
(min .. max) us per step.
    python tools/bnn_activations_timing.py [file to write the lines to]
    python tools/bnn_activations_timing.py --tree DIR --only tanh --rounds 3 [file]      (DIR: the checkout whose package and library run)"""
import os
import sys
import time

import numpy as np
import torch

B, DS, K, N = 512, 4096, 50, 1024
MODELS = ["tanh", "leaky_relu", "elu", "silu", "gelu"]


def compiled(model):
    from brancher_amd import bnn, workloads as W
    m = W.build_bayesian_neural_network(W.native_api(), dataset_size=DS, batch_size=B, n_features=784, n_hidden=20, n_classes=10, activation=model)
    return bnn.CompiledBnn(m, m.posterior_model, "pathwise")


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


def main(models, rounds, out_path):
    rows = []
    for rnd in range(rounds):
        for model in models:
            c = compiled(model)
            us = timed(c)
            line = "784-20-10  B %4d N %5d  %-10s %-8s %s  median %8.1f us/step  (min %8.1f .. max %8.1f)  six: %s" % (
                B, N, model, c.middle_path(), c.data_path(), float(np.median(us)), min(us), max(us), " ".join("%.1f" % u for u in us))
            print(line, flush=True); rows.append(line)
    if out_path:
        open(out_path, "w").write("\n".join(rows) + "\n")


if __name__ == "__main__":
    args = sys.argv[1:]
    tree = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    models, rounds = MODELS, 2
    for flag in ("--tree", "--only", "--rounds"):
        if flag in args:
            value = args[args.index(flag) + 1]
            del args[args.index(flag):args.index(flag) + 2]
            tree, models, rounds = (os.path.abspath(value) if flag == "--tree" else tree, [value] if flag == "--only" else models,
                                    int(value) if flag == "--rounds" else rounds)
    sys.path.insert(0, tree)
    main(models, rounds, args[0] if args else None)
