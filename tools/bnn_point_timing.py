"""What point-estimated tensors cost, and save, per fused step (CompiledBnn.train -> bsvi_bnn_step) at the 784-20-10 classifier of BASELINE
config 4's scale (minibatch 512, 1 024 samples, Adam) -> profiles/r24/bnn_point.txt.
    normal      every tensor under its mean-field Normal: built without the builder's keyword, it launches the kernels of every model
                before the feature (the line that also runs on a build without the feature: --only normal)
    trunk       point=("weights1", "b1"): the shared first layer — one first product broadcast to the samples, one second product behind
                the sum over the samples
    trunk_off   the same model under BSVI_BNN_SHARED1=0: both products per sample, the POINT instantiations of bnn_draw / bnn_row_sums
    map         point="all" at ONE sample: what `inference.MAP` runs
Device events around K steps after warm-up and 300 ms of untimed steps (an idle MI355X takes that long to ramp); six timed regions per
line, the models alternating inside every round and each measured twice, so that drift and a line's own spread show: median (min .. max)
us per step.
    python tools/bnn_point_timing.py [file to write the lines to]
    python tools/bnn_point_timing.py --only normal [file]
    python tools/bnn_point_timing.py --steps normal|trunk|trunk_off|map K      (one model, K steps after warm-up: the run to put under
                                                                                `rocprofv3 --kernel-trace --stats -- python ...`)"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from brancher_amd import bnn, workloads as W

B, DS, K = 512, 4096, 50
MODELS = dict(normal=({}, 1024, None), trunk=(dict(point=("weights1", "b1")), 1024, "shared"),
              trunk_off=(dict(point=("weights1", "b1")), 1024, "per_sample"), map=(dict(point="all"), 1, "shared"))


def compiled(model):
    kw, n, first = MODELS[model]
    m = W.build_bayesian_neural_network(W.native_api(), dataset_size=DS, batch_size=B, n_features=784, n_hidden=20, n_classes=10, **kw)
    before = os.environ.pop("BSVI_BNN_SHARED1", None)
    if model == "trunk_off":
        os.environ["BSVI_BNN_SHARED1"] = "0"
    try:
        c = bnn.CompiledBnn(m, m.posterior_model, "pathwise")
        if first is not None:                     # (the switch is read once per handle, at this question)
            assert c.first_layer_path() == first, c.first_layer_path()
    finally:
        os.environ.pop("BSVI_BNN_SHARED1", None)
        if before is not None:
            os.environ["BSVI_BNN_SHARED1"] = before
    return c, n


def timed(c, n, reps=6, spin_ms=300.0):
    train = lambda k: c.train(k, n, "Adam", seed=0, lr=1e-3)
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
            c, n = compiled(model)
            us = timed(c, n)
            line = "784-20-10  B %4d N %5d  %-9s %-8s %s  median %8.1f us/step  (min %8.1f .. max %8.1f)  six: %s" % (
                B, n, model, c.middle_path(), c.data_path(), float(np.median(us)), min(us), max(us), " ".join("%.1f" % u for u in us))
            print(line, flush=True); rows.append(line)
    if out_path:
        open(out_path, "w").write("\n".join(rows) + "\n")


if __name__ == "__main__":
    args = sys.argv[1:]
    if args[:1] == ["--steps"]:
        c, n = compiled(args[1])
        c.train(20, n, "Adam", seed=0, lr=1e-3); torch.cuda.synchronize()
        c.train(int(args[2]), n, "Adam", seed=0, lr=1e-3); torch.cuda.synchronize()
    elif args[:1] == ["--only"]:
        main([args[1]], args[2] if len(args) > 2 else None)
    else:
        main(["normal", "trunk", "trunk_off", "map"], args[0] if args else None)
