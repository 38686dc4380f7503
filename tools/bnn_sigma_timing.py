"""What a learnable sigma costs per fused step (CompiledBnn.train -> bsvi_bnn_step) against the same 784-20-1 regression network with a
constant sigma, on the same build -> profiles/r16/bnn_sigma.txt.  Two sizes: the example's (minibatch 30, 50 samples) and BASELINE config
4's scale (minibatch 512, 1 024 samples).  Device events around K steps after warm-up and 300 ms of untimed steps (an idle MI355X takes
that long to ramp); six timed regions per line, the two models alternating inside every round and each pair measured twice, so that
drift and the constant line's own spread show: median (min .. max) us per step.
    python tools/bnn_sigma_timing.py [file to write the lines to]
    python tools/bnn_sigma_timing.py --steps learnable|constant example|cfg4 K      (one model, K steps after warm-up: the run to put
                                                                                     under `rocprofv3 --kernel-trace --stats -- python ...`)"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from brancher_amd import bnn, workloads as W

SIZES = dict(cfg4=("config 4 scale", 512, 1024, 4096, 50), example=("example size", 30, 50, 512, 200))      # label, B, N, DS, steps per region


def compiled(kind, size):
    _, B, N, DS, _ = SIZES[size]
    kw = dict(learnable_sigma=True, sigma_init=0.5) if kind == "learnable" else {}
    m = W.build_bnn_regression(W.native_api(), dataset_size=DS, batch_size=B, n_features=784, n_hidden=20, n_outputs=1, sigma=0.3, **kw)
    c = bnn.CompiledBnn(m, m.posterior_model, "pathwise")
    assert c.program.scale_learnable == (kind == "learnable")
    return c, N


def timed(c, n, K, reps=6, spin_ms=300.0):
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


def main(out_path):
    rows = []
    for size, (label, B, N, DS, K) in SIZES.items():
        for rnd in range(2):
            for kind in ("constant", "learnable"):
                c, n = compiled(kind, size)
                us = timed(c, n, K)
                line = "%-15s B %4d N %5d  sigma %-9s %-8s %s  median %8.1f us/step  (min %8.1f .. max %8.1f)  six: %s" % (
                    label, B, N, kind, c.middle_path(), c.data_path(), float(np.median(us)), min(us), max(us), " ".join("%.1f" % u for u in us))
                print(line, flush=True); rows.append(line)
    if out_path:
        open(out_path, "w").write("\n".join(rows) + "\n")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--steps":
        c, n = compiled(sys.argv[2], sys.argv[3])
        c.train(20, n, "Adam", seed=0, lr=1e-3); torch.cuda.synchronize()
        c.train(int(sys.argv[4]), n, "Adam", seed=0, lr=1e-3); torch.cuda.synchronize()
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else None)
