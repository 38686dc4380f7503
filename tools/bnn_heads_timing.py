"""What a scale head costs per fused step (CompiledBnn.train -> bsvi_bnn_step) and per predict call, at BASELINE config 4's scale
(minibatch 512, 1 024 samples): the heads network 784-20-(10+10) against the constant-sigma Normal network 784-20-20 — the same
products, the same walk, the epilogue's transform and derivative per (sample, row, output) the difference -> profiles/r19/bnn_heads.txt.
One model per process (a new model, a new warm-up), so that a caller can alternate builds and models:
    python tools/bnn_heads_timing.py constant|heads [--tree DIR] [--outputs C]
(DIR: the checkout whose package is measured, default: this one — `constant` uses nothing the parent commit lacks; C: targets per row,
default 10: heads 784-20-(C+C) against constant 784-20-2C.  C = 1 is the size bnn_mid_gen serves; 20 rows in the last layer are beyond
its LDS tile and bnn_upper_gen's registers at this minibatch, so the static kernel in memory serves both models)
Device events around K steps after warm-up and 300 ms of untimed steps (an idle MI355X takes that long to ramp); six timed regions per
line: median (min .. max) us per step / per call.  The predict call: 512 rows, 1 024 samples, outputs and draws asked for."""
import os
import sys
import time

import numpy as np
import torch

ARGS = sys.argv[1:]
TREE = os.path.abspath(ARGS[ARGS.index("--tree") + 1]) if "--tree" in ARGS else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, TREE)
from brancher_amd import bnn, workloads as W  # noqa: E402

B, N, DS, K, M = 512, 1024, 4096, 50, 512
C_OUT = int(ARGS[ARGS.index("--outputs") + 1]) if "--outputs" in ARGS else 10


def compiled(kind):
    kw = dict(n_outputs=C_OUT, scale_head="softplus", scale_floor=0.05) if kind == "heads" else dict(n_outputs=2 * C_OUT, sigma=0.3)
    m = W.build_bnn_regression(W.native_api(), dataset_size=DS, batch_size=B, n_features=784, n_hidden=20, **kw)
    c = bnn.CompiledBnn(m, m.posterior_model, "pathwise")
    assert c.program.layers[-1]["rows"] == 2 * C_OUT and c.program.summary()["scale"] == ("head" if kind == "heads" else "constant")
    return c


def regions(run, reps=6, spin_ms=300.0):
    run(); torch.cuda.synchronize()
    t = time.perf_counter()
    while (time.perf_counter() - t) * 1e3 < spin_ms:
        run(); torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); count = run(); b.record(); b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / count)
    return out


def line(what, kind, c, us):
    return "%-8s %-8s 784-20-%-3d %-10s %s %s  median %8.1f us  (min %8.1f .. max %8.1f)  six: %s" % (
        what, kind, 2 * C_OUT, os.path.basename(TREE), c.middle_path(), c.data_path(), float(np.median(us)), min(us), max(us), " ".join("%.1f" % u for u in us))


if __name__ == "__main__":
    kind = ARGS[0]
    c = compiled(kind)

    def steps():
        c.train(K, N, "Adam", seed=0, lr=1e-3)
        return K

    print(line("step", kind, c, regions(steps)), flush=True)
    rows = torch.from_numpy(c.program.dataset[:M]).to(c.device)

    def calls():
        for i in range(10):
            c.predict(rows, N, seed=1, offset=i, want_outputs=True, want_draws=True)
        return 10

    print(line("predict", kind, c, regions(calls)), flush=True)
