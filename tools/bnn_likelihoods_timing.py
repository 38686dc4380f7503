"""What the Laplace and Cauchy regression likelihoods cost per fused step (CompiledBnn.train -> bsvi_bnn_step) and per predict call, at
BASELINE config 4's scale (minibatch 512, 1 024 samples): 784-20-C under an observed Normal, Laplace or Cauchy with a learnable scale
per output — the same products, the same walk, the epilogue's value and score per (sample, row, output) the difference
-> profiles/r20/bnn_likelihoods.txt.  One model per process (a new model, a new warm-up), so that a caller can alternate builds and
families:
    python tools/bnn_likelihoods_timing.py normal|laplace|cauchy [--tree DIR] [--outputs C] [--predict]
(DIR: the checkout whose package is measured, default: this one — `normal` uses nothing the parent commit lacks; C: outputs, default 1:
the size bnn_mid_gen serves; 10: beyond its LDS tile and bnn_upper_gen's registers at this minibatch, the static kernel in memory.
BSVI_BNN_CAUCHY_LOG=log1p in the environment: the generated kernels take log1pf(u^2) in the place of the hardware logarithm.)
Device events around K steps after warm-up and 300 ms of untimed steps (an idle MI355X takes that long to ramp); six timed regions per
line: median (min .. max) us per step / per call.  --predict: the predict call as well, 512 rows, 1 024 samples, draws asked for (and
the variance, where the family has one)."""
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
C_OUT = int(ARGS[ARGS.index("--outputs") + 1]) if "--outputs" in ARGS else 1


def compiled(family):
    kw = dict(likelihood=family) if family != "normal" else {}          # (the parent commit's builder has no such keyword)
    sigma = 0.3 if C_OUT == 1 else list(np.linspace(0.3, 0.8, C_OUT))
    m = W.build_bnn_regression(W.native_api(), dataset_size=DS, batch_size=B, n_features=784, n_hidden=20, n_outputs=C_OUT, sigma=sigma,
                               learnable_sigma=True, **kw)
    c = bnn.CompiledBnn(m, m.posterior_model, "pathwise")
    assert c.program.scale_learnable and c.program.summary().get("family", "normal") == family
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


def line(what, family, c, us):
    return "%-8s %-8s 784-20-%-3d %-10s %s %s %s  median %8.1f us  (min %8.1f .. max %8.1f)  six: %s" % (
        what, family, C_OUT, os.path.basename(TREE), c.middle_path(), c.data_path(), os.environ.get("BSVI_BNN_CAUCHY_LOG", ""),
        float(np.median(us)), min(us), max(us), " ".join("%.1f" % u for u in us))


if __name__ == "__main__":
    family = ARGS[0]
    c = compiled(family)

    def steps():
        c.train(K, N, "Adam", seed=0, lr=1e-3)
        return K

    print(line("step", family, c, regions(steps)), flush=True)
    if "--predict" in ARGS:
        rows = torch.from_numpy(c.program.dataset[:M]).to(c.device)

        def calls():
            for i in range(10):
                c.predict(rows, N, seed=1, offset=i, want_draws=True)
            return 10

        print(line("predict", family, c, regions(calls)), flush=True)
