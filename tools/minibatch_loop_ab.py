"""Minibatched observations inside the in-kernel training loop against the launch-by-launch path (A/B, one process).

Times `train(2000, n, "SGD", lr=1e-3)` of the minibatched linear regression (workloads.build_minibatch_linear_regression:
40 rows, batches of 8, 3 features) at n = 64 and n = 300 samples, with and without `minibatch_loop`, alternating, six runs a
side, each side on its own compiled model, after an untimed spin-up of the same calls (300 ms, as bench.py's
`untimed_spinup_iterations`: an idle MI355X takes that long to ramp).  A run is a host clock around the call and a device
synchronise.  The launch-by-launch side is what the parent commit does for this model.

A third model runs the same in-kernel loop with the gather phase compiled out (BSVI_SPEC_DEFINES: SPEC_DEBUG_NO_GATHER — the
observation table keeps the rows it was uploaded with): the difference is what the phase costs per iteration.

usage: python3 tools/minibatch_loop_ab.py [iterations] [runs a side]"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                        # noqa: E402
from brancher_amd import engine, native, workloads as W     # noqa: E402

K = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
RUNS = int(sys.argv[2]) if len(sys.argv) > 2 else 6
SPINUP_S = 0.3
assert torch.cuda.is_available(), "this measurement needs an MI355X"


def model():
    return engine.compile_model(W.build_minibatch_linear_regression(W.native_api()), None, "pathwise")


def call(c, n, **kw):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    c.train(K, n, "SGD", seed=0, lr=1e-3, **kw)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / K


for n in (64, 300):
    # the loop without the gather phase FIRST: a tuned compilation is not kept in the process's code cache, an untuned one is
    os.environ["BSVI_SPEC_DEFINES"] = "#define SPEC_DEBUG_NO_GATHER 1"
    bare = model()
    call(bare, n, minibatch_loop=True)
    del os.environ["BSVI_SPEC_DEFINES"]
    assert bare.last_mode == "persistent"
    loop, step = model(), model()
    sides = [("in-kernel", loop, dict(minibatch_loop=True)), ("launch by launch", step, {}), ("in-kernel, gather compiled out", bare, dict(minibatch_loop=True))]
    t_spin, spun = time.perf_counter(), 0
    while time.perf_counter() - t_spin < SPINUP_S or spun < 2:
        for _, c, kw in sides:
            call(c, n, **kw)
        spun += 1
    assert loop.last_mode == "persistent" and step.last_mode == "stepwise" and bare.last_mode == "persistent"
    variant = None
    times = {name: [] for name, _, _ in sides}
    for _ in range(RUNS):
        for name, c, kw in sides:
            times[name].append(call(c, n, **kw))
            if name == "in-kernel":
                variant = native.load().bsvi_spec_last_variant()
    geo = loop.native.engine(n, 2)
    print("n = %d samples, %d iterations per call, %d runs a side after %d untimed rounds; loop kernel variant %s, %d workgroup(s) of %d threads"
          % (n, K, RUNS, spun, variant, geo.get("n_blocks", 0), geo.get("n_threads", 0)))
    for name, _, _ in sides:
        t = times[name]
        print("  %-32s us/iteration: median %8.3f  min %8.3f  max %8.3f   runs %s"
              % (name, statistics.median(t), min(t), max(t), " ".join("%.3f" % x for x in t)))
    a, b, g = times["in-kernel"], times["launch by launch"], times["in-kernel, gather compiled out"]
    print("  launch by launch / in-kernel: %.2f x (medians); every in-kernel run faster than every launch-by-launch run: %s"
          % (statistics.median(b) / statistics.median(a), max(a) < min(b)))
    print("  the gather phase: %+.3f us/iteration (medians; the loop without it spreads %.3f us over its runs)"
          % (statistics.median(a) - statistics.median(g), max(g) - min(g)))
