"""batched=True against batched=False on a logistic regression: us per iteration, and the evaluation call's share (device events)."""
import time

import numpy as np
import torch

from brancher_amd import dense, inference, native, workloads as W
from brancher_amd.variables import ProbabilisticModel, RootVariable


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)


def setup(n, c, p, rows, batched):
    model = W.build_map_logistic_regression(W.native_api(), dataset_size=rows, n_features=p, n_classes=c)
    rng = np.random.RandomState(0)
    parts = [ProbabilisticModel([RootVariable(0.01 * rng.normal(size=(c, p)), "weights", learnable=True)]) for _ in range(n)]
    return model, parts, inference.SteinVariationalGradientDescent(batched=batched)


def run(state, iters):
    model, parts, method = state
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    inference.perform_inference(model, number_iterations=iters, optimizer="SGD", lr=1e-5, inference_method=method, posterior_model=parts)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6, np.asarray(model.diagnostics["loss curve"])[:2]


for n, c, p, rows, iters in ((64, 10, 784, 512, 300), (5, 3, 4, 5, 1000)):      # windows of 0.2 s and more
    say("shape: %d particles, %d x %d, %d rows" % (n, c, p, rows))
    states = {b: setup(n, c, p, rows, b) for b in (True, False)}
    for b in (True, False):
        t0 = time.perf_counter()
        _, curve = run(states[b], 2)
        say("batched=%s: first two iterations, compilation included, %.2f s; loss %s" % (b, time.perf_counter() - t0, curve))
    times = {True: [], False: []}
    for _ in range(6):
        for b in (True, False):
            times[b].append(run(states[b], iters)[0])
    for b in (True, False):
        say("batched=%s: median %.1f us per iteration (min %.1f, max %.1f; 6 x %d iterations, perform_inference end to end)" % (
            b, np.median(times[b]), min(times[b]), max(times[b]), iters))
    say("ratio of medians: %.2f" % (np.median(times[False]) / np.median(times[True])))
    # the evaluation call alone (head + fused kernel [+ join]): device events around 200 calls on the batched plan's own tables
    plan = states[True][2]._plan
    compiled = plan["compiled"]
    ws = plan["workspace"]
    for _ in range(10):
        native.dense_particles_fwd_bwd(compiled.handle, compiled.params, compiled.out, plan["theta"], plan["grad"], plan["loss"], seed=1, workspace=ws)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(200):
        native.dense_particles_fwd_bwd(compiled.handle, compiled.params, compiled.out, plan["theta"], plan["grad"], plan["loss"], seed=1, workspace=ws)
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1000 / 200
    say("bsvi_dense_particles_fwd_bwd alone: %.1f us per call (device events, 200 calls back to back) = %.1f %% of the batched iteration" % (
        us, 100 * us / np.median(times[True])))
