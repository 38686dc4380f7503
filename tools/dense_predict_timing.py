"""Posterior predictive of the dense-link path (`CompiledDense.predict`, `SteinVariationalGradientDescent.predict`; csrc/dense_predict.inc)
against what a user would otherwise write, in ONE job on the GPU machine -> profiles/r29/dense_predict.txt.
  (a) a 10 x 784 logistic regression, sampled weight sets: (N 10, M 1), the reference scripts' call, and (N 64, M 10 000), a whole test
      set — `predict` against torch.softmax(torch.einsum(...)) in f32 on the same drawn weights, and against the detour this model takes
      today (`engine._bnn_predictor`: a second lowering as a one-layer network, the parameters copied through the host, bsvi_bnn_predict)
  (b) 64 particles of 10 x 784 on 10 000 rows through `SteinVariationalGradientDescent.predict`, against the loop of the reference's
      playground written in torch: particle by particle, softmax of one matrix product, summed.
Warm-up, 300 ms of untimed repeats (an idle MI355X takes that long to ramp), then six timed regions of K calls each, a host clock around
work that ends in a device synchronise: median (min .. max) per call; the lines alternate inside every region, so drift shows in all.
Usage:  python tools/dense_predict_timing.py [file to write the lines to]          (default: bench_outputs/dense_predict_timing.txt)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = ((10, 1, 200), (64, 10000, 10))           # (N, M, calls per timed region)
DEFAULT_OUT = os.path.join(ROOT, "bench_outputs", "dense_predict_timing.txt")


def timed(np, torch, calls, k):
    for f in calls.values():
        for _ in range(5):
            f()
    torch.cuda.synchronize()
    t = time.perf_counter()
    while (time.perf_counter() - t) * 1e3 < 300.0:
        for f in calls.values():
            f()
        torch.cuda.synchronize()
    us = {name: [] for name in calls}
    for _ in range(6):
        for name, f in calls.items():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(k):
                f()
            torch.cuda.synchronize()
            us[name].append((time.perf_counter() - t0) * 1e6 / k)
    lines = ["    %-22s median %9.1f us/call  (min %9.1f .. max %9.1f)  six regions of %d calls" % (name, float(np.median(v)), min(v), max(v), k)
             for name, v in us.items()]
    first = float(np.median(us[next(iter(us))]))
    lines.append("    " + "    ".join("%s / %s %.2f" % (next(iter(us)), name, first / float(np.median(v))) for name, v in list(us.items())[1:]))
    return lines


def main(out_path):
    import numpy as np
    import torch
    from brancher_amd import dense, engine, inference, workloads as W
    from brancher_amd.variables import ProbabilisticModel, RootVariable
    lines = []
    api = W.native_api()
    model = W.build_logistic_regression(api, dataset_size=512, batch_size=32)
    c = engine.compile_model(model, model.posterior_model, None)
    assert isinstance(c, dense.CompiledDense) and (c.program.n_classes, c.program.n_features) == (10, 784)
    loc, scale = (torch.from_numpy(a.astype(np.float32)).to(c.device) for a in dense.row_parameters(c.program, c.params.cpu().numpy()))
    for n, m, k in SHAPES:
        rows = torch.from_numpy(np.random.RandomState(0).uniform(0, 1, size=(m, 784)).astype(np.float32)).to(c.device)
        first = c.predict(rows, n, seed=1, offset=0, want_noise=True)
        w = (loc[:, None] + scale[:, None] * first["noise"]).t().reshape(n, 10, 784).contiguous()
        torch_line = lambda: torch.softmax(torch.einsum("ncp,mp->nmc", w, rows), -1).mean(0)
        detour = lambda: engine._bnn_predictor(model, c).predict(rows, n, seed=1, offset=0)
        err = float((first["mean"] - torch_line()).abs().max())
        lines.append("(a) N %3d M %5d  sampled sets of 10 x 784; |mean - torch on the same weights| %.2e" % (n, m, err))
        lines += timed(np, torch, dict(predict=lambda: c.predict(rows, n, seed=1, offset=0), torch_same_weights=torch_line, bnn_detour=detour), k)
    # (b) the ensemble of 64 particles
    n, m, k = 64, 10000, 10
    pmodel = W.build_map_logistic_regression(api, dataset_size=64, n_features=784, n_classes=10)
    rng = np.random.RandomState(0)
    parts = [ProbabilisticModel([RootVariable(0.05 * rng.normal(size=(10, 784)), "weights", learnable=True)]) for _ in range(n)]
    method = inference.SteinVariationalGradientDescent(batched=True)
    inference.perform_inference(pmodel, number_iterations=2, optimizer="SGD", lr=0.001, inference_method=method, posterior_model=parts)
    rows = torch.from_numpy(rng.uniform(0, 1, size=(m, 784)).astype(np.float32)).to(method.last_compiled.device)
    theta = method._plan["theta"][:, :7840].reshape(n, 10, 784)

    def playground():      # particle by particle, as development_playgrounds/SVGD_logistic_regression.py sums its answers
        total = torch.zeros(m, 10, device=rows.device)
        for i in range(n):
            total += torch.softmax(rows @ theta[i].t(), -1)
        return total / n
    err = float((method.predict(pmodel, parts, rows)["mean"] - playground()).abs().max())
    lines.append("(b) %d particles of 10 x 784 on %d rows, the plan's table read in place; |mean - torch loop| %.2e" % (n, m, err))
    lines += timed(np, torch, dict(svgd_predict=lambda: method.predict(pmodel, parts, rows), torch_particle_loop=playground), k)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)


if __name__ == "__main__":
    main(os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else DEFAULT_OUT)
