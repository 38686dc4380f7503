"""The local reparameterisation estimator of the dense-link path (`LocalReparameterizationEstimator`, csrc/dense_local.inc) against the
Pathwise estimator of the same model, in ONE job on the GPU machine -> profiles/r31/dense_local.txt.
  BASELINE config 4: a 10 x 784 logistic regression, minibatch 512 of 60 000 rows of uint8-valued pixels, Adam lr 5e-3, at
  number_samples 64, 1 024 (the config's own) and 4 096.  Timed is `CompiledDense.train(K, N, "Adam")`, the loop `perform_inference` runs:
  per iteration one bsvi_dense_local_fwd_bwd and one bsvi_optimizer_step | one bsvi_dense_step.
Warm-up, 300 ms of untimed repeats (an idle MI355X takes that long to ramp), then six timed regions of K iterations each, a host clock
around work that ends in a device synchronise: median (min .. max) per iteration; the two estimators alternate inside every region, so
drift shows in both.  The last line of a size is the loss of both after the timed iterations (the same ELBO, other draws).
Usage:  python tools/dense_local_timing.py [file to write the lines to] [--quick]     (default: bench_outputs/dense_local_timing.txt;
--quick: a dataset of 2 048 rows and two regions, to rehearse the job)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SAMPLES = ((64, 200), (1024, 200), (4096, 100))           # (number_samples, iterations per timed region)
DEFAULT_OUT = os.path.join(ROOT, "bench_outputs", "dense_local_timing.txt")


def timed(np, torch, calls, k, regions):
    for f in calls.values():
        f(5)
    torch.cuda.synchronize()
    t = time.perf_counter()
    while (time.perf_counter() - t) * 1e3 < 300.0:
        for f in calls.values():
            f(20)
        torch.cuda.synchronize()
    us = {name: [] for name in calls}
    for _ in range(regions):
        for name, f in calls.items():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            f(k)
            torch.cuda.synchronize()
            us[name].append((time.perf_counter() - t0) * 1e6 / k)
    lines = ["    %-10s median %8.1f us/iteration  (min %8.1f .. max %8.1f)  %d regions of %d iterations" % (name, float(np.median(v)), min(v), max(v), regions, k)
             for name, v in us.items()]
    first, second = (float(np.median(v)) for v in us.values())
    lines.append("    pathwise / local %.2f" % (second / first))
    return lines


def main(out_path, quick):
    import numpy as np
    import torch
    from brancher_amd import dense, engine, workloads as W
    from brancher_amd.gradient_estimators import LocalReparameterizationEstimator, PathwiseDerivativeEstimator
    lines = ["device: %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__)]
    api = W.native_api()
    shape = dict(dataset_size=2048 if quick else 60000, batch_size=512, n_features=784, n_classes=10, pixels="uint8")
    for n, k in SAMPLES:
        engines = {}
        for name, est in (("local", LocalReparameterizationEstimator), ("pathwise", PathwiseDerivativeEstimator)):
            model = W.build_logistic_regression(api, **shape)
            engines[name] = engine.compile_model(model, model.posterior_model, est)
            assert isinstance(engines[name], dense.CompiledDense)
        calls = {name: (lambda K, c=c: c.train(K, n, "Adam", lr=5e-3)) for name, c in engines.items()}
        lines.append("10 x 784, minibatch 512, number_samples %d, Adam (pathwise data path: %s)" % (n, engines["pathwise"].data_path()))
        lines += timed(np, torch, calls, k if not quick else 20, 2 if quick else 6)
        lines.append("    loss after the timed iterations: " + ", ".join(
            "%s %.1f" % (name, float(c.evaluate(n, seed=3, offset=1 << 40)["loss"])) for name, c in engines.items()))
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)


if __name__ == "__main__":
    argv = [a for a in sys.argv[1:] if a != "--quick"]
    main(os.path.abspath(argv[0]) if argv else DEFAULT_OUT, "--quick" in sys.argv)
