"""The predictive of a particle ensemble of a Bayesian neural network (`CompiledBnn.predict_particles`; csrc/bnn_ensemble.inc) against
what a user would otherwise write, in ONE job on the GPU machine -> profiles/r30/bnn_particles_predict.txt.
  64 particles of 784-20-10 on 10 000 rows and on one row, 16 particles of 64-8-1 on 48 rows — the fused kernel against a torch f32
  loop on the device over the same table (`bmm` + activation + `softmax`, then the mean), and for the first size `CompiledBnn.predict`
  with 64 sampled weight sets, the nearest existing kernel path (it draws its sets from a posterior: other weights, the same work).
Warm-up, 300 ms of untimed repeats (an idle MI355X takes that long to ramp), then six timed regions of K calls each, a host clock around
work that ends in a device synchronise: median (min .. max) per call; the lines alternate inside every region, so drift shows in all.
Usage:  python tools/bnn_particles_predict_timing.py [file to write the lines to]     (default: bench_outputs/bnn_particles_predict_timing.txt)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((64, (784, 20, 10), 10000, 10, True), (64, (784, 20, 10), 1, 200, False), (16, (64, 8, 1), 48, 200, False))   # N, widths, M, calls, sampled line
DEFAULT_OUT = os.path.join(ROOT, "bench_outputs", "bnn_particles_predict_timing.txt")


def main(out_path):
    import numpy as np
    import torch
    from dense_predict_timing import timed
    from brancher_amd import bnn, workloads as W
    lines = []
    for n, widths, m, k, sampled in SHAPES:
        build = W.build_bnn_regression if widths[-1] == 1 else W.build_bayesian_neural_network
        model = build(W.native_api(), point="all", widths=list(widths), dataset_size=64, batch_size=32)
        c = bnn.CompiledBnn(model, model.posterior_model)
        p = c.program
        g = torch.Generator().manual_seed(0)
        table = torch.zeros(n, (p.n_rows + 3) // 4 * 4)
        table[:, :p.n_rows] = 0.05 * torch.randn(n, p.n_rows, generator=g)
        table, rows = table.to(c.device), torch.rand(m, widths[0], generator=g).to(c.device)
        t = {s["name"]: table[:, s["row0"]:s["row0"] + s["size"]].reshape(n, s["rows"], s["cols"]) for s in p.tensors}

        def torch_loop():
            h = rows.expand(n, -1, -1)
            for i, layer in enumerate(p.layers):
                h = torch.baddbmm(t[layer["bias"]].transpose(1, 2), h, t[layer["weights"]].transpose(1, 2))
                h = torch.tanh(h) if i + 1 < len(p.layers) else h
            return (torch.softmax(h, -1) if widths[-1] > 1 else h).mean(0)
        err = float((c.predict_particles(table, rows)["mean"] - torch_loop()).abs().max())
        lines.append("%d particles of %s on %d rows, the table read in place; |mean - torch loop| %.2e" % (n, "-".join(map(str, widths)), m, err))
        calls = dict(predict_particles=lambda: c.predict_particles(table, rows), torch_bmm_loop=torch_loop)
        if sampled:
            q = build(W.native_api(), widths=list(widths), dataset_size=64, batch_size=32)
            cq = bnn.CompiledBnn(q, q.posterior_model)
            calls["predict_64_sampled"] = lambda: cq.predict(rows, n, seed=1, offset=0)
        lines += timed(np, torch, calls, k)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)


if __name__ == "__main__":
    main(os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else DEFAULT_OUT)
