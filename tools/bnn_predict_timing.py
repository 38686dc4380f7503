"""Posterior predictive of the 784-20-10 Bayesian neural network (`CompiledBnn.predict`, bsvi_bnn_predict) against what a user would
otherwise write — the same draws pushed through torch.bmm + tanh + softmax in f32 on the same device — in ONE job on the GPU machine
-> profiles/r15/bnn_predict.txt.  Two shapes: (N 10, M 1), the reference script's call, and (N 64, M 10 000), a whole test set.

Without arguments this is the driver: every step is a fresh child process under a time limit of its own, and the first step that fails,
faults or runs into its limit ends the job (nothing more is started on the GPU):
    build     the library, if it is not there (make with at most 16 jobs)
    time      warm-up, 300 ms of untimed repeats of the timed call (an idle MI355X takes that long to ramp), then six timed regions of K
              calls each, a host clock around work that ends in a device synchronise: median (min .. max) per call; predict and the two
              torch lines alternate inside every region, so drift shows in both
    kernels   the per-kernel split of one predict call of each shape: rocprofv3 --kernel-trace --stats in a run of its own
Usage:  python tools/bnn_predict_timing.py [file to write the lines to]          (default: bench_outputs/bnn_predict_timing.txt;
        the tracer writes beside it, into bnn_predict_prof/)"""
import csv
import glob
import os
import signal
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = ((10, 1, 200), (64, 10000, 10))           # (N, M, calls per timed region)
DEFAULT_OUT = os.path.join(ROOT, "bench_outputs", "bnn_predict_timing.txt")
LIMITS = dict(build=1500, time=420, kernels=420)


def setup():
    import numpy as np
    import torch
    from brancher_amd import bnn, workloads as W
    model = W.build_bayesian_neural_network(W.native_api(), dataset_size=512, batch_size=30, q_scale1=4e-4, q_loc_scale=1.0)
    c = bnn.CompiledBnn(model, model.posterior_model, "pathwise")
    p = c.program
    assert [(l["rows"], l["cols"]) for l in p.layers] == [(20, 784), (10, 20)]
    loc, scale = (torch.from_numpy(a.astype(np.float32)).to(c.device) for a in bnn.row_parameters(p, c.params.cpu().numpy()))
    return np, torch, c, loc, scale


def torch_line(torch, c, loc, scale, rows, n, eps=None):
    """what a user would write: W = mu + s eps for every tensor, bmm + tanh, bmm, softmax, the mean over the samples"""
    p = c.program
    if eps is None:
        eps = torch.randn((n, p.n_rows), device=c.device)
    w = loc[None, :] + scale[None, :] * eps
    t = {t["name"]: w[:, t["row0"]:t["row0"] + t["size"]].reshape(n, t["rows"], t["cols"]) for t in p.tensors}
    x = rows.t().unsqueeze(0).expand(n, -1, -1)                                  # [N, P, M]
    hidden = torch.tanh(torch.bmm(t["weights1"], x) + t["b1"])
    probs = torch.softmax(torch.bmm(t["weights2"], hidden) + t["b2"], dim=1)     # [N, C, M]
    return probs.mean(dim=0).t()


def step_time(out_path):
    np, torch, c, loc, scale = setup()
    lines = []
    for n, m, k in SHAPES:
        rows = torch.from_numpy(np.random.RandomState(0).randint(0, 256, size=(m, 784)).astype(np.float32)).to(c.device)
        first = c.predict(rows, n, seed=1, offset=0, want_noise=True)
        eps = first["noise"].t().contiguous()
        ref = torch_line(torch, c, loc, scale, rows, n, eps)
        err = float((first["mean"] - ref).abs().max())
        calls = dict(predict=lambda: c.predict(rows, n, seed=1, offset=0),
                     torch_with_draw=lambda: torch_line(torch, c, loc, scale, rows, n),
                     torch_given_draw=lambda: torch_line(torch, c, loc, scale, rows, n, eps))
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
        med = {name: float(np.median(v)) for name, v in us.items()}
        lines.append("N %3d M %5d  data path %s, forward kernel in %s, rows per pass %d; |mean - torch on the same draws| %.2e" % (
            n, m, first["data_path"], c.predict_path(), first["rows_per_pass"], err))
        for name, v in us.items():
            lines.append("    %-17s median %9.1f us/call  (min %9.1f .. max %9.1f)  six regions of %d calls: %s" % (
                name, med[name], min(v), max(v), k, " ".join("%.1f" % u for u in v)))
        lines.append("    predict / torch_with_draw %.2f    predict / torch_given_draw %.2f" % (
            med["predict"] / med["torch_with_draw"], med["predict"] / med["torch_given_draw"]))
    emit(lines, out_path)


def step_profiled():
    """one warmed predict call of each shape plus the torch line, for the tracer"""
    np, torch, c, loc, scale = setup()
    for n, m, _ in SHAPES:
        rows = torch.from_numpy(np.random.RandomState(0).randint(0, 256, size=(m, 784)).astype(np.float32)).to(c.device)
        for _ in range(3):
            c.predict(rows, n, seed=1, offset=0)
            torch_line(torch, c, loc, scale, rows, n)
        torch.cuda.synchronize()


def step_kernels(out_path):
    out = os.path.join(os.path.dirname(os.path.abspath(out_path)), "bnn_predict_prof")
    subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "predict", "--",
                    sys.executable, os.path.abspath(__file__), "--step", "profiled"], check=True, cwd=ROOT,
                   stdout=subprocess.DEVNULL, stderr=subprocess.STDOUT)
    found = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
    lines = ["kernels of three predict calls and three torch lines per shape (both shapes in one trace), by total time:"]
    if not found:
        lines.append("    no kernel_stats.csv under " + out + "")
    else:
        with open(found[0]) as f:
            rows = list(csv.DictReader(f))
        for r in rows[:24]:
            lines.append("    %-70s calls %5s  total %10.1f us  average %9.1f us  %5s %%" % (
                r.get("Name", "?")[:70], r.get("Calls", "?"), float(r.get("TotalDurationNs", 0)) / 1e3, float(r.get("AverageNs", 0)) / 1e3,
                r.get("Percentage", "?")))
    emit(lines, out_path)


def emit(lines, out_path):
    for line in lines:
        print(line, flush=True)
    with open(out_path, "a") as f:
        f.write("\n".join(lines) + "\n")


def driver(out_path):
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    open(out_path, "w").close()
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    steps = []
    if not os.path.exists(os.path.join(ROOT, "brancher_amd", "libbsvi.so")):
        steps.append(("build", ["make", "-C", os.path.join(ROOT, "brancher_amd", "csrc"), "-j16"]))
    steps += [(name, [sys.executable, os.path.abspath(__file__), "--step", name, out_path]) for name in ("time", "kernels")]
    for name, cmd in steps:
        child = subprocess.Popen(cmd, cwd=ROOT, env=env, start_new_session=True)
        try:
            rc = child.wait(timeout=LIMITS[name])
        except subprocess.TimeoutExpired:
            os.killpg(child.pid, signal.SIGKILL)            # (the step's whole process group: the tracer and the program under it)
            child.wait()
            rc = 124
        if rc:
            print("step %s ended with status %d: nothing more is started" % (name, rc), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--step":
        path = sys.argv[3] if len(sys.argv) > 3 else DEFAULT_OUT
        dict(time=lambda: step_time(path), kernels=lambda: step_kernels(path), profiled=step_profiled)[sys.argv[2]]()
    else:
        sys.exit(driver(os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else DEFAULT_OUT))
