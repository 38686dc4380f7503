"""SHA-256 of everything a Bayesian-neural-network handle computes, one line per (model, estimator, middle kernel), so that two builds
can be compared bit for bit (diff the two outputs: every line must be equal):
    python tools/bnn_outputs_digest.py [--tree DIR]
(DIR: the checkout whose package and library run, default: this one.)  Per line: the loss, the per-sample f (and log q under BlackBox)
and the gradients of one `evaluate` of 70 samples, the parameters after five fused Adam steps, and `predict`'s mean, variance and draws
on 40 rows — fixed seeds throughout.  Every model runs under both estimators and three times: as selected, under BSVI_BNN_MID=0, and
under BSVI_BNN_MID=0 BSVI_BNN_JIT=0 (the static kernel).  The models: the cases of tools/bnn_source_dump.py at minibatch 17, a
32-16-16-4 network on data="normal" (the static kernel in memory, f32 products), a Laplace / Cauchy / Normal mixture of priors, the
same under latent prior scales per layer, and a classifier under one global latent prior scale."""
import hashlib
import os
import sys

import numpy as np
import torch

ARGS = sys.argv[1:]
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE = os.path.abspath(ARGS[ARGS.index("--tree") + 1]) if "--tree" in ARGS else HERE
sys.path.insert(0, TREE)
from brancher_amd import bnn, workloads as W  # noqa: E402
import bnn_source_dump as S  # noqa: E402  (beside this file: the cases)

N, ROWS = 70, 40
NARROW = dict(prior_scale=0.3, prior_loc=0.1, q_loc_scale=0.5)
MIX = dict(dataset_size=40, batch_size=33, n_features=36, n_hidden=5, hidden2=4, n_outputs=3, activation="relu", data="normal",
           sigma=[0.3, 0.5, 0.8], prior=dict(weights1="cauchy", b1="laplace", weights2="laplace", b2="cauchy", weights3="normal", b3="laplace"),
           **NARROW)                                                   # 36-5-4-3 (tests/test_gpu_bnn_priors.py, test_gpu_bnn_hier.py)
MODELS = {name: (dict(kw, batch_size=17, dataset_size=40), env) for name, (kw, env) in S.CASES.items()}
MODELS["32-16-16-4 normal data (upper_mem)"] = (dict(widths=[32, 16, 16, 4], batch_size=17, dataset_size=40, data="normal", q_scale=0.3), {})
MODELS["36-5-4-3 prior mixture"] = (MIX, {})
MODELS["36-5-4-3 prior mixture, latent scales per layer"] = (dict(MIX, scale_latent="layer"), {})
MODELS["16-6-3 classifier, global latent scale"] = (dict(classifier=True, dataset_size=40, batch_size=17, n_features=16, n_hidden=6, n_classes=3,
                                                         pixels="integers", prior_scale=0.3, prior_loc=0.1, q_scale=0.1, q_loc_scale=0.5,
                                                         scale_latent="global"), {})
SWITCHES = (("selected", {}), ("MID=0", dict(BSVI_BNN_MID="0")), ("MID=0 JIT=0", dict(BSVI_BNN_MID="0", BSVI_BNN_JIT="0")))


def sha(t):
    a = np.ascontiguousarray(t.detach().cpu().numpy() if torch.is_tensor(t) else t)
    return hashlib.sha256(a.tobytes()).hexdigest()[:16]


def line(name, kw, estimator):
    m = S.build(W, kw)
    c = bnn.CompiledBnn(m, m.posterior_model, estimator)
    res = c.evaluate(N, seed=3, offset=5, want_fvalues=True)
    out = ["loss " + sha(res["loss"]), "f " + sha(res["f"]), "grads " + sha(res["grads"])]
    if "lq" in res:
        out.append("lq " + sha(res["lq"]))
    c.train(5, N, "Adam", seed=4, lr=1e-2)
    out.append("params " + sha(c.params))
    p = c.predict(torch.from_numpy(c.program.dataset[:ROWS]).to(c.device), N, seed=5, offset=6, want_draws=True)
    out += ["%s %s" % (k, sha(p[k])) for k in ("mean", "var", "draws") if k in p]
    return "%s %s" % (c.middle_path(), " ".join(out))


if __name__ == "__main__":
    for name, (kw, case_env) in MODELS.items():
        for estimator in ("pathwise", "blackbox"):
            for tag, switches in SWITCHES:
                env = dict(case_env, **switches)
                os.environ.update(env)
                try:
                    print("%-50s %-8s %-11s %s" % (name, estimator, tag, line(name, kw, estimator)), flush=True)
                finally:
                    for k in env:
                        del os.environ[k]
