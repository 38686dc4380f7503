"""
Generates tests/golden/bnn_point/*.npz — networks of the Bayesian-neural-network family with POINT-ESTIMATED tensors
(workloads.build_bnn_regression / build_bayesian_neural_network with point=...: a learnable `RootVariable` named like a weight tensor
in the posterior model, the reference's idiom of `inference.MAP`, inference.py:251-275) — by running the REAL reference through
oracle/gen_golden.py, as tools/gen_golden_bnn_hier.py does for the hierarchical priors: the same recording harness (which calls
`update_observed_submodel()` before it evaluates, as `perform_inference` does), the same arrays — the loss, the per-sample terms and
every gradient under Pathwise and BlackBox, and for a posterior of roots alone the loss of the reference's `MAP.compute_loss`
("loss_map"; `record_map` below adds that loss once more with the minibatch it was taken on).  The cases are registered in
`gen_golden.CASES` at run time and the fixtures live in a subdirectory, for that tool's reasons.  No trajectory: a few KB each.

    trunk      64-9-1 tanh regression, weights1 and b1 points under a Bayesian last layer (Normal weights2 and b2): the gradients land
               on the roots `weights1` and `b1` and on the loc and scale of the two Normal tensors
    all-point  32-6-3 Categorical classifier, every tensor a point: nothing is drawn, the entropy is zero, the loss is
               -log p(theta, minibatch)

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_bnn_point.py [case ...]        (BSVI_GOLDEN_OUT: another directory)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, ROOT)

import gen_golden  # noqa: E402

SUBDIR = "bnn_point"
NARROW = dict(prior_loc=0.1, prior_scale=0.3, q_loc_scale=0.5)
CASES = {
    "bnn_point_trunk_P64_H9_C1_DS40_B17_N3": ("build_bnn_regression", dict(dataset_size=40, batch_size=17, n_features=64, n_hidden=9, n_outputs=1,
                                                                            point=["weights1", "b1"], **NARROW), 3, 171, None),
    "bnn_point_all_P32_H6_C3_DS24_B8_N3": ("build_bayesian_neural_network", dict(dataset_size=24, batch_size=8, widths=[32, 6, 3],
                                                                                  pixels="integers", point="all", **NARROW), 3, 173, None),
}


def register():
    gen_golden.CASES.update(CASES)
    if not os.environ.get("BSVI_GOLDEN_OUT"):
        gen_golden.OUT = os.path.join(ROOT, "tests", "golden", SUBDIR)


def record_map(case, api):
    """the reference's `MAP.compute_loss` once more on a model of roots alone, with the minibatch it drew beside its value ("map/loss",
    "map/minibatch/indices"): the harness records "loss_map" without the rows, which a test cannot evaluate again"""
    import numpy as np
    from brancher import inference
    import brancher_amd.workloads as W
    builder, kwargs, _, seed, _ = CASES[case]
    model = getattr(W, builder)(api, **kwargs)
    model.update_observed_submodel()
    q = model.posterior_model
    if not all(type(v).__name__ == "RootVariable" for v in q.flatten()):
        return
    drawn = {}
    obs, orig = model.observed_submodel, model.observed_submodel._get_sample

    def capture(*a, **k):
        res = orig(*a, **k)
        drawn.update({var.name: np.array([int(i) for i in val], dtype=np.int64) for var, val in res.items() if type(var).__name__ == "RandomIndices"})
        return res

    obs._get_sample = capture
    np.random.seed(seed)
    loss = inference.MAP().compute_loss(model, q, None, 1)
    path = os.path.join(gen_golden.OUT, case + ".npz")
    out = dict(np.load(path))
    out["map/loss"] = np.float32(loss.detach().numpy().reshape(-1)[0])
    for name, rows in drawn.items():
        out["map/minibatch/" + name] = rows
    np.savez_compressed(path, **out)
    print("%-28s map/loss=%.6f on rows %s" % (case, out["map/loss"], drawn))


if __name__ == "__main__":
    register()
    api = gen_golden.reference_api()
    for case in sys.argv[1:] or list(CASES):
        gen_golden.run_case(case, api)
        record_map(case, api)
