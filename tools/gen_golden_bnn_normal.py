"""
Generates tests/golden/bnn_normal/*.npz — the regression models of the Bayesian-neural-network family (a Normal likelihood over
the matmul chain, workloads.build_bnn_regression) — by running the REAL reference through oracle/gen_golden.py: the same
recording harness, the same arrays as the `bnn_*` fixtures (loss, per-sample terms, every gradient for Pathwise / BlackBox /
Taylor1 and the two user-defined estimators, a short Adam trajectory).  The cases are registered in `gen_golden.CASES` at run
time, so the generator's own case table — which the parity tests walk — is untouched; the fixtures live in a subdirectory for
the same reason (an .npz directly in tests/golden/ is looked up in that table).

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_bnn_normal.py [case ...]        (BSVI_GOLDEN_OUT: another directory)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, ROOT)

import gen_golden  # noqa: E402

SUBDIR = "bnn_normal"
BUILDER = "build_bnn_regression"
# (Each case has exactly TWO latent tensors.  The reference adds the log-probabilities of a variable's parents, and the entropies of
#  the posterior's variables, in the order of a SET hashed by address; with two terms the sum is the same either way, so the
#  fixtures regenerate bit for bit in any process.  Biases on the deeper network are covered against the oracle on the GPU.)
CASES = {
    # one tanh hidden layer without biases, one output, one sigma; integer features (exactly bf16: the three-piece products)
    "bnn_normal_tanh_P32_H6_C1_DS30_B12_N5": (BUILDER, dict(dataset_size=30, batch_size=12, n_features=32, n_hidden=6, n_outputs=1,
                                                            bias=False),
                                               5, 131, dict(iters=4, n=4, optimizer="Adam", lr=5e-3)),
    # one layer with its bias (Bayesian linear regression), two outputs with a sigma each; normal features (the f32-input products)
    "bnn_normal_linear_P16_C2_DS24_B10_N6": (BUILDER, dict(dataset_size=24, batch_size=10, n_features=16, n_hidden=0, n_outputs=2,
                                                           sigma=[0.4, 0.7], data="normal"),
                                              6, 133, dict(iters=4, n=5, optimizer="Adam", lr=5e-3)),
}


def register():
    gen_golden.CASES.update(CASES)
    # every latent a mean-field Normal: Taylor1 is recorded; and the two user-defined estimators, as for the classifiers
    gen_golden.TAYLOR1_BUILDERS = tuple(gen_golden.TAYLOR1_BUILDERS) + (BUILDER,)
    gen_golden.CUSTOM_ESTIMATOR_BUILDERS = tuple(gen_golden.CUSTOM_ESTIMATOR_BUILDERS) + (BUILDER,)
    if not os.environ.get("BSVI_GOLDEN_OUT"):
        gen_golden.OUT = os.path.join(ROOT, "tests", "golden", SUBDIR)


if __name__ == "__main__":
    register()
    api = gen_golden.reference_api()
    for case in sys.argv[1:] or list(CASES):
        gen_golden.run_case(case, api)
