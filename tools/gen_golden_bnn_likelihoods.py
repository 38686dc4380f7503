"""
Generates tests/golden/bnn_lik/*.npz — the regression models of the Bayesian-neural-network family under an observed LAPLACE and an
observed CAUCHY likelihood (workloads.build_bnn_regression(likelihood="laplace" | "cauchy"): the reference's
`LaplaceVariable(chain, b, "y")` and `CauchyVariable(chain, gamma, "y", learnable=True)`) — by running the REAL reference through
oracle/gen_golden.py, as tools/gen_golden_bnn_sigma.py does for the Normal likelihood with a learnable sigma: the same recording
harness, the same arrays (loss, per-sample terms, every gradient for Pathwise / BlackBox / Taylor1 and the two user-defined estimators,
a short Adam trajectory).  The cases are registered in `gen_golden.CASES` at run time and the fixtures live in a subdirectory, for that
tool's reasons.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_bnn_likelihoods.py [case ...]        (BSVI_GOLDEN_OUT: another directory)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, ROOT)

import gen_golden  # noqa: E402

SUBDIR = "bnn_lik"
BUILDER = "build_bnn_regression"
# (Each case has exactly TWO latent tensors: with two terms the reference's sums over sets hashed by address are the same in either
#  order, so the fixtures regenerate bit for bit in any process — tools/gen_golden_bnn_normal.py.)
CASES = {
    # Laplace: one tanh hidden layer without biases, one output, a constant scale; integer features (exactly bf16: the three-piece products)
    "bnn_lik_laplace_tanh_P32_H6_C1_DS30_B12_N5": (BUILDER, dict(dataset_size=30, batch_size=12, n_features=32, n_hidden=6, n_outputs=1,
                                                                 bias=False, sigma=0.3, likelihood="laplace"),
                                                    5, 151, dict(iters=4, n=4, optimizer="Adam", lr=5e-3)),
    # Cauchy: one layer with its bias, two outputs with a learnable scale each that starts away from the teacher's; normal features
    # (the f32-input products)
    "bnn_lik_cauchy_linear_P16_C2_DS24_B10_N6": (BUILDER, dict(dataset_size=24, batch_size=10, n_features=16, n_hidden=0, n_outputs=2,
                                                               sigma=[0.4, 0.7], data="normal", learnable_sigma=True, sigma_init=[0.6, 0.5],
                                                               likelihood="cauchy"),
                                                  6, 153, dict(iters=4, n=5, optimizer="Adam", lr=5e-3)),
}


def register():
    gen_golden.CASES.update(CASES)
    # every latent a mean-field Normal: Taylor1 is recorded; and the two user-defined estimators, as for the classifiers
    if BUILDER not in gen_golden.TAYLOR1_BUILDERS:
        gen_golden.TAYLOR1_BUILDERS = tuple(gen_golden.TAYLOR1_BUILDERS) + (BUILDER,)
    if BUILDER not in gen_golden.CUSTOM_ESTIMATOR_BUILDERS:
        gen_golden.CUSTOM_ESTIMATOR_BUILDERS = tuple(gen_golden.CUSTOM_ESTIMATOR_BUILDERS) + (BUILDER,)
    if not os.environ.get("BSVI_GOLDEN_OUT"):
        gen_golden.OUT = os.path.join(ROOT, "tests", "golden", SUBDIR)


if __name__ == "__main__":
    register()
    api = gen_golden.reference_api()
    for case in sys.argv[1:] or list(CASES):
        gen_golden.run_case(case, api)
