"""
Generates tests/golden/bnn_priors/*.npz — the regression models of the Bayesian-neural-network family whose weights and biases carry a
LAPLACE or a CAUCHY prior (workloads.build_bnn_regression(prior=...): the reference's `LaplaceVariable` / `CauchyVariable` in place of
`NormalVariable(0, 10)`, the posterior still mean-field Normal) — by running the REAL reference through oracle/gen_golden.py, as
tools/gen_golden_bnn_sigma.py does for the learnable sigma: the same recording harness, the same arrays (loss, per-sample terms, every
gradient for Pathwise / BlackBox / Taylor1, a short Adam trajectory).  The cases are registered in `gen_golden.CASES` at run time and
the fixtures live in a subdirectory, for that tool's reasons.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_bnn_priors.py [case ...]        (BSVI_GOLDEN_OUT: another directory)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, ROOT)

import gen_golden  # noqa: E402

SUBDIR = "bnn_priors"
BUILDER = "build_bnn_regression"
# (Each case has exactly TWO latent tensors: with two terms the reference's sums over sets hashed by address are the same in either
#  order, so the fixtures regenerate bit for bit in any process — tools/gen_golden_bnn_normal.py.  The priors are narrow (scale 0.3) and
#  off centre (loc 0.1) and the posterior means lie half a posterior scale from zero, so that the prior's gradient is a visible share of
#  every recorded gradient and sign(w - loc) differs between the samples of a row.)
PRIOR = dict(prior_scale=0.3, prior_loc=0.1, q_loc_scale=0.5)
CASES = {
    # one tanh hidden layer without biases, one output, Laplace priors; integer features (exactly bf16: the three-piece products)
    "bnn_laplace_tanh_P32_H6_C1_DS30_B12_N5": (BUILDER, dict(dataset_size=30, batch_size=12, n_features=32, n_hidden=6, n_outputs=1,
                                                             bias=False, sigma=0.3, prior="laplace", **PRIOR),
                                                5, 151, dict(iters=4, n=4, optimizer="Adam", lr=5e-3)),
    # one layer with its bias (Bayesian linear regression), two outputs, Cauchy priors; normal features (the f32-input products)
    "bnn_cauchy_linear_P16_C2_DS24_B10_N6": (BUILDER, dict(dataset_size=24, batch_size=10, n_features=16, n_hidden=0, n_outputs=2,
                                                           sigma=[0.4, 0.7], data="normal", prior="cauchy", **PRIOR),
                                              6, 153, dict(iters=4, n=5, optimizer="Adam", lr=5e-3)),
}


def register():
    gen_golden.CASES.update(CASES)
    # every latent's posterior a mean-field Normal: Taylor1 is recorded
    gen_golden.TAYLOR1_BUILDERS = tuple(gen_golden.TAYLOR1_BUILDERS) + (BUILDER,)
    if not os.environ.get("BSVI_GOLDEN_OUT"):
        gen_golden.OUT = os.path.join(ROOT, "tests", "golden", SUBDIR)


if __name__ == "__main__":
    register()
    api = gen_golden.reference_api()
    for case in sys.argv[1:] or list(CASES):
        gen_golden.run_case(case, api)
