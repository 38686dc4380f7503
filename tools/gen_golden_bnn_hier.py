"""
Generates tests/golden/bnn_hier/*.npz — the regression models of the Bayesian-neural-network family under a HIERARCHICAL prior
(workloads.build_bnn_regression(scale_latent=...): the reference's `LogNormalVariable` as the `scale` of a `NormalVariable` /
`LaplaceVariable` weight tensor, a learnable `LogNormalVariable` of the same name in the posterior) — by running the REAL reference
through oracle/gen_golden.py, as tools/gen_golden_bnn_likelihoods.py does for the Laplace and Cauchy likelihoods: the same recording
harness, the same arrays (loss, per-sample terms, every gradient for Pathwise / BlackBox and the two user-defined estimators, a short
Adam trajectory).  The cases are registered in `gen_golden.CASES` at run time and the fixtures live in a subdirectory, for that tool's
reasons.  Taylor1 is not recorded: the mean of a LogNormal is not the value at its zero draw, and the BNN path refuses the estimator
for these models.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_bnn_hier.py [case ...]        (BSVI_GOLDEN_OUT: another directory)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, ROOT)

import gen_golden  # noqa: E402

SUBDIR = "bnn_hier"
BUILDER = "build_bnn_regression"
# (Each case has exactly TWO latents — ONE weight tensor and ONE scale latent: with two terms the reference's sums over sets hashed by
#  address are the same in either order, so the fixtures regenerate bit for bit in any process — tools/gen_golden_bnn_normal.py.)
CASES = {
    # 16-2 linear, Normal prior under the latent itself, normal features (the f32-input products)
    "bnn_hier_normal_linear_P16_C2_DS24_B10_N6": (BUILDER, dict(dataset_size=24, batch_size=10, n_features=16, n_hidden=0, n_outputs=2,
                                                                bias=False, sigma=[0.4, 0.7], data="normal", prior_loc=0.1,
                                                                scale_latent="global", scale_latent_prior=(-0.5, 0.7),
                                                                scale_latent_q=(-0.8, 0.3)),
                                                  6, 161, dict(iters=4, n=5, optimizer="Adam", lr=5e-3)),
    # 32-1 linear, Laplace prior of scale 2.0 * tau, integer features (exactly bf16: the three-piece products)
    "bnn_hier_laplace_linear_P32_C1_DS30_B12_N5": (BUILDER, dict(dataset_size=30, batch_size=12, n_features=32, n_hidden=0, n_outputs=1,
                                                                 bias=False, sigma=0.3, prior="laplace", prior_loc=0.1,
                                                                 scale_latent={"tau": [["weights1", 2.0]]}, scale_latent_prior=(-1.0, 0.5),
                                                                 scale_latent_q=(-1.2, 0.25)),
                                                   5, 163, dict(iters=4, n=4, optimizer="Adam", lr=5e-3)),
}


def register():
    gen_golden.CASES.update(CASES)
    if BUILDER not in gen_golden.CUSTOM_ESTIMATOR_BUILDERS:
        gen_golden.CUSTOM_ESTIMATOR_BUILDERS = tuple(gen_golden.CUSTOM_ESTIMATOR_BUILDERS) + (BUILDER,)
    if not os.environ.get("BSVI_GOLDEN_OUT"):
        gen_golden.OUT = os.path.join(ROOT, "tests", "golden", SUBDIR)


if __name__ == "__main__":
    register()
    api = gen_golden.reference_api()
    for case in sys.argv[1:] or list(CASES):
        gen_golden.run_case(case, api)
