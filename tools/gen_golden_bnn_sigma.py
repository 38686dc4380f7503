"""
Generates tests/golden/bnn_sigma/*.npz — the regression models of the Bayesian-neural-network family with a LEARNABLE sigma
(workloads.build_bnn_regression(learnable_sigma=True): the reference's `NormalVariable(chain, sigma, "y", learnable=True)`, a
learnable root `y_scale` behind a softplus in the joint model's parameter group) — by running the REAL reference through
oracle/gen_golden.py, as tools/gen_golden_bnn_normal.py does for the constant sigma: the same recording harness, the same arrays
(loss, per-sample terms, every gradient — `grad_*/y_scale` among them — for Pathwise / BlackBox / Taylor1 and the two user-defined
estimators, a short Adam trajectory in which `y_scale` stays put on iteration 0 and moves afterwards).  The cases are registered in
`gen_golden.CASES` at run time and the fixtures live in a subdirectory, for that tool's reasons.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_bnn_sigma.py [case ...]        (BSVI_GOLDEN_OUT: another directory)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, ROOT)

import gen_golden  # noqa: E402

SUBDIR = "bnn_sigma"
BUILDER = "build_bnn_regression"
# (Each case has exactly TWO latent tensors: with two terms the reference's sums over sets hashed by address are the same in either
#  order, so the fixtures regenerate bit for bit in any process — tools/gen_golden_bnn_normal.py.  The model's sigma starts away from
#  the teacher's, so that u^2 - 1 does not cancel in the recorded gradient.)
CASES = {
    # one tanh hidden layer without biases, one output, one sigma; integer features (exactly bf16: the three-piece products)
    "bnn_sigma_tanh_P32_H6_C1_DS30_B12_N5": (BUILDER, dict(dataset_size=30, batch_size=12, n_features=32, n_hidden=6, n_outputs=1,
                                                           bias=False, sigma=0.3, learnable_sigma=True, sigma_init=0.5),
                                              5, 141, dict(iters=4, n=4, optimizer="Adam", lr=5e-3)),
    # one layer with its bias (Bayesian linear regression), two outputs with a sigma each; normal features (the f32-input products)
    "bnn_sigma_linear_P16_C2_DS24_B10_N6": (BUILDER, dict(dataset_size=24, batch_size=10, n_features=16, n_hidden=0, n_outputs=2,
                                                          sigma=[0.4, 0.7], data="normal", learnable_sigma=True, sigma_init=[0.6, 0.5]),
                                             6, 143, dict(iters=4, n=5, optimizer="Adam", lr=5e-3)),
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
