"""Regression with a Bayesian neural network: the first thing one tries with the family.

    y ~ NormalVariable(BF.matmul(weights2, BF.tanh(BF.matmul(weights1, x) + b1)) + b2, sigma)

Every weight matrix and bias is a latent under a mean-field Normal posterior, the noise scale sigma a constant of the model, and `x`
and the targets two EmpiricalVariables that share a RandomIndices variable — another minibatch in every iteration.  At 784 features
the model is far beyond the scalar engine: `engine.compile_model` sends it to the matrix-core path of the Bayesian-neural-network
family (two MFMA products with the minibatch, the Normal likelihood between them; csrc/bnn_kernel.inc).  Run on a machine with an
MI355X:

    python examples/bnn_regression.py
    python examples/bnn_regression.py --learn-sigma      # sigma learnable: NormalVariable(chain, 1.0, "y", learnable=True)
    python examples/bnn_regression.py --prior laplace    # LaplaceVariable(0, 0.5) on every weight and bias (the Bayesian lasso)
    python examples/bnn_regression.py --prior cauchy     # CauchyVariable(0, 0.5): heavy tails
    python examples/bnn_regression.py --scale-head       # input-dependent noise: a second head, sigma(x) = 0.05 + softplus(raw(x))
    python examples/bnn_regression.py --likelihood laplace    # median (L1) regression: LaplaceVariable(chain, b, "y")
    python examples/bnn_regression.py --likelihood cauchy     # the heavy-tailed fit for data with outliers: CauchyVariable(chain, gamma, "y")
    python examples/bnn_regression.py --hierarchical     # a latent prior scale per layer: NormalVariable(0, tau1, "weights1"), tau1 LogNormal
    python examples/bnn_regression.py --point weights1,b1     # a deterministic trunk under a Bayesian last layer: RootVariable("weights1"), ...
    python examples/bnn_regression.py --map              # every tensor a point estimate, trained with inference.MAP()
    python examples/bnn_regression.py --activation gelu  # BF.gelu in the place of BF.tanh; with keywords: leaky_relu:negative_slope=0.2

With --learn-sigma the model starts from a guess of 1.0 and learns the noise scale with the posterior (a learnable root `y_scale`
behind a softplus in the joint model's parameter group, stepped from the second iteration on, as the reference steps it); the learned
value is printed beside the teacher's.  With --prior the weights and biases carry a sparsity-inducing (Laplace) or heavy-tailed (Cauchy)
prior of scale 0.5, parameters of the model in their own right, and the posterior stays mean-field Normal.  The likelihood is not
rescaled from the minibatch to the dataset (as in the reference), so such a prior weighs as much as one minibatch of targets: the
run with --prior is a 64-8-1 network on minibatches of 512 rows, where the data have the say — at 784-20-1 and 30 rows the 15 729
weights would return to their prior.  With --scale-head the noise level depends on the input: a second head `weights_scale`, `b_scale`
on the hidden layer gives the scale of the Normal, `0.05 + BF.softplus(BF.matmul(weights_scale, hidden) + b_scale)`, latent like the
rest; the teacher's noise varies from row to row, and the run prints how well the predicted scale follows the size of the residuals.
With --likelihood the observed variable is a Laplace or a Cauchy variable over the same chain (it combines with every other switch): the
teacher's noise is drawn from that family, so under "cauchy" a few targets lie far from the rest — the run prints the median absolute
error beside the RMSE, which those few dominate.  With --hierarchical the prior scale of every layer is itself a latent: `tau1`,
a `LogNormalVariable(0, 1)`, scales the priors of weights1 and b1, `tau2` those of weights2 and b2, each under a learnable LogNormal
posterior (the hierarchical BNN of the textbooks: per-layer shrinkage learned with the weights; it combines with --prior).  The run is
the 64-8-1 network of --prior, for its reason, and prints the posterior medians exp(m_t) of the layers' scales after training.
With --point the tensors named are not random in the posterior: its members for them are learnable `RootVariable`s of the tensors' names
(the reference's idiom), trained as ordinary network weights under their prior, while the others keep their mean-field Normal —
`--point weights1,b1` is the usual way to make a wide network affordably Bayesian, and with all of weights1 a point the engine takes both
products with the minibatch once per iteration, not once per sample (`first_layer_path()` prints "shared").  With --map every tensor is
a point and `inference.MAP()` trains the network: the loss is -log p(theta, minibatch) on one sample, no entropy.
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from brancher_amd import engine, inference, workloads as W

LEARN_SIGMA = "--learn-sigma" in sys.argv[1:]
KW = dict(dataset_size=512, batch_size=30, n_features=784, n_hidden=20, n_outputs=1, sigma=0.5)
if LEARN_SIGMA:
    KW.update(learnable_sigma=True, sigma_init=1.0)
SCALE_HEAD = "--scale-head" in sys.argv[1:]
if SCALE_HEAD:
    if LEARN_SIGMA:
        sys.exit("--scale-head replaces sigma: not with --learn-sigma")
    KW.update(scale_head="softplus", scale_floor=0.05, dataset_size=2048, batch_size=512, n_features=64, n_hidden=8)
    del KW["sigma"]
PRIOR = None
if "--prior" in sys.argv[1:]:
    PRIOR = (sys.argv[sys.argv.index("--prior") + 1:] or [""])[0]
    if PRIOR not in ("laplace", "cauchy"):
        sys.exit("--prior laplace | cauchy")
    KW.update(prior=PRIOR, prior_scale=0.5, dataset_size=2048, batch_size=512, n_features=64, n_hidden=8)
HIERARCHICAL = "--hierarchical" in sys.argv[1:]
if HIERARCHICAL:
    KW.update(scale_latent="layer", scale_latent_prior=(0., 1.), scale_latent_q=(0., 0.2), dataset_size=2048, batch_size=512, n_features=64,
              n_hidden=8)
LIKELIHOOD = "normal"
if "--likelihood" in sys.argv[1:]:
    LIKELIHOOD = (sys.argv[sys.argv.index("--likelihood") + 1:] or [""])[0]
    if LIKELIHOOD not in ("laplace", "cauchy"):
        sys.exit("--likelihood laplace | cauchy")
    KW.update(likelihood=LIKELIHOOD)


POINT = ()
if "--map" in sys.argv[1:]:
    POINT = "all"
elif "--point" in sys.argv[1:]:
    POINT = tuple(n for n in (sys.argv[sys.argv.index("--point") + 1:] or [""])[0].split(",") if n)
    if not POINT:
        sys.exit("--point weights1,b1 (tensor names, comma-separated)")
if POINT:
    KW.update(point=POINT)
# --activation NAME[:k=v,...]: the function of the hidden layer — any of tanh, relu, sigmoid, softplus, leaky_relu, elu, selu, softsign,
# hardtanh, relu6, silu, gelu — with its keywords, as `--activation leaky_relu:negative_slope=0.2` or `--activation hardtanh:min_val=-2,max_val=2`
ACTIVATION = ("tanh", {})
if "--activation" in sys.argv[1:]:
    name, _, given = (sys.argv[sys.argv.index("--activation") + 1:] or [""])[0].partition(":")
    try:
        ACTIVATION = (name, {k: float(v) for k, v in (kv.split("=") for kv in given.split(",") if kv)})
    except ValueError:
        sys.exit("--activation NAME[:keyword=number,...]")
    if not name:
        sys.exit("--activation NAME[:keyword=number,...]")
    KW.update(activations=[ACTIVATION])


def value_of(params, name):
    """the posterior mean of a tensor: the loc of its Normal, or the value of its root"""
    return params[name + "_loc"] if name + "_loc" in params else params[name]


def dataset_of(variable):
    """[DS, rows] array behind an EmpiricalVariable"""
    a = np.asarray(variable.link.expressions()["dataset"].expr.attr.value, dtype=np.float64)
    return a.reshape(KW["dataset_size"], -1)


def posterior_mean_rmse(model):
    """root mean squared error, over the whole dataset, of the network evaluated at the posterior means of its weights"""
    y = next(v for v in model.flatten() if v.name == "y")
    X, Y = dataset_of(next(v for v in model.flatten() if v.name == "x")), dataset_of(y.dataset)
    p = engine.compile_model(model).named_params()
    hidden = W._np_activation(*ACTIVATION)(X @ value_of(p, "weights1").reshape(KW["n_hidden"], -1).T + value_of(p, "b1").reshape(1, -1))
    pred = hidden @ value_of(p, "weights2").reshape(KW["n_outputs"], -1).T + value_of(p, "b2").reshape(1, -1)
    if LIKELIHOOD != "normal":
        print("    median |error| of the posterior-mean prediction: %.3f" % float(np.median(np.abs(pred - Y))))
    return float(np.sqrt(np.mean((pred - Y) ** 2)))


model = W.build_bnn_regression(W.native_api(), **KW)
print("engine: %s, data path %s" % (type(engine.compile_model(model)).__name__, engine.compile_model(model).data_path()))
if LIKELIHOOD != "normal":
    print("likelihood:", engine.compile_model(model).program.summary()["family"])
if POINT:
    print("point estimates: %s; first layer %s" % (", ".join(engine.compile_model(model).program.summary()["point"]),
                                                  engine.compile_model(model).first_layer_path()))
if PRIOR:
    print("priors:", engine.compile_model(model).program.summary()["priors"])
print("RMSE of the posterior-mean prediction before training: %.3f (noise scale %s)"
      % (posterior_mean_rmse(model), "from the scale head" if SCALE_HEAD else "%.2f" % KW["sigma"]))
t0 = time.time()
inference.perform_inference(model, number_iterations=1500, number_samples=50, optimizer="Adam", lr=0.005,
                            inference_method=inference.MAP() if POINT == "all" else inference.ReverseKL())
seconds = time.time() - t0
loss = np.asarray(model.diagnostics["loss curve"])
print("1500 iterations in %.2f s; loss %.1f -> %.1f" % (seconds, loss[:20].mean(), loss[-20:].mean()))
print("RMSE of the posterior-mean prediction after training:  %.3f" % posterior_mean_rmse(model))
if LEARN_SIGMA:
    theta = float(engine.compile_model(model).named_params()["y_scale"].reshape(-1)[0])
    print("learned noise scale sigma = softplus(y_scale) = %.3f (started at %.2f; the teacher's noise: %.2f)"
          % (np.log1p(np.exp(theta)), KW["sigma_init"], KW["sigma"]))
if SCALE_HEAD:
    # the posterior predictive on the dataset's own rows: "scale" is sigma per sample and row, "var" the total variance
    c = engine.compile_model(model)
    y = next(v for v in model.flatten() if v.name == "y")
    X, Y = dataset_of(next(v for v in model.flatten() if v.name == "x")), dataset_of(y.dataset)
    res = c.predict(X.astype(np.float32), 64, seed=1, offset=0, want_outputs=True)
    sigma = res["scale"].mean(dim=0).cpu().numpy().reshape(-1)
    resid = np.abs(res["mean"].cpu().numpy().reshape(-1) - Y.reshape(-1))
    order = np.argsort(sigma)
    quarter = len(order) // 4
    print("predicted noise scale: %.3f .. %.3f over the rows; mean |residual| in the quarter of the rows with the smallest predicted "
          "scale %.3f, with the largest %.3f" % (sigma.min(), sigma.max(), resid[order[:quarter]].mean(), resid[order[-quarter:]].mean()))
if HIERARCHICAL:
    c = engine.compile_model(model)
    params = c.named_params()
    for latent, members in c.program.summary()["scale_latents"].items():
        print("posterior median of %s (the prior scale of %s): exp(%s_loc) = %.3f (started at %.3f)"
              % (latent, ", ".join(name for name, _ in members), latent, float(np.exp(params[latent + "_loc"].reshape(-1)[0])),
                 float(np.exp(KW["scale_latent_q"][0]))))
