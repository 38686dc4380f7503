"""
Bayesian neural networks on the dense-link path: lowering and engine for graphs whose likelihood goes through a CHAIN of
``BF.matmul`` links with latent weight matrices and latent biases,

    hidden = BF.tanh(BF.matmul(weights1, x) + b1)
    logits = BF.matmul(weights2, hidden) + b2
    k      = CategoricalVariable(logits=logits, name="k");  k.observe(labels)
    q:       NormalVariable(loc, scale, <same name>, learnable=True) for weights1, b1, weights2, b2

— the reference's `tests/test_MNIST_bayesian_neural_network.py:20-60` (any depth, any of tanh / relu / sigmoid / softplus /
leaky_relu / elu / selu / softsign / hardtanh / relu6 / silu / gelu between the layers, with torch's keywords; biases optional) — and the regression model of the same family, the chain as the loc of an observed Normal,

    y = NormalVariable(BF.matmul(weights2, hidden) + b2, sigma, name="y");  y.observe(targets)        # targets [DS, C, 1]

(or a `LaplaceVariable` / `CauchyVariable` in its place: median regression, the heavy-tailed fit — `program.family`,
`bsvi_bnn_set_likelihood_family`), with sigma (one value, or [C, 1]) a constant of the model (`bsvi_bnn_create_normal`) or learnable — the reference's
`NormalVariable(chain, 0.5, "y", learnable=True)`, or any a + b g(root) of a learnable root with g softplus / exp / sigmoid
(`bsvi_bnn_create_normal_learnable`) —, or computed from the input by a second head on the trunk of the first (heteroscedastic regression),

    loc   = BF.matmul(weights_loc, hidden) + b_loc
    scale = a + b * g(BF.matmul(weights_scale, hidden) + b_scale)          # g softplus / exp / sigmoid, a >= 0, b > 0
    y     = NormalVariable(loc, scale, name="y");  y.observe(targets)

whose four head tensors are latents like the rest and, to the library, ONE last layer of 2 C rows (`bsvi_bnn_create_normal_heads`); from
one layer (minibatched Bayesian linear regression) to eight.
`dense.lower_dense` serves ONE latent matrix without a bias; this module serves the rest of the family through `bsvi_bnn_*` (include/bsvi.h, csrc/bnn_kernel.inc).  The reference's semantics are kept as on the
dense path: priors and posteriors are matched by NAME, auto-created roots `<var>_<arg>` collide by name, no
minibatch rescaling of the likelihood (`variables.py:849` TODO).
"""
import ctypes as C
import numbers

import numpy as np
import torch

from brancher_amd import distributions as D
from brancher_amd import lowering, native
from brancher_amd import symbolic as sym
from brancher_amd.lowering import LoweringError, _Lowering
from brancher_amd.native import OUT_HEADER, BnnArgs, BnnDesc, BnnLayer
from brancher_amd.variables import RandomVariable, RootVariable

LIK_CATEGORICAL, LIK_BERNOULLI, LIK_NORMAL = 0, 1, 2
ACTIVATIONS = dict(tanh=1, relu=2, sigmoid=3, softplus=4,      # bsvi_bnn_activation (include/bsvi.h); relu6 is hardtanh(0, 6)
                   leaky_relu=5, elu=6, selu=7, softsign=8, hardtanh=9, relu6=9, silu=10, gelu=11)
# the kinds with parameters (bsvi_bnn_set_activation_params): name -> ((keyword, torch's default), ...) in torch's positional order, and
# what each must satisfy; PLAIN_KEYWORDS: the keywords the other new names take, with the one value that is served
ACTIVATION_PARAMS = dict(leaky_relu=(("negative_slope", 0.01),), elu=(("alpha", 1.0),), hardtanh=(("min_val", -1.0), ("max_val", 1.0)))
ACTIVATION_RULES = dict(leaky_relu=(lambda s: s > 0, "negative_slope > 0"), elu=(lambda a: a > 0, "alpha > 0"),
                        hardtanh=(lambda lo, hi: lo < hi, "min_val < max_val"))
PLAIN_KEYWORDS = dict(leaky_relu=dict(inplace=False), elu=dict(inplace=False), selu=dict(inplace=False), hardtanh=dict(inplace=False),
                      relu6=dict(inplace=False), silu=dict(inplace=False), gelu=dict(approximate="none"))
NO_BIAS = 0xFFFFFFFF
MAX_LAYERS = 8                                                         # BNN_MAX_LAYERS (csrc/bnn_kernel.inc)
MIDDLE_PATHS = ("mid_gen", "upper_gen", "upper_lds", "upper_mem")      # bsvi_bnn_select::BnnMiddle (csrc/bnn_select.h)
FIRST_LAYER_PATHS = ("per_sample", "shared")                           # bsvi_bnn_shared_first
PREDICT_PATHS = ("global", "lds")                                      # bsvi_bnn_predict_lds
# the families of the loc-scale regression likelihood (bsvi_bnn_set_likelihood_family): the name a refusal gives the observed variable
LIKELIHOOD_FAMILIES = {D.DIST_NORMAL: "Normal", D.DIST_LAPLACE: "Laplace", D.DIST_CAUCHY: "Cauchy"}
PRIOR_KINDS = {D.DIST_NORMAL: "normal", D.DIST_LAPLACE: "laplace", D.DIST_CAUCHY: "cauchy"}      # bsvi_bnn_set_row_priors (BSVI_DIST_*)
MAX_SCALE_LATENTS = 18                                                 # BNN_MAX_LATENTS: eight layers' weights and biases, two scale-head tensors
NO_LATENT = 0xFF                                                       # row_latent of a row whose prior scale is a constant or a learnable root


class BnnProgram:
    """What `lower_bnn` extracts from the graph."""
    estimator = "pathwise"
    family = D.DIST_NORMAL     # of a LIK_NORMAL program: D.DIST_NORMAL | DIST_LAPLACE | DIST_CAUCHY (the observed variable's distribution)
    scale_learnable = False
    scale_head = None          # (transform, a, b) of a scale head: sigma = a + b g(second head); the last layer then has 2 C rows
    # latent prior scales (a hierarchical prior; bsvi_bnn_set_scale_latents): [dict(name, tensors=[(tensor name, multiplier b)])] in the
    # order of their first tensor; then `row_latent` (a byte per row, NO_LATENT for none) and `latent_uniform` [4][T] (q loc, q scale,
    # prior loc, prior scale) exist, and the noise has a row per latent behind the weights' (n_noise = n_rows + T)
    scale_latents = ()
    # point estimates: `row_point` (a byte per row: 1 — the row is not random in the posterior, w = its q loc entry; bsvi_bnn_set_point_rows)
    # and `point` of every entry of `tensors`; entropy_weight is 0 when every row is a point (MAP)
    row_point = None

    def summary(self):
        s = dict(kind="bnn", layers=[(l["rows"], l["cols"], l["activation"]) for l in self.layers], n_rows=self.n_rows,
                 dataset_size=self.dataset_size, batch_size=self.batch_size, n_params=self.n_params,
                 likelihood=("categorical", "bernoulli", "normal")[self.likelihood], latents=[t["name"] for t in self.tensors])
        if self.likelihood == LIK_NORMAL:
            s["scale"] = "head" if self.scale_head else "learnable" if self.scale_learnable else "constant"
            if self.family != D.DIST_NORMAL:
                s["family"] = LIKELIHOOD_FAMILIES[self.family].lower()
        if any("activation_params" in l for l in self.layers):      # (a kind behind softplus: every hidden layer's function by name)
            s["activations"] = [activation_text(l) for l in self.layers[:-1]]
        s["priors"] = {t["name"]: t.get("prior", "normal") for t in self.tensors}
        if any(t.get("point") for t in self.tensors):
            s["point"] = [t["name"] for t in self.tensors if t["point"]]
        if self.scale_latents:
            s["scale_latents"] = {l["name"]: [(name, b) for name, b in l["tensors"]] for l in self.scale_latents}
        return s


def _is_random(v):
    return isinstance(v, RandomVariable) and getattr(v, "_type", None) != "Deterministic node"


def _activation(e):
    """the node between two layers -> (name, (p0, p1) of bsvi_bnn_set_activation_params | None for the four kinds without parameters), or
    the refusal: it names the function and the cause"""
    name = e.attr[0] if e.op == "call" and isinstance(e.attr[0], str) else None
    if name not in ACTIVATIONS:
        raise LoweringError("bnn path: between two layers stands one of BF.%s%s" % (" / BF.".join(ACTIVATIONS), " (not BF.%s)" % name if name else ""))
    kwargs = e.attr[1]
    if name not in PLAIN_KEYWORDS and name not in ACTIVATION_PARAMS:
        if len(e.args) != 1 or kwargs:
            raise LoweringError("bnn path: between two layers stands one of BF.%s (BF.%s takes the layer alone)" % (" / BF.".join(ACTIVATIONS), name))
        return name, (None if ACTIVATIONS[name] <= ACTIVATIONS["softplus"] else (0.0, 0.0))
    where = "bnn path: BF.%s between two layers: " % name
    plain = lambda x: x.attr if isinstance(x, sym.Expr) and x.op == "const" else x

    def number(x, what):
        v = plain(x)
        if isinstance(v, (sym.Expr, bool, np.bool_)) or not isinstance(v, numbers.Real):
            raise LoweringError(where + "%s is not a number (a parameter of an activation is a Python number: a variable or an array is not "
                                "served)" % what)
        return float(v)

    spec = ACTIVATION_PARAMS.get(name, ())
    if len(e.args) - 1 > len(spec):
        raise LoweringError(where + "%d positional arguments behind the layer (it takes %s)"
                            % (len(e.args) - 1, ", ".join(k for k, _ in spec) or "none"))
    values, given = [d for _, d in spec], set()
    for (k, _), a in zip(spec, e.args[1:]):
        values[len(given)] = number(a, k)
        given.add(k)
    for k, v in kwargs.items():
        if k in [s for s, _ in spec]:
            if k in given:
                raise LoweringError(where + "%s is given twice" % k)
            values[[s for s, _ in spec].index(k)] = number(v, k)
        elif k in PLAIN_KEYWORDS.get(name, {}):
            served, got = PLAIN_KEYWORDS[name][k], plain(v)
            if isinstance(got, sym.Expr) or type(got) is not type(served) or got != served:
                raise LoweringError(where + "%s=%r is not served (only %s=%r)" % (k, "an expression" if isinstance(got, sym.Expr) else got, k, served))
        else:
            raise LoweringError(where + "unknown keyword %r" % k)
    if name in ACTIVATION_RULES:
        holds, rule = ACTIVATION_RULES[name]
        with np.errstate(over="ignore"):      # (as the library receives them: single precision — 1e-50 is 0 there, 1e39 is inf)
            rounded = [float(np.float32(v)) for v in values]
        if not (all(np.isfinite(v) for v in rounded) and holds(*rounded)):
            raise LoweringError(where + "it needs finite parameters with %s in single precision (got %s)"
                                % (rule, ", ".join("%s=%g" % (k, v) for (k, _), v in zip(spec, values))))
    if name == "relu6":
        values = [0.0, 6.0]
    return name, tuple(values + [0.0] * (2 - len(values)))


def activation_text(layer):
    """`leaky_relu(negative_slope=0.2)`: a layer's activation as `summary()` shows it"""
    name = layer.get("activation_name") or {v: k for k, v in reversed(list(ACTIVATIONS.items()))}.get(layer["activation"], "none")
    spec = ACTIVATION_PARAMS.get("hardtanh" if name == "relu6" else name, ())
    if name == "relu6" or not spec:
        return name
    return "%s(%s)" % (name, ", ".join("%s=%g" % (k, v) for (k, _), v in zip(spec, layer["activation_params"])))


def _chain(e):
    """logits expression -> ([(W variable, bias variable | None, (name, parameters) of the layer's activation | None)] bottom up, x variable)"""
    def is_call(x, names):
        return x.op == "call" and isinstance(x.attr[0], str) and x.attr[0] in names

    def affine(x):
        if x.op == "add":
            a, b = x.args
            if is_call(a, ("matmul",)) and b.op == "var":
                return a, b.attr
            if is_call(b, ("matmul",)) and a.op == "var":
                return b, a.attr
            raise LoweringError("bnn path: a layer must be BF.matmul(weights, input) [+ bias]")
        if is_call(x, ("matmul",)):
            return x, None
        raise LoweringError("bnn path: a layer must be BF.matmul(weights, input) [+ bias]")

    mm, bias = affine(e)
    if len(mm.args) != 2 or mm.args[0].op != "var":
        raise LoweringError("bnn path: the first matmul operand must be the weight variable")
    W, inner = mm.args[0].attr, mm.args[1]
    if inner.op == "var":
        return [[W, bias, None]], inner.attr
    act = _activation(inner)
    below, x = _chain(inner.args[0])
    below[-1][2] = act
    return below + [[W, bias, None]], x


def _depends_on_latent(e):
    """does a link expression read a random variable (through deterministic nodes too)?"""
    if e.op == "var":
        v = e.attr
        if getattr(v, "_type", None) == "Deterministic node":
            return any(_depends_on_latent(x.expr) for x in v.link.expressions().values())
        return isinstance(v, RandomVariable)
    return any(_depends_on_latent(a) for a in e.args if hasattr(a, "op"))


def _random_variables(e):
    """the random variables a link expression reads (through deterministic nodes too), in the order met"""
    if e.op == "var":
        v = e.attr
        if getattr(v, "_type", None) == "Deterministic node":
            return [r for x in v.link.expressions().values() for r in _random_variables(x.expr)]
        return [v] if isinstance(v, RandomVariable) else []
    return [r for a in e.args if hasattr(a, "op") for r in _random_variables(a)]


def _latent_scale(v):
    """the prior scale of the tensor `v` when it reads a latent: b * tau -> (tau, b) — tau itself, b * tau, tau * b or tau / b with a
    number b > 0 —, or the refusal"""
    e = v.link.expressions()["scale"].expr
    taus = _random_variables(e)
    if len({id(t) for t in taus}) > 1:
        raise LoweringError("bnn path: the prior scale of %r is computed from two latent variables (%s): a tensor takes one scale latent"
                            % (v.name, ", ".join(repr(t.name) for t in taus)))
    number = lambda x: float(np.asarray(x.attr).reshape(-1)[0]) if x.op == "const" and np.size(x.attr) == 1 else None
    b = None
    if e.op == "var" and e.attr is taus[0]:
        b = 1.0
    elif e.op in ("mul", "truediv") and len(e.args) == 2:
        l, r = e.args
        if l.op == "var" and l.attr is taus[0] and number(r) is not None:
            b = number(r) if e.op == "mul" else (1.0 / number(r) if number(r) else None)
        elif e.op == "mul" and r.op == "var" and r.attr is taus[0] and number(l) is not None:
            b = number(l)
    if b is None or not (b > 0 and np.isfinite(b)):
        raise LoweringError("bnn path: the prior scale of %r must be its scale latent %r times a number b > 0 (tau, b * tau, tau * b or tau / b)"
                            % (v.name, taus[0].name))
    return taus[0], float(b)


LEARNABLE_SCALE_TRANSFORMS = ("softplus", "exp", "sigmoid")          # what keeps sigma off zero whatever a step does to its root


def _normal_scale(L, k, links, n_outputs, joint_roots=(), family="Normal"):
    """the scale of the Normal likelihood -> (first entry of the uniform table, stride, learnable): one for every output (stride 0) or
    one per output (stride 1); a constant (an entry among the table's constants), or a + b g(root) of a learnable root of the joint
    model with g one of softplus / exp / sigmoid, a >= 0, b > 0 (an entry with a gradient: bsvi_bnn_create_normal_learnable)"""
    e = links["scale"].expr
    m = L.match_uniform(L.from_expr(e, L.p_value))
    if m is None:
        raise LoweringError("bnn path: the scale of the %s likelihood %r must be a constant or a transform of one" % (family, k.name))
    leaf, g, a, b = m
    learnable = leaf.op == "root" and leaf.attr.learnable
    if learnable and (g not in LEARNABLE_SCALE_TRANSFORMS or not (a >= 0 and b > 0) or leaf.attr not in joint_roots):
        # (a bare root: a step can carry it through zero)
        raise LoweringError("bnn path: the scale of the %s likelihood %r is learnable (it must be a constant of the model, or "
                            "a + b * g(root) of a learnable root of the joint model with g one of %s, a >= 0 and b > 0)"
                            % (family, k.name, " / ".join(LEARNABLE_SCALE_TRANSFORMS)))
    size = int(np.prod(leaf.shape))
    shape = tuple(int(d) for d in leaf.shape)
    if size != 1 and (size != n_outputs or shape[-1] != 1):
        raise LoweringError("bnn path: the scale of the %s likelihood %r has shape %r: neither one value nor one per output [%d, 1]"
                            % (family, k.name, shape[1:], n_outputs))
    is_param, k0 = L.uniform_entries(leaf, g, a, b)
    return k0, (1 if size > 1 else 0), bool(is_param)


def _has_matmul(e):
    return (e.op == "call" and e.attr[0] == "matmul") or any(_has_matmul(a) for a in e.args if hasattr(a, "op"))


def _scale_head(k, e, family="Normal"):
    """the scale of a Normal likelihood computed from a matmul: a + b g(second head) -> (g, a, b, the head's chain, its x), or the cause"""
    def number(x):
        return float(np.asarray(x.attr).reshape(-1)[0]) if x.op == "const" and np.size(x.attr) == 1 else None

    def peel(x):      # x == a + b * core with numbers a, b -> (core, a, b)
        if x.op in ("add", "sub", "mul", "truediv"):
            l, r = x.args
            cl, cr = number(l), number(r)
            if cl is not None and cr is None and x.op != "truediv":
                core, a, b = peel(r)
                return dict(add=(core, cl + a, b), sub=(core, cl - a, -b), mul=(core, cl * a, cl * b))[x.op]
            if cr is not None and cl is None and (x.op != "truediv" or cr != 0.0):
                core, a, b = peel(l)
                return dict(add=(core, a + cr, b), sub=(core, a - cr, b), mul=(core, a * cr, b * cr), truediv=(core, a / (cr or 1.), b / (cr or 1.)))[x.op]
        return x, 0.0, 1.0

    form = "a + b * g(BF.matmul(weights, hidden) [+ bias]) with g one of %s, a >= 0 and b > 0" % " / ".join(LEARNABLE_SCALE_TRANSFORMS)
    core, a, b = peel(e)
    if core.op != "call" or core.attr[0] not in LEARNABLE_SCALE_TRANSFORMS or len(core.args) != 1 or core.attr[1]:
        what = "BF.%s" % core.attr[0] if core.op == "call" and isinstance(core.attr[0], str) else "the operation %r" % core.op
        try:      # (the bare head)
            _chain(core)
            what = "missing"
        except LoweringError:
            pass
        raise LoweringError("bnn path: the transform of the scale head of the %s likelihood %r is %s (the scale must be %s)" % (family, k.name, what, form))
    if not (a >= 0 and b > 0):
        raise LoweringError("bnn path: the scale head of the %s likelihood %r has a = %g, b = %g (the scale must be %s)" % (family, k.name, a, b, form))
    try:
        chain, x_var = _chain(core.args[0])
    except LoweringError as err:
        raise LoweringError("bnn path: the scale head of the %s likelihood %r is not a chain of matmul layers (%s)" % (family, k.name, err)) from None
    return core.attr[0], float(a), float(b), chain, x_var


def lower_bnn(joint, posterior, estimator="pathwise"):
    # "taylor1" (gradient_estimators.py:47-56): f at the posterior's analytic means — every latent of the network is a mean-field Normal,
    # whose mean is its loc (distributions.py:137 through torch), so the program is the Pathwise one evaluated on the draw eps = 0
    # (CompiledBnn supplies it); the entropy of a Normal does not depend on the draw.  The reference tiles the means to number_samples
    # identical rows and averages: kept (N identical samples), so that the value rounds as the reference's does.
    if estimator not in ("pathwise", "blackbox", "taylor1"):
        raise LoweringError("the bnn path implements the Pathwise, BlackBox and Taylor1 estimators")
    L = _Lowering(joint, posterior, estimator)
    q_flat = posterior._flatten()
    L.q_by_name = {v.name: v for v in q_flat}
    L.q_roots = {v for v in posterior.variables if isinstance(v, RootVariable)}
    for v in sorted(L.q_roots, key=lambda v: v.name):
        if v.learnable:
            L.param_offset(v.parameter, 0)
    joint_roots = [v for v in joint.flatten() if isinstance(v, RootVariable)]
    for v in sorted(joint_roots, key=lambda v: v.name):
        if v.learnable:
            L.param_offset(v.parameter, 1)
    q_random = [v for v in q_flat if _is_random(v)]
    # (a regression model whose noise scale is a latent is named as such, before the posterior of that latent is looked at)
    for v in joint._flatten():
        if _is_random(v) and v.distribution.kind in LIKELIHOOD_FAMILIES and v.is_observed and getattr(v, "has_random_dataset", False) \
                and _depends_on_latent(v.link.expressions()["scale"].expr) and not _has_matmul(v.link.expressions()["scale"].expr):
            # (a scale computed from a matmul is a scale head, or refused below with its own cause)
            raise LoweringError("bnn path: the scale of the %s likelihood %r is a latent variable or computed from one "
                                "(it must be a constant of the model)" % (LIKELIHOOD_FAMILIES[v.distribution.kind], v.name))
    p_random = [v for v in joint._flatten() if _is_random(v)]
    # latent prior scales: the latents that the prior scale of an unobserved Normal / Laplace / Cauchy variable reads.  Their posterior is a
    # LogNormal of the same name, not one of the weights' Normals: by name they stand outside the checks of the weights' posterior
    scale_vars = []
    for v in p_random:
        if v.distribution.kind in PRIOR_KINDS and not v.is_observed:
            for t in _random_variables(v.link.expressions()["scale"].expr):
                if all(t is not o for o in scale_vars):
                    scale_vars.append(t)
    scale_names = {t.name for t in scale_vars}
    q_weights = [v for v in q_random if v.name not in scale_names]
    for v in q_weights:
        if v.distribution.kind != D.DIST_NORMAL:
            raise LoweringError("bnn path: the posterior must be mean-field Normal variables (or RootVariables named like the network's "
                                "tensors: point estimates): %r is %s" % (v.name, type(v.distribution).__name__.replace("Distribution", "")))
    # the likelihood: a Categorical / Binomial(1) over logits, or — regression — an OBSERVED Normal, Laplace or Cauchy whose loc is the chain
    liks = [v for v in p_random if v.distribution.kind in (D.DIST_CATEGORICAL, D.DIST_BINOMIAL, D.DIST_BERNOULLI)
            or (v.distribution.kind in LIKELIHOOD_FAMILIES and v.is_observed)]
    if len(liks) != 1:
        raise LoweringError("bnn path: expected one matmul likelihood")
    k = liks[0]
    normal = k.distribution.kind in LIKELIHOOD_FAMILIES      # (LIK_NORMAL: the loc-scale regression likelihood, whatever its family)
    family = LIKELIHOOD_FAMILIES.get(k.distribution.kind)
    if not k.is_observed or not k.has_random_dataset:
        raise LoweringError("bnn path: the likelihood must be observed through an EmpiricalVariable of labels")
    links = k.link.expressions()
    if normal:
        try:
            chain, x_var = _chain(links["loc"].expr)
        except LoweringError as err:
            raise LoweringError("bnn path: the loc of the %s likelihood %r is not a chain of matmul layers (%s)" % (family, k.name, err)) from None
    else:
        if "logits" not in links:
            raise LoweringError("bnn path: the likelihood must be parameterised by logits")
        chain, x_var = _chain(links["logits"].expr)
    if len(chain) > MAX_LAYERS:
        raise LoweringError("bnn path: the network has %d layers, the kernels serve at most %d" % (len(chain), MAX_LAYERS))
    # a scale head: sigma = a + b g(BF.matmul(weights_scale, H) [+ b_scale]) on the trunk H of the loc head
    head = None
    if normal and _depends_on_latent(links["scale"].expr):
        g, ha, hb, chain_s, x_s = _scale_head(k, links["scale"].expr, family)
        same = len(chain_s) == len(chain) and x_s is x_var and all(
            ls[0] is ll[0] and ls[1] is ll[1] and ls[2] == ll[2] for ls, ll in zip(chain_s[:-1], chain[:-1]))
        if not same:
            raise LoweringError("bnn path: the two heads of the %s likelihood %r stand on different trunks (both must be "
                                "BF.matmul(weights, H) [+ bias] on the same H: the same x, the same latent variables and activations)" % (family, k.name))
        Ws, bs = chain_s[-1][0], chain_s[-1][1]
        if (bs is None) != (chain[-1][1] is None):
            raise LoweringError("bnn path: one head of the %s likelihood %r has a bias and the other has none (either both or neither)" % (family, k.name))
        head = (g, ha, hb, Ws, bs)
    latents = []
    for W, b, _ in chain:
        latents.append(W)
        if b is not None:
            latents.append(b)
    if head:
        head_vars = [v for v in (chain[-1][0], chain[-1][1], head[3], head[4]) if v is not None]
        trunk_names = [v.name for v in latents[:len(latents) - (2 if chain[-1][1] is not None else 1)]]
        for v in head_vars:
            if v.name in trunk_names or sum(1 for o in head_vars if o.name == v.name) > 1:
                raise LoweringError("bnn path: the head tensor %r of the %s likelihood %r is used twice (in the trunk, or by both heads)"
                                    % (v.name, family, k.name))
        latents += [v for v in (head[3], head[4]) if v is not None]
    names = [v.name for v in latents]
    if len(set(names)) != len(names):
        raise LoweringError("bnn path: a latent tensor is used by two layers")
    # point estimates (inference.py:251-275, by name as everywhere): a RootVariable of the posterior model that carries the name of a
    # network tensor makes that tensor a point — w = the root's value for every sample, no entropy and no log q (the reference gives a
    # root the log-probability 0), its prior as before; learnable=False: a frozen tensor, a constant entry.  Every tensor a point: MAP
    q_point = {v.name: v for v in q_flat if isinstance(v, RootVariable) and v.name in names}
    read_by_q = {id(a) for v in q_random for a in v.ancestors}
    for v in q_flat:
        if isinstance(v, RootVariable) and v.name in scale_names:
            raise LoweringError("bnn path: the posterior member %r is a RootVariable named like a scale latent: the posterior of a scale "
                                "latent must be a LogNormal variable (a point estimate of a prior scale is not implemented)" % v.name)
    for v in getattr(posterior, "_input_variables", ()):
        if isinstance(v, RootVariable) and v.name not in names and id(v) not in read_by_q:
            raise LoweringError("bnn path: the posterior member %r is neither a Normal variable nor a RootVariable named like a tensor of "
                                "the network (%s)" % (v.name, ", ".join(names)))
    for v in q_weights:
        if v.name in q_point:
            raise LoweringError("bnn path: the posterior holds a RootVariable and a random variable both named %r" % v.name)
    if not q_weights and not q_point:
        raise LoweringError("bnn path: the posterior must be mean-field Normal variables")
    # latent prior scales of the network's tensors: tensor -> (latent, multiplier); every refusal names the variable and the cause
    scale_of, taus = {}, []
    for v in latents:
        if _is_random(v) and v.distribution.kind in PRIOR_KINDS and _random_variables(v.link.expressions()["scale"].expr):
            tau, b = _latent_scale(v)
            scale_of[v.name] = (tau, b)
            if all(tau is not o for o in taus):
                taus.append(tau)
    for name in q_point:
        if name in scale_of:
            raise LoweringError("bnn path: the point tensor %r has a prior scale that reads the scale latent %r (a point estimate under a "
                                "latent prior scale is not implemented: give the tensor a Normal posterior or a constant prior scale)"
                                % (name, scale_of[name][0].name))
    for tau in taus:
        q_tau = L.q_by_name.get(tau.name)
        if tau.distribution.kind != D.DIST_LOGNORMAL:
            raise LoweringError("bnn path: the scale latent %r must be a LogNormal variable: it is %s"
                                % (tau.name, type(tau.distribution).__name__.replace("Distribution", "")))
        if q_tau is None or not _is_random(q_tau) or q_tau.distribution.kind != D.DIST_LOGNORMAL:
            raise LoweringError("bnn path: the posterior of the scale latent %r must be a LogNormal variable of the same name: it is %s"
                                % (tau.name, "missing" if q_tau is None else type(getattr(q_tau, "distribution", None)).__name__.replace("Distribution", "")))
        if any(t.name == tau.name for t in latents):
            raise LoweringError("bnn path: the scale latent %r is also a tensor of the network" % tau.name)
        for var, where in ((tau, "prior"), (q_tau, "posterior")):
            if any(_random_variables(x.expr) for x in var.link.expressions().values()):
                raise LoweringError("bnn path: the %s of the scale latent %r depends on another latent variable (its loc and scale must be "
                                    "constants or parameter transforms)" % (where, tau.name))
    if taus and estimator == "taylor1":
        raise LoweringError("bnn path: the Taylor1 estimator does not serve a model with scale latents (%s): the mean of a LogNormal is "
                            "exp(m + s^2 / 2), not the value at the zero draw the estimator is evaluated on" % ", ".join(repr(t.name) for t in taus))
    if len(taus) > MAX_SCALE_LATENTS:
        raise LoweringError("bnn path: the model has %d scale latents, the kernels serve at most %d" % (len(taus), MAX_SCALE_LATENTS))
    others = [v for v in p_random if v is not k and v not in latents and v.distribution.kind != D.DIST_EMPIRICAL
              and all(v is not t for t in taus)]
    if others or sorted(names + [t.name for t in taus]) != sorted([v.name for v in q_random] + list(q_point)):
        raise LoweringError("bnn path: every latent of the network needs a Normal posterior of the same name, and nothing else may be latent")
    for v in latents:
        # (loc / scale families on the whole real line: a Normal posterior covers their support — LogNormal, Beta and the rest do not)
        if not _is_random(v) or v.distribution.kind not in PRIOR_KINDS:
            raise LoweringError("bnn path: weights and biases must be Normal, Laplace or Cauchy variables: the prior of %r is %s"
                                % (v.name, type(getattr(v, "distribution", None)).__name__.replace("Distribution", "") or "no distribution"))
    labels_var = k.dataset

    def minibatch_source(v, what):
        if getattr(v, "_type", None) != "Empirical" or not v.is_observed:
            raise LoweringError("bnn path: %s must be an observed EmpiricalVariable" % what)
        exprs = v.link.expressions()
        ds = exprs["dataset"].expr
        if ds.op != "var" or not isinstance(ds.attr, RootVariable) or "indices" not in exprs:
            raise LoweringError("bnn path: %s must index an array dataset through a RandomIndices variable" % what)
        ind = exprs["indices"].expr
        from brancher_amd.standard_variables import RandomIndices
        if ind.op != "var" or not isinstance(ind.attr, RandomIndices):
            raise LoweringError("bnn path: %s must be indexed by a RandomIndices variable" % what)
        return np.asarray(ds.attr.value, dtype=np.float32), ind.attr

    X, ind_x = minibatch_source(x_var, "x")
    Y, ind_y = minibatch_source(labels_var, "labels")
    if ind_x is not ind_y:
        raise LoweringError("bnn path: x and labels must share one RandomIndices variable")
    DS = X.shape[1]
    # labels: one per row; targets of the Normal likelihood: one per row and output, [DS][C] row-major
    if normal and (Y.ndim < 2 or Y.shape[1] != DS):
        raise LoweringError("bnn path: dataset sizes of x and labels differ")
    Xm, Ym = X.reshape(DS, -1), (Y.reshape(DS, -1) if normal else Y.reshape(-1))
    if Ym.shape[0] != DS:
        raise LoweringError("bnn path: dataset sizes of x and labels differ")
    P = Xm.shape[1]
    if P % 4:
        raise LoweringError("bnn path: the number of features must be a multiple of 4")

    def row_params(var, ctx, scale=None):
        # (scale: the multiplier b of a tensor under a scale latent — a constant in the place of its prior scale)
        nodes = L.node_params(var, ctx) if scale is None else [
            L.from_expr(var.link.expressions()["loc"].expr, ctx), L.mk("carr", (), np.full((1,), scale, dtype=np.float32), (1, 1, 1))]
        out = []
        for node in nodes:
            m = L.match_uniform(node)
            if m is None:
                raise LoweringError("bnn path: the parameters of %r must be constants or parameter transforms" % var.name)
            leaf, g, a, b = m
            is_param, k0 = L.uniform_entries(leaf, g, a, b)
            out.append((is_param, k0, int(np.prod(leaf.shape)), leaf.shape))
        return out

    # the latent vector: weights1 first (bsvi_bnn_desc), then the other tensors layer by layer
    order = [chain[0][0]] + ([chain[0][1]] if chain[0][1] is not None else [])
    for W, b, _ in chain[1:]:
        order += [W] + ([b] if b is not None else [])
    if head:
        # to the library the two heads are ONE last layer of 2 C rows: weights_loc | weights_scale a row-major [2 C, cols] block of the
        # latent vector, b_loc | b_scale the column behind it
        Wl, bl = chain[-1][0], chain[-1][1]
        order = [v for v in order if v is not Wl and v is not bl] + [Wl, head[3]] + ([bl, head[4]] if bl is not None else [])
    tensors, row0, entries = [], 0, []
    for v in order:
        pl, ps = row_params(v, L.p_value, scale_of[v.name][1] if v.name in scale_of else None)
        if v.name in q_point:
            # the q loc is the root's own entries (identity; parameters if it is learnable, else constants), the q scale the constant 0
            # (as lower_dense): never read as a scale — `row_point` tells the kernels
            root = q_point[v.name]      # (its value is stored behind the sample and datapoint axes, as every root's)
            raw = tuple(int(d) for d in np.shape(root.parameter.numpy() if root.learnable else root.value))[2:]
            if len(raw) != 2:
                raise LoweringError("bnn path: the RootVariable %r has shape %r: the value of a tensor is a matrix [rows, cols] or a column "
                                    "[rows, 1]" % (v.name, raw))
            leaf = L.q_value(q_point[v.name])
            is_param, k0 = L.uniform_entries(leaf, "identity", 0.0, 1.0)
            ql = (is_param, k0, int(np.prod(leaf.shape)), leaf.shape)
            _, z0 = L.const_operand(0.0)
            qs = (False, z0, 1, (1, 1, 1))
            for ent in (pl, ps):
                if ent[2] > 1 and tuple(int(d) for d in ent[3]) != tuple(int(d) for d in leaf.shape):
                    raise LoweringError("bnn path: the RootVariable %r has shape %r but the tensor it names is %r"
                                        % (v.name, tuple(int(d) for d in leaf.shape[1:]), tuple(int(d) for d in ent[3][1:])))
        else:
            ql, qs = row_params(L.q_by_name[v.name], L.q_value)
        shape = tuple(int(s) for s in ql[3])
        if len(shape) != 3 or shape[0] != 1:
            raise LoweringError("bnn path: %r must be a matrix [rows, cols] or a column [rows, 1]" % v.name)
        size = shape[1] * shape[2]
        for ent in (ql, qs, pl, ps):
            if ent[2] not in (1, size):
                raise LoweringError("bnn path: a parameter of %r has an unsupported shape" % v.name)
        tensors.append(dict(name=v.name, row0=row0, rows=shape[1], cols=shape[2], size=size, prior=PRIOR_KINDS[v.distribution.kind],
                            point=v.name in q_point))
        entries.append((ql, qs, pl, ps))
        row0 += size
    R = row0
    by_name = {t["name"]: t for t in tensors}
    layers, width = [], P
    for W, b, act in chain:
        t = by_name[W.name]
        if t["cols"] != width:
            raise LoweringError("bnn path: %r is [%d, %d] but its input has %d rows" % (W.name, t["rows"], t["cols"], width))
        bias0 = NO_BIAS
        if b is not None:
            tb = by_name[b.name]
            if (tb["rows"], tb["cols"]) != (t["rows"], 1):
                raise LoweringError("bnn path: bias %r must be a column [%d, 1]" % (b.name, t["rows"]))
            bias0 = tb["row0"]
        layers.append(dict(rows=t["rows"], cols=t["cols"], weight_row0=t["row0"], bias_row0=bias0,
                           activation=ACTIVATIONS[act[0]] if act else 0, weights=W.name, bias=b.name if b is not None else None))
        if act and act[1] is not None:      # (one of the kinds behind softplus: the layers of the four old kinds are what they were)
            layers[-1].update(activation_name=act[0], activation_params=act[1])
        width = t["rows"]
    if head:
        ts, last = by_name[head[3].name], layers[-1]
        if ts["cols"] != last["cols"]:
            raise LoweringError("bnn path: %r is [%d, %d] but its input has %d rows" % (ts["name"], ts["rows"], ts["cols"], last["cols"]))
        if head[4] is not None and (by_name[head[4].name]["rows"], by_name[head[4].name]["cols"]) != (ts["rows"], 1):
            raise LoweringError("bnn path: bias %r must be a column [%d, 1]" % (head[4].name, ts["rows"]))
        if Ym.shape[1] != width or ts["rows"] != width:
            raise LoweringError("bnn path: the targets have %d columns but the heads of the %s likelihood %r have %d (loc) and %d (scale) "
                                "rows" % (Ym.shape[1], family, k.name, width, ts["rows"]))
        last.update(weights_scale=ts["name"], bias_scale=head[4].name if head[4] is not None else None)
    lik = LIK_NORMAL if normal else LIK_CATEGORICAL if k.distribution.kind == D.DIST_CATEGORICAL else LIK_BERNOULLI
    scale_entries = None
    if normal:
        if Ym.shape[1] != width:
            raise LoweringError("bnn path: the targets have %d columns but the last layer has %d rows" % (Ym.shape[1], width))
        if head:
            layers[-1]["rows"] = 2 * width
        else:
            scale_entries = _normal_scale(L, k, links, width, joint_roots, family)
    if lik == LIK_BERNOULLI:
        if width != 1:
            raise LoweringError("bnn path: a Bernoulli/Binomial likelihood needs a single output")
        if k.distribution.kind == D.DIST_BINOMIAL:
            tc = L.match_uniform(L.from_expr(links["total_count"].expr, L.p_value))
            if tc is None or tc[0].op != "root" or float(np.asarray(tc[0].attr.value).reshape(-1)[0]) != 1.0:
                raise LoweringError("bnn path: Binomial likelihood supports total_count = 1 only")

    # the scale latents' own parameters: one value each, constants or parameter transforms
    latent_entries = []
    for tau in taus:
        ents = row_params(L.q_by_name[tau.name], L.q_value) + row_params(tau, L.p_value)
        for ent in ents:
            if ent[2] != 1:
                raise LoweringError("bnn path: the scale latent %r has %d values (a scale latent is one value: one scale for a whole tensor)"
                                    % (tau.name, max(e[2] for e in ents)))
        latent_entries.append(ents)
    uni, n_up = L.uniform_table()
    prog = BnnProgram()
    prog.estimator = estimator
    L.fill_parameter_tables(prog, uni, n_up)
    row_uniform = np.zeros((4, R), dtype=np.uint32)
    for t, ents in zip(tensors, entries):
        for q, (is_param, k0, size, _) in enumerate(ents):
            base = k0 if is_param else n_up + k0
            row_uniform[q, t["row0"]:t["row0"] + t["size"]] = base + (np.arange(t["size"]) if size > 1 else 0)
    prog.uniform = uni
    prog.consts = np.concatenate(L.consts) if L.consts else np.zeros(0, np.float32)
    prog.row_uniform = row_uniform
    # the prior of every row (bsvi_bnn_set_row_priors): one kind per tensor
    kind_of = {name: kind for kind, name in PRIOR_KINDS.items()}
    prog.row_prior = np.concatenate([np.full(t["size"], kind_of[t["prior"]], dtype=np.uint8) for t in tensors])
    # point-estimated rows (bsvi_bnn_set_point_rows): one byte per row
    prog.row_point = np.concatenate([np.full(t["size"], 1 if t["point"] else 0, dtype=np.uint8) for t in tensors])
    prog.layers, prog.tensors, prog.n_rows = layers, tensors, R
    prog.n_features, prog.n_classes, prog.dataset_size, prog.batch_size = P, width, DS, int(ind_x.batch_size)
    prog.likelihood = lik
    if normal:
        prog.family = k.distribution.kind
    if head:
        prog.scale_head = head[:3]
    elif normal:
        # (constants stand behind the entries with a gradient in the uniform table; a learnable scale is one of those)
        prog.scale_learnable = scale_entries[2]
        prog.scale_uniform, prog.scale_stride = (0 if prog.scale_learnable else n_up) + scale_entries[0], scale_entries[1]
    prog.dataset = np.ascontiguousarray(Xm, dtype=np.float32)
    prog.labels = np.ascontiguousarray(Ym, dtype=np.float32)
    prog.indices_name = ind_x.name
    prog.x_name, prog.likelihood_name = x_var.name, k.name       # (engine.posterior_sample: the variables a prediction is keyed by)
    # (every row a point: the loss is -log p(theta, minibatch), inference.MAP)
    prog.lik_weight, prog.prior_weight, prog.entropy_weight = 1.0, 1.0, (0.0 if prog.row_point.all() else 1.0)
    prog.n_noise = R
    if taus:
        index = {t.name: i for i, t in enumerate(taus)}
        prog.scale_latents = [dict(name=t.name, tensors=[(x["name"], scale_of[x["name"]][1]) for x in tensors
                                                         if x["name"] in scale_of and scale_of[x["name"]][0] is t]) for t in taus]
        prog.row_latent = np.concatenate([np.full(x["size"], index[scale_of[x["name"]][0].name] if x["name"] in scale_of else NO_LATENT,
                                                  dtype=np.uint8) for x in tensors])
        prog.latent_uniform = np.array([[k0 if is_param else n_up + k0 for is_param, k0, _, _ in ents] for ents in latent_entries],
                                       dtype=np.uint32).T.copy()
        prog.n_noise = R + len(taus)
    prog.bmax = 1
    return prog


def row_parameters(p, theta=None):
    """(q loc [R], q scale [R]) of a lowered program at the flat parameter values `theta` (default: the values the program was lowered
    with) — the uniform table evaluated on the host, in double precision: what `bnn_head_body` leaves in `rowp` on the device"""
    if theta is None:
        theta = np.zeros(max(p.n_params, 1), dtype=np.float64)
        for par, off, size, _ in p.parameters:
            theta[off:off + size] = par.numpy().reshape(-1)
    theta = np.asarray(theta, dtype=np.float64)
    UT = lowering.UT
    g = {UT["identity"]: lambda x: x, UT["softplus"]: lambda x: np.where(x > 20.0, x, np.log1p(np.exp(np.minimum(x, 20.0)))),
         UT["sigmoid"]: lambda x: 1.0 / (1.0 + np.exp(-x)), UT["exp"]: np.exp, UT["log"]: np.log, UT["tanh"]: np.tanh,
         UT["sqrt"]: np.sqrt, UT["square"]: np.square}
    uni = p.uniform
    x = np.where(uni["is_param"] != 0, theta[np.minimum(uni["src"], theta.size - 1)],
                 np.asarray(p.consts, dtype=np.float64)[np.minimum(uni["src"], max(len(p.consts), 1) - 1)] if len(p.consts) else 0.0)
    values = np.empty(len(uni), dtype=np.float64)
    for t in np.unique(uni["transform"]):
        sel = uni["transform"] == t
        values[sel] = g[int(t)](x[sel])
    values = uni["a"].astype(np.float64) + uni["b"].astype(np.float64) * values
    return values[p.row_uniform[0]], values[p.row_uniform[1]]


def make_desc(p):
    """bsvi_bnn_desc of a lowered program -> (desc, the arrays it points into: keep them alive as long as the desc)"""
    layers = (BnnLayer * len(p.layers))(*[BnnLayer(rows=l["rows"], cols=l["cols"], weight_row0=l["weight_row0"],
                                                    bias_row0=l["bias_row0"], activation=l["activation"]) for l in p.layers])
    k = dict(uniform=np.ascontiguousarray(p.uniform), consts=np.ascontiguousarray(p.consts, dtype=np.float32),
             ptr=np.ascontiguousarray(p.param_uniform_ptr, dtype=np.uint32),
             idx=np.ascontiguousarray(p.param_uniform_idx, dtype=np.uint32),
             rows=np.ascontiguousarray(p.row_uniform, dtype=np.uint32), dataset=p.dataset, labels=p.labels, layers=layers)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None
    d = BnnDesc(abi_version=native.ABI_VERSION, n_params=p.n_params, n_consts=k["consts"].size, n_uniform=len(k["uniform"]),
                n_uniform_grad=p.n_uniform_grad, n_layers=len(p.layers), n_rows=p.n_rows, n_features=p.n_features,
                dataset_size=p.dataset_size, batch_size=p.batch_size, likelihood=p.likelihood,
                estimator=lowering.EST[getattr(p, "estimator", "pathwise")], lik_weight=p.lik_weight,
                prior_weight=p.prior_weight, entropy_weight=p.entropy_weight, layers=C.cast(layers, C.c_void_p),
                row_uniform=ptr(k["rows"]), uniform=ptr(k["uniform"]), consts=ptr(k["consts"]),
                param_uniform_ptr=ptr(k["ptr"]), param_uniform_idx=ptr(k["idx"]), dataset=ptr(k["dataset"]), labels=ptr(k["labels"]))
    return d, k


class CompiledBnn:
    """Engine for a Bayesian neural network; same surface as dense.CompiledDense."""

    def data_path(self):
        """which matrix-core path serves the two products with the minibatch: "bf16x3" when every dataset value is exactly a
        bf16 number (three bf16 MFMAs on the exact pieces of the f32 operand), else "f32" (the f32-input MFMA kernels)"""
        return "bf16x3" if self._exact_data else "f32"

    def middle_path(self):
        """which kernel serves the upper layers, the likelihood and the reverse sweep of the next launch (csrc/bnn_select.h, from the
        network's size and BSVI_BNN_MID / BSVI_BNN_JIT as they stand at the first launch or call of this): "mid_gen" and "upper_gen"
        are generated for the network (compiled here if no launch has yet; one that does not compile reports what serves instead),
        "upper_lds" and "upper_mem" the static kernel with its activations in LDS or in global memory"""
        kind = int(self.lib.bsvi_bnn_middle(self.handle))
        if not 0 <= kind < len(MIDDLE_PATHS):
            raise native.NativeError("bsvi_bnn_middle returned %d" % kind)
        return MIDDLE_PATHS[kind]

    def first_layer_path(self):
        """how the two products with the minibatch are taken (csrc/bnn_select.h, shared_first: from the point rows and BSVI_BNN_SHARED1
        as they stand at the first launch or call of this): "shared" — weights1 is a point estimate, the same matrix for every sample, so
        the first product is taken once and the second after the sum over the samples — or "per_sample" (both products per sample, as for any network)"""
        kind = int(self.lib.bsvi_bnn_shared_first(self.handle))
        if kind not in (0, 1):
            raise native.NativeError("bsvi_bnn_shared_first returned %d" % kind)
        return FIRST_LAYER_PATHS[kind]

    def __init__(self, joint_model, posterior_model, estimator="pathwise", device=None, program=None):
        from brancher_amd import engine
        self.device = device or engine._device()
        self.program = program if program is not None else lower_bnn(joint_model, posterior_model, estimator)
        p = self.program
        lib = native.load()
        if lib.bsvi_device_count() < 1:
            raise native.NativeError("no MI355X / HIP device visible: the engine cannot run (no CPU fallback)")
        self.lib = lib
        d, self._keep = make_desc(p)
        handle = C.c_void_p()
        if p.likelihood == LIK_NORMAL and getattr(p, "scale_head", None):
            g, a, b = p.scale_head
            native.check(lib.bsvi_bnn_create_normal_heads(C.byref(d), lowering.UT[g], a, b, C.byref(handle)))
        elif p.likelihood == LIK_NORMAL:
            create = lib.bsvi_bnn_create_normal_learnable if getattr(p, "scale_learnable", False) else lib.bsvi_bnn_create_normal
            native.check(create(C.byref(d), p.scale_uniform, p.scale_stride, C.byref(handle)))
        else:
            native.check(lib.bsvi_bnn_create(C.byref(d), C.byref(handle)))
        self.handle = handle
        if p.likelihood == LIK_NORMAL and getattr(p, "family", D.DIST_NORMAL) != D.DIST_NORMAL:      # (without the call the family is Normal)
            native.check(lib.bsvi_bnn_set_likelihood_family(handle, int(p.family)))
        row_prior = np.ascontiguousarray(getattr(p, "row_prior", np.zeros(0)), dtype=np.uint8)
        if (row_prior != D.DIST_NORMAL).any():             # (without the call every row is Normal)
            native.check(lib.bsvi_bnn_set_row_priors(handle, row_prior.ctypes.data_as(C.c_void_p), row_prior.size))
        if getattr(p, "scale_latents", None):              # (without the call no prior scale is latent)
            row_latent = np.ascontiguousarray(p.row_latent, dtype=np.uint8)
            self._keep["latent_uniform"] = lu = np.ascontiguousarray(p.latent_uniform, dtype=np.uint32)
            native.check(lib.bsvi_bnn_set_scale_latents(handle, len(p.scale_latents), row_latent.ctypes.data_as(C.c_void_p), row_latent.size,
                                                        lu.ctypes.data_as(C.c_void_p)))
        row_point = getattr(p, "row_point", None)
        if row_point is not None and np.any(row_point):    # (without the call no row is a point)
            row_point = np.ascontiguousarray(row_point, dtype=np.uint8)
            native.check(lib.bsvi_bnn_set_point_rows(handle, row_point.ctypes.data_as(C.c_void_p), row_point.size))
        if any("activation_params" in l for l in p.layers):      # (without the call torch's defaults hold; a model of the four old kinds makes none)
            act_p = np.ascontiguousarray([l.get("activation_params", (0.0, 0.0)) for l in p.layers], dtype=np.float32)
            native.check(lib.bsvi_bnn_set_activation_params(handle, act_p.ctypes.data_as(C.c_void_p), len(p.layers)))
        self._exact_data = bool(lib.bsvi_bnn_exact_data(handle))
        dev = self.device
        self.n_params = p.n_params
        theta = np.zeros(p.n_params, dtype=np.float32)
        for par, off, size, _ in p.parameters:
            theta[off:off + size] = par.numpy().reshape(-1)
        self.params = _engine.broadcast_from_rank0(torch.from_numpy(theta).to(dev))
        self.out = torch.zeros(OUT_HEADER + max(p.n_params, 1), device=dev)
        active = np.ascontiguousarray(p.param_active, dtype=np.uint8)
        group = p.param_group
        first_group = 0 if np.any(active[group == 0]) else 1
        self.mask_all = torch.from_numpy(active.copy()).to(dev)
        self.mask_first = torch.from_numpy((active * (group == first_group)).astype(np.uint8)).to(dev)
        self._workspaces = {}
        self.iteration = 0
        self.grads_valid = False
        self.last_mode = None
        for par, off, size, _ in p.parameters:
            par.bind(self, off)

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                self.lib.bsvi_bnn_destroy(self.handle)
                self.handle = None
        except Exception:
            pass

    # ParameterStore protocol
    def read_params(self, offset, size):
        return self.params[offset:offset + size].detach().cpu().numpy()

    def write_params(self, offset, values):
        self.params[offset:offset + values.size] = torch.from_numpy(np.ascontiguousarray(values)).to(self.device)

    def read_grads(self, offset, size):
        if not self.grads_valid:
            return None
        o = OUT_HEADER + offset
        return self.out[o:o + size].detach().cpu().numpy()

    def workspace(self, n_local):
        ws = self._workspaces.get(n_local)
        if ws is None:
            # (zeroed once: the pad columns of the product operands are never written)
            ws = torch.zeros(int(self.lib.bsvi_bnn_workspace_bytes(self.handle, n_local)), dtype=torch.uint8, device=self.device)
            self._workspaces[n_local] = ws
        return ws

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _args(self, n_local, n_global, base, noise=None, indices=None, seed=None, offset=0, noise_out=None,
              indices_out=None, fvalue_out=None, logq_out=None, f_weight=None, q_weight=None):
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        if getattr(self.program, "estimator", "pathwise") == "taylor1":
            # f at the posterior's means: the draw eps = 0, whatever was drawn (the reference draws too and reads the means:
            # gradient_estimators.py:50-55) — a caller's noise (parity tests replay the reference's) is not read
            noise = self._zero_noise(n_local)
        if not isinstance(seed, int) or seed is True:      # (train() resolves the call's seed ONCE and hands the integer down)
            seed = _engine.shared_seed(seed, self.device)
        return BnnArgs(params_dev=ptr(self.params), noise_dev=ptr(noise), indices_dev=ptr(indices), seed=seed, offset=int(offset),
                       n_samples_local=n_local, n_samples_global=n_global, sample_base=base, out_dev=ptr(self.out),
                       noise_out_dev=ptr(noise_out), indices_out_dev=ptr(indices_out), fvalue_out_dev=ptr(fvalue_out),
                       logq_out_dev=ptr(logq_out), workspace_dev=ptr(self.workspace(n_local)), stream=self._stream(),
                       f_weight_dev=ptr(f_weight), q_weight_dev=ptr(q_weight))

    def _zero_noise(self, n_local):
        z = self.__dict__.setdefault("_zeros", {}).get(n_local)
        if z is None:
            z = self._zeros[n_local] = torch.zeros((self.program.n_noise, n_local), device=self.device)
        return z

    def noise_from_named(self, named, n):
        """{variable name: [N, 1, rows, cols]}  ->  [n_noise, N] (the latent vector's row order; a scale latent, [N, 1, 1, 1], is row
        n_rows + t behind the weights'; a point tensor has no draw: its name is not asked for and its rows stay 0)"""
        out = np.zeros((self.program.n_noise, n), dtype=np.float32)
        for t in self.program.tensors:
            if t.get("point"):
                continue
            a = np.asarray(named[t["name"]], dtype=np.float32)
            out[t["row0"]:t["row0"] + t["size"]] = a.reshape(a.shape[0], -1).T
        for i, l in enumerate(self.program.scale_latents):
            out[self.program.n_rows + i] = np.asarray(named[l["name"]], dtype=np.float32).reshape(-1)
        return out

    def named_noise(self, noise, n):
        """[n_rows, N] -> {variable name: [N, 1, rows, cols]} (what the oracle takes; the point tensors, which have no draw, are left out)"""
        noise = np.asarray(noise)
        named = {t["name"]: noise[t["row0"]:t["row0"] + t["size"]].T.reshape(n, 1, t["rows"], t["cols"]) for t in self.program.tensors
                 if not t.get("point")}
        if noise.shape[0] > self.program.n_rows:          # (the draw of a training launch; `predict` reports the weights' rows alone)
            for i, l in enumerate(self.program.scale_latents):
                named[l["name"]] = noise[self.program.n_rows + i].reshape(n, 1, 1, 1)
        return named

    def _noise_tensor(self, noise, n_global, base, n_local, rows=None):
        if noise is None:
            return None
        if isinstance(noise, dict):
            noise = self.noise_from_named(noise, n_global)
        # (a training launch reads row n_rows + t for scale latent t: a matrix of the weights' rows alone is refused here, not read past)
        rows = self.program.n_noise if rows is None else rows
        if self.program.scale_latents and noise.shape[0] != rows:
            raise ValueError("noise must have {} rows: got {}".format(rows, noise.shape[0]))
        if isinstance(noise, np.ndarray):
            return torch.from_numpy(np.ascontiguousarray(noise[:, base:base + n_local], dtype=np.float32)).to(self.device)
        return noise if noise.shape[1] == n_local else noise[:, base:base + n_local].contiguous()

    def _indices_tensor(self, minibatch):
        if minibatch is None:
            return None
        if isinstance(minibatch, dict):
            minibatch = minibatch[self.program.indices_name]
        idx = np.asarray(minibatch, dtype=np.int64).reshape(-1)
        # the kernel reads labels[row] and dataset[row] (csrc/bnn_kernel.inc, bnn_gather): rows outside the dataset are refused here
        if idx.size != self.program.batch_size or (idx.size and (idx.min() < 0 or idx.max() >= self.program.dataset_size)):
            raise ValueError("minibatch indices must be {} rows in [0, {}): got {} rows in [{}, {}]".format(
                self.program.batch_size, self.program.dataset_size, idx.size, idx.min() if idx.size else "-", idx.max() if idx.size else "-"))
        return torch.as_tensor(idx.astype(np.int32)).to(self.device)

    def evaluate(self, number_samples, noise=None, minibatch=None, seed=None, offset=None, want_noise=False,
                 want_fvalues=False, want_indices=False, **_):
        from brancher_amd import engine
        rank, world = engine.dist_info()
        base, n_local = engine.shard(number_samples, rank, world)
        if n_local == 0:
            raise ValueError("number_samples={} is smaller than the number of GPUs {}".format(number_samples, world))
        if offset is None:
            offset = self.iteration
            self.iteration += 1
        dev, p = self.device, self.program
        noise_t = self._noise_tensor(noise, number_samples, base, n_local)
        idx_t = self._indices_tensor(minibatch)
        noise_o = torch.empty((p.n_noise, n_local), device=dev) if want_noise else None
        idx_o = torch.empty(p.batch_size, device=dev, dtype=torch.int32) if want_indices else None
        fvals = torch.empty(n_local, device=dev) if want_fvalues else None
        logq = torch.zeros(n_local, device=dev) if want_fvalues and getattr(p, "estimator", "pathwise") == "blackbox" else None
        args = self._args(n_local, number_samples, base, noise_t, idx_t, seed, offset, noise_o, idx_o, fvals, logq)
        native.check(self.lib.bsvi_bnn_fwd_bwd(self.handle, C.byref(args)))
        engine.allreduce_sums(self.out)
        engine.check_exchange(self.device, self.params)
        native.check(self.lib.bsvi_bnn_finalize(self.handle, C.c_void_p(self.out.data_ptr()), number_samples, self._stream()))
        self.grads_valid = True
        res = dict(loss=self.out[2], finite=self.out[3], nonfinite_count=self.out[1],
                   grads=self.out[OUT_HEADER:OUT_HEADER + p.n_params], n_local=n_local, sample_base=base)
        if want_noise:
            res["noise"] = noise_o
        if want_indices:
            res["indices"] = idx_o
        if want_fvalues:
            res["f"] = fvals
            if logq is not None:
                res["lq"] = logq
        return res

    def predict_path(self):
        """where the forward-only kernel of `predict` keeps the small tensors and its two activation buffers (csrc/bnn_select.h,
        predict_lds: from the network's size alone): "lds" or "global\""""
        kind = int(self.lib.bsvi_bnn_predict_lds(self.handle))
        if kind not in (0, 1):
            raise native.NativeError("bsvi_bnn_predict_lds returned %d" % kind)
        return PREDICT_PATHS[kind]

    def _predict_rows(self, x):
        """the caller's rows as a contiguous f32 device tensor [M, P]: from [M, P], [M, P, 1] or the reference's [1, M, P, 1]"""
        a = x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x, dtype=np.float32))
        if a.ndim == 4 and a.shape[0] == 1:
            a = a[0]
        if a.ndim == 3 and a.shape[-1] == 1:
            a = a[..., 0]
        P = self.program.n_features
        if a.ndim != 2:
            raise ValueError("predict takes rows as [M, {P}], [M, {P}, 1] or [1, M, {P}, 1]: got shape {}".format(
                tuple(x.shape) if hasattr(x, "shape") else np.shape(x), P=P))
        if a.shape[1] != P:
            raise ValueError("the rows have {} features, the model was built on {}".format(a.shape[1], P))
        if a.shape[0] < 1:
            raise ValueError("predict needs at least one row")
        return a.to(device=self.device, dtype=torch.float32).contiguous()

    def predict(self, x, number_samples, seed=None, offset=None, noise=None, want_outputs=False, want_draws=False, want_noise=False,
                rows_per_pass=None, sample_base=0):
        """Posterior predictive on rows the caller hands in (bsvi_bnn_predict): `number_samples` weight sets from the CURRENT posterior
        — the draw of a training launch at the same (seed, offset, sample_base), or `noise` ([n_rows, N], or named as the oracle
        takes it) — and the chain forward on every row of `x`.  Device tensors: "probs" [N, M, C] (softmax probabilities | sigmoid of
        the logit | the Normal's loc), "mean" [M, C] (their mean over the samples, fixed order), "var" [M, C] (Normal likelihood only:
        population variance of the loc over the samples + sigma^2; with a scale head + the mean over the samples of sigma^2; a Laplace
        likelihood adds 2 sigma^2, a Cauchy likelihood has no variance and no "var" key), and on request
        "outputs" [N, M, C] (logits | loc; a scale head adds "scale" [N, M, C], sigma of every sample and row), "draws"
        [N, M, C] (one draw of the likelihood per sample and row: one-hot | 0 / 1 | real) and "noise" [n_rows, N] (the eps drawn).
        offset=None draws from the sampling range (1 << 62) + tick, as the samplers of the engine do; `self.iteration`, `self.out` and
        the gradients are left alone.  Not sharded: every rank computes all N samples, no collective.  rows_per_pass (a multiple of
        32; default: from the network's size) bounds the workspace and changes no value."""
        p, dev, N = self.program, self.device, int(number_samples)
        if N < 1:
            raise ValueError("number_samples must be at least 1")
        rows = self._predict_rows(x)
        M, Cn = int(rows.shape[0]), p.n_classes
        rpp = 0 if rows_per_pass is None else int(rows_per_pass)
        if rpp < 0 or rpp % 32:
            raise ValueError("rows_per_pass must be a multiple of 32: got {}".format(rows_per_pass))
        if offset is None:
            _engine._sample_tick[0] += 1
            offset = (1 << 62) + _engine._sample_tick[0]
        if getattr(p, "estimator", "pathwise") == "taylor1":
            noise = self._zero_noise(N)                       # (f at the posterior's means: `_args`)
        if isinstance(noise, dict):                           # (named as the oracle takes it: the weights' rows; a scale latent's draw is not read)
            noise = self.noise_from_named(dict({l["name"]: np.zeros(N) for l in p.scale_latents}, **noise), N)[:p.n_rows]
        noise_t = self._noise_tensor(noise, N, 0, N, rows=p.n_rows)
        if noise_t is not None and tuple(noise_t.shape) != (p.n_rows, N):
            raise ValueError("noise must be [{}, {}]: got {}".format(p.n_rows, N, tuple(noise_t.shape)))
        if not isinstance(seed, int) or seed is True:
            seed = _engine.shared_seed(seed, dev)
        key = (N, M, rpp)
        ws = self.__dict__.get("_predict_ws")
        if ws is None or ws[0] != key:                        # (one workspace kept: the shape of the last call)
            ws = self._predict_ws = (key, torch.zeros(int(self.lib.bsvi_bnn_predict_workspace_bytes(self.handle, N, M, rpp)),
                                                      dtype=torch.uint8, device=dev))
        new = lambda *shape: torch.empty(shape, device=dev)
        probs, mean = new(N, M, Cn), new(M, Cn)
        # (a Cauchy likelihood has no variance: no "var" key)
        var = new(M, Cn) if p.likelihood == LIK_NORMAL and getattr(p, "family", D.DIST_NORMAL) != D.DIST_CAUCHY else None
        heads = bool(getattr(p, "scale_head", None))        # (z_out is then [N, M, 2 C]: the loc, then sigma itself)
        outputs = new(N, M, 2 * Cn if heads else Cn) if want_outputs else None
        draws = new(N, M, Cn) if want_draws else None
        noise_o = new(p.n_rows, N) if want_noise else None      # (the posterior of the weights does not involve a scale latent)
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        args = native.BnnPredictArgs(params_dev=ptr(self.params), x_dev=ptr(rows), noise_dev=ptr(noise_t), seed=int(seed),
                                     offset=int(offset), n_samples_local=N, sample_base=int(sample_base), n_rows=M, rows_per_pass=rpp,
                                     z_out=ptr(outputs), p_out=ptr(probs), mean_out=ptr(mean), var_out=ptr(var), draw_out=ptr(draws),
                                     noise_out=ptr(noise_o), workspace_dev=ptr(ws[1]), stream=self._stream())
        native.check(self.lib.bsvi_bnn_predict(self.handle, C.byref(args)))
        res = dict(probs=probs, mean=mean, n_rows=M, seed=int(seed), offset=int(offset),
                   rows_per_pass=int(self.lib.bsvi_bnn_predict_rows_per_pass(self.handle, N, M, rpp)),
                   data_path="bf16x3" if self.lib.bsvi_bnn_predict_last_exact() == 1 else "f32")
        if heads and outputs is not None:
            outputs, res["scale"] = outputs[..., :Cn], outputs[..., Cn:]      # (views of the one buffer: no copy on the device)
        for k, t in (("var", var), ("outputs", outputs), ("draws", draws), ("noise", noise_o)):
            if t is not None:
                res[k] = t
        return res

    def evaluate_weighted(self, number_samples, f_weight, q_weight, seed, offset, noise=None, minibatch=None):
        """The second pass of a user-defined gradient estimator (`engine.custom_estimator_loss`), as `CompiledDense.evaluate_weighted`:
        the draw and the minibatch of (seed, offset) again, and -(sum_n a_n grad f_n + b_n grad log q_n) in the output block
        (bsvi_bnn_args::f_weight_dev / q_weight_dev; the model must have been created with the BlackBox estimator)."""
        from brancher_amd import engine
        rank, world = engine.dist_info()
        base, n_local = engine.shard(number_samples, rank, world)
        a = f_weight.reshape(-1)[base:base + n_local].contiguous().float()
        b = q_weight.reshape(-1)[base:base + n_local].contiguous().float()
        noise_t = self._noise_tensor(noise, number_samples, base, n_local)
        idx_t = self._indices_tensor(minibatch)
        args = self._args(n_local, number_samples, base, noise_t, idx_t, seed, int(offset), f_weight=a, q_weight=b)
        native.check(self.lib.bsvi_bnn_fwd_bwd(self.handle, C.byref(args)))
        engine.allreduce_sums(self.out)
        engine.check_exchange(self.device, self.params)
        native.check(self.lib.bsvi_bnn_finalize(self.handle, C.c_void_p(self.out.data_ptr()), 1, self._stream()))
        self.grads_valid = True
        return self.out[OUT_HEADER:OUT_HEADER + self.program.n_params]

    def _seed(self, seed):
        return _engine.shared_seed(seed, self.device)

    def named_grads(self):
        g = self.out[OUT_HEADER:].detach().cpu().numpy()
        return {par.name: g[off:off + size].reshape(par.shape).copy() for par, off, size, _ in self.program.parameters}

    def named_params(self):
        t = self.params.detach().cpu().numpy()
        return {par.name: t[off:off + size].reshape(par.shape).copy() for par, off, size, _ in self.program.parameters}

    def train(self, number_iterations, number_samples, optimizer="Adam", noise_seq=None, minibatch_seq=None, seed=None,
              pretraining_iterations=0, allow_persistent=True, _force_sharded_path=False, **opt_params):
        from brancher_amd import engine
        cfg = native.make_opt_cfg(optimizer, **opt_params)
        rank, world = engine.dist_info()
        base, n_local = engine.shard(number_samples, rank, world)
        if n_local == 0:
            raise ValueError("number_samples={} is smaller than the number of GPUs {}".format(number_samples, world))
        dev, p = self.device, self.program
        K = int(number_iterations)
        engine.broadcast_from_rank0(self.params)      # ranks step their own copies: they must start from the same values
        loss_curve, finite, state = engine.training_buffers(K, p.n_params, dev)
        ptr = lambda t: C.c_void_p(t.data_ptr())
        offset0 = self.iteration
        self.iteration += K
        self.grads_valid = True
        # (the call's Philox key once: with seed=None on several ranks `shared_seed` is a broadcast and a host sync — not per iteration)
        seed = int(engine.shared_seed(seed, dev))
        for it in range(K):
            nz = None if noise_seq is None else self._noise_tensor(noise_seq[it], number_samples, base, n_local)
            mb = None if minibatch_seq is None else self._indices_tensor(minibatch_seq[it])
            args = self._args(n_local, number_samples, base, nz, mb, seed, offset0 + it)
            mask = self.mask_all if it > pretraining_iterations else self.mask_first
            if world == 1 and not _force_sharded_path:
                native.check(self.lib.bsvi_bnn_step(self.handle, C.byref(args), C.byref(cfg), ptr(self.params), ptr(state),
                                                    ptr(mask), C.c_void_p(loss_curve.data_ptr() + 4 * it),
                                                    C.c_void_p(finite.data_ptr() + 4 * it)))
            else:
                native.check(self.lib.bsvi_bnn_fwd_bwd(self.handle, C.byref(args)))
                engine.allreduce_sums(self.out)
                native.check(self.lib.bsvi_finalize_step(
                    C.byref(cfg), ptr(self.params), ptr(self.out), ptr(state), ptr(mask), p.n_params, number_samples,
                    C.c_void_p(loss_curve.data_ptr() + 4 * it), C.c_void_p(finite.data_ptr() + 4 * it), self._stream()))
        self.last_mode = "stepwise" if world == 1 else "stepwise+allreduce"
        if world > 1:
            engine.check_exchange(self.device, self.params)
        return loss_curve[:K], finite[:K]


# every native call of a compiled program runs with its device current (engine._bound_to_device)
from brancher_amd import engine as _engine  # noqa: E402  (engine imports this module lazily)
CompiledBnn = _engine._bound_to_device(CompiledBnn)
