"""Every link operator of include/bsvi.h (`bsvi_unop`, `bsvi_binop`) in every kernel that defines it, op by op, against torch in
DOUBLE precision (oracle/svi_oracle.py) — value and reverse mode, at interior points of the op's domain and at its edges.

The reverse mode of the op table is written out four times: the interpreter (`unop` / `unop_grad` / `unop_rare*` of
bsvi_device.h, the BIN arms of elbo_kernel.hip), the specialiser's emitted BIN text (specialize.cpp), the covariance-expression
emitter (mvn.cpp: tests/test_gpu_mvn_ops.py) and the uniform-table transforms (`utransform*` of bsvi_device.h,
`utransform_common` / `spec_utransform_grad` of spec_main.h).  This file holds the first, second and fourth to the reference.

Model: the smallest one that puts the op on a path to the loss, through the public API only —
    prior z ~ Normal(0, 1),  posterior z ~ Normal(loc, 1) with loc learnable,  observed y ~ Normal(op(z) * w + c, s)
with z a VECTOR of points (op applied elementwise, vector observation): with loc = 0 and scale = 1 (a root holding 1, not a number,
which would pass through softplus(inverse_softplus(1)): 1 in float32, dist_math.h, but not in the double oracle) z equals the
supplied noise exactly (asserted through `want_samples`), every sample holds all points, and `named_grads()["z_mean"][d]` (the
posterior's location is a learnable root) is the gradient at point d alone — no mean over samples that could cancel.  The prior is
centred on the points, so that no term of the size of a point (1e6, the largest) stands beside the op's own.

Bound (tests/test_gpu_random_models.py `check_against_the_oracles`): error <= max(4 x |float32 oracle - float64 oracle|,
1e-5 x max(1, scale)), the 1e-5 being BASELINE.json's; applied to the interior points together and to every edge point on its own,
so that a huge value at one edge (exp(88), 1 / 1e-18) widens nobody else's bound.  Where the double reference is inf or NaN the same class and sign are required and
nothing else is compared.  No flat relaxation per op.

Points whose value or derivative is not finite (sqrt'(0), log(0), x ** -2 at 0, d/db (-2) ** 3 ...) are run as a group of their
own, so that the finite group also checks the loss of the launch without per-sample outputs.

Launch kinds.  "diagnostic" asks for per-sample outputs, "lean" does not.  Prescribing z means supplying the noise, and in the
specialised engine a launch with supplied noise is served by the diagnostic variant of the generated kernel whatever it asks for
(specialize.cpp), in the training loop too: with per-sample operands the two ids differ in the kernel only under the
interpreter.  The parameter / constant cases need no prescribed z and draw in the kernel: the noise for the oracle is what a
diagnostic launch reports for (seed, offset), and the lean launch and the training loop then draw it themselves — the generated
lean kernel and the in-kernel loop with its owners' `spec_utransform_grad`.
"""
import numpy as np
import pytest
import torch

from brancher_amd import engine, lowering, workloads as W
from oracle.svi_oracle import Oracle

pytestmark = pytest.mark.gpu

F = np.float32
TINY = float(np.finfo(F).tiny)          # smallest normal
PI = float(F(np.pi))
INF = float("inf")
N_INTERIOR = 48


def nxt(x, towards):
    return float(np.nextafter(F(x), F(towards)))


class _TorchNS:
    """`BF.<name>` on torch tensors, resolved as the oracle resolves it"""

    def __getattr__(self, name):
        if name == "delta":
            return lambda x, y: (x == y).to(x.dtype)
        return getattr(torch, name) if hasattr(torch, name) else getattr(torch.nn.functional, name)


def _signed(lo, hi):
    def draw(rng, n):
        return rng.uniform(lo, hi, n) * rng.choice([-1.0, 1.0], n)
    return draw


def _uniform(lo, hi):
    return lambda rng, n: rng.uniform(lo, hi, n)


def _call(name):
    return lambda NS, v: getattr(NS, name)(v)


def _powi(imm):
    return lambda NS, v: v ** imm


# name -> (link, interior draw, edge points); unary ops take points x, binary ops pairs (a, b)
UNARY = {
    "copy": (lambda NS, v: v, _uniform(-3, 3), [0.0]),
    "neg": (_call("neg"), _uniform(-3, 3), [0.0]),
    "exp": (_call("exp"), _uniform(-4, 4), [-104.0, -1e-8, 1e-8, 88.0]),
    "log": (_call("log"), _uniform(0.05, 20), [0.0, 1.0, 1e-30, 1e30]),            # (1e-30: the derivative times the term behind it still a float32)
    "sqrt": (_call("sqrt"), _uniform(0.05, 20), [0.0, 1.0, TINY, 1e30]),
    "sin": (_call("sin"), _uniform(-6, 6), [0.0, PI, -PI, 1e4, 1e6]),
    "cos": (_call("cos"), _uniform(-6, 6), [0.0, PI, -PI, 1e4, 1e6]),
    "tanh": (_call("tanh"), _uniform(-4, 4), [20.0, -20.0, 90.0, -90.0]),
    "abs": (_call("abs"), _uniform(-3, 3), [0.0, TINY, -TINY]),
    "sigmoid": (_call("sigmoid"), _uniform(-6, 6), [20.0, -20.0, 90.0, -90.0]),
    "softplus": (_call("softplus"), _uniform(-6, 6), [20.0, nxt(20, INF), nxt(20, -INF), -104.0, 88.0]),
    "relu": (_call("relu"), _uniform(-3, 3), [0.0, TINY, -TINY]),
    "reciprocal": (_call("reciprocal"), _signed(0.05, 20), [0.0, 1.0, 1e-18, 1e30]),      # (1e-18: the derivative, -1e36, still a float32)
    "log1p": (_call("log1p"), _uniform(-0.9, 20), [-1.0, 1.0, 1e-8, -1e-8, 1e30]),
    "expm1": (_call("expm1"), _uniform(-4, 4), [-104.0, -1e-8, 1e-8, 88.0]),
    "square": (_call("square"), _uniform(-3, 3), [0.0, TINY, 1e18]),
}
# POWI: 2, -1 and 0.5 are the inlined forms of `unop`, the others go through `unop_rare` (powf); non-integer exponents at x >= 0 only.
# "tiny" is the smallest normal, except under a negative exponent, where its power or the derivative (-1 / tiny ** 2) is no float32:
# 1e-10 there (x ** -2 = 1e20, derivative -2e30).
for _imm in (2.0, -1.0, 0.5, 3.0, -2.0, 1.5, 0.0, 1.0):
    _integer = _imm == int(_imm)
    UNARY["powi[%g]" % _imm] = (_powi(_imm), _signed(0.3, 3) if _integer else _uniform(0.05, 5),
                                [0.0, TINY if _imm >= 0 else 1e-10, 2.0] + ([-2.0] if _integer else []))

BINARY = {
    "add": (lambda NS, a, b: a + b, (_uniform(-3, 3), _uniform(-3, 3)), [(0.0, 0.0)]),
    "sub": (lambda NS, a, b: a - b, (_uniform(-3, 3), _uniform(-3, 3)), [(0.0, 0.0)]),
    "mul": (lambda NS, a, b: a * b, (_uniform(-3, 3), _uniform(-3, 3)), [(0.0, 0.0)]),
    "truediv": (lambda NS, a, b: a / b, (_uniform(-3, 3), _signed(0.2, 3)),
                [(1.5, 1e-18), (1.5, -1e-18), (1.5, -2.0), (-1.5, -0.5), (0.0, 1.0)]),
    "pow": (lambda NS, a, b: a ** b, (_uniform(0.2, 3), _uniform(-2, 2)),
            [(0.0, 2.0), (0.0, 0.0), (2.0, 0.0), (0.0, 0.5), (-2.0, 3.0)]),
    "delta": (lambda NS, a, b: NS.delta(a, b), (_uniform(-3, 3), _uniform(-3, 3)),
              [(1.0, 1.0), (1.0, 2.0), (1.0, nxt(1, 2)), (nxt(1, 0), 1.0), (0.0, 0.0)]),
}
# the seven ops a learnable parameter reaches through the uniform table (lowering.UT), not through a UN instruction
TRANSFORMS = ("softplus", "sigmoid", "exp", "log", "tanh", "sqrt", "square")

C_OFFSET, S_OBS = 0.1, 0.8


def op_link(name):
    return (UNARY.get(name) or BINARY[name])[0]


def op_points(name):
    """float32 points of one op, [P, arity]: seeded interior points, then the edges (delta: half of the interior pairs equal)"""
    _, draw, edges = UNARY.get(name) or BINARY[name]
    rng = np.random.RandomState(sum(ord(ch) for ch in name))
    if name in UNARY:
        pts = np.concatenate([draw(rng, N_INTERIOR), edges])[:, None]
    else:
        a, b = draw[0](rng, N_INTERIOR), draw[1](rng, N_INTERIOR)
        if name == "delta":
            b[::2] = a[::2]
        pts = np.concatenate([np.stack([a, b], 1), np.asarray(edges, dtype=np.float64)])
    return pts.astype(F)


def op_reference(name, pts, dtype):
    """value and partial derivatives of the op alone in `dtype`: which points are finite, and how large the value is"""
    cols = [torch.tensor(pts[:, k].astype(np.float64), dtype=dtype, requires_grad=True) for k in range(pts.shape[1])]
    y = op_link(name)(_TorchNS(), *cols)
    if y.requires_grad:
        y.sum().backward()
    ders = [np.zeros(len(pts)) if c.grad is None else c.grad.double().numpy() for c in cols]
    return y.detach().double().numpy(), ders


def split_points(name):
    """(finite, other): points at which value and derivatives are finite in float32 AND double, and the rest"""
    pts = op_points(name)
    fine = np.ones(len(pts), dtype=bool)
    for dtype in (torch.float32, torch.float64):
        y, ders = op_reference(name, pts, dtype)
        fine &= np.isfinite(y) & np.all([np.isfinite(d) for d in ders], axis=0)
    return pts[fine], pts[~fine]


def weights_for(name, pts):
    """w of  op(z) * w + c : 0.7, scaled down by a power of two where the op's value is huge (exp(88), 1 / 1e-18), so that the
    Normal term behind the op stays inside float32 and the comparison is about the op"""
    y, _ = op_reference(name, pts, torch.float64)
    w = np.full(len(pts), 0.7)
    big = np.isfinite(y) & (np.abs(y) > 1e3)
    w[big] = 0.7 * 2.0 ** -np.round(np.log2(np.abs(y[big])))
    return w.astype(F).reshape(-1, 1)


def data_for(name, n_points, n_data):
    rng = np.random.RandomState(7 + n_data + sum(ord(ch) for ch in name))
    return rng.normal(0.3, 1.0, size=(n_data, n_points, 1)).astype(F)


def build_sample_model(api, name, pts, n_data):
    """the op on per-sample values: z (and u for a binary op) are vectors of len(pts) elements whose posterior has a learnable
    location (a root: `named_grads()["z_mean"]`; "z_loc" and "z_scale" are the names of the prior's own roots) and the constant scale 1, so that z IS the supplied noise in every precision"""
    P = len(pts)
    col = lambda v: np.full((P, 1), v, dtype=np.float64)
    latents, q = [], []
    for latent in ("z", "u")[:pts.shape[1]]:
        # (the prior is centred on the points: with Normal(0, 1) the gradient at x = 1e6 is the difference of two numbers of that size)
        latents.append(api.NormalVariable(pts[:, len(latents)].astype(np.float64).reshape(P, 1), col(1.0), latent))
        # (the scale is a root, used as it is: a number would go through softplus(inverse_softplus(1)), which is 1 in float32 only)
        q.append(api.NormalVariable(api.RootVariable(col(0.0), latent + "_mean", learnable=True), api.RootVariable(col(1.0), latent + "_unit"), latent))
    y = api.NormalVariable(op_link(name)(api.BF, *latents) * weights_for(name, pts) + C_OFFSET, S_OBS, "y")
    model = api.ProbabilisticModel([y])
    y.observe(data_for(name, P, n_data))
    model.set_posterior_model(api.ProbabilisticModel(q))
    return model


def build_operand_model(api, name, pts, n_data, kind):
    """the op on a learnable parameter with no sampled ancestor (kind "param": theta, a vector; for the seven transforms the
    uniform table computes it, for the others a UN / BIN instruction on a uniform operand) or on a constant (kind "const").
    The op's value is the posterior's location, so theta's gradient runs through the op's derivative at every element."""
    P = len(pts)
    col = lambda v: np.full((P, 1), v, dtype=np.float64)
    first = pts[:, :1].astype(np.float64)
    operands = [api.RootVariable(first, "theta", learnable=True) if kind == "param" else first]
    if pts.shape[1] == 2:
        operands.append(pts[:, 1:].astype(np.float64))
    if kind == "const":      # (an expression needs one symbolic operand: a root that is not learnable is a constant of the model)
        operands[0] = api.RootVariable(first, "theta", learnable=False)
    z = api.NormalVariable(col(0.0), col(1.0), "z")
    y = api.NormalVariable(z * 0.5 + C_OFFSET, S_OBS, "y")
    model = api.ProbabilisticModel([y])
    y.observe(data_for(name, P, n_data))
    loc = op_link(name)(api.BF, *operands) * weights_for(name, pts) + C_OFFSET
    model.set_posterior_model(api.ProbabilisticModel([api.NormalVariable(loc, col(1.0), "z", learnable=True)]))
    return model


def layout(pts, n):
    """noise [n, 1, P, 1] per latent: every sample holds all P points, so element d of a gradient is point d alone"""
    P = len(pts)
    return {latent: np.tile(pts[None, :, k], (n, 1)).reshape(n, 1, P, 1).astype(F) for k, latent in enumerate(("z", "u")[:pts.shape[1]])}


def same_class(got, ref, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (what, "NaN", got, ref)
    inf = np.isinf(ref)
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(np.sign(got[inf]), np.sign(ref[inf])), (what, "inf", got, ref)


def close(got, r64, r32, what, groups=None, overflow_ok=False):
    """The bound of the module's docstring over each group of elements (default: all of them together): the largest error
    against 4 x the largest float32-oracle error, or 1e-5 of the largest magnitude (at least 1).  Non-finite reference: same
    class and sign, nothing else.  Where the double reference is finite and the float32 oracle is not, there is no yardstick and
    nothing to compare: allowed (`overflow_ok`, and printed) only in the group of non-finite points."""
    got = np.asarray(got, dtype=np.float64).reshape(-1)
    r64, r32 = np.asarray(r64, dtype=np.float64).reshape(-1), np.asarray(r32, dtype=np.float64).reshape(-1)
    assert got.shape == r64.shape == r32.shape, (what, got.shape, r64.shape, r32.shape)
    odd = ~np.isfinite(r64)
    same_class(got[odd], r64[odd], what)
    for idx in ([np.arange(len(got))] if groups is None else groups):
        idx = np.asarray(idx)[~odd[idx]]
        if not len(idx):
            continue
        yard = np.abs(r32[idx] - r64[idx])
        if not np.isfinite(yard).all():         # (torch's own float32 arithmetic left float32 there)
            assert overflow_ok, (what, "the float32 oracle is not finite at", idx[~np.isfinite(yard)], r64[idx], r32[idx])
            print("%s: no float32 yardstick at %s (double %s, float32 %s)" % (what, idx[~np.isfinite(yard)], r64[idx], r32[idx]))
            continue
        yard = yard.max()
        tol = max(4.0 * yard, 1e-5 * max(1.0, np.abs(r64[idx]).max()))
        err = np.abs(got[idx] - r64[idx])
        print("%s [%d..%d]: err %.3g, float32 oracle %.3g, bound %.3g" % (what, idx[0], idx[-1], np.nanmax(err), yard, tol))
        assert (err <= tol).all(), (what, idx[~(err <= tol)], got[idx], r64[idx], r32[idx])


def point_groups(n_points, n_interior):
    """the interior points as one group, every edge point on its own: a huge edge value does not widen the bound of the others"""
    return ([np.arange(n_interior)] if n_interior else []) + [[d] for d in range(n_interior, n_points)]


def or_zero(g, like):
    return np.zeros_like(like) if g is None else np.asarray(g).reshape(like.shape)


def named_reference(build, n, estimator, noise):
    out = []
    for dtype in (torch.float64, torch.float32):
        with np.errstate(all="ignore"):
            out.append(Oracle(build(), dtype=dtype).loss_and_grads(n, estimator, noise))
    return out


def instructions(program):
    """the (kind, flags) of the UN / BIN instructions of a lowered program"""
    kinds = {lowering.OP["BIN"]: "BIN", lowering.OP["UN"]: "UN"}
    words = [int(row[0]) for row in program.code]
    return {(kinds[w & 0xFF], (w >> 8) & 0xFF) for w in words if (w & 0xFF) in kinds}


def expected_instruction(name):
    if name in BINARY:
        return ("BIN", lowering.BINOP[name])
    return ("UN", lowering.UNOP["powi" if name.startswith("powi") else name])


def check_launches(build, pts, n, estimator, launch, engine_name, finite, name=None, groups=None):
    """one model, one launch kind, against the oracles on the same noise; `groups`: see `close`"""
    compiled = engine.compile_model(build(), None, estimator)
    if name is not None and name != "copy":        # (the identity link is the operand itself: no instruction)
        assert expected_instruction(name) in instructions(compiled.program), (name, instructions(compiled.program))
    assert compiled.native.engine(n, 0)["engine"] == engine_name          # (0: the evaluation entry point, bsvi_elbo_fwd_bwd)
    noise = layout(pts, n)
    r64, r32 = named_reference(build, n, estimator, noise)
    if launch == "diagnostic":
        res = compiled.evaluate(n, noise=noise, want_noise=True, want_samples=True, want_fvalues=True)
        drawn = compiled.samples_by_name(res["samples"])
        for latent, v in noise.items():
            assert np.array_equal(drawn[latent].reshape(v.shape), v), latent      # z IS the supplied point
        close(res["f"].cpu().numpy(), r64["f"], r32["f"], "f", overflow_ok=not finite)
        if estimator == "blackbox":
            close(res["lq"].cpu().numpy(), r64["lq"], r32["lq"], "log q")
    else:
        res = compiled.evaluate(n, noise=noise)
    if finite:
        close(float(res["loss"].item()), r64["loss"], r32["loss"], "loss")
    grads = compiled.named_grads()
    for pname, g in r64["grads"].items():
        close(grads[pname], or_zero(g, grads[pname]), or_zero(r32["grads"][pname], grads[pname]), "d/d%s" % pname, groups,
              overflow_ok=not finite)
    return compiled


def all_ops():
    return list(UNARY) + list(BINARY)


@pytest.fixture(params=["specialised", "interpreter"])
def engine_name(request, monkeypatch):
    monkeypatch.setenv("BSVI_JIT", "1" if request.param == "specialised" else "0")
    return request.param


@pytest.mark.parametrize("launch", ["diagnostic", "lean"])
@pytest.mark.parametrize("name", all_ops())
def test_op_on_sampled_values_matches_torch_double(name, launch, engine_name):
    """pathwise, per-sample operands: the interior points and the finite edges with 3 samples / 1 datapoint and 65 samples / 5
    datapoints (one wave, and a ragged second one), then the points where torch itself returns inf or NaN (class and sign).
    Among the finite points: powi[0] at x = 0 and pow at (0, 2), (0, 0), (2, 0), where torch's derivatives are 0 and the plain
    rules b * a ** (b - 1) and a ** b * log(a) are 0 * inf."""
    api = W.native_api()
    fine, other = split_points(name)
    assert len(fine) >= N_INTERIOR and len(fine) + len(other) <= 64
    for n, n_data in ((3, 1), (65, 5)):
        check_launches(lambda: build_sample_model(api, name, fine, n_data), fine, n, "pathwise", launch, engine_name, True, name,
                       point_groups(len(fine), N_INTERIOR))
    if len(other):
        check_launches(lambda: build_sample_model(api, name, other, 1), other, max(3, len(other)), "pathwise", launch, engine_name, False, name)


@pytest.mark.parametrize("launch", ["diagnostic", "lean"])
@pytest.mark.parametrize("name", ["tanh", "abs", "pow"])
def test_op_under_the_blackbox_estimator_matches_torch_double(name, launch, engine_name):
    """BlackBox (log q times f) for one smooth op, one kinked op and POW, at the interior points, all of them under one bound as in
    tests/test_gpu_random_models.py.  (The score term f * d log q / d loc cancels against f * d log q / dz * dz / d loc: exactly in
    torch's autograd, to rounding in the kernel — a residue of ~2e-6 * |f * noise| that no float32 yardstick of a single element
    shows; measured at tanh(20), where the pathwise part is 0: -2.8e-3 with f = -80 and noise = 20.)"""
    api = W.native_api()
    interior = split_points(name)[0][:N_INTERIOR]
    for n, n_data in ((3, 1), (65, 5)):
        check_launches(lambda: build_sample_model(api, name, interior, n_data), interior, n, "blackbox", launch, engine_name, True)


def operand_points(name):
    """three interior points and every finite edge (softplus at 20 +- 1 ulp, sigmoid / tanh at +-20 among them)"""
    fine, _ = split_points(name)
    return np.concatenate([fine[:3], fine[N_INTERIOR:]])


@pytest.mark.parametrize("kind", ["param", "const"])
@pytest.mark.parametrize("name", all_ops())
def test_op_on_a_parameter_or_a_constant_matches_torch_double(name, kind, engine_name):
    """The op on an operand that is the same for every sample.  A learnable parameter reaches the seven transforms through the
    uniform table (`utransform` / `utransform_grad`; in the specialised kernels `utransform_common` / `spec_utransform_grad`)
    and every other op through a UN / BIN instruction on a uniform operand; theta's gradient isolates each parameter value.
    The kernel draws: a diagnostic launch at (seed, offset) reports its noise, the oracle is evaluated on it, and the lean launch
    and ONE SGD step of the training loop — whose owners compute the derivative themselves — draw the same noise again."""
    api = W.native_api()
    pts = operand_points(name)
    n, lr, seed, offset = 65, 1e-2, 23, 4
    build = lambda: build_operand_model(api, name, pts, 5, kind)
    compiled = engine.compile_model(build(), None, "pathwise")
    assert compiled.native.engine(n, 0)["engine"] == engine_name and compiled.native.engine(n, 2)["engine"] == engine_name
    if name in TRANSFORMS:       # the uniform table computes the op: no instruction
        assert lowering.UT[name] in set(int(t) for t in compiled.program.uniform["transform"])
        assert expected_instruction(name) not in instructions(compiled.program)
    elif name != "copy":
        assert expected_instruction(name) in instructions(compiled.program)
    theta_groups = [[d] for d in range(len(pts))]
    r64 = r32 = None
    for launch in ("diagnostic", "lean"):
        if launch == "diagnostic":
            res = compiled.evaluate(n, seed=seed, offset=offset, want_noise=True, want_fvalues=True)
            rows = res["noise"].cpu().numpy()
            noise = {latent: rows[s.base:s.base + s.size].T.reshape((n,) + tuple(s.shape)) for latent, s in compiled.program.slot_by_name.items()}
            r64, r32 = named_reference(build, n, "pathwise", noise)
            close(res["f"].cpu().numpy(), r64["f"], r32["f"], "f")
        else:
            res = compiled.evaluate(n, seed=seed, offset=offset)        # no noise, no outputs: the lean kernel draws for itself
        close(float(res["loss"].item()), r64["loss"], r32["loss"], "%s loss" % launch)
        grads = compiled.named_grads()
        assert ("theta" in grads) == (kind == "param")
        for pname, g in r64["grads"].items():
            close(grads[pname], or_zero(g, grads[pname]), or_zero(r32["grads"][pname], grads[pname]), "%s d/d%s" % (launch, pname),
                  theta_groups if pname == "theta" else None)
    # one SGD step on the draw of the same (seed, offset): theta' = theta - lr * gradient, for every parameter of the model
    before = compiled.named_params()
    compiled.iteration = offset
    losses, finite = compiled.train(1, n, "SGD", seed=seed, lr=lr)
    assert bool(finite.all())
    if engine_name == "specialised":
        assert compiled.last_mode == "persistent", compiled.last_mode        # the in-kernel loop, not a launch per iteration
    close(losses.cpu().numpy(), r64["loss"], r32["loss"], "training loss")
    after = compiled.named_params()
    for pname, g in r64["grads"].items():
        step = (before[pname].astype(np.float64) - after[pname]) / lr
        # the float32 store of theta' rounds the step by half an ulp of theta / lr
        slack = np.abs(before[pname]).reshape(-1) * float(np.finfo(F).eps) / lr
        got, g64, g32 = step.reshape(-1), or_zero(g, step).reshape(-1), or_zero(r32["grads"][pname], step).reshape(-1)
        tol = np.maximum(4.0 * np.abs(g32 - g64), 1e-5 * np.maximum(1.0, np.abs(g64))) + slack
        assert (np.abs(got - g64) <= tol).all(), (pname, compiled.last_mode, got, g64)


# ---- probs -> logits (BSVI_U_P2L): torch clamps with the eps of the DTYPE, so inside the clamp the reference is float32
EPS32 = float(np.finfo(F).eps)
P2L_EDGES = [0.0, 1.0, EPS32, float(F(1.0) - F(EPS32)), 1e-9, nxt(EPS32, 0.0), nxt(float(F(1.0) - F(EPS32)), 1.0)]


class _P2LFloat32(torch.autograd.Function):
    """torch.distributions.utils.probs_to_logits evaluated in float32 — value and derivative — inside a double graph"""

    @staticmethod
    def forward(ctx, probs):
        from torch.distributions.utils import probs_to_logits
        with torch.enable_grad():
            p32 = probs.detach().float().requires_grad_(True)
            logits = probs_to_logits(p32, is_binary=True)
            grad, = torch.autograd.grad(logits.sum(), p32)
        ctx.save_for_backward(grad.double())
        return logits.detach().double()

    @staticmethod
    def backward(ctx, g):
        return g * ctx.saved_tensors[0]


def test_reference_helper_clamps_like_torch_in_float32():
    """`_P2LFloat32`, the reference of the cases below, itself: gradient 0 outside the clamp, 8388609 = 1 / eps + 1 / (1 - eps) at
    both of its ends, value +-15.942384719848633 = logit(eps) (no kernel runs here)"""
    p = torch.tensor(P2L_EDGES, dtype=torch.float64, requires_grad=True)
    y = _P2LFloat32.apply(p)
    y.sum().backward()
    value, grad = y.detach().numpy(), p.grad.numpy()
    assert list(grad) == [0.0, 0.0, 8388609.0, 8388609.0, 0.0, 0.0, 0.0]
    assert list(value) == [-15.942384719848633, 15.942384719848633, -15.942384719848633, 15.942384719848633,
                           -15.942384719848633, -15.942384719848633, 15.942384719848633]


def build_p2l_model(api, dist, pts, total):
    """observed k ~ Bernoulli(probs = z) or Binomial(total, probs = z): the sampled value itself is the probability"""
    P = len(pts)
    col = lambda v: np.full((P, 1), v, dtype=np.float64)
    z = api.NormalVariable(col(0.0), col(1.0), "z")
    if dist == "bernoulli":
        k = api.BernulliVariable(probs=z, name="k")
        data = (np.arange(2 * P).reshape(2, P, 1) % 2).astype(F)           # a success and a failure at every point
        data[:, 1::2] = data[::-1, 1::2]
    else:
        k = api.BinomialVariable(total, probs=z, name="k")
        data = np.stack([np.zeros(P), np.full(P, total), np.arange(P) % (total + 1)]).reshape(3, P, 1).astype(F)
    model = api.ProbabilisticModel([k])
    k.observe(data)
    q = api.NormalVariable(api.RootVariable(col(0.0), "z_mean", learnable=True), api.RootVariable(col(1.0), "z_unit"), "z")
    model.set_posterior_model(api.ProbabilisticModel([q]))
    return model


@pytest.mark.parametrize("launch", ["diagnostic", "lean"])
@pytest.mark.parametrize("dist", ["bernoulli", "binomial"])
def test_p2l_matches_torch(dist, launch, engine_name, monkeypatch):
    """p2l: interior probabilities in [1e-3, 1 - 1e-3] against the oracle in double; at 0, 1, eps, 1 - eps, 1e-9 and one ulp
    outside either clamp end the reference is probs_to_logits in float32 EXACTLY (value and derivative), with the likelihood
    behind it in double: k = 0 and k = total at every point, so a clamp end that is one ulp off changes a gradient from
    0 to -1 (Bernoulli failure at p = eps: -sigmoid(logit) * 8388609) and a value from -15.94 to -20.72."""
    api = W.native_api()
    rng = np.random.RandomState(3)
    interior = np.concatenate([rng.uniform(1e-3, 1 - 1e-3, N_INTERIOR - 2), [1e-3, 1 - 1e-3]]).astype(F)[:, None]
    for n, total in ((3, 1), (65, 7)):
        compiled = check_launches(lambda: build_p2l_model(api, dist, interior, total), interior, n, "pathwise", launch, engine_name, True)
        assert ("UN", lowering.UNOP["p2l"]) in instructions(compiled.program)
    import torch.distributions.bernoulli as tb, torch.distributions.binomial as tn
    clamp32 = lambda probs, is_binary=False: _P2LFloat32.apply(probs)
    monkeypatch.setattr(tb, "probs_to_logits", clamp32)
    monkeypatch.setattr(tn, "probs_to_logits", clamp32)
    edges = np.asarray(P2L_EDGES, dtype=F)[:, None]
    compiled = check_launches(lambda: build_p2l_model(api, dist, edges, 200 if dist == "binomial" else 1), edges, len(edges), "pathwise",
                              launch, engine_name, True, groups=point_groups(len(edges), 0))
    assert ("UN", lowering.UNOP["p2l"]) in instructions(compiled.program)
