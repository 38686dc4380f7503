"""The covariance-expression emitter (mvn.cpp `emit_expression`) op by op: it has a value and derivative table of its own — the third
of the four definitions of the link operators (tests/test_gpu_link_ops.py holds the other three to the reference) — with `powf`,
`r = 1 / b; a * r` for a division and a softplus derivative without the `x > 20` arm.

A hand-written instruction list, as `gp_node` of tests/test_gpu_mvn.py writes one, through `native.mvn_desc` and the C ABI:
    C = 2 I + 0.2 * M * op(input)        D = 3, N = 37, M symmetric with spectral norm 0.4
positive definite while |op| < 25; every case checks that in the double reference before it trusts it.  log N(value | loc, C) and
the coefficient of the input per sample against torch.distributions.MultivariateNormal + autograd in double; the bound of
tests/test_gpu_mvn.py: max(4 x torch's own float32 error, 2e-6 of the scale) — at D = 3 the float32 yardstick is computed live
(no blocked LAPACK path, one thread's summation order).

`powi[0]` at x = 0, `pow[input ** 0]` and `pow[0 ** input]` are the cases where the plain rules imm * x ** (imm - 1) and
t * log(a) are 0 * inf and torch's derivative is 0."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from brancher_amd import lowering, workloads as W

pytestmark = pytest.mark.gpu

D, N = 3, 37
B, U = lowering.BINOP, lowering.UNOP


# name -> (instructions computing op from temp 1 (the input), torch function, input range, points that must be among the inputs)
def un(flag, imm=0.0):
    return [("UN", flag, 1, 0, imm)]


def bin_first(flag, k):        # input (op) k
    return [("IMM", 0, 0, 0, k), ("BIN", flag, 1, 2, 0.0)]


def bin_second(flag, k):       # k (op) input
    return [("IMM", 0, 0, 0, k), ("BIN", flag, 2, 1, 0.0)]


CASES = {
    "copy": (un(U["copy"]), lambda x: x, (-3, 3), [0.0]),
    "neg": (un(U["neg"]), lambda x: -x, (-3, 3), [0.0]),
    "exp": (un(U["exp"]), torch.exp, (-3, 2.5), [-104.0]),
    "log": (un(U["log"]), torch.log, (0.05, 20), [1.0, 0.01]),
    "sqrt": (un(U["sqrt"]), torch.sqrt, (0.05, 20), [1.0, 400.0]),
    "sin": (un(U["sin"]), torch.sin, (-6, 6), [0.0, float(np.float32(np.pi)), 1e4]),
    "cos": (un(U["cos"]), torch.cos, (-6, 6), [0.0, float(np.float32(np.pi)), 1e4]),
    "tanh": (un(U["tanh"]), torch.tanh, (-4, 4), [20.0, -20.0]),
    "abs": (un(U["abs"]), torch.abs, (-3, 3), [0.0]),
    "sigmoid": (un(U["sigmoid"]), torch.sigmoid, (-6, 6), [20.0, -20.0, 90.0]),
    # (the derivative here is sigmoid(x) without the `x > 20` arm of `unop_grad`: in float32 sigmoid(x) IS 1 beyond 17)
    "softplus": (un(U["softplus"]), torch.nn.functional.softplus, (-6, 6), [20.0, float(np.nextafter(np.float32(20), np.float32(21))), 22.0, -104.0]),
    "reciprocal": (un(U["reciprocal"]), torch.reciprocal, (0.1, 5), [1.0, -0.25, 1e6]),
    "square": (un(U["square"]), torch.square, (-3, 3), [0.0, 4.5]),
    "powi[3]": (un(U["powi"], 3.0), lambda x: x ** 3.0, (-2, 2), [0.0, -2.5]),
    "powi[-2]": (un(U["powi"], -2.0), lambda x: x ** -2.0, (0.4, 3), [-0.5]),
    "powi[1.5]": (un(U["powi"], 1.5), lambda x: x ** 1.5, (0.05, 5), [0.0]),
    "powi[0]": (un(U["powi"], 0.0), lambda x: x ** 0.0, (-3, 3), [0.0]),
    "powi[1]": (un(U["powi"], 1.0), lambda x: x ** 1.0, (-3, 3), [0.0]),
    "sub[input - k]": (bin_first(B["sub"], 0.75), lambda x: x - 0.75, (-3, 3), []),
    "sub[k - input]": (bin_second(B["sub"], 0.75), lambda x: 0.75 - x, (-3, 3), []),
    "truediv[input / k]": (bin_first(B["truediv"], -1.6), lambda x: x / -1.6, (-3, 3), []),
    "truediv[k / input]": (bin_second(B["truediv"], 1.3), lambda x: 1.3 / x, (0.1, 5), [-0.2, 1e6]),
    "pow[input ** k]": (bin_first(B["pow"], 2.5), lambda x: x ** 2.5, (0.05, 3), [0.0]),
    "pow[input ** 0]": (bin_first(B["pow"], 0.0), lambda x: x ** torch.zeros_like(x), (0.05, 3), [0.0]),
    "pow[k ** input]": (bin_second(B["pow"], 1.7), lambda x: 1.7 ** x, (-3, 3), [0.0]),
    "pow[0 ** input]": (bin_second(B["pow"], 0.0), lambda x: torch.zeros_like(x) ** x, (0.2, 3), [0.0]),
}
REFUSED_UN = ["relu", "log1p", "expm1", "p2l"]


def matrices():
    rng = np.random.RandomState(5)
    a = rng.normal(0.0, 1.0, (D, D))
    m = a + a.T
    m *= 0.4 / np.abs(np.linalg.eigvalsh(m)).max()
    return np.stack([m, 2.0 * np.eye(D)]).astype(np.float32)


def node_for(op_code):
    # temps: 0 = M, 1 = input, 2.. = op, then 0.2 * M * op + 2 I
    k = 2 + len(op_code)
    code = [("MAT", 0, 0, 0, 0.0), ("INPUT", 0, 0, 0, 0.0)] + list(op_code) + [
        ("IMM", 0, 0, 0, 0.2), ("BIN", B["mul"], 0, k, 0.0), ("BIN", B["mul"], k + 1, k - 1, 0.0), ("MAT", 0, 1, 0, 0.0),
        ("BIN", B["add"], k + 2, k + 3, 0.0)]
    rng = np.random.RandomState(9)
    return types.SimpleNamespace(code=code, mats=matrices(), loc=rng.normal(0.0, 0.3, D).astype(np.float32),
                                 value=rng.normal(0.0, 1.0, D).astype(np.float32), dim=D,
                                 uniform_inputs=np.zeros(0, dtype=lowering.UNIFORM_DTYPE), slot_inputs=[0], weight=1.0)


def inputs_for(name):
    _, _, (lo, hi), must = CASES[name]
    rng = np.random.RandomState(sum(ord(ch) for ch in name))
    return np.concatenate([must, rng.uniform(lo, hi, N - len(must))]).astype(np.float32)


def reference(name, node, x, dtype):
    fn = CASES[name][1]
    x_t = torch.tensor(x.astype(np.float64), dtype=dtype, requires_grad=True)
    mats = torch.tensor(node.mats.astype(np.float64), dtype=dtype)
    cov = mats[1][None] + 0.2 * mats[0][None] * fn(x_t)[:, None, None]
    if dtype == torch.float64:       # the premise of the case: finite and positive definite, with room to spare
        eig = np.linalg.eigvalsh(cov.detach().numpy())
        assert np.isfinite(eig).all() and eig.min() > 0.5, (name, eig.min())
    lp = torch.distributions.MultivariateNormal(torch.tensor(node.loc.astype(np.float64), dtype=dtype), covariance_matrix=cov) \
        .log_prob(torch.tensor(node.value.astype(np.float64), dtype=dtype).expand(N, D))
    lp.sum().backward()
    return lp.detach().double().numpy(), x_t.grad.double().numpy()


@pytest.mark.parametrize("name", list(CASES))
def test_covariance_expression_op_matches_torch_double(name):
    from brancher_amd import native
    lib = native.load()
    dev = torch.device("cuda:0")
    node, x = node_for(CASES[name][0]), inputs_for(name)
    lp64, g64 = reference(name, node, x, torch.float64)
    lp32, g32 = reference(name, node, x, torch.float32)
    assert np.isfinite(lp64).all() and np.isfinite(g64).all()
    d, keep = native.mvn_desc(node)
    handle = C.c_void_p()
    native.check(lib.bsvi_mvn_create(C.byref(d), C.byref(handle)))
    assert int(lib.bsvi_mvn_rows_out(C.byref(d))) == 2
    samples = torch.zeros(4, N)
    samples[2] = torch.from_numpy(x)
    samples_d, params_d = samples.to(dev), torch.zeros(4, device=dev)
    out = torch.full((2, N), float("nan"), device=dev)
    args = native.MvnArgs(params_dev=params_d.data_ptr(), samples_dev=samples_d.data_ptr(), rows_out_dev=out.data_ptr(),
                          n_samples_local=N, value_row0=0, stream=None)
    args.input_rows[0] = 2
    native.check(lib.bsvi_mvn_eval(handle, C.byref(args)))
    torch.cuda.synchronize()
    got = out.cpu().double().numpy()
    lib.bsvi_mvn_destroy(handle)
    # rows: the coefficient of the input, then e with  e + coefficient * input = log p
    lp = got[1] + got[0] * x.astype(np.float64)
    for mine, ref, ref32, key in ((got[0], g64, g32, "d/dinput"), (lp, lp64, lp32, "log p")):
        scale = np.abs(ref).max() + 1e-30
        err, yard = np.abs(mine - ref).max() / scale, np.abs(ref32 - ref).max() / scale
        print("%s %s: err %.3g, torch float32 %.3g (of the scale %.3g)" % (name, key, err, yard, scale))
        assert err <= max(4.0 * yard, 2e-6), (name, key, err, yard, mine, ref)


def refused_node(kind, flag):
    return node_for([(kind, flag, 1, 1 if kind == "BIN" else 0, 0.0)])


@pytest.mark.parametrize("name", REFUSED_UN + ["delta"])
def test_ops_without_a_derivative_rule_are_refused_by_the_library(name):
    """relu, log1p, expm1, p2l and delta have no rule in the emitter: `bsvi_mvn_create` says so, it does not emit something else"""
    from brancher_amd import native
    lib = native.load()
    node = refused_node("BIN", B["delta"]) if name == "delta" else refused_node("UN", U[name])
    d, keep = native.mvn_desc(node)
    handle = C.c_void_p()
    with pytest.raises(native.NativeError) as info:
        native.check(lib.bsvi_mvn_create(C.byref(d), C.byref(handle)))
    assert ("binary" if name == "delta" else "unary") + " op without a derivative rule in a covariance expression" in str(info.value)
    assert not handle.value


def covariance_model(api, link, n=12):
    """(12 elements: up to 10 the lowering unrolls the term into the per-sample program, beyond it the batched kernel serves it)"""
    rng = np.random.RandomState(0)
    a = rng.normal(0.0, 1.0, (n, n))
    m = api.RootVariable((0.4 * (a + a.T) / np.abs(np.linalg.eigvalsh(a + a.T)).max()).astype(np.float32), "m")
    eye = api.RootVariable((2.0 * np.eye(n)).astype(np.float32), "eye")
    s = api.LogNormalVariable(-0.5, 0.3, "s")
    f = api.MultivariateNormalVariable(loc=np.zeros((n,)), covariance_matrix=m * 0.2 * link(api.BF, s) + eye, name="f")
    y = api.NormalVariable(f, 0.3, name="y")
    model = api.ProbabilisticModel([y])
    y.observe(rng.normal(0.0, 1.0, (1, n)).astype(np.float32))
    model.set_posterior_model(api.ProbabilisticModel([api.LogNormalVariable(-0.4, 0.2, "s", learnable=True),
                                                      api.NormalVariable(loc=np.zeros((n,)), scale=0.8, name="f", learnable=True)]))
    return model


@pytest.mark.parametrize("name", ["relu", "log1p", "expm1", "delta"])
def test_ops_without_a_derivative_rule_are_refused_by_the_lowering(name):
    """the same refusal one level up: a covariance link with such an op raises a LoweringError that names it (p2l is no link
    function: only `probs=` of a Binomial / Bernoulli lowers to it), while the same model with tanh lowers to the batched kernel"""
    api = W.native_api()
    link = (lambda BF, s: BF.delta(s, 1.0)) if name == "delta" else (lambda BF, s: getattr(BF, name)(s))
    with pytest.raises(lowering.LoweringError) as info:
        lowering.lower(covariance_model(api, link), None, "pathwise")
    assert name in str(info.value) and "covariance expression is not served by the batched kernel" in str(info.value)
    program = lowering.lower(covariance_model(api, lambda BF, s: BF.tanh(s)), None, "pathwise")
    assert len(program.externals) == 1
