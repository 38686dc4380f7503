"""The noise the kernels DRAW against the host reference of the stream (oracle/philox_ref.py) — not the noise they report
against itself.  Every other parity test replays the draws a launch reports; a kernel that drew the wrong noise and reported
it faithfully passed them all.  Here:

  words       device Philox words, bit for bit (bsvi_debug_math fn 7)
  transforms  u01 bit for bit, Box-Muller (library and hardware units), Cauchy and Laplace base noise at the extreme words
              and on random ones (fn 8); the reparameterised draw and its adjoints on supplied noise (fn 5)
  streams     the noise every path reports = the predictor's: interpreter, specialised, dense (fused and six launches), BNN,
              amortised (with its per-sample minibatch rows) — each of them at sample counts 1, 63, 64, 65, 300, 1500, 4096 with
              two seeds x five offsets, and as two- and three-shard splits with a non-zero sample base; the dense path's
              784 x 10 shape at 24 samples only (7840 noise rows); the scalar gather's minibatch rows; the reduce node's data
  carry       training across offset 2^32 in every launch mode
  oracle      the oracle on PREDICTED noise against training that draws in the kernel: the loop the benchmark times

Bounds.  Words, u01, Bernoulli draws and minibatch rows: exact.  Normal draws: absolute error against the double-precision
reference <= 16 x the error of the same formula in single precision on the host (the hardware log / sin / cos units are
specified looser than libm, and the sin / cos error is absolute), never above 1e-4 — a structural mistake (wrong row, swapped
pair, wrong counter word) is an error of order 1.  Cauchy: compared as ANGLES (the tangent is ill-conditioned at the ends):
4 ulp of pi/2.  Laplace: 4 ulp of 1.  Beta: a rejection decision at a single / double precision borderline may flip — draws that
differ by more than 1e-4 are counted, at most 0.1 % of them (the reference's own single-against-double rate is under a quarter
of that: tests/test_noise_reference_cpu.py).

Measured on an MI355X (every test prints its figures: `pytest -s`).  Yardstick — Box-Muller in single precision on the host
against double precision, 2^16 samples x 8 rows: 1.55e-06, so the Normal bound is 2.48e-05.  Device, 2^16 random word pairs:
Box-Muller on the hardware units 7.95e-07, with the library functions 1.61e-06; Cauchy angle 1.19e-07 (bound 4.77e-07); Laplace
2.98e-08 (bound 2.38e-07).  Streams, worst over all sizes, seeds and offsets: Normal rows of the scalar engines 5.9e-07, of the
dense / BNN path 8.3e-07, of the amortised path 1.1e-06, LogNormal 1.3e-06, Beta 6.0e-07 with none of ~400 000 draws left out.
Training on in-kernel draws against the oracle on predicted noise: loss curves within 3e-07 relative, parameters within 2.4e-07.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import rel_err, yardstick_grad_check
from brancher_amd import distributions as D
from brancher_amd import engine, native, workloads as W
from oracle import philox_ref as R

pytestmark = pytest.mark.gpu

SEEDS = (1234, 0x1234567890ABC)                                  # the second one has a high word
OFFSETS = (0, 7, (1 << 32) - 1, 1 << 32, (1 << 62) + 3)
SIZES = (1, 63, 64, 65, 300, 1500, 4096)
EDGE_WORDS = (0, 0xff, 0x7fffff00, 0x80000000, 0xfffffe00, 0xffffff00, 0xffffffff)
CAUCHY_ANGLE_TOL = 4 * float(np.spacing(np.float32(np.pi / 2)))
LAPLACE_TOL = 4 * 2.0 ** -24
BETA_TOL, BETA_LEFT_OUT = 1e-4, 1e-3
TOL = 1e-5                                                       # test_gpu_parity's, for the trajectories


def _normal_yardstick():
    """the error of Box-Muller evaluated in single precision on the host, against double precision: 2^16 samples x 8 rows"""
    s = np.arange(1 << 16)
    return float(np.abs(R.normal_rows(SEEDS[1], 3, s, np.arange(8), dtype=np.float32).astype(np.float64)
                        - R.normal_rows(SEEDS[1], 3, s, np.arange(8))).max())


NORMAL_YARDSTICK = _normal_yardstick()
NORMAL_TOL = min(16 * NORMAL_YARDSTICK, 1e-4)


# ---- the hook ----------------------------------------------------------------------------------------------------------
def hook(fn, dist, x, p0, p1):
    """bsvi_debug_math on three arrays of 32-bit words (float32 values or uint32 bit patterns) -> uint32 [4, n]"""
    lib, dev = native.load(), torch.device("cuda:0")
    n = len(x)
    bits = lambda v: torch.from_numpy(np.ascontiguousarray(v).view(np.int32).copy()).to(dev)
    xs, a, b = (bits(np.asarray(v, dtype=np.float32) if np.asarray(v).dtype.kind == "f" else np.asarray(v, dtype=np.uint32))
                for v in (x, p0, p1))
    out = torch.zeros(4 * n, device=dev, dtype=torch.int32)
    native.check(lib.bsvi_debug_math(fn, dist, C.c_void_p(xs.data_ptr()), C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()),
                                     C.c_void_p(out.data_ptr()), n, None))
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32).reshape(4, n)


def device_philox(c0, c1, c2, c3, k0, k1):
    u = lambda *v: np.concatenate([np.asarray(w, dtype=np.uint32) for w in v])
    m = len(c0)
    return hook(native.DEBUG_MATH_PHILOX_WORDS, 0, u(c0, c1), u(c2, c3), u(k0, k1))[:, :m]


def test_device_philox_words_equal_the_reference():
    rng = np.random.RandomState(7)
    m = 1 << 16
    c = [rng.randint(0, 1 << 32, m, dtype=np.uint64).astype(np.uint32) for _ in range(6)]
    got = device_philox(*c)
    want = np.stack(R.philox4x32(*c))
    assert np.array_equal(got, want)
    # corners: all zero, all ones, a carry out of every multiplier word, high words of seed and offset alone
    F = 0xffffffff
    corners = [(0, 0, 0, 0, 0, 0), (F, F, F, F, F, F), (F, 0, F, 0, 0, 0), (0, F, 0, F, 0, 0), (0x80000000, 0, 0x80000000, 0, F, F),
               (1, 0x80000000, 0, 0, 5, 0), (1, 0x80000000, 0, 1, 5, 0), (1, 0x80000000, 0, 0, 5, 1), (1, 0x80000000, F, 0, 5, 0),
               (1, 0x80000000, 0, 0x40000000, 5, 0x12345), (1, 0x40000000, 3, 0x40000000, F, 0x7fffffff)]
    cc = np.array(corners, dtype=np.uint32).T
    assert np.array_equal(device_philox(*cc), np.stack(R.philox4x32(*cc)))
    assert len({tuple(w) for w in device_philox(*cc).T}) == len(corners)           # seed_hi and offset_hi each change the block


def transforms(a, b):
    a, b = np.asarray(a, dtype=np.uint32), np.asarray(b, dtype=np.uint32)
    q0, q1 = (hook(native.DEBUG_MATH_NOISE_TRANSFORMS, d, a, b, b).view(np.float32) for d in (0, 1))
    return dict(u01=q0[0], bm=(q0[1], q0[2]), cauchy=q0[3], laplace=q1[0], bm_fast=(q1[1], q1[2]), u01_b=q1[3])


def check_transforms(a, b, label):
    t = transforms(a, b)
    assert np.array_equal(t["u01"].view(np.uint32), R.u01(a).view(np.uint32)), label
    assert np.array_equal(t["u01_b"].view(np.uint32), R.u01(b).view(np.uint32)), label
    for name in ("bm", "bm_fast", "cauchy", "laplace"):
        for v in (t[name] if isinstance(t[name], tuple) else (t[name],)):
            assert np.all(np.isfinite(v)), (label, name, [hex(int(w)) for w in np.asarray(a)[~np.isfinite(v)][:4]])
    z = R.box_muller(a, b)
    errs = {}
    for name in ("bm", "bm_fast"):
        errs[name] = max(np.abs(t[name][j].astype(np.float64) - z[j]).max() for j in (0, 1))
    errs["cauchy"] = np.abs(np.arctan(t["cauchy"].astype(np.float64)) - np.clip(R.cauchy_angle(a), -np.pi / 2, np.pi / 2)).max()
    errs["laplace"] = np.abs(t["laplace"].astype(np.float64) - R.laplace_noise(a)).max()
    print("%s: |device - reference|: Box-Muller libm %.3g, hardware units %.3g (host single-precision yardstick %.3g, bound %.3g); "
          "Cauchy angle %.3g (bound %.3g); Laplace %.3g (bound %.3g)" % (label, errs["bm"], errs["bm_fast"], NORMAL_YARDSTICK, NORMAL_TOL,
                                                                       errs["cauchy"], CAUCHY_ANGLE_TOL, errs["laplace"], LAPLACE_TOL))
    assert errs["bm"] <= NORMAL_TOL and errs["bm_fast"] <= NORMAL_TOL, (label, errs)
    assert errs["cauchy"] <= CAUCHY_ANGLE_TOL and errs["laplace"] <= LAPLACE_TOL, (label, errs)
    # the supports: Laplace base noise in [eps - 1, 1) (log1p(-|e|) finite), the Cauchy angle inside (-pi/2, pi/2): the sign of the
    # tangent is the sign of u - 1/2
    lap = t["laplace"].astype(np.float64)
    assert lap.min() >= R.FLOAT_EPS - 1.0 and lap.max() < 1.0, label
    # ... so the DRAWS made from this base noise are finite (Laplace: loc - scale * sign(e) * log1p(-|e|))
    one, zero = np.ones(len(a), dtype=np.float32), np.zeros(len(a), dtype=np.float32)
    for dist, e in ((D.DIST_LAPLACE, t["laplace"]), (D.DIST_CAUCHY, t["cauchy"])):
        draw = hook(5, dist, e, zero, one).view(np.float32)
        assert np.all(np.isfinite(draw)), (label, dist)
    side = np.sign(R.u01(a).astype(np.float64) - 0.5)
    assert np.all(np.sign(t["cauchy"])[side != 0] == side[side != 0]), label


def test_transforms_of_the_extreme_words():
    """u01 reaches exactly 1.0f at the top words: every transform must stay finite and inside its support there"""
    a, b = (v.reshape(-1) for v in np.meshgrid(np.array(EDGE_WORDS, dtype=np.uint32), np.array(EDGE_WORDS, dtype=np.uint32)))
    assert R.u01(np.uint32(0xffffff00)) == 1.0
    check_transforms(a, b, "edge words")


def test_transforms_of_random_words():
    rng = np.random.RandomState(11)
    a, b = (rng.randint(0, 1 << 32, 1 << 16, dtype=np.uint64).astype(np.uint32) for _ in range(2))
    check_transforms(a, b, "2^16 random words")


# ---- the reparameterised draw on supplied noise (fn 5) ---------------------------------------------------------------------
def torch_draw(dist, p0, p1, e, dtype):
    a, b = (torch.tensor(np.asarray(v, dtype=np.float32), dtype=dtype, requires_grad=True) for v in (p0, p1))
    t = torch.tensor(np.asarray(e, dtype=np.float32), dtype=dtype)
    if dist == D.DIST_BETA:
        # the draw is its own noise; implicit reparameterisation (torch dirichlet.py _Dirichlet_backward on x = [z, 1 - z])
        x, conc = torch.stack([t, 1 - t], -1), torch.stack([a, b], -1).detach()
        g = torch._dirichlet_grad(x, conc, conc.sum(-1, True).expand_as(conc))
        go = torch.tensor([1.0, 0.0], dtype=dtype)
        g = g * (go - (x * go).sum(-1, True))
        return dict(value=t.numpy(), d_p0=g[:, 0].numpy(), d_p1=g[:, 1].numpy())
    if dist in (D.DIST_NORMAL, D.DIST_CAUCHY):
        v = a + t * b
    elif dist == D.DIST_LOGNORMAL:
        v = torch.exp(a + t * b)
    elif dist == D.DIST_LAPLACE:
        v = a - b * torch.sign(t) * torch.log1p(-t.abs())           # torch laplace.py rsample
    else:
        v = a + 0 * b
    v.sum().backward()
    return dict(value=v.detach().numpy(), d_p0=a.grad.numpy(), d_p1=b.grad.numpy())


def draw_cases():
    rng = np.random.RandomState(5)
    n = 512
    loc, scale, eps = rng.normal(0, 2, n), np.exp(rng.uniform(-2, 1.5, n)), rng.normal(0, 1, n)
    top = float(np.float32(1.0 - 2.0 ** -24))
    lap = np.concatenate([[0.0, -0.0, top, -top, R.FLOAT_EPS - 1.0, 1 - 1e-3, 1e-3 - 1, 1e-30, -1e-30], rng.uniform(-1, 1, n - 9)])
    yield "normal", D.DIST_NORMAL, loc, scale, eps
    yield "normal, far tails", D.DIST_NORMAL, loc, scale, eps * 6
    yield "lognormal", D.DIST_LOGNORMAL, loc * 0.5, scale * 0.3, eps
    yield "lognormal near overflow", D.DIST_LOGNORMAL, np.full(n, 86.5), np.full(n, 1.5), rng.uniform(0, 1, n)    # up to exp(88): 1.7e38
    yield "lognormal near underflow", D.DIST_LOGNORMAL, np.full(n, -80.0), np.full(n, 1.5), -rng.uniform(0, 4.5, n)
    yield "cauchy", D.DIST_CAUCHY, loc, scale, np.tan(np.pi * (rng.uniform(0, 1, n) - 0.5))
    yield "cauchy at the ends of the angle", D.DIST_CAUCHY, loc, scale, np.tan(np.float32(1.57079625)) * rng.choice([-1.0, 1.0], n)
    yield "laplace", D.DIST_LAPLACE, loc, scale, lap
    yield "laplace |e| close to 1", D.DIST_LAPLACE, loc, scale, np.sign(eps) * (1 - np.exp(rng.uniform(np.log(2.0 ** -24), np.log(1e-3), n)))
    yield "deterministic", D.DIST_DETERMINISTIC, loc, scale, eps
    nb = 4000                                                      # every branch of dirichlet_grad_one (test_gpu_math's coverage)
    alpha, beta = (np.exp(rng.uniform(np.log(0.1), np.log(40), nb)) for _ in range(2))
    z = rng.beta(alpha, beta).clip(1e-6, 1 - 1e-6)
    for label, sel in (("small z", z < 0.1), ("middle", (z >= 0.1) & (z <= 0.9)), ("large z", z > 0.9),
                       ("both concentrations large", (alpha > 6) & (beta > 6)), ("one concentration below one", (alpha < 1) | (beta < 1))):
        assert sel.sum() > 50
        yield "beta, " + label, D.DIST_BETA, alpha[sel], beta[sel], z[sel]


@pytest.mark.parametrize("case", list(draw_cases()), ids=lambda c: c[0])
def test_reparameterised_draw_and_adjoints_on_supplied_noise(case):
    """sample_from_noise_generic / sample_bwd_generic against torch in double precision; the bound is the suite's yardstick rule:
    as close to it as torch in single precision is (x4), or 1e-5 of the scale"""
    label, dist, p0, p1, e = case
    p0, p1, e = (np.asarray(v, dtype=np.float32) for v in (p0, p1, e))
    got = hook(5, dist, e, p0, p1).view(np.float32).astype(np.float64)
    exact, single = torch_draw(dist, p0, p1, e, torch.float64), torch_draw(dist, p0, p1, e, torch.float32)
    assert all(np.all(np.isfinite(v)) for v in exact.values()), label
    named = dict(value=got[0], d_p0=got[2], d_p1=got[3])
    assert all(np.all(np.isfinite(v)) for v in named.values()), label
    for k in named:
        print("%s %s: |device - double| %.3g, |single - double| %.3g, scale %.3g" % (
            label, k, np.abs(named[k] - exact[k]).max(), np.abs(single[k] - exact[k]).max(), np.abs(exact[k]).max()))
    # (per output: one scale for value and adjoints together would let the largest of them hide the others)
    for k in named:
        yardstick_grad_check({k: named[k]}, {k: exact[k]}, {k: single[k]})


# ---- streams: what a launch reports against the predictor --------------------------------------------------------------
def softplus32(raw):
    raw = np.float32(raw)
    return float(raw if raw > 20 else np.log1p(np.exp(raw, dtype=np.float32), dtype=np.float32))


def program_rows(c):
    """(row, dist, p0, p1) of every noise row of a scalar program; the parameters of the draws that are their own noise come
    from the model's CURRENT parameter values"""
    par = {k: np.asarray(v, dtype=np.float32).reshape(-1) for k, v in c.named_params().items()}
    rows = []
    for name, s in c.program.slot_by_name.items():
        for j in range(s.size):
            if s.dist == D.DIST_BETA:
                p0, p1 = softplus32(par[name + "_concentration1"][j]), softplus32(par[name + "_concentration0"][j])
            elif s.dist == D.DIST_BERNOULLI:
                p0, p1 = par[name + "_logits"][j], 0.0
            elif s.dist == D.DIST_BINOMIAL:
                p0, p1 = par[name + "_total_count"][j], par[name + "_logits"][j]
            else:
                p0 = p1 = 0.0
            rows.append((s.base + j, s.dist, p0, p1))
    return rows


class StreamCheck:
    """compares reported rows with predicted ones under the module's bounds and keeps the worst figures"""

    def __init__(self):
        self.worst = {}
        self.beta_total = self.beta_out = 0

    def row(self, dist, got, want, where):
        got = np.asarray(got, dtype=np.float64)
        assert got.shape == want.shape and np.all(np.isfinite(got)), where
        if dist in (D.DIST_NORMAL, D.DIST_LOGNORMAL):
            err, tol = np.abs(got - want).max(), NORMAL_TOL
        elif dist == D.DIST_CAUCHY:
            err, tol = np.abs(np.arctan(got) - np.arctan(want)).max(), CAUCHY_ANGLE_TOL
        elif dist == D.DIST_LAPLACE:
            err, tol = np.abs(got - want).max(), LAPLACE_TOL
        elif dist == D.DIST_BETA:
            bad = np.abs(got - want) > BETA_TOL
            self.beta_total += got.size
            self.beta_out += int(bad.sum())
            err, tol = (np.abs(got - want)[~bad].max() if (~bad).any() else 0.0), BETA_TOL
        else:
            err, tol = np.abs(got - want).max(), 0.0
        self.worst[dist] = max(self.worst.get(dist, 0.0), float(err))
        assert err <= tol, (where, dist, err, tol)

    def finish(self, label):
        print(label, "worst |reported - predicted| per distribution code:", {k: "%.3g" % v for k, v in sorted(self.worst.items())},
              "Beta draws left out: %d of %d" % (self.beta_out, self.beta_total))
        assert self.beta_out <= BETA_LEFT_OUT * self.beta_total, (self.beta_out, self.beta_total)


def set_beta(c, name, alpha, beta):
    inv = lambda v: np.array([np.log(np.expm1(v))], dtype=np.float32)
    for par, off, size, _ in c.program.parameters:
        if par.name == name + "_concentration1":
            c.write_params(off, inv(alpha))
        if par.name == name + "_concentration0":
            c.write_params(off, inv(beta))


SCALAR_MODELS = [
    ("build_readme_ar", dict(T=20), "pathwise", None),
    ("build_heavy_tails", dict(n_obs=12), "pathwise", None),
    ("build_beta_binomial", dict(n_obs=30), "pathwise", None),                  # Beta(1, 1): both gammas on the alpha >= 1 branch
    ("build_beta_binomial", dict(n_obs=30), "pathwise", (0.3, 0.7)),            # both below one: the boost draw
    ("build_beta_binomial", dict(n_obs=30), "pathwise", (40.0, 0.5)),
    ("build_beta_binomial", dict(n_obs=30), "pathwise", (2.0, 5.0)),
    ("build_beta_ar", dict(T=20), "pathwise", None),
    ("build_discrete_latent", dict(n_obs=8), "blackbox", None),
    ("build_cauchy_binomial_latents", dict(total=13), "blackbox", None),
    ("build_cauchy_binomial_latents", dict(total=7), "blackbox", None),
]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("jit", ["0", "1"], ids=["interpreter", "specialised"])
@pytest.mark.parametrize("builder,kwargs,estimator,beta", SCALAR_MODELS,
                         ids=[m[0][6:] + ("" if m[3] is None else "_%g_%g" % m[3]) + ("_%d" % m[1]["total"] if "total" in m[1] else "")
                              for m in SCALAR_MODELS])
def test_scalar_engines_report_the_predicted_noise(builder, kwargs, estimator, beta, jit, n, monkeypatch):
    monkeypatch.setenv("BSVI_JIT", jit)
    c = engine.compile_model(getattr(W, builder)(W.native_api(), **kwargs), None, estimator)
    if beta is not None:
        set_beta(c, "p", *beta)
    served = c.native.engine(n, 0)["engine"]
    assert served == ("specialised" if jit == "1" else "interpreter"), served      # no quiet fall-back: each engine's own draw sites
    rows = program_rows(c)
    assert len(rows) == c.program.n_noise
    check = StreamCheck()
    for seed in SEEDS:
        for offset in OFFSETS:
            got = c.evaluate(n, seed=seed, offset=offset, want_noise=True)["noise"].cpu().numpy()
            want = R.scalar_noise(rows, seed, offset, 0, n)
            for row, dist, _, _ in rows:
                check.row(dist, got[row], want[row], (builder, served, n, hex(seed), hex(offset), row))
    check.finish("%s %s n=%d:" % (builder, served, n))


@pytest.mark.parametrize("jit", ["0", "1"], ids=["interpreter", "specialised"])
@pytest.mark.parametrize("builder,kwargs,n,splits", [
    ("build_readme_ar", dict(T=20), 3000, ((0, 1300), (1300, 1700))),
    ("build_readme_ar", dict(T=20), 3000, ((0, 65), (65, 2871), (2936, 64))),
    ("build_heavy_tails", dict(n_obs=12), 1000, ((0, 1), (1, 999))),
    ("build_beta_ar", dict(T=20), 640, ((0, 300), (300, 340))),
])
def test_shards_report_the_noise_of_their_global_samples(builder, kwargs, n, splits, jit, monkeypatch):
    """a shard (sample_base, n_local) of a launch over n samples draws the noise of samples base .. base + n_local - 1: the base is
    applied once, and nothing else of the shard's geometry enters the counter"""
    monkeypatch.setenv("BSVI_JIT", jit)
    c = engine.compile_model(getattr(W, builder)(W.native_api(), **kwargs), None, "pathwise")
    rows = program_rows(c)
    check = StreamCheck()
    seed, offset = SEEDS[1], OFFSETS[4]
    for base, n_local in splits:
        noise_o = torch.zeros((c.program.n_noise, n_local), device=c.device)
        c.native.ensure_shares(n_local)
        c.native.attach_shares()
        args = c._elbo_args(n_local, n, base, None, seed, offset, None, noise_o, None)
        native.check(c.lib.bsvi_elbo_fwd_bwd(c.native.handle, C.byref(args)))
        torch.cuda.synchronize()
        got, want = noise_o.cpu().numpy(), R.scalar_noise(rows, seed, offset, base, n_local)
        for row, dist, _, _ in rows:
            check.row(dist, got[row], want[row], (builder, jit, base, n_local, row))
    check.finish("%s shards %s:" % (builder, splits))


# ---- the matrix paths: dense, BNN, amortised — every one has its own sample_base arithmetic ------------------------------------
FWD_BWD = dict(CompiledDense="bsvi_dense_fwd_bwd", CompiledBnn="bsvi_bnn_fwd_bwd", CompiledAmortized="bsvi_amort_fwd_bwd")


def launch_shard(c, n_local, n_global, base, seed, offset):
    """one forward / backward launch of a dense, BNN or amortised model over the shard (base, n_local) of n_global samples, through
    the argument block a rank of a sharded run fills: -> (reported noise, reported minibatch rows)"""
    kind = type(c).__name__
    amortised = kind == "CompiledAmortized"
    p, dev = c.program, c.device
    noise_o = torch.zeros((n_local * p.batch_size, p.latent_dim) if amortised else (p.n_noise, n_local), device=dev)
    idx_o = torch.full((n_local, p.batch_size) if amortised else (p.batch_size,), -7, device=dev, dtype=torch.int32)
    args = c._args(n_local, n_global, base, None, None, seed, offset, noise_o, idx_o)
    native.check(getattr(c.lib, FWD_BWD[kind])(c.handle, C.byref(args)))
    torch.cuda.synchronize()
    return noise_o.cpu().numpy(), idx_o.cpu().numpy()


def check_matrix_path(c, check, n_local, n_global, base, seed, offset, ds, where):
    got, idx = launch_shard(c, n_local, n_global, base, seed, offset)
    p = c.program
    if type(c).__name__ == "CompiledAmortized":
        want = R.amortized_noise(seed, offset, base, n_local, p.batch_size, p.latent_dim)
        samples = np.arange(base, base + n_local, dtype=np.uint64)[:, None]
        rows = R.minibatch_row(seed, offset, ds, samples, np.broadcast_to(np.arange(p.batch_size), (n_local, p.batch_size)))
    else:
        want = R.dense_noise(seed, offset, base, n_local, p.n_noise)
        rows = R.minibatch_index(seed, offset, ds, np.arange(p.batch_size))          # one minibatch for all samples: no base in it
    check.row(D.DIST_NORMAL, got, want, where)
    assert np.array_equal(idx, rows), where


DENSE_SMALL = dict(dataset_size=300, batch_size=130, n_features=100, n_classes=3)
BNN_SMALL = dict(dataset_size=40, batch_size=17, n_features=64, n_hidden=9, hidden2=6, n_classes=5, q_scale1=3e-3, q_loc_scale=1.0,
                 activation="relu")
VAE_SMALL = dict(dataset_size=80, batch_size=10, n_features=96, hidden1=160, hidden2=48, seed=5)
# (base, n_local) of a run over n_global samples: ragged shards, a one-sample shard, a base that is no multiple of anything
SPLITS = [(3000, ((0, 1300), (1300, 1700))), (3000, ((0, 65), (65, 2871), (2936, 64))), (130, ((0, 1), (1, 63), (64, 66)))]


def matrix_model(path, monkeypatch, **kw):
    api = W.native_api()
    if path.startswith("dense"):
        monkeypatch.setenv("BSVI_DENSE_FUSED", "0" if path == "dense-six-launch" else "1")
        c = engine.compile_model(W.build_logistic_regression(api, pixels="uint8", q_scale=0.02, **dict(DENSE_SMALL, **kw)), None, "pathwise")
        return c, dict(DENSE_SMALL, **kw)["dataset_size"], "CompiledDense"
    if path == "bnn":
        return engine.compile_model(W.build_bayesian_neural_network(api, **BNN_SMALL), None, "pathwise"), BNN_SMALL["dataset_size"], "CompiledBnn"
    c = engine.compile_model(W.build_vae(api, **dict(VAE_SMALL, latent_size=int(path[-1]))), None, "pathwise")
    return c, VAE_SMALL["dataset_size"], "CompiledAmortized"


MATRIX_PATHS = ["dense-fused", "dense-six-launch", "bnn", "amortised-2", "amortised-3", "amortised-5"]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("path", MATRIX_PATHS)
def test_matrix_paths_report_the_predicted_noise_and_minibatch(path, n, monkeypatch):
    c, ds, kind = matrix_model(path, monkeypatch)
    assert type(c).__name__ == kind
    check = StreamCheck()
    for seed in SEEDS:
        for offset in OFFSETS:
            check_matrix_path(c, check, n, n, 0, seed, offset, ds, (path, n, hex(seed), hex(offset)))
    # `evaluate` reports what the launch above reports
    res = c.evaluate(n, seed=SEEDS[1], offset=OFFSETS[3], want_noise=True, want_indices=True)
    got, idx = launch_shard(c, n, n, 0, SEEDS[1], OFFSETS[3])
    assert np.array_equal(res["noise"].cpu().numpy(), got) and np.array_equal(res["indices"].cpu().numpy(), idx)
    check.finish("%s n=%d:" % (path, n))


@pytest.mark.parametrize("n_global,splits", SPLITS, ids=["2-shards", "3-shards", "small-shards"])
@pytest.mark.parametrize("path", MATRIX_PATHS)
def test_matrix_path_shards_report_the_noise_of_their_global_samples(path, n_global, splits, monkeypatch):
    """dense_eps4 / the BNN's draw use sample_base + n, the amortised latents row sample_base * B + r and its minibatches sample
    sample_base + s: a base ignored, applied twice or scaled wrongly is an error of order 1 in every draw of the second shard"""
    c, ds, _ = matrix_model(path, monkeypatch)
    check = StreamCheck()
    for seed, offset in ((SEEDS[1], OFFSETS[4]), (SEEDS[0], OFFSETS[2])):
        for base, n_local in splits:
            check_matrix_path(c, check, n_local, n_global, base, seed, offset, ds, (path, base, n_local, hex(seed), hex(offset)))
    check.finish("%s shards %s:" % (path, splits))


@pytest.mark.parametrize("fused", ["1", "0"], ids=["fused", "six-launch"])
@pytest.mark.parametrize("kw,n", [(dict(dataset_size=96, batch_size=40, n_features=784, n_classes=10), 24),
                                  (dict(dataset_size=64, batch_size=32, n_features=32, n_classes=1), 65)])
def test_dense_path_at_other_shapes(kw, n, fused, monkeypatch):
    """the example's 784 x 10 weights (7840 noise rows) and the one-logit model, whole and as two shards"""
    c, ds, _ = matrix_model("dense-fused" if fused == "1" else "dense-six-launch", monkeypatch, **kw)
    check = StreamCheck()
    for seed in SEEDS:
        for offset in OFFSETS:
            check_matrix_path(c, check, n, n, 0, seed, offset, ds, ("dense", fused, n, hex(seed), hex(offset)))
    for base, n_local in ((0, n // 3), (n // 3, n - n // 3)):
        check_matrix_path(c, check, n_local, n, base, SEEDS[1], OFFSETS[4], ds, ("dense", fused, base, n_local))
    check.finish("dense %s %s:" % (fused, kw))


def test_scalar_engine_minibatch_rows_equal_the_predicted_bijection():
    """bsvi_minibatch_gather: the dense path's keyed bijection; group 0 draws with the call's key.  Over 2000 offsets every dataset
    row is chosen equally often (the reference's own condition, on the device)."""
    from scipy import stats
    kw = dict(dataset_size=40, batch_size=8)
    c = engine.compile_model(W.build_minibatch_normal_mean(W.native_api(), **kw), None, "pathwise")
    counts = np.zeros(kw["dataset_size"])
    for offset in list(OFFSETS) + list(range(100, 2100)):
        res = c.evaluate(4, seed=SEEDS[1], offset=offset, want_indices=True)
        (rows,) = [v.cpu().numpy() for v in res["indices"].values()]
        assert np.array_equal(rows, R.minibatch_index(SEEDS[1], offset, kw["dataset_size"], np.arange(kw["batch_size"]))), offset
        counts += np.bincount(rows, minlength=kw["dataset_size"])
    assert stats.chisquare(counts).pvalue > 1e-4


def test_reduce_node_draws_the_predicted_data():
    """A variable observed by flag only is drawn on the device (mvn.cpp, reduce_data_kernel) and never reported.  The launch that
    draws it must give the per-sample values of the launch that is HANDED the predicted data.  Bound: four times what a noise
    error at the Normal bound does to those values (measured by handing in data perturbed by it), or 1e-5 of their scale; data of a
    neighbouring offset — any structural mistake — must be far outside it."""
    c = engine.compile_model(W.build_population_receptive_fields(W.native_api(), field=40, n_data=15), None, "pathwise")
    (node,) = c.program.externals
    assert node.kind == "reduce" and node.drawn
    mean, scale = (np.asarray(v, dtype=np.float64).reshape(-1) for v in (node.data_mean, node.data_scale))
    n, rng = 64, np.random.RandomState(3)
    for seed, offset in ((SEEDS[0], 7), (SEEDS[1], OFFSETS[2]), (SEEDS[1], OFFSETS[4])):
        values = lambda **kw: c.evaluate(n, seed=seed, offset=offset, want_fvalues=True, **kw)["f"].cpu().numpy().astype(np.float64)
        given = lambda eps: values(minibatch={node.drawn_name: mean + scale * eps})
        eps = R.reduce_data_noise(seed, offset, mean.size)
        f_drawn, f_pred = values(), given(eps)
        yard = np.abs(given(eps + NORMAL_TOL * rng.choice([-1.0, 1.0], eps.size)) - f_pred).max()
        bound = max(4 * yard, 1e-5 * np.abs(f_pred).max())
        err, other = np.abs(f_drawn - f_pred).max(), np.abs(given(R.reduce_data_noise(seed, offset + 1, mean.size)) - f_pred).max()
        print("reduce node data, seed %#x offset %#x: |drawn - predicted| %.3g, bound %.3g, another offset's data %.3g" % (seed, offset, err, bound, other))
        assert err <= bound and other > 10 * bound


# ---- training on in-kernel draws: the carry into the high offset word, and the oracle on predicted noise -----------------------
MODES = (("persistent", dict()), ("stepwise", dict(allow_persistent=False)), ("graph", dict(_force_sharded_path=True)))


def named_noise(c, rows_by_index, n):
    noise = np.stack([rows_by_index[r] for r in range(c.program.n_noise)])
    return {name: noise[s.base:s.base + s.size].T.reshape((n,) + tuple(s.shape)) for name, s in c.program.slot_by_name.items()}


class PredictedNoise:
    """noise_seq of the oracle: iteration `it` draws at offset0 + it.  Rows that are their own noise (Beta) depend on the
    parameters of that iteration: they are read from the oracle at the moment it asks."""

    def __init__(self, c, oracle, seed, offset0, n):
        self.c, self.oracle, self.seed, self.offset0, self.n = c, oracle, seed, offset0, n

    def __getitem__(self, it):
        par = {k: v.detach().numpy().astype(np.float32).reshape(-1) for k, v in self.oracle.named_parameters().items()}
        rows = []
        for name, s in self.c.program.slot_by_name.items():
            for j in range(s.size):
                p0 = p1 = 0.0
                if s.dist == D.DIST_BETA:
                    p0, p1 = softplus32(par[name + "_concentration1"][j]), softplus32(par[name + "_concentration0"][j])
                rows.append((s.base + j, s.dist, p0, p1))
        return named_noise(self.c, R.scalar_noise(rows, self.seed, self.offset0 + it, 0, self.n), self.n)


def train_all_modes_against_the_oracle(builder, kwargs, n, iters, optimizer, opt_kw, seed, offset0):
    from oracle.svi_oracle import Oracle
    api = W.native_api()
    runs = {}
    for mode, opts in MODES:
        c = engine.compile_model(getattr(W, builder)(api, **kwargs), None, "pathwise")
        c.iteration = offset0
        losses, finite = c.train(iters, n, optimizer, seed=seed, **opts, **opt_kw)
        assert c.last_mode == mode and bool(finite.all()) and c.iteration == offset0 + iters
        runs[mode] = (losses.cpu().numpy(), c.named_params())
    o = Oracle(getattr(W, builder)(api, **kwargs))
    ref_losses = o.train(iters, n, optimizer, noise_seq=PredictedNoise(c, o, seed, offset0, n), **opt_kw)
    ref_after = {k: v.detach().numpy() for k, v in o.named_parameters().items()}
    for mode, (losses, params) in runs.items():
        # path against path, as test_sharded_step_sequence_equals_the_fused_single_gpu_step
        np.testing.assert_allclose(losses, runs["persistent"][0], rtol=2e-6, atol=1e-6)
        for name, p in params.items():
            np.testing.assert_allclose(p, runs["persistent"][1][name], rtol=2e-6, atol=1e-7)
        # against the oracle, the bound of test_training_trajectory_matches_reference_golden
        print(builder, optimizer, mode, "loss curve rel. error %.3g" % rel_err(losses, ref_losses),
              "parameters %.3g" % max(np.abs(p - ref_after[k].reshape(p.shape)).max() for k, p in params.items()))
        assert rel_err(losses, ref_losses) <= TOL, mode
        for name, p in params.items():
            e = ref_after[name].reshape(p.shape)
            assert np.abs(p - e).max() <= 2e-5 * (1 + np.abs(e).max()), (mode, name)


@pytest.mark.parametrize("optimizer,opt_kw", [("SGD", dict(lr=1e-3)), ("Adam", dict(lr=5e-3))])
def test_offset_carry_during_training_in_every_launch_mode(optimizer, opt_kw):
    """ten iterations from offset 2^32 - 5: the low offset word wraps inside the call (the in-kernel loops add the iteration to the
    offset themselves; the graph path adds a device counter)"""
    train_all_modes_against_the_oracle("build_readme_ar", dict(T=20), 300, 10, optimizer, opt_kw, SEEDS[1], (1 << 32) - 5)


@pytest.mark.parametrize("builder,kwargs,n,optimizer,opt_kw", [
    ("build_readme_ar", dict(T=20), 300, "SGD", dict(lr=1e-3)),
    ("build_readme_ar", dict(T=20), 300, "Adam", dict(lr=5e-3)),
    ("build_beta_binomial", dict(n_obs=30), 300, "Adam", dict(lr=1e-2)),
])
def test_oracle_on_predicted_noise_judges_training_on_in_kernel_draws(builder, kwargs, n, optimizer, opt_kw):
    """`c.train(K, n, seed=...)` with no noise handed in — the loop the benchmark times — against the oracle fed the noise the
    stream contract predicts for (seed, offset0 + iteration)"""
    train_all_modes_against_the_oracle(builder, kwargs, n, 25, optimizer, opt_kw, SEEDS[0], 3)
