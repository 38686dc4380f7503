"""Node arithmetic of the kernel (csrc/dist_math.h) against torch.distributions on CPU —
value and every partial derivative, per distribution — through the bsvi_debug_math hook."""
import ctypes as C

import numpy as np
import pytest
import torch
from torch import distributions as td

from brancher_amd import native
from brancher_amd import distributions as D

pytestmark = pytest.mark.gpu


def run(fn, dist, x, p0, p1):
    lib = native.load()
    dev = torch.device("cuda:0")
    n = len(x)
    xs, a, b = (torch.tensor(np.asarray(v, dtype=np.float32)).to(dev) for v in (x, p0, p1))
    out = torch.zeros(4 * n, device=dev)
    native.check(lib.bsvi_debug_math(fn, dist, C.c_void_p(xs.data_ptr()), C.c_void_p(a.data_ptr()),
                                     C.c_void_p(b.data_ptr()), C.c_void_p(out.data_ptr()), n, None))
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(4, n)


def close(a, b, tol=2e-5):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert np.all(np.abs(a - b) <= tol * (1.0 + np.abs(b))), np.abs(a - b).max()


def test_special_functions():
    x = np.concatenate([np.linspace(0.05, 3, 40), np.linspace(3, 60, 40)]).astype(np.float32)
    t = torch.tensor(x)
    close(run(0, 0, x, x, x)[0], torch.digamma(t).numpy())
    close(run(1, 0, x, x, x)[0], torch.polygamma(1, t).numpy())
    close(run(6, 0, x, x, x)[0], torch.lgamma(t).numpy())


def test_dirichlet_grad_all_branches():
    rng = np.random.RandomState(0)
    alpha = np.exp(rng.uniform(np.log(0.1), np.log(40), 4000)).astype(np.float32)
    beta = np.exp(rng.uniform(np.log(0.1), np.log(40), 4000)).astype(np.float32)
    x = rng.beta(alpha, beta).astype(np.float32).clip(1e-6, 1 - 1e-6)
    total = alpha + beta
    ref = torch._dirichlet_grad(torch.tensor(x), torch.tensor(alpha), torch.tensor(total)).numpy()
    got = run(2, 0, x, alpha, total)[0]
    close(got, ref, 5e-5)


CASES = [
    (D.DIST_NORMAL, lambda a, b: td.Normal(a, b), "real"),
    (D.DIST_LOGNORMAL, lambda a, b: td.LogNormal(a, b), "pos"),
    (D.DIST_CAUCHY, lambda a, b: td.Cauchy(a, b), "real"),
    (D.DIST_LAPLACE, lambda a, b: td.Laplace(a, b), "real"),
    (D.DIST_BETA, lambda a, b: td.Beta(a, b), "unit"),
]


@pytest.mark.parametrize("dist,make,support", CASES)
def test_logp_entropy_and_gradients(dist, make, support):
    rng = np.random.RandomState(dist)
    n = 512
    if dist == D.DIST_BETA:
        p0 = np.exp(rng.uniform(-1.5, 2.5, n)); p1 = np.exp(rng.uniform(-1.5, 2.5, n))
        p0[:8] = 1.0; p1[4:12] = 1.0       # torch.xlogy masks the (alpha-1)==0 terms
    else:
        p0 = rng.normal(0, 2, n); p1 = np.exp(rng.uniform(-2, 1.5, n))
    x = {"real": rng.normal(0, 3, n), "pos": np.exp(rng.normal(0, 1, n)), "unit": rng.uniform(0.02, 0.98, n)}[support]
    x, p0, p1 = (v.astype(np.float32) for v in (x, p0, p1))
    tx, ta, tb = (torch.tensor(v, requires_grad=True) for v in (x, p0, p1))
    lp = make(ta, tb).log_prob(tx)
    lp.sum().backward()
    got = run(3, dist, x, p0, p1)
    close(got[0], lp.detach().numpy())
    close(got[1], tx.grad.numpy()); close(got[2], ta.grad.numpy()); close(got[3], tb.grad.numpy())
    ta.grad = None; tb.grad = None
    H = make(ta, tb).entropy()
    H.sum().backward()
    got = run(4, dist, x, p0, p1)
    close(got[0], H.detach().numpy())
    close(got[2], np.zeros(n) if ta.grad is None else ta.grad.numpy())
    close(got[3], tb.grad.numpy())


def test_discrete_logp():
    rng = np.random.RandomState(3)
    n = 256
    logits = rng.normal(0, 3, n).astype(np.float32)
    total = rng.randint(1, 12, n).astype(np.float32)
    k = np.floor(rng.uniform(0, 1, n) * (total + 1)).clip(0, total).astype(np.float32)
    tl = torch.tensor(logits, requires_grad=True)
    lp = td.Binomial(torch.tensor(total), logits=tl).log_prob(torch.tensor(k))
    lp.sum().backward()
    got = run(3, D.DIST_BINOMIAL, k, total, logits)
    close(got[0], lp.detach().numpy()); close(got[3], tl.grad.numpy())
    xb = (rng.uniform(0, 1, n) < 0.5).astype(np.float32)
    tl = torch.tensor(logits, requires_grad=True)
    lp = td.Bernoulli(logits=tl).log_prob(torch.tensor(xb))
    lp.sum().backward()
    got = run(3, D.DIST_BERNOULLI, xb, logits, logits)
    close(got[0], lp.detach().numpy()); close(got[2], tl.grad.numpy())
    tl.grad = None
    H = td.Bernoulli(logits=tl).entropy()
    H.sum().backward()
    got = run(4, D.DIST_BERNOULLI, xb, logits, logits)
    close(got[0], H.detach().numpy()); close(got[2], tl.grad.numpy())


# ---- against torch in DOUBLE precision: the draws of the generic nodes, and the special functions and log-densities at their edges.
# Same bound, 2e-5 * (1 + |ref|): the 1e-5 parity promise in the header of dist_math.h.
def f64(v):
    return torch.tensor(np.asarray(v, dtype=np.float32).astype(np.float64))


DRAWS = [D.DIST_NORMAL, D.DIST_CAUCHY, D.DIST_LOGNORMAL, D.DIST_LAPLACE, D.DIST_DETERMINISTIC]


@pytest.mark.parametrize("dist", DRAWS)
def test_draw_from_noise_and_its_adjoints(dist):
    """fn 5: `sample_from_noise_generic` and `sample_bwd_generic` — the value of a draw from its noise and both parameter
    adjoints against the closed forms in double (Laplace: loc - scale * sign(e) * log1p(-|e|), torch laplace.py:83-86), the
    Laplace noise at 0, at +-(1 - 2^-24) — the clamp of `laplace_noise` — and at +-1e-8"""
    rng = np.random.RandomState(40 + dist)
    n = 200
    p0 = rng.normal(0, 1.5, n)
    p1 = np.exp(rng.uniform(-2, 1.0, n))
    if dist == D.DIST_LAPLACE:
        edge = 1.0 - 2.0 ** -24
        e = np.concatenate([[0.0, edge, -edge, 1e-8, -1e-8], rng.uniform(-1, 1, n - 5)])
    else:
        e = np.concatenate([[0.0], rng.normal(0, 1.5, n - 1)])
    e, p0, p1 = (v.astype(np.float32) for v in (e, p0, p1))
    assert dist != D.DIST_LAPLACE or (np.abs(e) < 1).all()
    te, ta, tb = f64(e), f64(p0).requires_grad_(True), f64(p1).requires_grad_(True)
    if dist in (D.DIST_NORMAL, D.DIST_CAUCHY):
        v = ta + te * tb
    elif dist == D.DIST_LOGNORMAL:
        v = torch.exp(ta + te * tb)
    elif dist == D.DIST_LAPLACE:
        v = ta - tb * te.sign() * torch.log1p(-te.abs())
    else:
        v = ta + 0.0 * tb
    v.sum().backward()
    got = run(5, dist, e, p0, p1)
    close(got[0], v.detach().numpy())
    close(got[2], ta.grad.numpy())
    close(got[3], tb.grad.numpy())


def test_special_functions_beyond_the_interior():
    """digamma on the reflection branch (negative non-integers), at exactly 10 (the constant of the recurrence's end), at 1e-3 and
    1e6; trigamma below 0.5 and at negative arguments; lgamma around its zeros at 1 and 2"""
    x = np.array([-0.5, -1.5, -2.3, -7.75, -0.01, -10.5, -31.25, 10.0, 2.0, 1e-3, 1e6, 9.999999, 10.000001], dtype=np.float32)
    close(run(0, 0, x, x, x)[0], torch.digamma(f64(x)).numpy())
    x = np.array([0.49, 0.3, 0.1, 1e-3, -0.5, -1.5, -2.3, -7.75, -0.01, -10.5, 0.5], dtype=np.float32)
    close(run(1, 0, x, x, x)[0], torch.polygamma(1, f64(x)).numpy())
    x = np.concatenate([1.0 + np.array([-1e-2, -1e-3, -1e-6, 0.0, 1e-6, 1e-3, 1e-2]), 2.0 + np.array([-1e-2, -1e-3, -1e-6, 0.0, 1e-6, 1e-3, 1e-2]),
                        [1.4616321]]).astype(np.float32)
    close(run(6, 0, x, x, x)[0], torch.lgamma(f64(x)).numpy())


def test_beta_at_total_two_and_small_alpha():
    """Beta log-density and entropy where alpha + beta == 2 (digamma(2) ends the recurrence at exactly 10) and with alpha < 0.2"""
    pairs = [(0.5, 1.5), (1.0, 1.0), (0.1, 1.9), (1.9, 0.1), (1.25, 0.75), (0.15, 0.15), (0.05, 3.0), (0.19, 40.0), (0.12, 0.8), (3.0, 0.07)]
    rng = np.random.RandomState(8)
    reps = 12
    p0 = np.repeat([a for a, _ in pairs], reps).astype(np.float32)
    p1 = np.repeat([b for _, b in pairs], reps).astype(np.float32)
    x = rng.uniform(0.02, 0.98, len(p0)).astype(np.float32)
    tx, ta, tb = (f64(v).requires_grad_(True) for v in (x, p0, p1))
    lp = td.Beta(ta, tb).log_prob(tx)
    lp.sum().backward()
    got = run(3, D.DIST_BETA, x, p0, p1)
    close(got[0], lp.detach().numpy())
    close(got[1], tx.grad.numpy()); close(got[2], ta.grad.numpy()); close(got[3], tb.grad.numpy())
    ta.grad = None; tb.grad = None
    H = td.Beta(ta, tb).entropy()
    H.sum().backward()
    got = run(4, D.DIST_BETA, x, p0, p1)
    close(got[0], H.detach().numpy())
    close(got[2], ta.grad.numpy()); close(got[3], tb.grad.numpy())


EXTREME_LOGITS = [30.0, -30.0, 90.0, -90.0]


def test_binomial_at_the_ends_of_its_support_and_extreme_logits():
    """k = 0 and k = n with n up to 200, logits from the interior and at +-30 and +-90: `sigmoid_hw` and `log1p_exp_neg_abs_hw`
    stay finite and inside the bound"""
    rng = np.random.RandomState(12)
    logits = np.concatenate([EXTREME_LOGITS, rng.normal(0, 3, 28)])
    total = np.array([1, 2, 7, 50, 200], dtype=np.float64)
    L, T_ = (v.reshape(-1) for v in np.meshgrid(logits, total))
    L, T_ = np.concatenate([L, L]).astype(np.float32), np.concatenate([T_, T_]).astype(np.float32)
    k = np.concatenate([np.zeros(len(L) // 2), T_[:len(L) // 2]]).astype(np.float32)
    tl = f64(L).requires_grad_(True)
    lp = td.Binomial(f64(T_), logits=tl).log_prob(f64(k))
    lp.sum().backward()
    got = run(3, D.DIST_BINOMIAL, k, T_, L)
    assert np.isfinite(got[0]).all() and np.isfinite(got[3]).all()
    close(got[0], lp.detach().numpy()); close(got[3], tl.grad.numpy())


def test_bernoulli_at_extreme_logits():
    logits = np.repeat(EXTREME_LOGITS + [17.0, -17.0, 0.0], 2).astype(np.float32)
    xb = np.tile([0.0, 1.0], len(logits) // 2).astype(np.float32)
    tl = f64(logits).requires_grad_(True)
    lp = td.Bernoulli(logits=tl).log_prob(f64(xb))
    lp.sum().backward()
    got = run(3, D.DIST_BERNOULLI, xb, logits, logits)
    assert np.isfinite(got[0]).all() and np.isfinite(got[2]).all()
    close(got[0], lp.detach().numpy()); close(got[2], tl.grad.numpy())
    tl.grad = None
    H = td.Bernoulli(logits=tl).entropy()
    H.sum().backward()
    got = run(4, D.DIST_BERNOULLI, xb, logits, logits)
    assert np.isfinite(got[0]).all() and np.isfinite(got[2]).all()
    close(got[0], H.detach().numpy()); close(got[2], tl.grad.numpy())
