"""Host reference of the engine's noise streams — numpy only, written from the contract in the comments of
brancher_amd/csrc/philox.h and bsvi_device.h, not from the device code's arithmetic.

The contract: every draw is a pure function of (seed, global sample index, noise row, iteration offset, attempt).

  words      philox4x32(c0, c1, c2, c3, k0, k1) with kPhiloxRounds rounds (read from philox.h)
  key        k0, k1 = the 64-bit seed (low, high); every path but the minibatch / drawn-data ones uses it as it is
  counter    c2, c3 = the 64-bit offset (low, high) on EVERY path; c0, c1 per path:
    scalar engines, Normal rows       c0 = sample, c1 = (row >> 2) | 0x80000000      rows 4g..4g+3 = the two Box-Muller pairs
    scalar engines, other draws       c0 = sample, c1 = (row & 0xffff) | (attempt & 0x7fff) << 16
                                      attempt: 0 for Cauchy / Laplace / LogNormal / Bernoulli, block i // 4 of a Binomial,
                                      (stream << 12) + try for the gammas of a Beta (stream 1: alpha, stream 2: beta)
    dense and BNN                     c0 = sample, c1 = (row >> 2) | 0x40000000
    amortised latents                 c0 = sample * B + b, c1 = d >> 1               one Box-Muller pair per call
    dense minibatch (Feistel round)   c0 = right half, c1 = round, k0 ^ 0x5bd1e995
    amortised minibatch               c0 = right half, c1 = round | sample << 2, k0 ^ 0x7f4a7c15
    reduce node's drawn data          c0 = element // 4, c1 = 0x52454455, k0 ^ 0x3c6ef372
  uniform    u01(x) = ((float)(x >> 8) + 0.5f) * 2^-24 in SINGLE precision: (0, 1], because for x >> 8 == 2^24 - 1 the sum
             rounds to 2^24 and the result is exactly 1.0f (probability 2^-24 per word)
  transforms evaluated here in double precision on that single-precision uniform (`dtype=np.float32` evaluates the same
             formulas in single precision: the yardstick of the comparison with the device)
"""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PHILOX_H = os.path.join(ROOT, "brancher_amd", "csrc", "philox.h")

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF
FLAG_NORMAL, FLAG_DENSE = 0x80000000, 0x40000000
KEY_DENSE_MINIBATCH, KEY_AMORT_MINIBATCH, KEY_REDUCE_DATA = 0x5bd1e995, 0x7f4a7c15, 0x3c6ef372
C1_REDUCE_DATA = 0x52454455
FLOAT_EPS = float(np.finfo(np.float32).eps)
BETA_MAX = 1.0 - FLOAT_EPS
BETA_MIN = float(np.finfo(np.float32).tiny)

# distribution codes (brancher_amd/distributions.py; repeated here so that this module imports nothing of the package)
NORMAL, LOGNORMAL, CAUCHY, LAPLACE, BETA, BINOMIAL, BERNOULLI = 1, 2, 3, 4, 5, 6, 7


def kernel_rounds():
    """the round count the kernels are compiled with"""
    with open(PHILOX_H) as f:
        m = re.search(r"constexpr\s+int\s+kPhiloxRounds\s*=\s*(\d+)\s*;", f.read())
    if not m:
        raise RuntimeError("kPhiloxRounds not found in " + PHILOX_H)
    return int(m.group(1))


def _u64(x):
    return np.asarray(x, dtype=np.uint64) & np.uint64(MASK32)


def philox4x32(c0, c1, c2, c3, k0, k1, rounds=None):
    """Philox4x32-`rounds` (Salmon et al., SC'11), vectorised; returns four uint32 arrays"""
    rounds = kernel_rounds() if rounds is None else rounds
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*[_u64(v) for v in (c0, c1, c2, c3, k0, k1)])
    m32, s32 = np.uint64(MASK32), np.uint64(32)
    for _ in range(rounds):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2           # 32 x 32 bits: fits 64
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & m32, (p0 >> s32) ^ c3 ^ k1, p0 & m32
        k0, k1 = (k0 + np.uint64(W0)) & m32, (k1 + np.uint64(W1)) & m32
    return tuple(v.astype(np.uint32) for v in (c0, c1, c2, c3))


def split64(v):
    """(low, high) words of a 64-bit seed or offset; an integer or an array of them"""
    if isinstance(v, np.ndarray):
        v = v.astype(np.uint64)
        return v & np.uint64(MASK32), v >> np.uint64(32)
    v = int(v) & 0xFFFFFFFFFFFFFFFF
    return v & MASK32, v >> 32


def u01(x):
    """single precision, bit for bit: the sum (x >> 8) + 0.5 is ROUNDED to 24 bits"""
    hi = (np.asarray(x, dtype=np.uint32) >> np.uint32(8)).astype(np.float32)
    return (hi + np.float32(0.5)) * np.float32(2.0 ** -24)


def box_muller(a, b, dtype=np.float64):
    """(z0, z1) = sqrt(-2 ln u(a)) * (cos, sin)(2 pi u(b))"""
    ua, ub = u01(a).astype(dtype), u01(b).astype(dtype)
    r = np.sqrt(dtype(-2.0) * np.log(ua))
    t = dtype(2.0 * np.pi) * ub
    return r * np.cos(t), r * np.sin(t)


def cauchy_angle(a, dtype=np.float64):
    """the angle whose tangent is the Cauchy base noise, in (-pi/2, pi/2]"""
    return dtype(np.pi) * (u01(a).astype(dtype) - dtype(0.5))


def cauchy_noise(a, dtype=np.float64):
    return np.tan(cauchy_angle(a, dtype))


def laplace_noise(a, dtype=np.float64):
    """torch laplace.py: uniform on [eps - 1, 1)"""
    e = dtype(FLOAT_EPS - 1.0) + dtype(2.0 - FLOAT_EPS) * u01(a).astype(dtype)
    return np.minimum(e, dtype(1.0 - 2.0 ** -24))


def sigmoid32(x):
    """the threshold of a Bernoulli / Binomial draw: 1 / (1 + exp(-logit)) in single precision"""
    x = np.asarray(x, dtype=np.float32)
    return (np.float32(1.0) / (np.float32(1.0) + np.exp(-x))).astype(np.float32)


# ---- counters ------------------------------------------------------------------------------------------------------
def raw_counter(row, attempt=0):
    return (np.asarray(row, dtype=np.uint64) & np.uint64(0xFFFF)) | ((np.asarray(attempt, dtype=np.uint64) & np.uint64(0x7FFF)) << np.uint64(16))


def raw_words(seed, offset, samples, row, attempt=0):
    (k0, k1), (o0, o1) = split64(seed), split64(offset)
    return philox4x32(samples, raw_counter(row, attempt), o0, o1, k0, k1)


def normal_draw(seed, offset, sample, row, flag=FLAG_NORMAL, dtype=np.float64):
    """the standard normal of (seed, offset, sample, row), every argument broadcast against the others"""
    row = np.asarray(row, dtype=np.uint64)
    (k0, k1), (o0, o1) = split64(seed), split64(offset)
    x = philox4x32(sample, (row >> np.uint64(2)) | np.uint64(flag), o0, o1, k0, k1)
    z0, z1 = box_muller(x[0], x[1], dtype)
    z2, z3 = box_muller(x[2], x[3], dtype)
    j = np.broadcast_to(row & np.uint64(3), z0.shape)
    return np.where(j == 0, z0, np.where(j == 1, z1, np.where(j == 2, z2, z3)))


def normal_rows(seed, offset, samples, rows, flag=FLAG_NORMAL, dtype=np.float64):
    """standard normals [len(rows), len(samples)] of the scalar engines (flag 0x80000000) or the dense / BNN path (0x40000000)"""
    return normal_draw(seed, offset, np.asarray(samples, dtype=np.uint64)[None, :], np.asarray(rows, dtype=np.uint64)[:, None],
                       flag, dtype)


def gamma(seed, offset, samples, row, alpha, stream, dtype=np.float64, max_tries=64):
    """Marsaglia & Tsang (2000) as ATen's sample_gamma, one attempt per Philox call: attempt (stream << 12) first feeds the
    boost u^(1/alpha) when alpha < 1, the following ones are the tries (words x, y: the normal; word z: the uniform)."""
    samples = np.asarray(samples, dtype=np.uint64)
    n = samples.size
    alpha = np.broadcast_to(np.asarray(alpha, dtype=np.float32), (n,)).astype(dtype)
    attempt = np.full(n, stream << 12, dtype=np.uint64)
    scale = np.ones(n, dtype=dtype)
    small = alpha < 1
    if small.any():
        x = raw_words(seed, offset, samples, row, attempt)
        boost = np.power(dtype(1.0) - u01(x[0]).astype(dtype), dtype(1.0) / np.where(small, alpha, dtype(1.0)))
        scale = np.where(small, boost, scale)
        attempt = attempt + small.astype(np.uint64)
        alpha = np.where(small, alpha + dtype(1.0), alpha)
    d = alpha - dtype(1.0 / 3.0)
    c = dtype(1.0) / np.sqrt(dtype(9.0) * d)
    out = scale * d
    todo = np.ones(n, dtype=bool)
    for _ in range(max_tries):
        if not todo.any():
            break
        x = raw_words(seed, offset, samples, row, attempt)
        n0, _ = box_muller(x[0], x[1], dtype)
        y = dtype(1.0) + c * n0
        with np.errstate(invalid="ignore", divide="ignore"):
            v = y * y * y
            u = dtype(1.0) - u01(x[2]).astype(dtype)
            xx = n0 * n0
            accept = (y > 0) & ((u < dtype(1.0) - dtype(0.0331) * xx * xx)
                                | (np.log(u) < dtype(0.5) * xx + d * (dtype(1.0) - v + np.log(v))))
        out = np.where(todo & accept, scale * d * v, out)
        todo = todo & ~accept
        attempt = attempt + np.uint64(1)
    return out


def beta_draw(seed, offset, samples, row, alpha, beta, dtype=np.float64):
    """Beta(alpha, beta) = Ga / (Ga + Gb) with the gammas on retry streams 1 and 2, clamped like torch's Beta.rsample"""
    ga = gamma(seed, offset, samples, row, alpha, 1, dtype)
    gb = gamma(seed, offset, samples, row, beta, 2, dtype)
    return np.clip(ga / (ga + gb), dtype(BETA_MIN), dtype(BETA_MAX))


def bernoulli_draw(seed, offset, samples, row, logit):
    x = raw_words(seed, offset, samples, row, 0)
    return (u01(x[0]) < sigmoid32(logit)).astype(np.float64)


def binomial_draw(seed, offset, samples, row, total, logit):
    """blocks of four: trial i uses word i % 4 of attempt i // 4"""
    samples = np.asarray(samples, dtype=np.uint64)
    p = sigmoid32(logit)
    k = np.zeros(samples.size)
    for i in range(0, int(total), 4):
        x = raw_words(seed, offset, samples, row, i >> 2)
        for j in range(min(4, int(total) - i)):
            k += (u01(x[j]) < p)
    return k


def scalar_noise(rows, seed, offset, sample_base, n, dtype=np.float64):
    """What a launch of a scalar engine (interpreter or specialised) must REPORT as noise for its samples
    sample_base .. sample_base + n - 1.  `rows` is a list of (row, dist, p0, p1): the node's parameters matter for the draws
    that are their own noise (Beta: alpha, beta; Bernoulli: logit; Binomial: total, logit).  Returns {row: array [n]}."""
    samples = np.arange(sample_base, sample_base + n, dtype=np.uint64)
    out = {}
    for row, dist, p0, p1 in rows:
        if dist == NORMAL:
            out[row] = normal_rows(seed, offset, samples, [row], FLAG_NORMAL, dtype)[0]
        elif dist == LOGNORMAL:
            x = raw_words(seed, offset, samples, row, 0)
            out[row] = box_muller(x[0], x[1], dtype)[0]
        elif dist == CAUCHY:
            out[row] = cauchy_noise(raw_words(seed, offset, samples, row, 0)[0], dtype)
        elif dist == LAPLACE:
            out[row] = laplace_noise(raw_words(seed, offset, samples, row, 0)[0], dtype)
        elif dist == BETA:
            out[row] = beta_draw(seed, offset, samples, row, p0, p1, dtype)
        elif dist == BERNOULLI:
            out[row] = bernoulli_draw(seed, offset, samples, row, p0)
        elif dist == BINOMIAL:
            out[row] = binomial_draw(seed, offset, samples, row, p0, p1)
        else:
            raise ValueError("no draw site for distribution code {}".format(dist))
    return out


def scalar_counters(rows, beta_tries=64):
    """every c1 word a scalar launch may feed to Philox for one sample, one entry per distinct CALL (the four Normal rows of a
    group share theirs; a Beta: the boost and up to `beta_tries` tries of each gamma).  Two calls of a launch never collide
    if and only if this list has no repeated entry: c0 is the sample, c2 / c3 the offset."""
    c1, groups = [], set()
    for row, dist, p0, p1 in rows:
        if dist == NORMAL:
            if (row >> 2) not in groups:
                groups.add(row >> 2)
                c1.append((row >> 2) | FLAG_NORMAL)
        elif dist == BETA:
            c1 += [int(raw_counter(row, (s << 12) + t)) for s in (1, 2) for t in range(beta_tries + 1)]
        elif dist == BINOMIAL:
            c1 += [int(raw_counter(row, i >> 2)) for i in range(0, int(np.max(p0)), 4)]
        else:
            c1.append(int(raw_counter(row, 0)))
    return np.asarray(c1, dtype=np.uint64)


def dense_noise(seed, offset, sample_base, n, n_rows, dtype=np.float64):
    """dense and BNN path: [n_rows, n]"""
    return normal_rows(seed, offset, np.arange(sample_base, sample_base + n), np.arange(n_rows), FLAG_DENSE, dtype)


def amortized_noise(seed, offset, sample_base, n, batch, dz, dtype=np.float64):
    """amortised path: [n * batch, dz]; row r of the launch is global row sample_base * batch + r"""
    (k0, k1), (o0, o1) = split64(seed), split64(offset)
    rg = np.arange(sample_base * batch, (sample_base + n) * batch, dtype=np.uint64)
    pairs = np.arange((dz + 1) // 2, dtype=np.uint64)
    x = philox4x32(rg[:, None], pairs[None, :], o0, o1, k0, k1)
    e0, e1 = box_muller(x[0], x[1], dtype)
    return np.stack([e0, e1], axis=2).reshape(rg.size, -1)[:, :dz]


def reduce_data_noise(seed, offset, n_elements, dtype=np.float64):
    """standard normals behind the drawn data of a reduce node: element i = word pair of call i // 4"""
    (k0, k1), (o0, o1) = split64(seed), split64(offset)
    q = np.arange((n_elements + 3) // 4, dtype=np.uint64)
    x = philox4x32(q, C1_REDUCE_DATA, o0, o1, k0 ^ KEY_REDUCE_DATA, k1)
    z0, z1 = box_muller(x[0], x[1], dtype)
    z2, z3 = box_muller(x[2], x[3], dtype)
    return np.stack([z0, z1, z2, z3], axis=1).reshape(-1)[:n_elements]


# ---- minibatches: a keyed bijection of [0, DS) -------------------------------------------------------------------------
def _feistel(b, ds, round_words, max_walk=64):
    """4-round Feistel network on the next power of four >= ds, cycle-walked into [0, ds).
    round_words(right, round) -> uint32 array: word x of the round's Philox call."""
    half_bits = 1
    while (1 << (2 * half_bits)) < ds:
        half_bits += 1
    mask = np.uint64((1 << half_bits) - 1)
    hb = np.uint64(half_bits)
    b = np.asarray(b, dtype=np.uint64)
    x = b.copy()
    done = np.zeros(x.shape, dtype=bool)
    for _ in range(max_walk):
        lft, rgt = (x >> hb) & mask, x & mask
        for rnd in range(4):
            h = round_words(rgt, rnd).astype(np.uint64)
            lft, rgt = rgt, lft ^ (h & mask)
        y = (lft << hb) | rgt
        x = np.where(done, x, y)
        done = done | (x < np.uint64(ds))
        if done.all():
            return x.astype(np.int64)
    return np.where(done, x, b % np.uint64(ds)).astype(np.int64)


def minibatch_index(seed, offset, ds, positions):
    """dense path / scalar-engine gather: dataset row behind minibatch position b, the same for every sample"""
    (k0, k1), (o0, o1) = split64(seed), split64(offset)
    return _feistel(positions, ds, lambda rgt, rnd: philox4x32(rgt, rnd, o0, o1, k0 ^ KEY_DENSE_MINIBATCH, k1)[0])


def minibatch_row(seed, offset, ds, sample, positions):
    """amortised path: every sample draws its own minibatch (`sample`: an integer, or an array that broadcasts against `positions`)"""
    (k0, k1), (o0, o1) = split64(seed), split64(offset)
    sample = np.asarray(sample, dtype=np.uint64)
    c1 = lambda rnd: (np.uint64(rnd) | (sample << np.uint64(2))) & np.uint64(MASK32)
    return _feistel(positions, ds, lambda rgt, rnd: philox4x32(rgt, c1(rnd), o0, o1, k0 ^ KEY_AMORT_MINIBATCH, k1)[0])
