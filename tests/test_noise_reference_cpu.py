"""The host reference of the noise streams (oracle/philox_ref.py) on its own: the published Philox known answers, the
single-precision uniform at its extreme words, the minibatch bijections, and the statistical conditions the streams must meet
— laws, independence along every axis of the contract (sample, row, offset, seed, attempt), no counter used twice.
tests/test_gpu_noise.py then holds the device to this reference draw by draw, so what passes here holds for the kernels."""
import numpy as np
import pytest
from scipy import stats

from oracle import philox_ref as R

N = 1 << 16
P_MIN = 1e-4
SEED, OFFSET = 0x1234567890ABC, 11          # fixed: every threshold below was checked with these


def test_philox4x32_10_known_answers():
    """Random123 kat_vectors, philox4x32 at 10 rounds"""
    kat = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for ctr, key, want in kat:
        got = R.philox4x32(*ctr, *key, rounds=10)
        assert " ".join("%08x" % int(w) for w in got) == want
    # vectorised = elementwise
    c = np.array([k[0] for k in kat], dtype=np.uint64).T
    k = np.array([k[1] for k in kat], dtype=np.uint64).T
    got = np.stack(R.philox4x32(*c, *k, rounds=10), axis=1)
    assert [" ".join("%08x" % int(w) for w in row) for row in got] == [k[2] for k in kat]


def test_kernel_round_count_is_crush_resistant():
    """philox.h: Philox4x32-7 is the fewest rounds that pass BigCrush (Salmon et al., Table 2); 10 is the paper's default"""
    assert 7 <= R.kernel_rounds() <= 10


def test_u01_at_the_extreme_words():
    words = np.array([0, 0xff, 0x100, 0x7fffff00, 0x80000000, 0xfffffe00, 0xfffffeff, 0xffffff00, 0xffffffff], dtype=np.uint32)
    u = R.u01(words)
    assert u.dtype == np.float32
    want = [2.0 ** -25, 2.0 ** -25, 3 * 2.0 ** -25, 0.5 - 2.0 ** -25, 0.5 + 2.0 ** -25, 1 - 3 * 2.0 ** -25, 1 - 3 * 2.0 ** -25, 1.0, 1.0]
    # 0.5 +- 2^-25 and 1 - 3 * 2^-25 need 25 bits: single precision rounds them to even
    assert np.array_equal(u, np.array(want, dtype=np.float64).astype(np.float32))
    assert u[3] == np.float32(0.5) - np.float32(2.0 ** -25) and u[4] == np.float32(0.5)
    assert u.min() > 0.0 and u.max() == 1.0                      # (0, 1]: the top word rounds to exactly one
    # every transform of every word is finite, and inside its law's support
    for a in words:
        for b in words:
            assert np.all(np.isfinite(R.box_muller(a, b))) and np.all(np.isfinite(R.box_muller(a, b, np.float32)))
        assert np.isfinite(R.cauchy_noise(a))
        e = R.laplace_noise(a)
        assert R.FLOAT_EPS - 1.0 <= e < 1.0 and np.isfinite(np.log1p(-abs(e)))


@pytest.mark.parametrize("ds", range(1, 301))
def test_minibatch_bijections_are_permutations(ds):
    pos = np.arange(ds)
    assert sorted(R.minibatch_index(SEED, OFFSET, ds, pos)) == list(range(ds))
    assert sorted(R.minibatch_row(SEED, OFFSET, ds, 5, pos)) == list(range(ds))


def test_minibatch_rows_are_uniform_over_offsets_and_differ_between_samples():
    ds, batch, n_off = 40, 8, 2500
    counts_d, counts_a = np.zeros(ds), np.zeros(ds)
    for off in range(n_off):
        d = R.minibatch_index(SEED, off, ds, np.arange(batch))
        a = R.minibatch_row(SEED, off, ds, 3, np.arange(batch))
        assert len(set(d)) == batch and len(set(a)) == batch
        counts_d += np.bincount(d, minlength=ds)
        counts_a += np.bincount(a, minlength=ds)
    assert stats.chisquare(counts_d).pvalue > P_MIN and stats.chisquare(counts_a).pvalue > P_MIN
    # position 0 alone is uniform too (not only the set of rows)
    first = np.array([R.minibatch_index(SEED, off, ds, np.arange(1))[0] for off in range(n_off)])
    assert stats.chisquare(np.bincount(first, minlength=ds)).pvalue > P_MIN
    # the amortised path: another sample, another minibatch
    assert not np.array_equal(R.minibatch_row(SEED, OFFSET, ds, 3, np.arange(batch)), R.minibatch_row(SEED, OFFSET, ds, 4, np.arange(batch)))


def ks(x, law, *args):
    return stats.kstest(np.asarray(x, dtype=np.float64).reshape(-1), law, args=args).pvalue


def laplace_cdf(e):
    """uniform on [eps - 1, 1)"""
    return (e + 1.0) / 2.0


SAMPLES = np.arange(N, dtype=np.uint64)


def test_laws_of_the_base_noise():
    assert ks(R.normal_rows(SEED, OFFSET, SAMPLES, [5])[0], "norm") > P_MIN
    assert ks(R.dense_noise(SEED, OFFSET, 0, N, 1), "norm") > P_MIN
    assert ks(R.amortized_noise(SEED, OFFSET, 0, N // 8, 8, 3), "norm") > P_MIN
    assert ks(R.reduce_data_noise(SEED, OFFSET, N), "norm") > P_MIN
    rows = [(2, R.LOGNORMAL, 0, 0), (3, R.CAUCHY, 0, 0), (4, R.LAPLACE, 0, 0)]
    z = R.scalar_noise(rows, SEED, OFFSET, 0, N)
    assert ks(z[2], "norm") > P_MIN
    assert ks(z[3], "cauchy") > P_MIN
    assert ks(z[4], laplace_cdf) > P_MIN


@pytest.mark.parametrize("alpha,beta", [(0.3, 0.7), (2.0, 5.0), (40.0, 0.5)])
def test_beta_law_and_borderline_rate(alpha, beta):
    b64 = R.beta_draw(SEED, OFFSET, SAMPLES, 7, alpha, beta)
    # (the clamp to [tiny, 1 - eps] moves mass at the edges of Beta(40, 0.5) by less than the test resolves)
    assert ks(b64, "beta", alpha, beta) > P_MIN
    # a rejection decision at a single / double precision borderline may flip: the reference's own disagreement rate must be under a
    # quarter of the 0.1 % the device comparison may leave out
    b32 = R.beta_draw(SEED, OFFSET, SAMPLES, 7, alpha, beta, dtype=np.float32)
    assert np.mean(np.abs(b32 - b64) > 1e-4) < 0.25e-3
    # the two gammas use retry streams 1 and 2 of the same row: independent
    ga, gb = R.gamma(SEED, OFFSET, SAMPLES, 7, alpha, 1), R.gamma(SEED, OFFSET, SAMPLES, 7, alpha, 2)
    assert abs(stats.spearmanr(ga, gb)[0]) < 5 / np.sqrt(N)


def test_bernoulli_and_binomial_laws():
    for logit in (-1.3, 0.2):
        p = float(R.sigmoid32(logit))
        k = R.bernoulli_draw(SEED, OFFSET, SAMPLES, 9, logit)
        assert stats.chisquare(np.bincount(k.astype(int), minlength=2), [N * (1 - p), N * p]).pvalue > P_MIN
    for total in (1, 7, 13):
        p = float(R.sigmoid32(0.4))
        k = R.binomial_draw(SEED, OFFSET, SAMPLES, 9, total, 0.4)
        assert stats.chisquare(np.bincount(k.astype(int), minlength=total + 1), N * stats.binom.pmf(np.arange(total + 1), total, p)).pvalue > P_MIN


AXES = {
    # one row across samples, one sample across rows, one (sample, row) across offsets (over a carry into the high word),
    # one (sample, row, offset) across seeds (over a carry into the high word)
    "samples": dict(seed=SEED, offset=OFFSET, sample=np.arange(N, dtype=np.uint64), row=6),
    "rows": dict(seed=SEED, offset=OFFSET, sample=77, row=np.arange(8192, dtype=np.uint64)),
    "offsets": dict(seed=SEED, offset=(1 << 32) - 2048 + np.arange(4096, dtype=np.uint64), sample=77, row=6),
    "seeds": dict(seed=(1 << 32) - 2048 + np.arange(4096, dtype=np.uint64), offset=OFFSET, sample=77, row=6),
}


@pytest.mark.parametrize("axis", sorted(AXES))
def test_laws_and_independence_along_each_axis_of_the_contract(axis):
    a = AXES[axis]
    n = max(np.size(v) for v in a.values())
    z = np.broadcast_to(R.normal_draw(a["seed"], a["offset"], a["sample"], a["row"]), (n,))
    assert ks(z, "norm") > P_MIN
    assert abs(np.corrcoef(z[:-1], z[1:])[0, 1]) < 5 / np.sqrt(n - 1)           # neighbours along the axis
    for flag in (R.FLAG_DENSE,):
        zd = np.broadcast_to(R.normal_draw(a["seed"], a["offset"], a["sample"], a["row"], flag), (n,))
        assert ks(zd, "norm") > P_MIN and abs(np.corrcoef(zd, z)[0, 1]) < 5 / np.sqrt(n)      # the flag separates the paths
    x = R.raw_words(a["seed"], a["offset"], a["sample"], a["row"], 0)
    u = np.broadcast_to(R.u01(x[0]).astype(np.float64), (n,))
    assert ks(u, "uniform") > P_MIN
    assert abs(np.corrcoef(u[:-1], u[1:])[0, 1]) < 5 / np.sqrt(n - 1)
    # the uniform-based draws are functions of that uniform; their own laws along the axis all the same
    w = np.broadcast_to(x[0], (n,))
    assert ks(R.cauchy_noise(w), "cauchy") > P_MIN and ks(R.laplace_noise(w), laplace_cdf) > P_MIN
    samples = np.broadcast_to(np.asarray(a["sample"], dtype=np.uint64), (n,))
    row = np.broadcast_to(np.asarray(a["row"], dtype=np.uint64), (n,))
    p = float(R.sigmoid32(0.4))
    k = R.bernoulli_draw(a["seed"], a["offset"], samples, row, 0.4)
    assert stats.chisquare(np.bincount(k.astype(int), minlength=2), [n * (1 - p), n * p]).pvalue > P_MIN
    for total in (1, 7, 13):
        k = R.binomial_draw(a["seed"], a["offset"], samples, row, total, 0.4)
        # (4096 draws leave the outer counts of Binomial(13) below five: pooled into their neighbours)
        want = n * stats.binom.pmf(np.arange(total + 1), total, p)
        got = np.bincount(k.astype(int), minlength=total + 1).astype(float)
        while len(want) > 2 and want[0] < 5:
            want, got = np.concatenate([[want[0] + want[1]], want[2:]]), np.concatenate([[got[0] + got[1]], got[2:]])
        while len(want) > 2 and want[-1] < 5:
            want, got = np.concatenate([want[:-2], [want[-2] + want[-1]]]), np.concatenate([got[:-2], [got[-2] + got[-1]]])
        assert stats.chisquare(got, want).pvalue > P_MIN, total
        assert abs(np.corrcoef(k[:-1], k[1:])[0, 1]) < 5 / np.sqrt(n - 1)
    b = R.beta_draw(a["seed"], a["offset"], samples, row, 0.3, 0.7)
    assert ks(b, "beta", 0.3, 0.7) > P_MIN
    assert abs(stats.spearmanr(b[:-1], b[1:])[0]) < 5 / np.sqrt(n - 1)


def test_adjacent_rows_are_uncorrelated_including_the_four_of_one_call():
    z = R.normal_rows(SEED, OFFSET, SAMPLES, np.arange(12))
    d = R.dense_noise(SEED, OFFSET, 0, N, 12)
    for zz in (z, d):
        cc = np.corrcoef(zz)
        assert np.abs(cc - np.eye(12)).max() < 5 / np.sqrt(N)
    am = R.amortized_noise(SEED, OFFSET, 0, N // 4, 4, 5)
    assert np.abs(np.corrcoef(am.T) - np.eye(5)).max() < 5 / np.sqrt(am.shape[0])
    rd = R.reduce_data_noise(SEED, OFFSET, N).reshape(-1, 4)
    assert np.abs(np.corrcoef(rd.T) - np.eye(4)).max() < 5 / np.sqrt(rd.shape[0])
    # squares too: the two normals of a Box-Muller pair share their radius only through independent angles
    assert np.abs(np.corrcoef(z ** 2) - np.eye(12)).max() < 5 / np.sqrt(N)


def test_no_counter_is_used_twice_in_a_launch():
    """the largest program: 20 480 noise rows (160 KB of LDS, 8 bytes a slot), every kind of draw on neighbouring rows"""
    kinds = [R.NORMAL, R.LOGNORMAL, R.CAUCHY, R.LAPLACE, R.BETA, R.BERNOULLI, R.BINOMIAL]
    rows = [(r, kinds[(r // 4) % len(kinds)], 13, 0.5) for r in range(20480)]
    c1 = R.scalar_counters(rows)
    assert len(np.unique(c1)) == len(c1)
    # the flags: a Normal call never meets a retry / block counter, nor the dense path's calls
    raw = c1[(c1 & np.uint64(R.FLAG_NORMAL)) == 0]
    dense = (np.arange(20480 // 4, dtype=np.uint64)) | np.uint64(R.FLAG_DENSE)
    assert len(np.intersect1d(raw, dense)) == 0 and len(np.intersect1d(c1, dense)) == 0
    # and the words of distinct counters are distinct blocks (a bijection per key)
    x = np.stack(R.philox4x32(3, c1, 7, 0, 11, 0), axis=1)
    assert len(np.unique(x, axis=0)) == len(c1)


def test_predictor_is_shard_invariant():
    rows = [(0, R.NORMAL, 0, 0), (1, R.NORMAL, 0, 0), (5, R.LAPLACE, 0, 0), (6, R.BETA, 0.3, 2.0), (7, R.BINOMIAL, 7, 0.1)]
    full = R.scalar_noise(rows, SEED, OFFSET, 0, 300)
    a, b = R.scalar_noise(rows, SEED, OFFSET, 0, 130), R.scalar_noise(rows, SEED, OFFSET, 130, 170)
    for r in full:
        assert np.array_equal(full[r], np.concatenate([a[r], b[r]]))
    assert np.array_equal(R.amortized_noise(SEED, OFFSET, 0, 9, 4, 3)[5 * 4:], R.amortized_noise(SEED, OFFSET, 5, 4, 4, 3))


def test_hook_function_numbers_of_the_header_and_the_binding_agree():
    """include/bsvi.h documents the noise-stream functions of bsvi_debug_math; brancher_amd/native.py names them"""
    import os
    import re
    from brancher_amd import native
    with open(os.path.join(R.ROOT, "include", "bsvi.h")) as f:
        text = f.read()
    doc = text[text.index("Test hook, not used by the product path"):text.index("int bsvi_debug_math(")]
    assert re.search(r"fn %d: raw Philox4x32 words" % native.DEBUG_MATH_PHILOX_WORDS, doc)
    assert re.search(r"fn %d: transforms of the raw words" % native.DEBUG_MATH_NOISE_TRANSFORMS, doc)
    # fns 0-6 and the C signature are what they were
    assert "fn 0 digamma" in doc and "5 reparameterised draw from noise x" in doc and "6 lgamma" in doc
    assert "int bsvi_debug_math(int fn, int dist, const float* x_dev, const float* p0_dev, const float* p1_dev,\n" \
           "                    float* out_dev, uint32_t n, void* stream);" in text
