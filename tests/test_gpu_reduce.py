"""The REDUCE node (bsvi_reduce_*, csrc/reduce_kernel.h with reduce_data_kernel / reduce_logp_kernel of mvn.cpp) through the C ABI:
    r[n][d] = sum_e A(e; in_n) X[d][e]
for an elementwise expression A of two meshes and up to eight scalar inputs, every row of the linear surrogate it hands back
(rows k * n_data + d = d r_d / d in_k, rows K * n_data + d = e_d with e_d + sum_k g_dk in_k = r_d, one last row: weight * log p of
drawn data) against torch in double precision — at element counts below, at and off the wave's 64 lanes, at 1 .. 300 datapoints,
with 0 .. 8 inputs, with constant data, the caller's data and data drawn on the device, and at the launches that need 64 KiB of
dynamic LDS, the first size above it and the last size under the library's cap.

A hand-written instruction list (as `gp_node` of tests/test_gpu_mvn.py writes one), meshes Mx / My = linspace(-1, 1) over columns / rows:
    A = exp(-0.5 ((Mx - in0)^2 + (My - in1)^2) / in2^2) in3 + in4 Mx + in5 My + in6 Mx My + in7
with as many of the terms as the case has inputs (none: A = Mx My); slot inputs first, then uniform ones.

Bound.  The yardstick is torch's float32 evaluation of the same expression and sums on the CPU against the double one, computed
live (no LAPACK in it).  A value passes when its error is at most the largest of 4 x the yardstick, 2e-6 of the block's largest
|reference| and (ceil(E / 64) + 7) 2^-24 sum_e |A_e X_de| (the derivative in place of A for a gradient row): the forward bound of the
kernel's own summation order — a lane adds ceil(E / 64) products, the butterfly six more sums — which keeps a correct kernel from
failing on cancellation; one dropped element is still ~E / (ceil(E / 64) + 7) 2^24 times outside it.  The log-probability row:
4 x the float32 yardstick or 2e-6 of sum |term|.

Every test prints err, yardstick and scale (`pytest -s`).  Largest measured err / yardstick per row kind on an MI355X:
    gradient rows     constant data 1.85 (16 x 16, 7 datapoints, d / d in6), handed data 2.03 (61 x 69, 57 datapoints, d / d in4)
    value rows (r)    constant data 2.57 (46 x 89), handed data 4.23 (5 x 13, no inputs: 9.7e-8 of the block's scale, inside its 2e-6)
    log p             at most 1.12 at every case but one; 12.2 at the single element (1.3e-7 absolute: one float32 rounding
                      of the result against a yardstick that happens to be 1e-8), inside 2e-6 of sum |term|
No case needs the summation-order term to pass: where 4 x the yardstick is exceeded, 2e-6 of the scale holds.  The three launches
at and above 64 KiB of dynamic LDS run and give the same figures as the small ones.  Data drawn on the device: |drawn - predicted|
0, 9.5e-7, 3.8e-6 and 1.3e-5 at 1, 45, 252 and 1 025 values against bounds of 1.2e-4 .. 5.3e-3; another offset's data 1.8 .. 39."""
import ctypes as C
import functools
import math
import types

import numpy as np
import pytest
import torch

from brancher_amd import lowering
from oracle import philox_ref as R

pytestmark = pytest.mark.gpu

B, U = lowering.BINOP, lowering.UNOP
ERR_INVALID, ERR_RESOURCE = -1, -5

# (rows, cols, n_data, slot inputs, uniform inputs, samples)
CASES = [(1, 1, 1, 1, 0, 1), (3, 5, 3, 2, 1, 37), (7, 9, 4, 3, 0, 37), (8, 8, 5, 3, 1, 37), (5, 13, 1, 0, 0, 37), (1, 257, 2, 0, 2, 37),
         (16, 16, 7, 4, 4, 37), (3, 3, 300, 1, 1, 37), (40, 40, 15, 3, 0, 37),
         (46, 89, 2, 3, 0, 5),        # exactly 65 536 B of dynamic LDS
         (65, 65, 2, 3, 0, 5),        # 67 632 B: the first launch above 64 KiB
         (61, 69, 57, 4, 4, 5)]       # 153 576 B: the last size under the cap of 153 600 B
WEIGHTED = (16, 16, 7, 4, 4, 37)      # the drawn node of this case has weight 0.37, every other one 1.0
DRAWN_ON_DEVICE = [(1, 1, 1), (3, 5, 3), (7, 9, 4), (5, 41, 5)]      # datapoints x elements = 1, 45, 252, 1 025
SEED, OFFSET = 0x5DEECE66D1234567, (1 << 32) + 5
SLOT_ROWS = (7, 2, 11, 4, 9, 0, 5, 13)                              # rows of the sample matrix the slot inputs are read from
SAMPLE_ROWS, N_PARAMS = 16, 24
SENTINEL = 12345.0


def lds_bytes(case):
    rows, cols, n_data, n_slot, n_uni, _ = case
    return (n_slot + n_uni + 1) * (rows * cols + n_data) * 4


def test_the_lds_sizes_the_cases_are_named_for():
    assert [lds_bytes(c) for c in CASES[-3:]] == [65536, 67632, 153576]


def expression_code(n_in):
    code = []

    def emit(*ins):
        code.append(ins)
        return len(code) - 1

    mat, inp, imm = (lambda a: emit("MAT", 0, a, 0, 0.0)), (lambda k: emit("INPUT", 0, k, 0, 0.0)), (lambda v: emit("IMM", 0, 0, 0, v))
    op2, op1 = (lambda op, a, b: emit("BIN", B[op], a, b, 0.0)), (lambda op, a: emit("UN", U[op], a, 0, 0.0))
    mx, my = mat(0), mat(1)
    if n_in == 0:
        op2("mul", mx, my)
        return code
    dx = op2("sub", mx, inp(0))
    sq = op2("mul", dx, dx)
    if n_in > 1:
        dy = op2("sub", my, inp(1))
        sq = op2("add", sq, op2("mul", dy, dy))
    t = op2("mul", imm(-0.5), sq)
    if n_in > 2:
        i2 = inp(2)
        t = op2("truediv", t, op2("mul", i2, i2))
    a = op1("exp", t)
    if n_in > 3:
        a = op2("mul", a, inp(3))
    if n_in > 4:
        a = op2("add", a, op2("mul", inp(4), mx))
    if n_in > 5:
        a = op2("add", a, op2("mul", inp(5), my))
    if n_in > 6:
        a = op2("add", a, op2("mul", inp(6), op2("mul", mx, my)))
    if n_in > 7:
        a = op2("add", a, inp(7))
    return code


def expression_torch(mx, my, v):
    """the same expression in torch: mx, my [E], v a list of [N, E] tensors -> [N, E]"""
    if not v:
        return mx * my
    sq = (mx - v[0]) ** 2
    if len(v) > 1:
        sq = sq + (my - v[1]) ** 2
    t = -0.5 * sq
    if len(v) > 2:
        t = t / (v[2] * v[2])
    a = torch.exp(t)
    if len(v) > 3:
        a = a * v[3]
    if len(v) > 4:
        a = a + v[4] * mx
    if len(v) > 5:
        a = a + v[5] * my
    if len(v) > 6:
        a = a + v[6] * (mx * my)
    if len(v) > 7:
        a = a + v[7]
    return a


class Case:
    """the inputs of one case (seeded by its shape) and its torch references"""

    def __init__(self, case):
        self.rows, self.cols, self.n_data, self.n_slot, self.n_uni, self.N = case
        self.E, self.K = self.rows * self.cols, self.n_slot + self.n_uni
        rng = np.random.RandomState(1000 * self.rows + 10 * self.cols + self.n_data)
        N, K = self.N, self.K
        self.mx = np.tile(np.linspace(-1.0, 1.0, self.cols)[None, :], (self.rows, 1)).astype(np.float32)
        self.my = np.tile(np.linspace(-1.0, 1.0, self.rows)[:, None], (1, self.cols)).astype(np.float32)

        def draw(k, n):
            if k == 2:
                return np.exp(rng.normal(-0.4, 0.25, n))
            if k == 3:
                return rng.uniform(0.5, 1.5, n)
            return rng.uniform(-0.8, 0.8, n) if k < 2 else rng.uniform(-1.5, 1.5, n)

        self.slot = [draw(k, N).astype(np.float32) for k in range(self.n_slot)]
        # uniform entries: value = a + b * softplus(params[src]) with a != 0, b != 1; the raw parameter from the value wanted
        self.uni = np.zeros(self.n_uni, dtype=lowering.UNIFORM_DTYPE)
        self.params = rng.normal(0.0, 1.0, N_PARAMS).astype(np.float32)
        for j in range(self.n_uni):
            k = self.n_slot + j
            a, b = (0.1 + 0.05 * j if k in (2, 3) else -(1.7 + 0.05 * j)), 0.7 + 0.1 * j
            y = (float(draw(k, 1)[0]) - a) / b
            assert y > 0.05
            src = 3 + 2 * j
            self.params[src] = math.log(math.expm1(y))
            self.uni[j] = (src, lowering.UT["softplus"], 1, 0, a, b)
        self.X = [rng.normal(0.0, 1.0, (self.n_data, self.E)).astype(np.float32) for _ in range(2)]
        self.mean = rng.normal(0.0, 1.0, (self.n_data, self.E)).astype(np.float32)
        self.scale = rng.uniform(0.5, 1.5, (self.n_data, self.E)).astype(np.float32)

    def node(self, drawn, weight=1.0, n_slot=None, uni=None, n_data=None):
        n_slot, uni = self.n_slot if n_slot is None else n_slot, self.uni if uni is None else uni
        return types.SimpleNamespace(code=expression_code(min(n_slot + len(uni), 8)), mats=np.stack([self.mx, self.my]), uniform_inputs=uni,
                                     slot_inputs=list(SLOT_ROWS[:n_slot]), rows=self.rows, cols=self.cols,
                                     n_data=self.n_data if n_data is None else n_data, drawn=drawn, weight=weight,
                                     data_mean=self.mean if drawn else self.X[0], data_scale=self.scale if drawn else None)

    def samples(self):
        s = np.zeros((SAMPLE_ROWS, self.N), dtype=np.float32)
        for k, v in enumerate(self.slot):
            s[SLOT_ROWS[k]] = v
        return s

    def values(self, dtype):
        """the input VALUES [K][N] (a uniform input: behind its transform, evaluated in `dtype` from the float32 parameter)"""
        v = [torch.tensor(s).to(dtype) for s in self.slot]
        for u in self.uni:
            p = torch.tensor(self.params[int(u["src"])]).to(dtype)
            a, b = torch.tensor(u["a"]).to(dtype), torch.tensor(u["b"]).to(dtype)
            v.append((a + b * torch.nn.functional.softplus(p)).expand(self.N).clone())
        return v

    @functools.lru_cache(maxsize=None)
    def expression(self, dtype):
        """A [N, E] and dA / d in_k [K][N, E] by autograd on the input values: every element has its own copy of each input, so one
        reverse pass of sum(A) leaves dA_e / d in_k in the copies (r_d is linear in A: d r_d / d in_k = sum_e dA_e / d in_k X_de)"""
        leaves = [v[:, None].expand(self.N, self.E).clone().requires_grad_(True) for v in self.values(dtype)]
        mx, my = (torch.tensor(m.reshape(-1)).to(dtype) for m in (self.mx, self.my))
        A = expression_torch(mx, my, leaves)
        if leaves:
            A.sum().backward()
        else:
            A = A[None].expand(self.N, self.E)
        return A.detach(), [l.grad for l in leaves]

    @functools.lru_cache(maxsize=None)
    def reference(self, which, dtype):
        """blocks [K + 1] of (sum_e term, sum_e |term|), each [N, n_data] in double: the gradient rows of input k, then r"""
        A, dA = self.expression(dtype)
        X = torch.tensor(self.X[which]).to(dtype)
        out = []
        for v in dA + [A]:
            terms = v[:, None, :] * X[None]
            out.append((terms.sum(-1).double().numpy(), terms.abs().sum(-1).double().numpy()))
        return out

    @functools.lru_cache(maxsize=None)
    def log_prob(self, which, dtype):
        """(sum, sum of |term|) of log N(X | mean, scale)"""
        lp = torch.distributions.Normal(torch.tensor(self.mean).to(dtype), torch.tensor(self.scale).to(dtype)).log_prob(torch.tensor(self.X[which]).to(dtype))
        return float(lp.sum()), float(lp.abs().sum().double())


@functools.lru_cache(maxsize=None)
def the_case(case):
    return Case(case)


class Handle:
    def __init__(self, node):
        from brancher_amd import native
        self.native, self.lib, self.node = native, native.load(), node
        self.desc, self.keep = native.reduce_desc(node)
        self.handle = C.c_void_p()
        native.check(self.lib.bsvi_reduce_create(C.byref(self.desc), C.byref(self.handle)))
        self.n_rows = int(self.lib.bsvi_reduce_rows_out(C.byref(self.desc)))

    def eval_rc(self, samples, params, data=None, seed=0, offset=0):
        """one evaluation into a NaN-filled output with a sentinel row behind it -> (return code, rows [n_rows, N] in double)"""
        dev = torch.device("cuda:0")
        N = samples.shape[1]
        samples_d, params_d = torch.tensor(samples).to(dev), torch.tensor(params).to(dev)
        data_d = torch.tensor(np.ascontiguousarray(data, dtype=np.float32)).to(dev) if data is not None else None
        out = torch.full((self.n_rows + 1, N), float("nan"), device=dev)
        out[-1] = SENTINEL
        args = self.native.ReduceArgs(params_dev=params_d.data_ptr(), samples_dev=samples_d.data_ptr(), rows_out_dev=out.data_ptr(), n_samples_local=N,
                                      data_dev=data_d.data_ptr() if data_d is not None else None, seed=seed, offset=offset, stream=None)
        for k, row in enumerate(self.node.slot_inputs):
            args.input_rows[k] = row
        rc = self.lib.bsvi_reduce_eval(self.handle, C.byref(args))
        torch.cuda.synchronize()
        got = out.cpu().double().numpy()
        assert (got[-1] == SENTINEL).all(), "the row behind the output was written"
        return rc, got[:-1]

    def eval(self, *args, **kw):
        rc, got = self.eval_rc(*args, **kw)
        self.native.check(rc)
        return got

    def close(self):
        self.lib.bsvi_reduce_destroy(self.handle)


def check_rows(tag, c, got, which):
    """the (K + 1) * n_data coefficient and value rows of one evaluation against the references of data set `which`"""
    ref, f32, values = c.reference(which, torch.float64), c.reference(which, torch.float32), [v.numpy() for v in c.values(torch.float64)]
    nd, K = c.n_data, c.K
    order = (math.ceil(c.E / 64) + 7) * 2.0 ** -24
    assert np.isfinite(got).all(), tag
    g = [got[k * nd:(k + 1) * nd].T for k in range(K)]
    mine = g + [got[K * nd:(K + 1) * nd].T + sum(g[k] * values[k][:, None] for k in range(K))]
    failed = []
    for k in range(K + 1):
        name = "d r / d in%d" % k if k < K else "r"
        (r64, a64), (r32, _) = ref[k], f32[k]
        err, yard, scale = np.abs(mine[k] - r64), np.abs(r32 - r64).max(), np.abs(r64).max()
        two, three = max(4.0 * yard, 2e-6 * scale), np.maximum(max(4.0 * yard, 2e-6 * scale), order * a64)
        print("%s %s: err %.3g, torch float32 %.3g (x %.2f), scale %.3g, worst err / bound %.3g%s"
              % (tag, name, err.max(), yard, err.max() / (yard + 1e-300), scale, (err / three).max(),
                 "" if (err <= two).all() else "  [passes by the summation-order term only]" if (err <= three).all() else "  [FAILS]"))
        if not (err <= three).all():
            failed.append((name, err.max(), yard, scale))
    assert not failed, (tag, failed)


def check_log_prob(tag, c, got, which, weight):
    assert (got[-1] == got[-1][0]).all(), tag
    (lp64, abs64), (lp32, _) = c.log_prob(which, torch.float64), c.log_prob(which, torch.float32)
    err, yard = abs(got[-1][0] - weight * lp64), abs(weight) * abs(lp32 - lp64)
    print("%s log p: err %.3g, torch float32 %.3g (x %.2f), sum |term| %.3g" % (tag, err, yard, err / (yard + 1e-300), abs(weight) * abs64))
    assert err <= max(4.0 * yard, 2e-6 * abs(weight) * abs64), (tag, err, yard, abs64)


def case_id(case):
    return "%dx%d_d%d_s%d_u%d" % case[:5]


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_constant_data_rows_match_torch_double(case):
    c = the_case(case)
    h = Handle(c.node(drawn=False))
    assert h.n_rows == (c.K + 1) * c.n_data + 1
    got = h.eval(c.samples(), c.params)
    rc, _ = h.eval_rc(c.samples(), c.params, data=c.X[1])               # refused on the host: a constant node takes no data
    h.close()
    assert rc == ERR_INVALID
    check_rows("constant " + case_id(case), c, got, 0)
    assert (got[-1] == 0.0).all()


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_drawn_node_handed_its_data_matches_torch_double(case):
    c, weight = the_case(case), 0.37 if case == WEIGHTED else 1.0
    h = Handle(c.node(drawn=True, weight=weight))
    assert h.n_rows == (c.K + 1) * c.n_data + 1
    first = h.eval(c.samples(), c.params, data=c.X[0])
    second = h.eval(c.samples(), c.params, data=c.X[1])                 # the same handle, other data: the first must not linger
    h.close()
    for which, got in ((0, first), (1, second)):
        tag = "given[%d] %s" % (which, case_id(case))
        check_rows(tag, c, got, which)
        check_log_prob(tag, c, got, which, weight)


def test_refusals_on_the_host():
    from brancher_amd import native
    lib = native.load()

    def create_rc(node):
        d, keep = native.reduce_desc(node)
        handle = C.c_void_p()
        rc = lib.bsvi_reduce_create(C.byref(d), C.byref(handle))
        assert rc != 0 and not handle.value
        return rc

    c = the_case(CASES[-1])
    assert create_rc(c.node(drawn=False, n_data=58)) == ERR_RESOURCE       # one datapoint over the LDS cap (the data: 57 rows; never read)
    nine = np.zeros(4, dtype=lowering.UNIFORM_DTYPE)
    assert create_rc(the_case(CASES[1]).node(drawn=False, n_slot=5, uni=nine)) == ERR_RESOURCE
    assert create_rc(the_case(CASES[0]).node(drawn=False, n_data=4097)) == ERR_RESOURCE


def _normal_tol():
    """the Normal bound of tests/test_gpu_noise.py: 16 x the error of Box-Muller in single precision on the host, at most 1e-4"""
    s = np.arange(1 << 16)
    yard = np.abs(R.normal_rows(0x1234567890ABC, 3, s, np.arange(8), dtype=np.float32).astype(np.float64) - R.normal_rows(0x1234567890ABC, 3, s, np.arange(8))).max()
    return min(16 * float(yard), 1e-4)


@pytest.mark.parametrize("shape", DRAWN_ON_DEVICE, ids=lambda s: "%dx%d_d%d" % s)
def test_data_drawn_on_the_device_is_the_predicted_data(shape):
    """Without `data_dev` the node draws X = mean + scale * eps itself (reduce_data_kernel: four normals per Philox call, a tail of
    1 .. 3 elements at these sizes, a second workgroup's partial sum at 1 025).  Its rows must be those of the same node HANDED the
    predicted data; bound and control as test_reduce_node_draws_the_predicted_data: four times what a noise error at the Normal
    bound does to the rows, or 1e-5 of their scale, and the data of the next offset far outside it."""
    c = the_case(shape + (2, 1, 37))
    h = Handle(c.node(drawn=True, weight=0.37))
    mean, scale = c.mean.astype(np.float64), c.scale.astype(np.float64)
    DE, tol, rng = mean.size, _normal_tol(), np.random.RandomState(3)
    given = lambda eps: h.eval(c.samples(), c.params, data=mean + scale * eps.reshape(mean.shape))
    eps = R.reduce_data_noise(SEED, OFFSET, DE)
    drawn, pred = h.eval(c.samples(), c.params, seed=SEED, offset=OFFSET), given(eps)
    yard = np.abs(given(eps + tol * rng.choice([-1.0, 1.0], DE)) - pred).max()
    other = np.abs(given(R.reduce_data_noise(SEED, OFFSET + 1, DE)) - pred).max()
    h.close()
    bound, err = max(4 * yard, 1e-5 * np.abs(pred).max()), np.abs(drawn - pred).max()
    print("drawn %s: |drawn - predicted| %.3g, bound %.3g, another offset's data %.3g" % (shape, err, bound, other))
    assert np.isfinite(drawn).all() and err <= bound and other > 10 * bound
