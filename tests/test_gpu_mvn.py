"""The batched multivariate-normal kernel (bsvi_mvn_*) through the C ABI: log N(x | m, C(s)) and its
gradients for a covariance that is an elementwise expression of constant matrices and per-sample / learnable scalars,
against torch.distributions.MultivariateNormal + autograd in double precision (what the reference computes,
brancher/distributions.py:314-331).

The yardstick of every check — torch's own float32 error — comes from tests/golden/mvn/torch_f32.npz: torch's float32
results on the CPU at 1, 2 and 4 threads (three summation orders), recorded by `python tests/test_gpu_mvn.py`, and the
yardstick is the largest of their errors.  Computed live from one run, it followed the host's BLAS / LAPACK code path and
thread count — the amplitude's coefficient moved between 1.2e-3 and 2.0e-3 of its scale at D = 515 and between 4.1e-4 and
5.3e-4 at D = 256 — and with it the verdict on the same kernel result.  The double-precision truth is computed live."""
import ctypes as C
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F32_FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mvn", "torch_f32.npz")
GP_CASES = [(5, True), (12, True), (32, True), (33, False), (64, True), (100, True), (100, False), (128, True), (131, False), (160, True),
            (192, True), (193, True), (200, False), (256, True), (322, False), (515, False)]
OTHER_FORMS, OTHER_DIMS = ["scale_tril", "precision_matrix"], [7, 33, 61, 130, 190, 257]


F32_THREADS = (1, 2, 4)


def recorded_f32(case):
    """torch's float32 results of one case as recorded in the fixture: one dict per thread count"""
    data = np.load(F32_FIXTURE)
    runs = {}
    for k in data.files:
        if k.startswith(case + "/"):
            threads, key = k[len(case) + 1:].split("/")
            runs.setdefault(threads, {})[key] = data[k].astype(np.float64)
    assert len(runs) == len(F32_THREADS), (case, sorted(runs))
    return list(runs.values())


def f32_error(runs, key, ref):
    """torch's own float32 error: the largest over the recorded runs"""
    return max(np.abs(r[key] - ref).max() for r in runs)


def gp_node(D, latent_x, weight=1.0, jitter=1e-2, seed=0):
    from brancher_amd import lowering
    rng = np.random.RandomState(seed)
    x = np.sort(rng.uniform(-2.0, 2.0, D))
    sq = ((x[:, None] - x[None, :]) ** 2).astype(np.float32)
    eye = (jitter * np.eye(D)).astype(np.float32)
    B, U = lowering.BINOP, lowering.UNOP
    # C = exp(sqdist * -0.5 / (ell * ell)) * amp + jitter I;   inputs: 0 = ell (a slot row), 1 = amp (a learnable parameter)
    code = [("MAT", 0, 0, 0, 0.0), ("IMM", 0, 0, 0, -0.5), ("BIN", B["mul"], 0, 1, 0.0), ("INPUT", 0, 0, 0, 0.0),
            ("BIN", B["mul"], 3, 3, 0.0), ("BIN", B["truediv"], 2, 4, 0.0), ("UN", U["exp"], 5, 0, 0.0), ("INPUT", 0, 1, 0, 0.0),
            ("BIN", B["mul"], 6, 7, 0.0), ("MAT", 0, 1, 0, 0.0), ("BIN", B["add"], 8, 9, 0.0)]
    uni = np.zeros(1, dtype=lowering.UNIFORM_DTYPE)
    uni["src"], uni["is_param"], uni["transform"], uni["a"], uni["b"] = 2, 1, lowering.UT["softplus"], 0.0, 1.0
    loc = rng.normal(0.0, 0.3, D).astype(np.float32)
    value = None if latent_x else rng.normal(0.0, 1.0, D).astype(np.float32)
    return types.SimpleNamespace(code=code, mats=np.stack([sq, eye]), loc=loc, value=value, dim=D, uniform_inputs=uni,
                                 slot_inputs=[0], weight=weight), sq, eye


@pytest.mark.parametrize("D,latent_x", GP_CASES)
def test_log_density_and_gradients_match_torch_double(D, latent_x):
    # (beyond 192 — the matrix of a sample in device memory — the jitter of the reference fixtures of that size, 5e-2: with 1e-2 the
    #  condition number passes 1e5 at 256 inputs and the amplitude's coefficient, a difference of two large traces, is 4.6-4.8 x
    #  torch's own float32 error there instead of within 4 x; the test below keeps that on record)
    check_against_torch(D, latent_x, gp_jitter(D), 4.0)


def gp_jitter(D):
    return 1e-2 if D <= 192 else 5e-2


def test_ill_conditioned_large_covariance_stays_within_eight_times_torch_float32():
    check_against_torch(256, True, 1e-2, 8.0)


def gp_case(D, latent_x, jitter):
    return "gp/D%d_%s_j%g" % (D, "latent" if latent_x else "observed", jitter)


def gp_inputs(D, latent_x, jitter, N=37):
    node, sq, eye = gp_node(D, latent_x, weight=0.5, seed=D, jitter=jitter)
    g = torch.Generator().manual_seed(D)
    ell = torch.exp(-0.4 + 0.25 * torch.randn(N, generator=g)).float()
    xs = torch.randn(D, N, generator=g).float() * 0.8
    params = torch.tensor([0.0, 0.0, 0.9, 0.0])                    # amp = softplus(params[2])
    return node, sq, eye, ell, xs, params


def gp_torch(D, latent_x, jitter, dtype):
    """torch: double precision as the truth, single precision (what the reference computes) as the yardstick — the covariance
    has a condition number of ~amp / jitter * D, so float32 results of ANY algorithm carry that many ulps"""
    node, sq, eye, ell, xs, params = gp_inputs(D, latent_x, jitter)
    N = ell.shape[0]
    ell_t = ell.to(dtype).clone().requires_grad_(True)
    p2 = params[2].to(dtype).clone().requires_grad_(True)
    x_t = (xs.to(dtype).T.clone() if latent_x else torch.tensor(node.value).to(dtype).expand(N, D).clone()).requires_grad_(True)
    amp = torch.nn.functional.softplus(p2)
    sq_t, eye_t = torch.tensor(sq).to(dtype), torch.tensor(eye).to(dtype)
    amps = amp.expand(N).clone()                       # (per-sample copies: their gradients are the per-sample coefficients)
    amps.retain_grad()
    Cm = torch.exp(sq_t[None] * -0.5 / (ell_t * ell_t)[:, None, None]) * amps[:, None, None] + eye_t[None]
    lp = torch.distributions.MultivariateNormal(torch.tensor(node.loc).to(dtype), covariance_matrix=Cm).log_prob(x_t)
    (0.5 * lp).sum().backward()
    out = dict(lp=0.5 * lp.detach().double().numpy(), ell=ell_t.grad.double().numpy(), amp=amps.grad.double().numpy(),
               amp_value=float(amp.detach()))
    if latent_x:
        out["x"] = x_t.grad.double().numpy().T
    return out


def check_against_torch(D, latent_x, jitter, factor):
    from brancher_amd import native
    lib = native.load()
    dev = torch.device("cuda:0")
    node, sq, eye, ell, xs, params = gp_inputs(D, latent_x, jitter)
    N = ell.shape[0]
    d, keep = native.mvn_desc(node)
    handle = C.c_void_p()
    native.check(lib.bsvi_mvn_create(C.byref(d), C.byref(handle)))
    n_out = int(lib.bsvi_mvn_rows_out(C.byref(d)))
    # sample rows: row 3 = ell, rows 5 .. 5 + D = x (when latent)
    samples = torch.zeros(5 + D + 2, N)
    samples[3] = ell
    samples[5:5 + D] = xs
    samples_d, params_d = samples.to(dev), params.to(dev)
    out = torch.full((n_out, N), float("nan"), device=dev)
    args = native.MvnArgs(params_dev=params_d.data_ptr(), samples_dev=samples_d.data_ptr(), rows_out_dev=out.data_ptr(),
                          n_samples_local=N, value_row0=5, stream=None)
    args.input_rows[0] = 3
    native.check(lib.bsvi_mvn_eval(handle, C.byref(args)))
    torch.cuda.synchronize()
    got = out.cpu().double().numpy()
    lib.bsvi_mvn_destroy(handle)

    ref, f32 = gp_torch(D, latent_x, jitter, torch.float64), recorded_f32(gp_case(D, latent_x, jitter))

    def close(mine, key):
        scale = np.abs(ref[key]).max() + 1e-30
        err, yard = np.abs(mine - ref[key]).max() / scale, f32_error(f32, key, ref[key]) / scale
        assert err <= max(factor * yard, 2e-6), (key, err, yard)

    row = 0
    close(got[row], "ell")
    row += 1
    if latent_x:
        close(got[row:row + D], "x")
        row += D
    g_amp = got[row]
    close(g_amp, "amp")
    row += 1
    # e + sum_k g_k input_k = weight * log p
    lin = got[0] * ell.double().numpy() + g_amp * ref["amp_value"]
    if latent_x:
        lin = lin + (got[1:1 + D] * xs.double().numpy()).sum(0)
    close(got[row] + lin, "lp")


def other_case(form, D):
    return "%s/D%d" % (form, D)


def other_inputs(form, D, N=29):
    from brancher_amd import lowering
    rng = np.random.RandomState(D)
    B = lowering.BINOP
    if form == "scale_tril":
        # L = M0 * s + M1: M0 strictly lower and small, M1 a positive diagonal
        m0 = (np.tril(rng.normal(0.0, 0.3 / np.sqrt(D), (D, D)), -1)).astype(np.float32)
        m1 = np.diag(rng.uniform(0.7, 1.3, D)).astype(np.float32)
    else:
        # P = M0 * s + M1: M0 a squared-exponential kernel matrix (PSD), M1 = 0.5 I
        x = np.sort(rng.uniform(-2.0, 2.0, D))
        m0 = np.exp(-0.5 * (x[:, None] - x[None, :]) ** 2 / 0.3 ** 2).astype(np.float32)
        m1 = (0.5 * np.eye(D)).astype(np.float32)
    code = [("MAT", 0, 0, 0, 0.0), ("INPUT", 0, 0, 0, 0.0), ("BIN", B["mul"], 0, 1, 0.0), ("MAT", 0, 1, 0, 0.0), ("BIN", B["add"], 2, 3, 0.0)]
    loc = rng.normal(0.0, 0.3, D).astype(np.float32)
    value = rng.normal(0.0, 1.0, D).astype(np.float32)
    node = types.SimpleNamespace(code=code, mats=np.stack([m0, m1]), loc=loc, value=value, dim=D,
                                 uniform_inputs=np.zeros(0, dtype=lowering.UNIFORM_DTYPE), slot_inputs=[0], weight=1.0, form=form)
    g = torch.Generator().manual_seed(D)
    sc = (0.6 + 0.8 * torch.rand(N, generator=g)).float()
    return node, sc


def other_torch(form, D, dtype):
    node, sc = other_inputs(form, D)
    N = sc.shape[0]
    s_t = sc.to(dtype).clone().requires_grad_(True)
    M = torch.tensor(node.mats[0]).to(dtype)[None] * s_t[:, None, None] + torch.tensor(node.mats[1]).to(dtype)[None]
    kw = dict(scale_tril=torch.tril(M)) if form == "scale_tril" else dict(precision_matrix=M)
    lp = torch.distributions.MultivariateNormal(torch.tensor(node.loc).to(dtype), **kw).log_prob(torch.tensor(node.value).to(dtype).expand(N, D))
    lp.sum().backward()
    return dict(lp=lp.detach().double().numpy(), g=s_t.grad.double().numpy())


@pytest.mark.parametrize("form", OTHER_FORMS)
@pytest.mark.parametrize("D", OTHER_DIMS)
def test_other_parameterisations_match_torch_double(form, D):
    """`scale_tril` and `precision_matrix` (distributions.py:314-331) on the kernel family, at sizes that are NOT whole blocks of
    four (the matrix in LDS is padded with an identity block), beyond one pass of 128 lane pairs and beyond what LDS holds (257:
    the matrix of a sample is then a block of device memory, MVN_SPILL): log p and the coefficient of
    the one scalar input against torch in double precision, torch's own float32 error as the yardstick."""
    from brancher_amd import native
    lib = native.load()
    dev = torch.device("cuda:0")
    node, sc = other_inputs(form, D)
    N = sc.shape[0]
    d, keep = native.mvn_desc(node)
    handle = C.c_void_p()
    native.check(lib.bsvi_mvn_create(C.byref(d), C.byref(handle)))
    n_out = int(lib.bsvi_mvn_rows_out(C.byref(d)))
    assert n_out == 2
    samples = torch.zeros(4, N)
    samples[2] = sc
    samples_d = samples.to(dev)
    out = torch.full((n_out, N), float("nan"), device=dev)
    params_d = torch.zeros(4, device=dev)
    args = native.MvnArgs(params_dev=params_d.data_ptr(), samples_dev=samples_d.data_ptr(), rows_out_dev=out.data_ptr(),
                          n_samples_local=N, value_row0=0, stream=None)
    args.input_rows[0] = 2
    native.check(lib.bsvi_mvn_eval(handle, C.byref(args)))
    torch.cuda.synchronize()
    got = out.cpu().double().numpy()
    lib.bsvi_mvn_destroy(handle)

    r64, f32 = other_torch(form, D, torch.float64), recorded_f32(other_case(form, D))
    for mine, name, key in ((got[0], "g", "d/ds"), (got[1] + got[0] * sc.double().numpy(), "lp", "log p")):
        ref = r64[name]
        scale = np.abs(ref).max() + 1e-30
        err, yard = np.abs(mine - ref).max() / scale, f32_error(f32, name, ref) / scale
        assert err <= max(4.0 * yard, 2e-6), (form, D, key, err, yard)


def test_not_positive_definite_gives_non_finite_rows():
    from brancher_amd import native
    lib = native.load()
    dev = torch.device("cuda:0")
    node, _, _ = gp_node(16, True, jitter=-5.0)
    d, keep = native.mvn_desc(node)
    handle = C.c_void_p()
    native.check(lib.bsvi_mvn_create(C.byref(d), C.byref(handle)))
    n_out = int(lib.bsvi_mvn_rows_out(C.byref(d)))
    samples = torch.ones(40, 8, device=dev)
    out = torch.zeros(n_out, 8, device=dev)
    params = torch.zeros(4, device=dev)
    args = native.MvnArgs(params_dev=params.data_ptr(), samples_dev=samples.data_ptr(), rows_out_dev=out.data_ptr(),
                          n_samples_local=8, value_row0=5, stream=None)
    args.input_rows[0] = 3
    native.check(lib.bsvi_mvn_eval(handle, C.byref(args)))
    torch.cuda.synchronize()
    assert not torch.isfinite(out[-1]).any()
    lib.bsvi_mvn_destroy(handle)


def record_f32_fixture(path=F32_FIXTURE):
    """(re)writes tests/golden/mvn/torch_f32.npz: torch's float32 results of every case above on the CPU, at each of F32_THREADS"""
    arrays = {}
    cases = [(D, x, gp_jitter(D)) for D, x in GP_CASES] + [(256, True, 1e-2)]
    for threads in F32_THREADS:
        torch.set_num_threads(threads)
        for D, latent_x, jitter in cases:
            for key, v in gp_torch(D, latent_x, jitter, torch.float32).items():
                if key != "amp_value":
                    arrays["%s/t%d/%s" % (gp_case(D, latent_x, jitter), threads, key)] = np.asarray(v, dtype=np.float32)
        for form in OTHER_FORMS:
            for D in OTHER_DIMS:
                for key, v in other_torch(form, D, torch.float32).items():
                    arrays["%s/t%d/%s" % (other_case(form, D), threads, key)] = np.asarray(v, dtype=np.float32)
    meta = dict(written_by="python tests/test_gpu_mvn.py", torch=torch.__version__.split("+")[0], threads=list(F32_THREADS), device="cpu")
    np.savez_compressed(path, meta=json.dumps(meta, sort_keys=True), **arrays)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    record_f32_fixture()
