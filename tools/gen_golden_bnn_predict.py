"""
Generates tests/golden/bnn_predict/bnn_predict_*.npz — what the REAL reference answers to the posterior-predictive call of its
classification scripts, `model._get_posterior_sample(N, input_values={x: rows})` (tests/test_MNIST_bayesian_neural_network.py:79),
for three small models of the Bayesian-neural-network family, on the CPU:

    classifier   16-5-3, tanh, biases        (workloads.build_bayesian_neural_network)
    bernoulli    16-4-1, tanh, biases        (the same builder, one logit: Binomial(1))
    regression   16-5-2, tanh, biases        (workloads.build_bnn_regression)

Per model: the posterior's parameters as the reference holds them, three given rows, the key set and the shapes of the call at N = 4 and
of the call without `input_values`, the columns of the DataFrame form, and at N_REF = 4000 (torch seeded) the per-(row, class)
frequencies of the reference's one-hot draws — for the regression model the per-(row, output) mean and variance of its draws.  Beside
them the predictive in DOUBLE precision at 10^5 weight samples (numpy; the posterior's row parameters through this project's lowering):
`p` per (row, class), or mean / variance / fourth central moment per (row, output).  Before a fixture is written the tool ASSERTS that
the reference's own statistics lie within 5 standard errors (the 1 / N_REF part of the test's bound) of that predictive: the bound of
tests/test_gpu_bnn_predict.py is then known to hold for the reference alone, and the predictive is checked against the reference.

The DataFrame form (`get_posterior_sample`) of the regression model with a sigma per output fails inside the reference (its input
reformatting does not broadcast the scale [C, 1] against the rows): the fixture then records the first line of the error in place of
the frame's columns, and the raw form, which works, is what the statistics come from.

The fixtures live in a subdirectory because an .npz directly in tests/golden/ is looked up in the case table of oracle/gen_golden.py.
These are data the reference writes; no program text of the reference is stored.

Usage:  PYTHONDONTWRITEBYTECODE=1 OMP_NUM_THREADS=1 python tools/gen_golden_bnn_predict.py        (BSVI_GOLDEN_OUT: another directory)
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, ROOT)

import gen_golden  # noqa: E402

SUBDIR = "bnn_predict"
N_SHAPES, N_REF, N_EXACT, CHUNK = 4, 4000, 100000, 10000
COMMON = dict(dataset_size=40, batch_size=8)
CASES = {
    "bnn_predict_classifier_16_5_3": ("build_bayesian_neural_network",
                                      dict(COMMON, widths=[16, 5, 3], pixels="integers", q_scale1=0.05, q_loc_scale=4.0)),
    "bnn_predict_bernoulli_16_4_1": ("build_bayesian_neural_network",
                                     dict(COMMON, widths=[16, 4, 1], pixels="integers", q_scale1=0.05, q_loc_scale=4.0)),
    "bnn_predict_regression_16_5_2": ("build_bnn_regression", dict(COMMON, widths=[16, 5, 2], sigma=[0.3, 0.6], q_scale=0.3)),
}


class ShapeKeyedNormals:
    """The reference walks a variable's parents as a SET hashed by address, so the order in which the latents consume torch's global
    generator differs from process to process.  While active, every standard-normal draw of torch.distributions (the reference's
    Normal samples: distributions.py:122 through torch normal.py:83-86) comes from a generator of its own, seeded by the draw's SHAPE
    and `seed` — the draws no longer depend on that order, and the fixtures regenerate bit for bit.  Two draws of one shape inside one
    block would be the same numbers: refused."""

    def __init__(self, seed):
        self.seed, self.seen = seed, set()

    def __enter__(self):
        import zlib
        import torch
        import torch.distributions.normal as tn
        self.tn, self._sn = tn, tn._standard_normal

        def standard_normal(shape, dtype, device):
            key = tuple(int(d) for d in shape)
            assert key not in self.seen, "two normal draws of shape %r in one call" % (key,)
            self.seen.add(key)
            g = torch.Generator().manual_seed(self.seed * 1000003 + zlib.crc32(repr(key).encode()))
            return torch.randn(key, generator=g, dtype=dtype, device=device)

        tn._standard_normal = standard_normal
        return self

    def __exit__(self, *exc):
        self.tn._standard_normal = self._sn


def given_rows():
    """three rows of 16 features, integers -3 .. 3 (exactly bf16), in the reference's layout [1, M, P, 1]"""
    return np.random.RandomState(1).randint(-3, 4, size=(1, 3, 16, 1)).astype(np.float32)


def row_parameters(program):
    """(q loc [R], q scale [R], sigma [C] or None) of a lowered program in double precision"""
    from brancher_amd import bnn, lowering
    loc, scale = bnn.row_parameters(program)
    sigma = None
    if program.likelihood == bnn.LIK_NORMAL:
        sigma = []
        for c in range(program.n_classes):
            e = program.uniform[program.scale_uniform + c * program.scale_stride]
            x = float(program.consts[e["src"]])
            g = {lowering.UT["identity"]: x, lowering.UT["softplus"]: float(np.log1p(np.exp(x)))}[int(e["transform"])]
            sigma.append(float(e["a"]) + float(e["b"]) * g)
        sigma = np.array(sigma)
    return loc, scale, sigma


ACT = {0: lambda v: v, 1: np.tanh, 2: lambda v: np.maximum(v, 0.0), 3: lambda v: 1.0 / (1.0 + np.exp(-v)), 4: lambda v: np.logaddexp(v, 0.0)}


def chain(program, weights, rows):
    """weights [n, R] (the latent vector per sample), rows [M, P] -> the head's outputs [n, M, C], in the dtype of `weights`"""
    h = np.broadcast_to(rows.astype(weights.dtype)[None], (weights.shape[0],) + rows.shape)
    for layer in program.layers:
        r, c, w0, b0 = layer["rows"], layer["cols"], layer["weight_row0"], layer["bias_row0"]
        w = weights[:, w0:w0 + r * c].reshape(-1, r, c)
        h = np.einsum("nmc,nrc->nmr", h, w)
        if b0 != 0xFFFFFFFF:
            h = h + weights[:, None, b0:b0 + r]
        h = ACT[layer["activation"]](h)
    return h


def exact_predictive(program, rows):
    """the predictive at N_EXACT weight samples in double precision: classifiers {p [M, C]}; regression {mean, var, m4 [M, C]} of y"""
    loc, scale, sigma = row_parameters(program)
    rng = np.random.RandomState(12345)
    M, C = rows.shape[0], program.n_classes
    s1, s2, s3, s4 = (np.zeros((M, C)) for _ in range(4))
    for _ in range(N_EXACT // CHUNK):
        z = chain(program, loc + scale * rng.normal(size=(CHUNK, loc.size)), rows.astype(np.float64))
        if program.likelihood == 0:
            z = np.exp(z - z.max(axis=2, keepdims=True))
            z = z / z.sum(axis=2, keepdims=True)
        elif program.likelihood == 1:
            z = 1.0 / (1.0 + np.exp(-z))
        s1 += z.sum(0); s2 += (z ** 2).sum(0); s3 += (z ** 3).sum(0); s4 += (z ** 4).sum(0)
    m1, m2, m3, m4 = (s / N_EXACT for s in (s1, s2, s3, s4))
    if program.likelihood != 2:
        return dict(p=m1)
    v = m2 - m1 ** 2                                  # (double precision at O(1) values: fine here; the kernels sum about the mean)
    c4 = m4 - 4 * m1 * m3 + 6 * m1 ** 2 * m2 - 3 * m1 ** 4
    s2_ = sigma[None, :] ** 2
    return dict(mean=m1, var=v + s2_, m4=c4 + 6 * v * s2_ + 3 * s2_ ** 2, sigma=sigma)


def run_case(name, api, out_dir):
    import torch
    from brancher_amd import bnn, workloads as W
    builder, kw = CASES[name]
    model = getattr(W, builder)(api, **kw)
    x = next(v for v in model.flatten() if v.name == "x")
    lik = next(v for v in model.flatten() if v.name in ("k", "y"))
    rows = given_rows()
    rows_t = torch.tensor(rows)
    native = getattr(W, builder)(W.native_api(), **kw)
    program = bnn.lower_bnn(native, native.posterior_model)
    shape_of = lambda v: list(v.shape) if hasattr(v, "shape") else list(np.shape(v))
    data = {"rows": rows}
    torch.manual_seed(7)
    s = model._get_posterior_sample(N_SHAPES, input_values={x: rows_t})
    keys = {k.name: shape_of(v) for k, v in s.items()}
    torch.manual_seed(8)
    s0 = model._get_posterior_sample(N_SHAPES)
    keys_no_input = {k.name: shape_of(v) for k, v in s0.items()}
    torch.manual_seed(9)
    try:
        frame = model.get_posterior_sample(3, input_values={x: rows_t})
        frame_meta = dict(frame_rows=int(frame.shape[0]), frame_columns=sorted(str(c) for c in frame.columns))
    except RuntimeError as err:
        frame_meta = dict(frame_rows=None, frame_error="RuntimeError: " + str(err).splitlines()[0])
    for pname, root in gen_golden.named_parameters(model, model.posterior_model).items():
        data["param/" + pname] = root.link.parameter.detach().numpy().copy() if hasattr(root.link, "parameter") else np.asarray(root.value)
    torch.manual_seed(11)                              # (the Categorical / Bernoulli draw: the only one left on the global generator)
    with ShapeKeyedNormals(11):
        draws = model._get_posterior_sample(N_REF, input_values={x: rows_t})[lik].detach().numpy().astype(np.float64)
    draws = draws.reshape(N_REF, rows.shape[1], -1)
    exact = exact_predictive(program, rows[0, :, :, 0])
    meta = dict(builder=builder, kwargs=kw, likelihood=lik.name, n_shapes=N_SHAPES, n_ref=N_REF, n_exact=N_EXACT, keys=keys,
                keys_no_input=keys_no_input, **frame_meta)
    if program.likelihood == 2:
        data["ref_mean"], data["ref_var"] = draws.mean(0), draws.var(0)
        for k in ("mean", "var", "m4", "sigma"):
            data["exact_" + k] = exact[k]
        se_mean = np.sqrt(exact["var"] / N_REF)
        se_var = np.sqrt((exact["m4"] - exact["var"] ** 2) / N_REF)
        assert (np.abs(data["ref_mean"] - exact["mean"]) <= 5 * se_mean).all(), (data["ref_mean"], exact["mean"], se_mean)
        assert (np.abs(data["ref_var"] - exact["var"]) <= 5 * se_var).all(), (data["ref_var"], exact["var"], se_var)
    else:
        data["ref_freq"], data["p"] = draws.mean(0), exact["p"]
        se = np.sqrt(exact["p"] * (1 - exact["p"]) / N_REF)
        assert (np.abs(data["ref_freq"] - exact["p"]) <= 5 * se).all(), (data["ref_freq"], exact["p"], se)
    data["meta"] = np.array(json.dumps(meta, sort_keys=True))
    os.makedirs(out_dir, exist_ok=True)
    np.savez(os.path.join(out_dir, name + ".npz"), **data)
    print(name, "keys", sorted(keys), "| no input", sorted(keys_no_input))


if __name__ == "__main__":
    out = os.environ.get("BSVI_GOLDEN_OUT") or os.path.join(ROOT, "tests", "golden", SUBDIR)
    api = gen_golden.reference_api()
    for case in sys.argv[1:] or list(CASES):
        run_case(case, api, out)
