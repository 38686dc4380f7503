"""Digests of the two generated Bayesian-neural-network kernels' text (bnn_upper_gen, bnn_mid_gen) as a LIBRARY writes it, for the
cases below -> tests/golden/bnn_source/digests.json:
    python tools/bnn_source_dump.py [--tree DIR] OUT
(DIR: the checkout whose package and library write the text, default: this one.)  Needs a GPU: each case is lowered and compiled, and
one `evaluate` of 70 samples is made with BSVI_BNN_SOURCE_DUMP set — once as selected (bnn_mid_gen's text, where the case has one) and
once under BSVI_BNN_MID=0 (bnn_upper_gen's).  The committed file was recorded from the commit BEFORE
brancher_amd/csrc/bnn_source.h existed, so tests/test_bnn_source_cpu.py (the header alone, no GPU) and tests/test_gpu_bnn_source.py
(the library) hold the text to what the emitters inside bnn_kernel.inc wrote.
Normalisation: every line stripped, empty lines dropped, joined with "\\n"; the digest is the SHA-256 and the length of the result.
This module is also where the tests take the cases from (CASES, build, digest, describe): it imports nothing of the package on import."""
import hashlib
import json
import os
import struct
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACTS7 = ["tanh", "relu", "sigmoid", "softplus", "tanh", "relu", "sigmoid"]
SMALL = dict(batch_size=17, dataset_size=40)
R = dict(SMALL, n_features=16)                                        # build_bnn_regression: integer features (exactly bf16)
HEAD = dict(SMALL, widths=[16, 5, 4, 3])
BENCH = dict(classifier=True, dataset_size=60000, n_features=784, n_hidden=20, n_classes=10, q_scale1=4e-4, q_loc_scale=1.0)     # bench.py's "bnn"

# name: (builder keywords; classifier=True: build_bayesian_neural_network, else build_bnn_regression), environment
CASES = {
    "16-2 linear": (dict(R, n_hidden=0, n_outputs=2), {}),
    "16-1 linear no bias (Rs = 0)": (dict(R, n_hidden=0, n_outputs=1, bias=False), {}),
    "16-5-2 relu no bias": (dict(R, n_hidden=5, n_outputs=2, activation="relu", bias=False), {}),
    "16-5-1 B512 (pairs)": (dict(n_features=16, n_hidden=5, n_outputs=1, batch_size=512, dataset_size=512), {}),
    "16-4x7-2 eight layers": (dict(SMALL, widths=[16, 4, 4, 4, 4, 4, 4, 4, 2], activations=ACTS7), {}),
    "16-5-1 cauchy log1p": (dict(R, n_hidden=5, n_outputs=1, likelihood="cauchy"), dict(BSVI_BNN_CAUCHY_LOG="log1p")),
    "16-6-3 classifier": (dict(SMALL, classifier=True, n_features=16, n_hidden=6, n_classes=3, pixels="integers"), {}),
    "16-6-1 classifier": (dict(SMALL, classifier=True, n_features=16, n_hidden=6, n_classes=1, pixels="integers"), {}),
    "784-20-10 B30 (bench bnn)": (dict(BENCH, batch_size=30), {}),
    "784-20-10 B512 (bench bnn_cfg4scale)": (dict(BENCH, batch_size=512), {}),
}
for _f in ("normal", "laplace", "cauchy"):
    CASES["16-5-1 constant sigma %s" % _f] = (dict(R, n_hidden=5, n_outputs=1, likelihood=_f), {})
    CASES["16-5-3 learnable sigma %s" % _f] = (dict(R, n_hidden=5, n_outputs=3, sigma=[.3, .5, .8], learnable_sigma=True, likelihood=_f), {})
for _g, _f in (("softplus", "normal"), ("exp", "normal"), ("sigmoid", "normal"), ("exp", "laplace"), ("exp", "cauchy")):
    CASES["16-5-4-3 head %s %s" % (_g, _f)] = (dict(HEAD, scale_head=_g, likelihood=_f), {})
KINDS = ("upper", "mid")
N_SAMPLES = 70


def build(W, kw):
    kw = dict(kw)
    if kw.get("likelihood") == "normal":
        del kw["likelihood"]                  # (the default; a tree from before the keyword builds the same model)
    builder = W.build_bayesian_neural_network if kw.pop("classifier", False) else W.build_bnn_regression
    return builder(W.native_api(), **kw)


def normalise(text):
    return "\n".join(l.strip() for l in text.splitlines() if l.strip())


def digest(text):
    t = normalise(text).encode()
    return dict(sha256=hashlib.sha256(t).hexdigest(), length=len(t))


def describe(p, env):
    """a lowered BnnProgram -> the arguments of tests/c_abi/bnn_source_text.cpp behind the kind"""
    from brancher_amd import lowering
    bits = lambda x: struct.unpack("<I", struct.pack("<f", x))[0]
    g, a, b = getattr(p, "scale_head", None) or (None, 0.0, 1.0)
    args = [p.n_rows, p.n_features, p.batch_size, p.likelihood, int(getattr(p, "family", 1)), int(bool(getattr(p, "scale_learnable", False))),
            lowering.UT[g] if g else 0, bits(a), bits(b), int(env.get("BSVI_BNN_CAUCHY_LOG") == "log1p"), len(p.layers)]
    for l in p.layers:
        args += [l["rows"], l["cols"], l["weight_row0"], l["bias_row0"], l["activation"]]
    return [str(int(x)) for x in args]


def library_digests(names=None):
    """{case: {kind: digest}} of what the library of the package on sys.path writes (every case is of a size both kernels serve);
    names: the cases, or a dict from case to the one kind wanted of it (default: every case, both kinds).  The library reads its switches
    when a handle first asks for its kernel, so every case runs in this process, a new handle per kind"""
    from brancher_amd import bnn, workloads as W
    result = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name in names or CASES:
            kw, case_env = CASES[name]
            result[name] = {}
            for kind, switches in (("mid", {}), ("upper", dict(BSVI_BNN_MID="0"))):
                if isinstance(names, dict) and names[name] != kind:
                    continue
                out = os.path.join(tmp, "src")
                path = out + ".mid" if kind == "mid" else out
                for f in (out, out + ".mid"):
                    if os.path.exists(f):
                        os.remove(f)
                env = dict(case_env, BSVI_BNN_SOURCE_DUMP=out, **switches)
                saved = {k: os.environ.get(k) for k in env}
                os.environ.update(env)
                try:
                    m = build(W, kw)
                    c = bnn.CompiledBnn(m, m.posterior_model, "pathwise")
                    c.evaluate(N_SAMPLES, seed=1, offset=0)
                    assert c.middle_path() == dict(mid="mid_gen", upper="upper_gen")[kind] and os.path.exists(path), (name, kind, c.middle_path())
                finally:
                    for k, v in saved.items():
                        if v is None:
                            os.environ.pop(k, None)
                        else:
                            os.environ[k] = v
                result[name][kind] = digest(open(path).read())
    return result


if __name__ == "__main__":
    args = sys.argv[1:]
    tree = HERE
    if "--tree" in args:
        tree = os.path.abspath(args[args.index("--tree") + 1])
        del args[args.index("--tree"):args.index("--tree") + 2]
    sys.path.insert(0, tree)
    d = library_digests()
    with open(args[0], "w") as f:
        json.dump(d, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d cases, %d texts -> %s" % (len(d), sum(len(v) for v in d.values()), args[0]))
