"""The posterior-predictive pass of the Bayesian-neural-network family (bsvi_bnn_predict, `CompiledBnn.predict`) as far as it goes without
a device: the argument checks of the entry point (in front of any device work, each with its named message), the struct as the header,
the binding and the library declare it, the host functions of csrc/bnn_select.h (the LDS arm at its boundary, the default pass, the
workspace monotone in rows and samples — tests/c_abi/bnn_predict_select.cpp, compiled with the sanitizers), the reference fixtures
(they regenerate bit for bit), and the likelihood's noise stream: its host reference, written here from the contract in csrc/philox.h
on oracle.philox_ref's philox4x32 / u01 / box_muller / split64, whose (key, counter) pairs meet none of the training streams."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from brancher_amd import bnn, native, workloads as W
from oracle import philox_ref as R

KEY_PREDICT = 0x2545F491
FIXTURES = ["bnn_predict_classifier_16_5_3", "bnn_predict_bernoulli_16_4_1", "bnn_predict_regression_16_5_2"]
CSRC = os.path.join(ROOT, "brancher_amd", "csrc")


# ---- the entry point ------------------------------------------------------------------------------------------------------------
def test_predict_checks_its_arguments_in_front_of_any_device_work():
    lib = native.load()
    one = C.c_void_p(256)                     # (never dereferenced: every check below returns first)

    def call(handle=None, **change):
        a = native.BnnPredictArgs(**dict(dict(params_dev=one, x_dev=one, n_samples_local=4, n_rows=3, workspace_dev=one), **change))
        if "struct_size" in change:
            a.struct_size = change["struct_size"]
        return lib.bsvi_bnn_predict(handle, C.byref(a)), lib.bsvi_last_error()

    assert lib.bsvi_bnn_predict(None, None) == -1 and b"null argument" in lib.bsvi_last_error()
    rc, msg = call(struct_size=C.sizeof(native.BnnPredictArgs) - 8)
    assert rc == -1 and b"bsvi_bnn_predict_args::struct_size" in msg
    rc, msg = call(x_dev=None)
    assert rc == -1 and b"x_dev is null" in msg
    rc, msg = call(n_rows=0)
    assert rc == -1 and b"n_rows is 0" in msg
    rc, msg = call(n_samples_local=0)
    assert rc == -1 and b"zero samples" in msg
    for bad in (1, 31, 33, 48):
        rc, msg = call(rows_per_pass=bad)
        assert rc == -1 and b"rows_per_pass must be a multiple of 32" in msg
    rc, msg = call(workspace_dev=None)
    assert rc == -1 and b"workspace_dev is null" in msg
    rc, msg = call(rows_per_pass=64)            # everything about the arguments is in order: what is missing is the model
    assert rc == -1 and b"null handle" in msg
    # (var_out on a classifier and the 32-bit index range need a model: tests/test_gpu_bnn_predict.py)
    assert lib.bsvi_bnn_predict_workspace_bytes(None, 4, 3, 0) == 0 and lib.bsvi_bnn_predict_rows_per_pass(None, 4, 3, 0) == 0
    assert lib.bsvi_bnn_predict_lds(None) == -1 and lib.bsvi_bnn_predict_last_exact() in (-1, 0, 1)
    assert native.ABI_VERSION == 11 and lib.bsvi_abi_version() == 11            # new exports only


def test_the_struct_is_the_same_in_the_header_the_binding_and_the_library(tmp_path):
    fields = [name for name, _ in native.BnnPredictArgs._fields_]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bsvi.h"\nint main(void) {\n'
                   '    printf("sizeof %zu\\n", sizeof(bsvi_bnn_predict_args));\n'
                   + "".join('    printf("%s %%zu\\n", offsetof(bsvi_bnn_predict_args, %s));\n' % (f, f) for f in fields)
                   + "    return 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    seen = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(seen["sizeof"]) == C.sizeof(native.BnnPredictArgs) == native.load().bsvi_bnn_predict_args_size()
    for f in fields:
        assert int(seen[f]) == getattr(native.BnnPredictArgs, f).offset, f
    assert native.BnnPredictArgs not in native.STRUCT_KINDS.values()            # the kinds are a closed list (tests/c_abi/check_abi.c)


def test_the_select_functions_of_the_predict_kernel(tmp_path):
    exe = tmp_path / "bnn_predict_select"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", CSRC, "-o", str(exe), os.path.join(ROOT, "tests", "c_abi", "bnn_predict_select.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and "bnn_predict_select: ok" in out.stdout, out.stdout + out.stderr


def test_the_python_names_follow_the_header():
    assert bnn.PREDICT_PATHS == ("global", "lds")
    kernel = open(os.path.join(CSRC, "bnn_kernel.inc")).read()
    assert re.search(r"BNN_KEY_PREDICT\s*=\s*0x%08Xu;" % KEY_PREDICT, kernel, re.I)
    assert ("%#x" % KEY_PREDICT) in open(os.path.join(CSRC, "philox.h")).read().lower()
    assert ("%#x" % KEY_PREDICT) in open(os.path.join(ROOT, "include", "bsvi.h")).read().lower()


def test_row_parameters_are_the_uniform_table_on_the_host():
    model = W.build_bnn_regression(W.native_api(), widths=[16, 5, 2], batch_size=8, dataset_size=40, sigma=[0.3, 0.6], q_scale=0.3)
    p = bnn.lower_bnn(model, model.posterior_model)
    assert p.x_name == "x" and p.likelihood_name == "y"
    loc, scale = bnn.row_parameters(p)
    assert loc.shape == scale.shape == (p.n_rows,) and loc.dtype == np.float64
    by_name = {par.name: par.numpy() for par, _, _, _ in p.parameters}
    t = next(t for t in p.tensors if t["name"] == "weights2")
    sl = slice(t["row0"], t["row0"] + t["size"])
    assert np.allclose(loc[sl], by_name["weights2_loc"].reshape(-1), rtol=1e-6)
    assert np.allclose(scale[sl], 0.3, rtol=1e-5) and np.allclose(scale[:p.layers[0]["rows"] * 16], scale[0]) and scale.min() > 0
    # other parameter values: the loc moves with them
    theta = np.zeros(p.n_params)
    for par, off, size, _ in p.parameters:
        theta[off:off + size] = par.numpy().reshape(-1) + (1.0 if par.name == "weights2_loc" else 0.0)
    assert np.allclose(bnn.row_parameters(p, theta)[0][sl], loc[sl] + 1.0)


# ---- the fixtures ------------------------------------------------------------------------------------------------------------------
def reference_present():
    from oracle import gen_golden
    return os.path.isdir(os.path.join(gen_golden.REF, "brancher"))


@pytest.mark.skipif(not reference_present(), reason="the reference is only present in the build container")
def test_the_fixtures_regenerate_bit_for_bit(tmp_path):
    env = dict(os.environ, BSVI_GOLDEN_OUT=str(tmp_path), PYTHONDONTWRITEBYTECODE="1", OMP_NUM_THREADS="1")
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_golden_bnn_predict.py")], check=True, env=env,
                   stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=600)
    for name in FIXTURES:
        new, old = np.load(os.path.join(str(tmp_path), name + ".npz")), np.load(os.path.join(GOLDEN, "bnn_predict", name + ".npz"))
        assert sorted(new.files) == sorted(old.files)
        for key in old.files:
            if key == "meta":
                assert json.loads(str(new[key])) == json.loads(str(old[key]))
            else:
                assert np.array_equal(new[key], old[key], equal_nan=True), (name, key)


@pytest.mark.parametrize("name", FIXTURES)
def test_the_fixtures_hold_what_the_device_tests_read(name):
    data = np.load(os.path.join(GOLDEN, "bnn_predict", name + ".npz"))
    meta = json.loads(str(data["meta"]))
    assert data["rows"].shape == (1, 3, 16, 1) and meta["n_ref"] == 4000 and meta["n_exact"] == 100000
    lik, n = meta["likelihood"], meta["n_shapes"]
    c = meta["kwargs"]["widths"][-1]
    assert meta["keys"][lik] == [n, 3, c, 1] and meta["keys"]["x"] == [1, 3, 16, 1] and meta["keys"]["weights1"][:2] == [n, 1]
    assert meta["keys_no_input"][lik] == [n, 8, c, 1] and meta["keys_no_input"]["x"] == [n, 8, 16, 1] and meta["keys_no_input"]["indices"] == [8]
    model = getattr(W, meta["builder"])(W.native_api(), **meta["kwargs"])
    for par, _, _, _ in bnn.lower_bnn(model, model.posterior_model).parameters:
        assert np.allclose(par.numpy().reshape(-1), data["param/" + par.name].reshape(-1), rtol=1e-6, atol=1e-7), par.name
    if lik == "k":
        p = data["p"]
        assert np.allclose(p.sum(axis=1), 1.0) if c > 1 else ((p > 0) & (p < 1)).all()
        assert (np.abs(data["ref_freq"] - p) <= 5 * np.sqrt(p * (1 - p) / meta["n_ref"])).all()       # what the tool asserted
    else:
        v = data["exact_var"]
        assert (v > data["exact_sigma"][None, :] ** 2).all() and (data["exact_m4"] > v ** 2).all()
        assert (np.abs(data["ref_mean"] - data["exact_mean"]) <= 5 * np.sqrt(v / meta["n_ref"])).all()


# ---- the likelihood's noise stream: host reference (the contract comment of csrc/philox.h) -----------------------------------------------
def predictive_counters(seed, offset, samples, rows, call=0):
    """(k0, k1, c0, c1, c2, c3) of the call that serves outputs 4 call .. 4 call + 3 of (sample, row); arrays broadcast"""
    (k0, k1), (o0, o1) = R.split64(seed), R.split64(offset)
    return (k0 ^ KEY_PREDICT, k1 ^ call, np.asarray(samples, dtype=np.uint64), np.asarray(rows, dtype=np.uint64), o0, o1)


def predictive_words(seed, offset, samples, rows, call=0):
    k0, k1, c0, c1, o0, o1 = predictive_counters(seed, offset, samples, rows, call)
    return R.philox4x32(c0, c1, o0, o1, k0, k1)


def categorical_draw(probs, u):
    """inverse CDF on the stored f32 probabilities [..., C]: partial sums in class order in single precision, the first class whose
    partial sum is >= u, the last class if none is"""
    cum = np.cumsum(np.asarray(probs, dtype=np.float32), axis=-1, dtype=np.float32)
    hit = cum >= np.asarray(u, dtype=np.float32)[..., None]
    return np.where(hit.any(axis=-1), hit.argmax(axis=-1), cum.shape[-1] - 1)


def bernoulli_draw(p, u):
    return (np.asarray(u, dtype=np.float32) < np.asarray(p, dtype=np.float32)).astype(np.float32)


def normal_noise(seed, offset, samples, rows, n_outputs, dtype=np.float64):
    """e [..., C]: output c takes normal c & 3 of the four Box-Muller normals of call c >> 2"""
    out = []
    for call in range((n_outputs + 3) // 4):
        x = predictive_words(seed, offset, samples, rows, call)
        out += list(R.box_muller(x[0], x[1], dtype)) + list(R.box_muller(x[2], x[3], dtype))
    return np.stack(out[:n_outputs], axis=-1)


def test_the_host_rules_of_the_draws():
    s, r = np.arange(20000)[:, None], np.arange(3)[None, :]
    u = R.u01(predictive_words(1234, 7, s, r)[0])
    assert u.dtype == np.float32 and u.min() > 0 and u.max() <= 1
    p = np.array([0.2, 0.5, 0.3], dtype=np.float32)
    pick = categorical_draw(np.broadcast_to(p, u.shape + (3,)), u)
    freq = np.stack([(pick == c).mean() for c in range(3)])
    assert (np.abs(freq - p) <= 5 * np.sqrt(p * (1 - p) / pick.size)).all()
    assert abs(bernoulli_draw(np.float32(0.3), u).mean() - 0.3) <= 5 * np.sqrt(0.21 / u.size)
    # u01 reaches exactly 1 and f32 probabilities may sum below it: the last class; a sum that reaches u earlier: that class
    short = np.array([0.25, 0.25, 0.49999994], dtype=np.float32)
    assert short.sum(dtype=np.float32) < 1 and categorical_draw(short, np.float32(1.0)) == 2
    assert categorical_draw(short, np.float32(0.25)) == 0 and categorical_draw(short, np.float32(0.25000003)) == 1
    assert categorical_draw(np.array([0.0, 1.0, 0.0], dtype=np.float32), np.float32(2.0 ** -25)) == 1
    e = normal_noise(99, 3, s, r, 6)
    assert e.shape == (20000, 3, 6) and abs(e.mean()) < 0.02 and abs(e.std() - 1) < 0.02
    assert np.abs(np.corrcoef(e.reshape(-1, 6).T) - np.eye(6)).max() < 0.02            # six outputs, two calls: no value used twice
    e32 = normal_noise(99, 3, s, r, 6, np.float32)
    assert np.abs(e32 - e).max() < 1e-4


def test_no_key_counter_pair_of_the_predictive_stream_is_one_of_a_training_stream():
    """over a grid of (seed, offset, sample, row, call): as tuples (k0, k1, c0, c1, c2, c3).  The training streams are those of
    oracle/philox_ref.py's contract, over the same seeds and offsets and every counter value that can coincide with a (sample, row)."""
    assert KEY_PREDICT not in (0, R.KEY_DENSE_MINIBATCH, R.KEY_AMORT_MINIBATCH, R.KEY_REDUCE_DATA)
    seeds = (0, 1234, 0x1234567890ABC, KEY_PREDICT, KEY_PREDICT ^ R.KEY_DENSE_MINIBATCH, (1 << 63) - 1)
    offsets = (0, 7, (1 << 32) - 1, 1 << 32, (1 << 62) + 3)
    samples, rows = np.arange(0, 70), np.array([0, 1, 2, 3, 31, 32, 33, 69, 0xFFFF, 0x10000, R.C1_REDUCE_DATA, 0x40000000, 0x80000000, 0x80000001])
    grid_s, grid_r = [a.reshape(-1) for a in np.meshgrid(samples, rows, indexing="ij")]

    def tuples(k0, k1, c0, c1, c2, c3):
        arrs = np.broadcast_arrays(*[np.asarray(v, dtype=np.uint64) for v in (k0, k1, c0, c1, c2, c3)])
        return set(zip(*[a.reshape(-1).tolist() for a in arrs]))

    for seed in seeds:
        (k0, k1) = R.split64(seed)
        for offset in offsets:
            o0, o1 = R.split64(offset)
            mine = set()
            for call in (0, 1, 2):
                t = tuples(*predictive_counters(seed, offset, grid_s, grid_r, call))
                assert len(t) == grid_s.size and not (t & mine)          # distinct inside the stream, also across the calls of one row
                mine |= t
            c0 = np.concatenate([grid_s, grid_r])                        # any training counter word may take any of these values
            c1 = np.concatenate([grid_r, grid_s])
            training = set()
            for key0 in (k0, k0 ^ R.KEY_DENSE_MINIBATCH, k0 ^ R.KEY_AMORT_MINIBATCH, k0 ^ R.KEY_REDUCE_DATA):
                for c1_form in (c1, c1 | R.FLAG_NORMAL, c1 | R.FLAG_DENSE, (c1 >> 2) | R.FLAG_DENSE, R.raw_counter(c1, 0), R.raw_counter(c1, 1),
                                np.full_like(c1, R.C1_REDUCE_DATA)):
                    training |= tuples(key0, k1, c0, c1_form, o0, o1)
            assert not (mine & training), (seed, offset)
    # the words themselves differ from the BNN path's weight noise at the same (seed, offset, sample, counter)
    a = predictive_words(1234, 7, grid_s, grid_r)[0]
    (k0, k1), (o0, o1) = R.split64(1234), R.split64(7)
    assert (a != R.philox4x32(grid_s, grid_r, o0, o1, k0, k1)[0]).mean() > 0.99
