"""The local reparameterisation estimator of the dense-link path without a device (csrc/dense_local.inc): the estimator class, which
lowerings accept and refuse it, the two entry points of the library, and the pure plan function (tests/c_abi/dense_local_plan.cpp)."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT
from brancher_amd import amortized, bnn, dense, gradient_estimators as ge, lowering, native, workloads as W


def test_the_estimator_class():
    assert issubclass(ge.LocalReparameterizationEstimator, ge._Fused) and ge.LocalReparameterizationEstimator.kernel_name == "local"
    assert lowering.EST["local"] == lowering.EST["pathwise"] == 0      # a Pathwise handle: no new enum value


def test_lowerings_accept_and_refuse():
    api = W.native_api()
    for model in (W.build_logistic_regression(api, n_features=12, n_classes=3), W.build_binary_logistic_regression(api)):
        program = dense.lower_dense(model, model.posterior_model, "local")
        assert program.estimator == "local" and not program.point_estimate
        for lower in (lowering.lower, bnn.lower_bnn, amortized.lower_amortized):
            with pytest.raises(lowering.LoweringError, match="local"):
                lower(model, model.posterior_model, "local")
    point = W.build_map_logistic_regression(api)
    with pytest.raises(lowering.LoweringError, match="point estimate: use Pathwise or MAP"):
        dense.lower_dense(point, point.posterior_model, "local")
    with pytest.raises(lowering.LoweringError, match="unknown gradient estimator 'nope'"):
        lowering.lower(point, point.posterior_model, "nope")


def test_the_entry_points():
    header = open(os.path.join(ROOT, "include", "bsvi.h")).read()
    lib = native.load()
    assert re.search(r"size_t bsvi_dense_local_workspace_bytes\(const bsvi_dense\* d, uint32_t n_samples\);", header)
    assert re.search(r"int bsvi_dense_local_fwd_bwd\(const bsvi_dense\* d, const bsvi_dense_local_args\* args\);", header)
    assert native.EXPORTS["bsvi_dense_local_workspace_bytes"] == (ctypes.c_size_t, [ctypes.c_void_p, ctypes.c_uint32])
    assert native.EXPORTS["bsvi_dense_local_fwd_bwd"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(native.DenseLocalArgs)])
    # the struct of the binding is the struct of the header: member for member, in order
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct bsvi_dense_local_args \{(.*?)\} bsvi_dense_local_args;", header, re.S).group(1), flags=re.S)
    members = [m.strip().split()[-1].lstrip("*") for decl in body.split(";") for m in decl.split(",") if m.strip()]
    assert members == [name for name, _ in native.DenseLocalArgs._fields_]
    # null arguments and a struct of another revision, each by name
    assert lib.bsvi_dense_local_fwd_bwd(None, None) == -1 and b"null argument" in lib.bsvi_last_error()
    args = native.DenseLocalArgs(n_samples=8)
    assert lib.bsvi_dense_local_fwd_bwd(None, ctypes.byref(args)) == -1 and b"null handle" in lib.bsvi_last_error()
    args.struct_size -= 8
    assert lib.bsvi_dense_local_fwd_bwd(None, ctypes.byref(args)) == -1 and b"bsvi_dense_local_args::struct_size" in lib.bsvi_last_error()


def test_the_plan_function(tmp_path):
    exe = tmp_path / "dense_local_plan"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "brancher_amd", "csrc"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "c_abi", "dense_local_plan.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and "dense_local_plan: ok" in out.stdout, out.stdout + out.stderr
    # every shape tests/test_gpu_dense_local_branches.py runs is one whose plan (tiles, chunks and rounds, tier, splits at 256 and at 32
    # CUs) the program pinned: a change of local_plan that moves a case off the branch its comment names fails above, without a device
    import test_gpu_dense_local_branches as branches
    pinned = {tuple(int(v) for v in line.split()[2:]) for line in out.stdout.splitlines() if line.startswith("named shape ")}
    run = {s[:4] for s in branches.SHAPES.values()} | {branches.SHARED, branches.DRAWN, branches.DRAWN_BERNOULLI, branches.TRAJECTORY}
    assert len(pinned) == 10 and run == pinned, (sorted(run), sorted(pinned))
