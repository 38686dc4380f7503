"""The predictive of a particle ensemble of a Bayesian neural network without a device (csrc/bnn_ensemble.inc): the pure size function
(tests/c_abi/bnn_ensemble_plan.cpp), what `CompiledBnn.predict_particles` and `SteinVariationalGradientDescent.predict_network` refuse in
front of any device work, each by the name of its limit, and the library's entry points."""
import os
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT
from brancher_amd import bnn, dense, inference, native, workloads as W
from brancher_amd.variables import ProbabilisticModel, RootVariable


def test_the_size_function(tmp_path):
    exe = tmp_path / "bnn_ensemble_plan"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "brancher_amd", "csrc"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "c_abi", "bnn_ensemble_plan.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and "bnn_ensemble_plan: ok" in out.stdout, out.stdout + out.stderr


def engine(widths=(64, 4, 3), **kw):      # a CompiledBnn as far as the checks in front of the device look: the lowered program, no handle
    model = W.build_bayesian_neural_network(W.native_api(), dataset_size=16, batch_size=16, widths=list(widths), **dict(dict(point="all"), **kw))
    compiled = object.__new__(bnn.CompiledBnn)
    compiled.program, compiled.device = bnn.lower_bnn(model, model.posterior_model), torch.device("cpu")
    return compiled


@pytest.mark.parametrize("kw,call,message", [
    ({}, lambda e: e.predict_particles(torch.zeros(2, 274), np.zeros((2, 64))), r"the table has 274 columns, a weight set of this model has 275 values"),
    ({}, lambda e: e.predict_particles(torch.zeros(2, 276), np.zeros((2, 68))), r"the rows have 68 features, the model was built on 64"),
    ({}, lambda e: e.predict_particles(torch.zeros(1, 276), np.zeros((2, 64))), r"1 particles, served are 2 \.\. 256"),
    (dict(point=("b1",)), lambda e: e.predict_particles(torch.zeros(2, 276), np.zeros((2, 64))), r"not every row is a point row"),
    (dict(widths=(64, bnn.MAX_ENSEMBLE_WIDTH + 1, 3)), lambda e: e.predict_particles(torch.zeros(2, 21832), np.zeros((2, 64))),
     r"a layer of 321 units, served are layers of up to 320"),
])
def test_what_the_ensemble_does_not_take_is_named(kw, call, message):
    with pytest.raises(ValueError, match=message):
        call(engine(**kw))


def test_a_model_the_bnn_path_does_not_lower_is_refused_with_the_path():
    model = W.build_logistic_regression(W.native_api(), dataset_size=8, batch_size=4, n_features=5, n_classes=3)
    name = dense.lower_dense(model, model.posterior_model).latent_name
    particles = [ProbabilisticModel([RootVariable(np.zeros((3, 5)), name, learnable=True)]) for _ in range(2)]
    with pytest.raises(ValueError, match=r"predict_network serves the particles of a Bayesian neural network \(the BNN path, CompiledBnn\)"):
        inference.SteinVariationalGradientDescent().predict_network(model, particles, np.zeros((2, 5)))


def test_the_entries_exist_and_refuse_by_name():
    lib, C = native.load(), native.C
    assert lib.bsvi_bnn_predict_particles_args_size() == C.sizeof(native.BnnPredictParticlesArgs) and lib.bsvi_abi_version() == 11
    one = C.c_void_p(256)                     # (never dereferenced: every check below returns first)
    args = native.BnnPredictParticlesArgs(theta_dev=one, ld=8, x_dev=one, n_particles=4, n_rows=3, workspace_dev=one)
    assert lib.bsvi_bnn_predict_particles(None, None) == -1 and b"bsvi_bnn_predict_particles: null argument" in lib.bsvi_last_error()
    assert lib.bsvi_bnn_predict_particles(None, C.byref(args)) == -1 and b"bsvi_bnn_predict_particles: null handle" in lib.bsvi_last_error()
    assert lib.bsvi_bnn_predict_particles_workspace_bytes(None, 4, 3) == 0 and b"null handle" in lib.bsvi_last_error()
    args.struct_size -= 8
    assert lib.bsvi_bnn_predict_particles(None, C.byref(args)) == -1 and b"bsvi_bnn_predict_particles_args::struct_size" in lib.bsvi_last_error()
