"""The posterior predictive of the dense-link path without a device (csrc/dense_predict.inc): what `CompiledDense.predict`,
`predict_particles`, `SteinVariationalGradientDescent.predict` and the library's entry points refuse in front of any device work, each by
the name of its limit."""
import numpy as np
import pytest
import torch

from brancher_amd import dense, inference, native, workloads as W


def engine(**kw):      # a CompiledDense as far as the checks in front of the device look: the lowered program, no handle
    model = W.build_logistic_regression(W.native_api(), dataset_size=8, batch_size=4, n_features=5, n_classes=3, **kw)
    compiled = object.__new__(dense.CompiledDense)
    compiled.program, compiled.device = dense.lower_dense(model, model.posterior_model), torch.device("cpu")
    return compiled


@pytest.mark.parametrize("call,message", [
    (lambda e: e.predict(np.zeros((2, 6)), 4), r"the rows have 6 features, the model was built on 5"),
    (lambda e: e.predict(np.zeros((2, 5)), 0), r"number_samples must be at least 1"),
    (lambda e: e.predict(np.zeros((2, 5)), 4, noise=np.zeros((15, 3))), r"noise must be \[15, 4\]: got \(15, 3\)"),
    (lambda e: e.predict(np.zeros((2, 5)), 4, noise={"weights": np.zeros((4, 1, 3, 4))}), r"noise must be \[15, 4\]: got \(12, 4\)"),
    (lambda e: e.predict_particles(torch.zeros(2, 14), np.zeros((2, 5))), r"the table has 14 columns, a weight set of this model has 3 x 5 = 15 values"),
])
def test_what_a_prediction_does_not_take_is_named(call, message):
    with pytest.raises(ValueError, match=message):
        call(engine())


def test_the_particles_of_a_bayesian_neural_network_are_refused_by_name():
    models = [W.build_bnn_regression(W.native_api(), dataset_size=16, batch_size=16, n_features=64, n_hidden=4, point="all") for _ in range(2)]
    with pytest.raises(ValueError, match=r"the predictive of the particles of a Bayesian neural network, or of another model, is not served"):
        inference.SteinVariationalGradientDescent(batched=True).predict(models[0], [m.posterior_model for m in models], np.zeros((2, 64)))


def test_the_entries_exist_and_refuse_by_name():
    lib = native.load()
    assert lib.bsvi_dense_predict_args_size() == native.C.sizeof(native.DensePredictArgs) and lib.bsvi_abi_version() == 11
    args = native.DensePredictArgs(n_sets=0, n_rows=3)
    assert lib.bsvi_dense_predict(None, None) == -1 and b"null argument" in lib.bsvi_last_error()
    assert lib.bsvi_dense_predict(None, native.C.byref(args)) == -1 and b"null handle" in lib.bsvi_last_error()
    assert lib.bsvi_dense_predict_workspace_bytes(None, 4, 3, 0) == 0 and b"null handle" in lib.bsvi_last_error()
