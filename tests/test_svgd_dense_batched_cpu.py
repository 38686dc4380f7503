"""`SteinVariationalGradientDescent(batched=True)` on a logistic regression without a device: what `dense.check_particles` refuses and by
which name, the two entry points of csrc/dense_particles.inc and their refusals."""
import numpy as np
import pytest

from brancher_amd import dense, inference, native, workloads as W
from brancher_amd.variables import ProbabilisticModel, RootVariable


def lowered(point=True, **kw):
    api = W.native_api()
    model = W.build_map_logistic_regression(api, dataset_size=8, **kw) if point else W.build_logistic_regression(api, dataset_size=8, batch_size=8, **kw)
    return dense.lower_dense(model, model.posterior_model)


@pytest.mark.parametrize("point,kw,n,message", [
    (False, dict(n_features=4, n_classes=3), 3, r"weights has a Normal posterior \(a particle is a model of one learnable RootVariable"),
    (True, dict(n_features=4, n_classes=33), 3, r"33 classes, served are 1 \.\. 32"),
    (True, dict(n_features=4, n_classes=3), 1, r"1 particles, served are 2 \.\. 256"),
    (True, dict(n_features=4, n_classes=3), 257, r"257 particles, served are 2 \.\. 256"),
    (True, dict(n_features=1025, n_classes=3), 3, r"1025 features, served are 1 \.\. 1024"),
])
def test_what_the_particle_kernel_does_not_serve_is_named(point, kw, n, message):
    with pytest.raises(ValueError, match=message):
        dense.check_particles(lowered(point, **kw), n)
    dense.check_particles(lowered(n_features=4, n_classes=3), 2)


def test_the_entries_exist_and_refuse_by_name():
    lib = native.load()
    assert hasattr(lib, "bsvi_dense_particles_fwd_bwd") and hasattr(lib, "bsvi_dense_particles_workspace_bytes") and lib.bsvi_abi_version() == 11
    for n in (1, 257):
        assert lib.bsvi_dense_particles_workspace_bytes(None, n) == 0 and b"served are 2 .. 256" in lib.bsvi_last_error()
        assert lib.bsvi_dense_particles_fwd_bwd(None, None, None, None, None, n, 8, None) == -1 and b"served are 2 .. 256" in lib.bsvi_last_error()
    assert lib.bsvi_dense_particles_workspace_bytes(None, 2) == 0 and b"null handle" in lib.bsvi_last_error()
    assert lib.bsvi_dense_particles_fwd_bwd(None, None, None, None, None, 2, 8, None) == -1 and b"null handle" in lib.bsvi_last_error()


def test_a_logistic_regression_is_accepted_with_a_list_of_particles():
    model = W.build_map_logistic_regression(W.native_api())
    parts = [ProbabilisticModel([RootVariable(np.full((3, 4), v), "weights", learnable=True)]) for v in (0.0, 1.0)]
    method = inference.SteinVariationalGradientDescent(batched=True)
    method.check_model_compatibility(model, parts, None)
    assert isinstance(method._program, dense.DenseProgram) and method._program.point_estimate
