"""`SteinVariationalGradientDescent(batched=True)` without a device: what is refused and by which name, and the two new entry points."""
import numpy as np
import pytest

from brancher_amd import bnn, inference, native, workloads as W
from brancher_amd.standard_variables import NormalVariable
from brancher_amd.variables import ProbabilisticModel, RootVariable


def lowered(**kw):
    model = W.build_bnn_regression(W.native_api(), dataset_size=16, batch_size=16, n_features=64, n_hidden=4, prior_loc=0.1, **kw)
    return bnn.lower_bnn(model, model.posterior_model)


@pytest.mark.parametrize("kw,n,message", [
    (dict(), 3, r"not every row is a point row: weights1, b1, weights2, b2 has a Normal posterior"),
    (dict(point="all", learnable_sigma=True), 3, r"a learnable sigma is not served"),
    (dict(point="all", scale_head="softplus"), 3, r"a scale head is not served"),
    (dict(scale_latent="global"), 3, r"scale latents \(tau\) are not served"),
    (dict(point="all"), 1, r"1 particles, served are 2 \.\. 256"),
    (dict(point="all"), 257, r"257 particles, served are 2 \.\. 256"),
])
def test_what_the_particle_kernels_do_not_serve_is_named(kw, n, message):
    with pytest.raises(ValueError, match=message):
        bnn.check_particles(lowered(**kw), n)
    bnn.check_particles(lowered(point="all"), 2)


def test_a_model_of_another_path_is_refused_with_the_path():
    obs = NormalVariable(NormalVariable(0.0, 2.0, "mu"), 1.0, "y")
    model = ProbabilisticModel([obs])
    obs.observe(np.array([0.3, -0.8, 1.9], dtype=np.float32).reshape(-1, 1))
    parts = [ProbabilisticModel([RootVariable(np.full((1, 1), v), "mu", learnable=True)]) for v in (0.0, 1.0)]
    with pytest.raises(ValueError, match=r"batched=True\): the model is served by the scalar path \(CompiledELBO\)"):
        inference.SteinVariationalGradientDescent(batched=True).check_model_compatibility(model, parts, None)


def test_the_default_is_unchanged_and_the_entries_exist():
    assert not inference.SteinVariationalGradientDescent().batched and hasattr(inference.SteinVariationalGradientDescent(batched=True), "run")
    lib = native.load()
    assert hasattr(lib, "bsvi_bnn_particles_fwd_bwd") and hasattr(lib, "bsvi_bnn_particles_workspace_bytes") and lib.bsvi_abi_version() == 11
    for n in (1, 257):
        assert lib.bsvi_bnn_particles_workspace_bytes(None, n) == 0 and b"served are 2 .. 256" in lib.bsvi_last_error()
    assert lib.bsvi_bnn_particles_workspace_bytes(None, 2) == 0 and b"null handle" in lib.bsvi_last_error()
    assert lib.bsvi_bnn_particles_fwd_bwd(None, None, None, None, None, 257, 8, None) == -1 and b"2 .. 256" in lib.bsvi_last_error()
