"""Stein variational gradient descent as far as it goes without a device: the method class and its refusals, the two entry points of
include/bsvi.h as `native` binds them."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from brancher_amd import inference, native
from brancher_amd.standard_variables import NormalVariable
from brancher_amd.variables import ProbabilisticModel, RootVariable

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def particle(shape=(2, 1), extra=()):
    return ProbabilisticModel([RootVariable(np.zeros(shape), "mu", learnable=True), RootVariable(np.zeros((3, 1)), "b", learnable=True), *extra])


def test_the_class_has_the_flags_of_the_reference():
    method = inference.SteinVariationalGradientDescent()
    assert (method.learnable_model, method.needs_sampler, method.learnable_sampler) == (False, False, False)
    assert not hasattr(method, "run") and method.bandwidth is None
    assert inference.SteinVariationalGradientDescent(bandwidth=0.5).bandwidth == 0.5
    method.check_model_compatibility(None, [particle(), particle()], None)
    method.check_model_compatibility(None, [particle() for _ in range(256)], None)


@pytest.mark.parametrize("particles,message", [
    (lambda: [particle(), particle(extra=[NormalVariable(0.0, 1.0, "z")])], r"particle 1: variable 'z' is a NormalVariable"),
    (lambda: [particle(), particle(), particle((4, 1))], r"particle 2: variable 'mu' has shape .*4, 1\), particle 0 has .*2, 1\)"),
    (lambda: [particle()], r"1 particles, the method takes 2 \.\. 256"),
    (lambda: [particle() for _ in range(257)], r"257 particles, the method takes 2 \.\. 256"),
], ids=["random variable", "shapes", "one", "257"])
def test_what_is_refused_is_named(particles, message):
    with pytest.raises(ValueError, match=message):
        inference.SteinVariationalGradientDescent().check_model_compatibility(None, particles(), None)


def test_the_entries_are_declared_and_bound_with_the_types_of_the_header():
    header = open(os.path.join(ROOT, "include", "bsvi.h")).read()
    c_types = {"const float*": C.c_void_p, "float*": C.c_void_p, "void*": C.c_void_p, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64,
               "float": C.c_float, "size_t": C.c_size_t, "int": C.c_int}
    lib = native.load()
    for name in ("bsvi_svgd_workspace_bytes", "bsvi_svgd_direction"):
        result, arguments = re.search(r"^(\w+) %s\(([^)]*)\);" % name, header, re.M).groups()
        declared = [c_types[a.strip().rsplit(" ", 1)[0]] for a in arguments.replace("\n", " ").split(",")]
        assert native.EXPORTS[name] == (c_types[result], declared) and hasattr(lib, name)
    assert lib.bsvi_svgd_workspace_bytes(64, 15910) > 0
    assert lib.bsvi_svgd_workspace_bytes(257, 8) == 0 and b"2 .. 256" in lib.bsvi_last_error()
    assert lib.bsvi_svgd_direction(None, None, None, 3, 5, 5, 0.0, None, None, None) == -1 and b"null argument" in lib.bsvi_last_error()
