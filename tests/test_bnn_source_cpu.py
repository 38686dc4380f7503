"""The text of the two generated Bayesian-neural-network kernels (brancher_amd/csrc/bnn_source.h: host only, no HIP, no environment)
against tests/golden/bnn_source/digests.json — what the emitters inside bnn_kernel.inc wrote before that header existed, recorded on a
device from that commit's library (tools/bnn_source_dump.py).  Every case is lowered on the CPU and handed to
tests/c_abi/bnn_source_text.cpp, compiled here from the header alone with the address and undefined-behaviour sanitizers; the digest of
what it prints (lines stripped, empty lines dropped) must be the recorded one, for bnn_upper_gen and for bnn_mid_gen.
tests/test_gpu_bnn_source.py shows that the library hands the header the same description."""
import importlib.util
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("bnn_source_dump", os.path.join(ROOT, "tools", "bnn_source_dump.py"))
dump = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(dump)
DIGESTS = json.load(open(os.path.join(ROOT, "tests", "golden", "bnn_source", "digests.json")))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("bnn_source") / "bnn_source_text"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "brancher_amd", "csrc"), "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "c_abi", "bnn_source_text.cpp")])
    return str(exe)


def test_the_recorded_digests_cover_every_case_and_both_kernels():
    assert sorted(DIGESTS) == sorted(dump.CASES)
    for name, kinds in DIGESTS.items():
        assert sorted(kinds) == sorted(dump.KINDS), name


@pytest.mark.parametrize("name", sorted(dump.CASES))
def test_the_header_writes_the_recorded_text(program, name):
    from brancher_amd import bnn, workloads as W
    kw, env = dump.CASES[name]
    model = dump.build(W, kw)
    args = dump.describe(bnn.lower_bnn(model, model.posterior_model, "pathwise"), env)
    for kind in dump.KINDS:
        run = subprocess.run([program, kind] + args, capture_output=True, text=True)
        assert run.returncode == 0, run.stderr
        assert dump.digest(run.stdout) == DIGESTS[name][kind], (name, kind)
