"""Which launches an iteration of the dense-link path makes, with which grids, LDS and derived arguments, and the layout of its workspace
(brancher_amd/csrc/dense_select.h: host only, no HIP, no environment) against its table: tests/c_abi/dense_select_table.cpp holds the
rows that tests/test_gpu_dense_fused.py runs on the device, both sides of every threshold, a sweep of the plan's invariants and every
switch flipped once — compiled here from the header alone, with the address and undefined-behaviour sanitizers."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "brancher_amd", "csrc")
KNOBS = ["BSVI_DENSE_XGEMM", "BSVI_DENSE_FUSED", "BSVI_DENSE_FOLD", "BSVI_XF_NS", "BSVI_XF_DEBUG", "BSVI_XB_DEBUG", "BSVI_XB_RB", "BSVI_XB_GROUPS"]


@pytest.fixture(scope="module")
def table_output(tmp_path_factory):
    exe = tmp_path_factory.mktemp("dense_select") / "dense_select_table"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", CSRC, "-o", str(exe), os.path.join(ROOT, "tests", "c_abi", "dense_select_table.cpp")])
    return subprocess.run([str(exe)], capture_output=True, text=True)


def test_plan_reproduces_the_table(table_output):
    assert table_output.returncode == 0, table_output.stdout + table_output.stderr
    assert "\n0 failures" in table_output.stdout


def test_the_device_test_runs_the_rows_of_the_table(table_output):
    import test_gpu_dense_fused
    rows = [tuple(l.split()[1:]) for l in table_output.stdout.splitlines() if l.startswith("device-row ")]
    mine = [tuple(str(v) for v in shape) + (",".join("%s=%s" % kv for kv in sorted(env.items())) or "-", call) + tuple(names)
            for shape, env, call, names in test_gpu_dense_fused.DENSE_PLAN_ROWS]
    assert rows == mine
    reached = {name for r in rows for name in r[7:]}
    assert len(rows) == 11 and {"dense_xfwd<0,1>", "dense_xfwd<0,2>", "dense_xbwd<0,2,7>", "dense_xbwd<0,4,7>", "dense_xbwd<0,4,9>", "dense_xbwd<0,4,9,noise>",
                                "xgemm_nt<logits>", "dense_ce", "xgemm_nt<grad>", "dense_xreduce", "dense_wsplit", "dense_head", "dense_prologue", "dense_gather",
                                "dense_noise", "dense_forward<4>", "dense_forward<16>", "dense_backward", "dense_rows", "dense_rows<sliced>", "dense_sample_sums",
                                "dense_epilogue", "dense_param_kernel", "dense_param_fold_kernel"} <= reached


def test_the_environment_is_read_in_one_place():
    header = open(os.path.join(CSRC, "dense_select.h")).read()
    assert "getenv" not in header and "#include <hip" not in header and '#include "hip' not in header
    lines = open(os.path.join(CSRC, "dense_kernel.inc")).read().splitlines()
    first = next(i for i, l in enumerate(lines) if l.startswith("static dsel::Switches dense_read_switches() {"))
    last = next(i for i in range(first, len(lines)) if lines[i] == "}")
    named = set()
    for i, l in enumerate(lines):
        for knob in re.findall(r"BSVI_[A-Z0-9_]+", l):
            if knob in KNOBS:
                assert first <= i <= last, "line %d names %s" % (i + 1, knob)
                named.add(knob)
        assert "getenv" not in l or first <= i <= last, "line %d reads the environment" % (i + 1)
    assert named == set(KNOBS)
