"""Which kernel serves a product of the amortised path, its grid and its derived arguments (brancher_amd/csrc/amort_select.h: host only,
no HIP, no environment) against its table: tests/c_abi/amort_select_table.cpp holds the rows that tests/test_gpu_amortized.py runs on
the device, both sides of every threshold, a sweep of the plans' invariants, every switch flipped once and the rule of the fused
likelihood — compiled here from the header alone, with the address and undefined-behaviour sanitizers."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "brancher_amd", "csrc")
KNOBS = ["BSVI_NARROW_GEN", "BSVI_SKINNY_ROWS", "BSVI_GEMM_HALF_BELOW", "BSVI_GEMM_PF", "BSVI_X6_V", "BSVI_X6_VAR", "BSVI_X6_DEBUG",
         "BSVI_XGEMM_TALL", "BSVI_XGEMM_GLDS", "BSVI_X6TN_SLOTS", "BSVI_X6_MODES", "BSVI_X6_NN_ONLY", "BSVI_X6_TN", "BSVI_X6_TN_DATA",
         "BSVI_AMORT_FUSE_LIK"]


@pytest.fixture(scope="module")
def table_output(tmp_path_factory):
    exe = tmp_path_factory.mktemp("amort_select") / "amort_select_table"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", CSRC, "-o", str(exe), os.path.join(ROOT, "tests", "c_abi", "amort_select_table.cpp")])
    return subprocess.run([str(exe)], capture_output=True, text=True)


def test_selection_reproduces_the_table(table_output):
    assert table_output.returncode == 0, table_output.stdout + table_output.stderr
    assert "\n0 failures" in table_output.stdout


def test_the_device_test_runs_the_rows_of_the_table(table_output):
    import test_gpu_amortized
    rows = [tuple(l.split()[1:]) for l in table_output.stdout.splitlines() if l.startswith("device-row ")]
    assert rows == [tuple(str(v) for v in r) for r in test_gpu_amortized.AMORT_KIND_ROWS]
    kinds = {r[-1] for r in rows}
    assert len(rows) >= 22 and {"outer<4>", "outer<8>", "skinny_tn", "rowdot<2>", "rowdot<4>", "rowdot<8>", "skinny_n", "skinny_k4nt<1>",
                                "skinny_k4nt<3>", "skinny_k4nt<8>", "skinny_k4", "skinny_k", "gemm<tn,64,2>", "gemm<nt,64,2>", "gemm<nt,128,2>",
                                "gemm<nn,64,2>", "gemm<nn,128,2>", "x6<nt,var1>", "x6<nn,var1>", "x6_r5<nt>", "x6_r5<nn>", "xgemm_glds<128>"} <= kinds


def test_the_environment_is_read_in_one_place():
    header = open(os.path.join(CSRC, "amort_select.h")).read()
    assert "getenv" not in header and "#include <hip" not in header
    lines = open(os.path.join(CSRC, "amort_kernel.hip")).read().splitlines()
    first = next(i for i, l in enumerate(lines) if "process_switches() {" in l)
    last = next(i for i, l in enumerate(lines) if i > first and l.startswith("static sel::Switches read_switches()"))
    last = next(i for i in range(last, len(lines)) if lines[i] == "}")
    for i, l in enumerate(lines):
        for knob in re.findall(r'"(BSVI_[A-Z0-9_]+)"', l):
            assert (knob in KNOBS) == (first <= i <= last), "line %d names %s" % (i + 1, knob)
    named = {k for l in lines[first:last + 1] for k in re.findall(r'"(BSVI_[A-Z0-9_]+)"', l)}
    assert named == set(KNOBS)
