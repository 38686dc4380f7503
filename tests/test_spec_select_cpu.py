"""The selection of the specialised kernels (brancher_amd/csrc/spec_select.h: host only, no HIP, no environment) against its
decision table: tests/c_abi/spec_select_table.cpp holds the rows — sizes, noise rows, geometries, switches, failed kernels,
exchange, gather — and is compiled here from the header alone, with the address and undefined-behaviour sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_selection_reproduces_the_decision_table(tmp_path):
    exe = tmp_path / "spec_select_table"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "brancher_amd", "csrc"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "c_abi", "spec_select_table.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
