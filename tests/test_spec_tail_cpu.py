"""Host side of the tail of the lean chain (spec_main.h SPEC_LEAN_TAIL; specialize.cpp): what
the generator emits for variant 6 with and without BSVI_SPEC_TAIL=0, and that every kernel variant still compiles for gfx950
— no GPU needed.  What the kernels compute is compared bit for bit with the previous form on the GPU
(tests/test_gpu_spec_tail.py)."""
import os
import re
import subprocess

import pytest

from conftest import Golden, golden_cases
from brancher_amd import lowering, native, workloads as W
from test_spec_chain_cpu import two_entry_program

SCALAR = [c for c in golden_cases() if not c.startswith("logreg") and not c.startswith("bnn")]
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
TAIL = "#define SPEC_LEAN_TAIL 1\n"


def headline(estimator="pathwise", T=20):
    model = W.build_readme_ar(W.native_api(), T=T)
    return lowering.lower(model, model.posterior_model, estimator)


def body(src):
    return src.split("void spec_body")[1]


def metadata(src, tmp_path, monkeypatch, tag):
    dump = str(tmp_path / ("%s.co" % tag))
    monkeypatch.setenv("BSVI_JIT_DUMP", dump)
    assert native.jit_compile(src + "\n// (unique: not served from the code cache) %s\n" % tag) > 0
    notes = subprocess.run([READELF, "--notes", dump], capture_output=True, text=True).stdout
    return {k: int(v) for k, v in re.findall(r"\.(private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count|vgpr_count|sgpr_count):\s+(\d+)", notes)}


def test_switch_regenerates_variant_6_as_it_was(monkeypatch):
    """BSVI_SPEC_TAIL=0, read when the program is created: variant 6 is the lean-chain prefix in front of variant 0's source,
    which is how it was generated before; by default it carries SPEC_LEAN_TAIL, and only variant 6 does.  The entropy
    constant as a table column (SPEC_UE) was measured and dropped: no variant reads one."""
    program = headline()
    monkeypatch.setenv("BSVI_SPEC_LEAN_CHAIN", "1")
    new = {v: native.specialised_source(program, v) for v in range(8)}
    monkeypatch.setenv("BSVI_SPEC_TAIL", "0")
    old = {v: native.specialised_source(program, v) for v in range(8)}
    prefix = "#define SPEC_WITH_DRAW_WAVE 1\n#define SPEC_WITH_DRAW_OWNERS 1\n#define SPEC_LEAN_CHAIN 1\n"
    assert old[6] == prefix + old[0]
    for v in range(8):
        assert "SPEC_LEAN_TAIL" not in old[v] and "SPEC_UE(" not in old[v] and "SPEC_ENT_COLUMN" not in old[v]
        assert "SPEC_UE(" not in new[v] and "SPEC_ENT_COLUMN" not in new[v]
        if v != 6:
            assert new[v] == old[v], v
            assert "SPEC_LEAN_TAIL" not in new[v]
    assert new[6] == prefix + TAIL + new[0]
    assert body(new[6]) == body(old[6])
    # variant 7, the source before the lean chain, sets none of it
    assert "SPEC_LEAN" not in new[7] and new[7] != ""


def test_body_keeps_its_sinks_and_positions(monkeypatch):
    program = headline()
    src = native.specialised_source(program, 6)
    assert TAIL in src
    assert src.count("spec_naff_sink(") == 41
    assert sorted(int(m) for m in re.findall(r"SPEC_DU\((\d+)u,", src)) == list(range(program.n_uniform_grad))
    # the body as it was (BSVI_SPEC_LEAN_BODY=0), whatever the variant
    monkeypatch.setenv("BSVI_SPEC_LEAN_BODY", "0")
    monkeypatch.setenv("BSVI_SPEC_LEAN_CHAIN", "1")
    was = native.specialised_source(program, 6)
    assert "SPEC_UE(" not in was and "SPEC_U(43)" in was
    assert body(was) == body(native.specialised_source(program, 7))


@pytest.mark.parametrize("estimator", ["pathwise", "blackbox"])
def test_every_variant_of_the_headline_compiles_with_the_new_defaults(estimator, tmp_path, monkeypatch):
    assert os.path.exists(READELF), "llvm-readelf of the ROCm toolchain reads the code objects' metadata"
    monkeypatch.setenv("BSVI_SPEC_LEAN_CHAIN", "1")
    program = headline(estimator)
    for variant in range(8):
        src = native.specialised_source(program, variant)
        assert src is not None, native.load().bsvi_last_error()
        meta = metadata(src, tmp_path, monkeypatch, "t%d" % variant)
        print(estimator, variant, meta)
        if estimator == "pathwise" or variant not in (1, 3):
            assert meta["vgpr_spill_count"] == 0 and meta["private_segment_fixed_size"] == 0, (variant, meta)


@pytest.mark.parametrize("case", SCALAR)
def test_scalar_cases_compile_with_the_new_defaults(case):
    model = Golden(case).build()
    program = lowering.lower(model, model.posterior_model, "pathwise")
    for variant in (2, 4, 6):
        src = native.specialised_source(program, variant)
        assert src is not None, native.load().bsvi_last_error()
        assert (TAIL in src) == (variant == 6)
        assert native.jit_compile(src) > 0


def test_two_entry_parameter_keeps_the_old_epilogue():
    """SPEC_OWN_ENTRIES 2: SPEC_LEAN_OWNERS is 0, and the tail's arrangements are compiled for the lean owners only — the
    header refuses to compile (SPEC_TAIL_MUST_BE_OFF) where one of them is on"""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "brancher_amd", "csrc")
    main = open(os.path.join(csrc, "spec_main.h")).read()
    for name, off in (("SPEC_DEFER_BOOK", "SPEC_DEBUG_NO_DEFER_BOOK"), ("SPEC_PLAIN_SGD", "SPEC_DEBUG_NO_PLAIN_SGD")):
        assert "#if SPEC_LEAN_OWNERS && defined(SPEC_LEAN_TAIL) && !defined(%s)\n#define %s 1" % (off, name) in main
    src = native.specialised_source(two_entry_program(), 6)
    assert src is not None, native.load().bsvi_last_error()
    assert "#define SPEC_OWN_ENTRIES 2\n" in src and TAIL in src
    check = "#define SPEC_TAIL_MUST_BE_OFF 1\n"
    assert native.jit_compile(check + src) > 0
    # (the check does fire: the headline's one-entry program has the arrangements on, and off again under the old switch)
    one = native.specialised_source(headline(), 6)
    with pytest.raises(native.NativeError):
        native.jit_compile(check + one)
    assert native.jit_compile(check + "#define SPEC_DEBUG_NO_LEAN_CHAIN 1\n" + one) > 0
