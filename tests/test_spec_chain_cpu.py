"""Host side of the lean chain of the specialised training loop (spec_main.h SPEC_LEAN_CHAIN / SPEC_OWN_ENTRIES, the folded
literal constants of specialize.cpp): what the generator emits and that every kernel variant it feeds still compiles for
gfx950 — no GPU needed.  What the kernels compute is compared bit for bit with the previous arrangement on the GPU
(tests/test_gpu_spec_chain.py).

Not here: a body under the lanes' mask with plain tile stores.  It was built twice and measured slower than the select per
position it removes — slowest sample wave 6 340 cycles with the selects, 6 684 with spec_body under `if (T.active)`, 8 000 with
the idle lanes' stores redirected to the padding of the tile's rows (profiles/r7/role_stamps.txt) — so SPEC_DU keeps its
`T.active ? (val) : 0.0f`."""
import copy
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import Golden, golden_cases
from brancher_amd import lowering, native, workloads as W

SCALAR = [c for c in golden_cases() if not c.startswith("logreg") and not c.startswith("bnn")]
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "brancher_amd", "csrc")


def headline(estimator="pathwise", T=20):
    model = W.build_readme_ar(W.native_api(), T=T)
    return lowering.lower(model, model.posterior_model, estimator)


def metadata(src, tmp_path, monkeypatch, tag):
    dump = str(tmp_path / ("%s.co" % tag))
    monkeypatch.setenv("BSVI_JIT_DUMP", dump)
    assert native.jit_compile(src + "\n// (unique: not served from the code cache) %s\n" % tag) > 0
    notes = subprocess.run([READELF, "--notes", dump], capture_output=True, text=True).stdout
    return {k: int(v) for k, v in re.findall(r"\.(private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count|vgpr_count|sgpr_count):\s+(\d+)", notes)}


@pytest.mark.parametrize("case", SCALAR)
def test_loop_variants_compile_for_gfx950(case):
    """tests/test_specialize_cpu.py compiles variants 0 and 1 of every scalar workload (the main loop with the folded
    constants and SPEC_OWN_ENTRIES); here the one-workgroup loop kernels with roles of their own: 4 (draw wave)
    and 6 (the owners on a draw wave, lean chain), and 2, the many-workgroup geometry with the folded constants.  Variants 3, 5
    and 7 are compiled for the headline program only (below)."""
    model = Golden(case).build()
    program = lowering.lower(model, model.posterior_model, "pathwise")
    for variant in (2, 4, 6):
        src = native.specialised_source(program, variant)
        assert src is not None, native.load().bsvi_last_error()
        assert "#define SPEC_OWN_ENTRIES" in src
        assert ("#define SPEC_LEAN_CHAIN 1" in src) == (variant == 6)
        assert native.jit_compile(src) > 0


@pytest.mark.parametrize("estimator", ["pathwise", "blackbox"])
def test_every_variant_of_the_headline_compiles_without_spilled_vector_registers(estimator, tmp_path, monkeypatch):
    """all eight variants (0 / 1 lean / diagnostic, 2 / 3 many workgroups, 4 draw wave, 5 exchange, 6 owners' wave with the
    lean chain, 7 the owners' wave as it was) of the README AR model, T = 20 — the headline program under Pathwise; no spilled
    vector register, no scratch"""
    assert os.path.exists(READELF), "llvm-readelf of the ROCm toolchain reads the code objects' metadata"
    monkeypatch.setenv("BSVI_SPEC_LEAN_CHAIN", "1")        # (set at creation: the previous source, variant 7, is generated too)
    program = headline(estimator)
    for variant in range(8):
        src = native.specialised_source(program, variant)
        assert src is not None, native.load().bsvi_last_error()
        meta = metadata(src, tmp_path, monkeypatch, "v%d" % variant)
        print(estimator, variant, meta)
        # (the diagnostic kernels of the BlackBox estimator, which no training loop runs, spilled before this as they do now)
        if estimator == "pathwise" or variant not in (1, 3):
            assert meta["vgpr_spill_count"] == 0 and meta["private_segment_fixed_size"] == 0, (variant, meta)
    # (the owners' wave keeps the epilogue's argument words in scalar registers across the second barrier: no more of them
    #  spill than in the kernel as it was — and that kernel is the library's previous source, text for text)
    lean = metadata(native.specialised_source(program, 6), tmp_path, monkeypatch, "lean")
    prev = metadata(native.specialised_source(program, 7), tmp_path, monkeypatch, "prev")
    assert lean["sgpr_spill_count"] <= prev["sgpr_spill_count"], (lean, prev)
    assert lean["vgpr_count"] <= prev["vgpr_count"], (lean, prev)


def test_headline_source_is_lean(monkeypatch):
    """the generated body reads no literal constant from the uniform table and the owners' code is compiled for one entry
    per parameter"""
    program = headline()
    assert native.specialised_source(program, 7) == ""     # (nobody pays for the comparison source unasked)
    monkeypatch.setenv("BSVI_SPEC_LEAN_CHAIN", "1")
    consts = np.asarray(program.consts, dtype=np.float32)
    assert list(consts[:2]) == [1.0, 0.0]
    k_one = [k for k in range(len(program.uniform)) if not program.uniform["is_param"][k] and program.uniform["src"][k] == 0]
    k_zero = [k for k in range(len(program.uniform)) if not program.uniform["is_param"][k] and program.uniform["src"][k] == 1]
    assert k_one == [43] and k_zero == [44]
    for variant in (0, 6):
        lean = native.specialised_source(program, variant)
        assert "SPEC_U(43)" not in lean and "SPEC_U(44)" not in lean
        assert "#define SPEC_OWN_ENTRIES 1\n" in lean
        assert lean.count("spec_naff_sink(") == 41
        assert sorted(int(m) for m in re.findall(r"SPEC_DU\((\d+)u,", lean)) == list(range(program.n_uniform_grad))
    assert "#define SPEC_LEAN_CHAIN 1\n" in native.specialised_source(program, 6)
    # the previous arrangement stays available (BSVI_SPEC_LEAN_CHAIN=0 launches it): the table reads, no new define
    prev = native.specialised_source(program, 7)
    assert "SPEC_U(43)" in prev and "SPEC_U(44)" in prev and "SPEC_LEAN" not in prev and "SPEC_OWN_ENTRIES" not in prev
    # the folded forms keep the rounding points of the products they replace (specialize.cpp, Emitter::affine)
    body = native.specialised_source(program, 0).split("void spec_body")[1]
    assert body.count("__builtin_fmaf(") > 0 and body.count("spec_plus(") > 0 and "asm" not in body
    # the many-workgroup geometry folds the same
    many = native.specialised_source(program, 2)
    assert "#define SPEC_ACCUMULATE_CHUNKS 1" in many and "SPEC_U(43)" not in many


def test_lean_body_switch(monkeypatch):
    """BSVI_SPEC_LEAN_BODY=0 (read when the program is created): the body as it was, in every variant"""
    program = headline()
    monkeypatch.setenv("BSVI_SPEC_LEAN_BODY", "0")
    monkeypatch.setenv("BSVI_SPEC_LEAN_CHAIN", "1")
    src = native.specialised_source(program, 6)
    assert "SPEC_U(43)" in src and "#define SPEC_LEAN_CHAIN 1\n" in src
    body = lambda s: s.split("void spec_body")[1]
    assert body(src) == body(native.specialised_source(program, 7))


def two_entry_program():
    """the headline's program with uniform entry 1 re-sourced to the parameter of entry 0: that parameter owns two entries
    (no builder of workloads.py makes one today)"""
    program = copy.copy(headline())
    uniform = np.array(program.uniform, copy=True)
    n_up = program.n_uniform_grad
    assert uniform["src"][0] != uniform["src"][1]
    uniform["src"][1] = uniform["src"][0]
    src = uniform["src"][:n_up].astype(np.int64)
    ptr = np.zeros(program.n_params + 1, dtype=np.uint32)
    np.add.at(ptr, src + 1, 1)
    program.uniform = uniform
    program.param_uniform_ptr = np.cumsum(ptr).astype(np.uint32)
    program.param_uniform_idx = np.argsort(src, kind="stable").astype(np.uint32)
    assert int(np.diff(program.param_uniform_ptr).max()) == 2
    return program


def test_two_entry_parameter_keeps_the_two_entry_code():
    """SPEC_OWN_ENTRIES 2: the owners' loops run over two entries and the owners' wave keeps the epilogue as it was (the lean one
    is compiled for one entry per parameter only)"""
    main = open(os.path.join(CSRC, "spec_main.h")).read()
    assert "!defined(SPEC_DEBUG_NO_LEAN_CHAIN) && SPEC_OWN_ENTRIES == 1\n#define SPEC_LEAN_OWNERS 1" in main
    program = two_entry_program()
    for variant in (0, 6):
        src = native.specialised_source(program, variant)
        assert src is not None, native.load().bsvi_last_error()
        assert "#define SPEC_OWN_ENTRIES 2\n" in src and "#define SPEC_GENERIC_OWNERS 0\n" in src
        assert native.jit_compile(src) > 0


def test_only_literal_one_and_zero_of_identity_const_entries_fold():
    """a const entry of 0.5, and a const entry with a transform, a shift or a factor, keep their table reads"""
    base = headline()
    assert "SPEC_U(43)" not in native.specialised_source(base, 0)

    def variant_of(change):
        program = copy.copy(base)
        program.uniform = np.array(base.uniform, copy=True)
        program.consts = np.array(base.consts, dtype=np.float32, copy=True)
        change(program)
        return native.specialised_source(program, 0)

    def half(p): p.consts[0] = 0.5
    def minus_zero(p): p.consts[1] = -0.0
    def softplus(p): p.uniform["transform"][43] = 1
    def shifted(p): p.uniform["a"][44] = 1.0
    def scaled(p): p.uniform["b"][43] = 2.0

    src = variant_of(half)
    assert "SPEC_U(43)" in src                                   # (x * 0.5 is read from the table; its + 0.0f may still go)
    src = variant_of(minus_zero)
    assert "SPEC_U(44)" in src and "SPEC_U(43)" not in src      # (x + -0.0f is not x + 0.0f for x = 0.0f ... only +0.0f folds)
    src = variant_of(softplus)
    assert "SPEC_U(43)" in src
    src = variant_of(shifted)
    assert "SPEC_U(44)" in src and "SPEC_U(43)" not in src
    src = variant_of(scaled)
    assert "SPEC_U(43)" in src
