"""Host side of the trimmed specialised kernels (specialize.cpp BSVI_SPEC_TRIM; spec_prelude.h SPEC_TRIM): repeated constant
entries of the uniform table read once (SPEC_SAME), no zero-add in the reverse step of an entropy-only node (SPEC_ENT_NOISE),
idle lanes masked in the flush of the transpose tile instead of in every store (SPEC_FLUSH_MASK).  What the generator emits with
the switch off and on, and what the compiler makes of variant 6 of the headline program — no GPU needed.  What the kernels compute
is compared bit for bit with the switch off on the GPU (tests/test_gpu_spec_trim.py).

tests/golden/spec_trim_parent_sources.json holds SHA-256 and length of the eight variants' sources of four programs as the
library generated them before this switch existed (tools/spec_source_digests.py prints the same digests)."""
import collections
import copy
import hashlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

from brancher_amd import lowering, native, workloads as W
from test_spec_chain_cpu import two_entry_program

HERE = os.path.dirname(os.path.abspath(__file__))
LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")
ITEMS = ("SPEC_DEBUG_NO_SHARED_CONST", "SPEC_DEBUG_NO_ENT_NOISE", "SPEC_DEBUG_NO_FLUSH_MASK")


def lower(model):
    return lowering.lower(model, model.posterior_model, "pathwise")


def headline(T=20):
    return lower(W.build_readme_ar(W.native_api(), T=T))


def programs():
    api = W.native_api()
    return {"readme_ar_T20": headline(20), "readme_ar_T200": headline(200),
            "beta_binomial": lower(W.build_beta_binomial(api)), "two_entry": two_entry_program()}


def body(src):
    return src.split("void spec_body")[1]


def test_switch_off_generates_every_source_as_it_was(monkeypatch):
    """BSVI_SPEC_TRIM=0, read when the program is created: all eight variants of four programs, byte for byte"""
    with open(os.path.join(HERE, "golden", "spec_trim_parent_sources.json")) as f:
        parent = json.load(f)
    monkeypatch.setenv("BSVI_SPEC_LEAN_CHAIN", "1")      # (variant 7, the source before the lean chain, exists only when this is set)
    monkeypatch.setenv("BSVI_SPEC_TRIM", "0")
    made = programs()
    assert sorted(made) == sorted(parent)
    for name, program in made.items():
        for variant in range(8):
            src = native.specialised_source(program, variant) or ""
            was = parent[name][variant]
            assert len(src) == was["bytes"] and hashlib.sha256(src.encode()).hexdigest() == was["sha256"], (name, variant)
            assert "SPEC_TRIM" not in src and "SPEC_SAME(" not in src and "SPEC_ENT_NOISE(" not in src


def test_switch_on_marks_every_variant(monkeypatch):
    """by default every variant of a program carries SPEC_TRIM, the twenty likelihood terms of the headline read one entry, and
    the 21 sampled nodes' scale gradients are one fused multiply-add; the positions and the sinks are what they were"""
    monkeypatch.setenv("BSVI_SPEC_LEAN_CHAIN", "1")
    program = headline()
    uniform = program.uniform
    noise = [k for k in range(len(uniform)) if not uniform["is_param"][k] and uniform["transform"][k] == 1]
    assert noise == list(range(45, 65))                   # measure_noise, once per likelihood term
    for variant in range(8):
        src = native.specialised_source(program, variant)
        assert "#define SPEC_TRIM 1\n" in src, variant
        for k in noise[1:]:
            assert "SPEC_UR(SPEC_SAME(%d, 45))" % k in src and "SPEC_UL(SPEC_SAME(%d, 45))" % k in src
            assert "SPEC_UR(%d)" % k not in src and "SPEC_UL(%d)" % k not in src
        assert "SPEC_UR(45)" in src and "SPEC_SAME(45," not in src
        assert body(src).count("SPEC_ENT_NOISE(gs, ") == 21
        assert src.count("spec_naff_sink(") == 41
        assert sorted(int(m) for m in re.findall(r"SPEC_DU\((\d+)u,", src)) == list(range(program.n_uniform_grad))
    # parameters and observations are never shared, whatever their values
    src = native.specialised_source(program, 0)
    for a, b in re.findall(r"SPEC_SAME\((\d+), (\d+)\)", src):
        assert int(b) < int(a) < len(uniform) and not uniform["is_param"][int(a)] and not uniform["is_param"][int(b)]


def test_constants_that_differ_keep_their_entries():
    """same value bits, same transform, same a and b — anything else is another constant"""
    base = headline()

    def source_of(change):
        program = copy.copy(base)
        program.uniform = np.array(base.uniform, copy=True)
        program.consts = np.array(base.consts, dtype=np.float32, copy=True)
        change(program)
        return native.specialised_source(program, 0)

    def value(p): p.consts[p.uniform["src"][50]] += 0.25
    def minus_zero(p):
        p.consts[p.uniform["src"][45:65]] = 0.0
        p.consts[p.uniform["src"][50]] = -0.0
    def transform(p): p.uniform["transform"][50] = 3
    def shift(p): p.uniform["a"][50] = 0.5
    def factor(p): p.uniform["b"][50] = 2.0

    assert "SPEC_UR(SPEC_SAME(50, 45))" in native.specialised_source(base, 0)
    for change in (value, minus_zero, transform, shift, factor):
        src = source_of(change)
        assert "SPEC_UR(50)" in src and "SPEC_UL(50)" in src and "SPEC_SAME(50," not in src, change.__name__
        assert "SPEC_UR(SPEC_SAME(51, 45))" in src and "SPEC_UR(SPEC_SAME(49, 45))" in src, change.__name__

    def all_apart(p):
        for i, k in enumerate(range(45, 65)):
            p.consts[p.uniform["src"][k]] += 0.01 * i
    assert "SPEC_SAME(" not in source_of(all_apart)


def code_object(src, tmp_path, monkeypatch, tag):
    """(opcode counts, metadata) of a generated translation unit compiled for gfx950"""
    dump = str(tmp_path / ("%s.co" % tag))
    monkeypatch.setenv("BSVI_JIT_DUMP", dump)
    assert native.jit_compile(src + "\n// (unique: not served from the code cache) %s\n" % tag) > 0
    text = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", dump], capture_output=True, text=True).stdout
    ops = collections.Counter(line.split()[0] for line in text.splitlines() if line.startswith("\t"))
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", dump], capture_output=True, text=True).stdout
    meta = {k: int(v) for k, v in re.findall(r"\.(private_segment_fixed_size|vgpr_spill_count|vgpr_count):\s+(\d+)", notes)}
    count = lambda prefix: sum(n for op, n in ops.items() if op.startswith(prefix))
    return dict(total=sum(ops.values()), cndmask=count("v_cndmask"), ds_read=count("ds_read"), valu=count("v_")), meta


def test_headline_loop_kernel_is_shorter_and_spills_nothing(tmp_path, monkeypatch):
    """variant 6 of README AR T = 20, the kernel bench.py measures: no spilled vector register, at most the 228 registers it
    had, and fewer selects, fewer LDS reads and fewer instructions altogether than the same source generated with the switch off"""
    assert os.path.exists(os.path.join(LLVM, "llvm-objdump")), "llvm-objdump of the ROCm toolchain disassembles the code objects"
    program = headline()
    on_src = native.specialised_source(program, 6)
    monkeypatch.setenv("BSVI_SPEC_TRIM", "0")
    off_src = native.specialised_source(program, 6)
    monkeypatch.delenv("BSVI_SPEC_TRIM")
    assert "#define SPEC_TRIM 1\n" in on_src and "SPEC_TRIM" not in off_src
    on, on_meta = code_object(on_src, tmp_path, monkeypatch, "on")
    off, off_meta = code_object(off_src, tmp_path, monkeypatch, "off")
    print("switch off:", off, off_meta)
    print("switch on: ", on, on_meta)
    assert on_meta["vgpr_spill_count"] == 0 and on_meta["private_segment_fixed_size"] == 0, on_meta
    assert on_meta["vgpr_count"] <= 228, on_meta
    assert on["cndmask"] < off["cndmask"], (on, off)
    assert on["ds_read"] < off["ds_read"], (on, off)
    assert on["total"] < off["total"], (on, off)
    # the three items switched off one by one in the trimmed source give the untrimmed kernel's counts back
    none, none_meta = code_object("".join("#define %s 1\n" % d for d in ITEMS) + on_src, tmp_path, monkeypatch, "none")
    print("all three items off:", none, none_meta)
    assert none == off and none_meta == off_meta


@pytest.mark.parametrize("variant", [0, 2, 7])
def test_other_variants_compile_trimmed(variant, tmp_path, monkeypatch):
    """the step kernel, the many-workgroup kernel (the flush takes each chunk's count) and the owners' wave as it was"""
    monkeypatch.setenv("BSVI_SPEC_LEAN_CHAIN", "1")
    src = native.specialised_source(headline(), variant)
    assert "#define SPEC_TRIM 1\n" in src
    counts, meta = code_object(src, tmp_path, monkeypatch, "v%d" % variant)
    print(variant, counts, meta)
    assert meta["vgpr_spill_count"] == 0 and meta["private_segment_fixed_size"] == 0, meta
