"""Instruction counts of a kernel variant of the headline program (README AR, T = 20) with the grouped table (spec_prelude.h
SPEC_QUADS) and without it (SPEC_DEBUG_NO_QUADS), and of the owners' loop compiled for one optimizer (spec_main.h
SPEC_OPT_LITERAL 0, 1, 2): hiprtc on the host, llvm-objdump and llvm-readelf of the ROCm toolchain on the code object — no GPU
needed.  Whole-kernel counts, and the counts between the kernel's barriers in the order of the code (the longest stretch with
LDS reads of the table is the sample waves' body and flush).

usage: python3 tools/spec_quads_counts.py [variant, default 6] [directory for the code objects and disassemblies]"""
import collections
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from brancher_amd import lowering, native, workloads as W     # noqa: E402

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")
variant = int(sys.argv[1]) if len(sys.argv) > 1 else 6
out = sys.argv[2] if len(sys.argv) > 2 else tempfile.mkdtemp(prefix="spec_quads_")
os.makedirs(out, exist_ok=True)


def counts(src, tag):
    dump = os.path.join(out, tag + ".co")
    os.environ["BSVI_JIT_DUMP"] = dump
    native.jit_compile(src + "\n// %s\n" % tag)
    text = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", dump], capture_output=True, text=True).stdout
    with open(os.path.join(out, tag + ".s"), "w") as f:
        f.write(text)
    stretches, ops = [collections.Counter()], collections.Counter()
    for line in text.splitlines():
        if not line.startswith("\t"):
            continue
        op = line.split()[0]
        ops[op] += 1
        stretches[-1][op] += 1
        if op == "s_barrier":
            stretches.append(collections.Counter())
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", dump], capture_output=True, text=True).stdout
    meta = {k: int(v) for k, v in re.findall(r"\.(vgpr_spill_count|vgpr_count|sgpr_count|group_segment_fixed_size):\s+(\d+)", notes)}
    total = lambda c, prefix: sum(n for op, n in c.items() if op.startswith(prefix))
    row = dict(total=sum(ops.values()), valu=total(ops, "v_"), ds_read=total(ops, "ds_read"), ds_read_b128=ops["ds_read_b128"],
               ds_read2_b32=ops["ds_read2_b32"], s_waitcnt=ops["s_waitcnt"], v_div_scale_f32=ops["v_div_scale_f32"],
               f64=sum(n for op, n in ops.items() if op.endswith("_f64")), s_cbranch=total(ops, "s_cbranch"), **meta)
    return row, [(sum(c.values()), total(c, "ds_read"), c["s_waitcnt"]) for c in stretches]


model = W.build_readme_ar(W.native_api(), T=20)
src = native.specialised_source(lowering.lower(model, model.posterior_model, "pathwise"), variant)
print("variant %d of README AR T = 20; groups: %s" % (variant, (re.findall(r"#define SPEC_Q_GROUPS (\d+)", src) or ["none"])[0]))
for tag, defines in (("no_quads", "#define SPEC_DEBUG_NO_QUADS 1\n"), ("default", ""), ("literal_1", "#define SPEC_OPT_LITERAL 1\n"),
                     ("literal_2", "#define SPEC_OPT_LITERAL 2\n"), ("no_quads_literal_1", "#define SPEC_DEBUG_NO_QUADS 1\n#define SPEC_OPT_LITERAL 1\n")):
    row, stretches = counts(defines + src, tag)
    print("%-20s %s" % (tag, row))
    print("%-20s between barriers (instructions, ds_read*, s_waitcnt): %s" % ("", stretches))
