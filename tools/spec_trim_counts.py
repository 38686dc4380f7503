"""Instruction counts of a kernel variant of the headline program (README AR, T = 20) with the trimmed kernels' switch off, on,
and on without each item (specialize.cpp BSVI_SPEC_TRIM; spec_prelude.h SPEC_DEBUG_NO_*): hiprtc on the host, llvm-objdump and
llvm-readelf of the ROCm toolchain on the code object — no GPU needed.  The counts are whole-kernel counts: the compiler
interleaves blocks, so counting by region is not reliable.

usage: python3 tools/spec_trim_counts.py [variant, default 6] [directory for the code objects and disassemblies]"""
import collections
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ["BSVI_SPEC_LEAN_CHAIN"] = "1"            # (variant 7, the source before the lean chain, exists only when this is set)
from brancher_amd import lowering, native, workloads as W     # noqa: E402

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")
ITEMS = ("SPEC_DEBUG_NO_SHARED_CONST", "SPEC_DEBUG_NO_ENT_NOISE", "SPEC_DEBUG_NO_FLUSH_MASK")
variant = int(sys.argv[1]) if len(sys.argv) > 1 else 6
out = sys.argv[2] if len(sys.argv) > 2 else tempfile.mkdtemp(prefix="spec_trim_")
os.makedirs(out, exist_ok=True)


def counts(src, tag):
    dump = os.path.join(out, tag + ".co")
    os.environ["BSVI_JIT_DUMP"] = dump
    native.jit_compile(src + "\n// %s\n" % tag)
    text = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", dump], capture_output=True, text=True).stdout
    with open(os.path.join(out, tag + ".s"), "w") as f:
        f.write(text)
    ops = collections.Counter(line.split()[0] for line in text.splitlines() if line.startswith("\t"))
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", dump], capture_output=True, text=True).stdout
    meta = {k: int(v) for k, v in re.findall(r"\.(vgpr_spill_count|sgpr_spill_count|vgpr_count):\s+(\d+)", notes)}
    total = lambda prefix: sum(n for op, n in ops.items() if op.startswith(prefix))
    return dict(total=sum(ops.values()), valu=total("v_"), v_cndmask=total("v_cndmask"), ds_read=total("ds_read"), s_waitcnt=ops["s_waitcnt"],
                zero_adds=len(re.findall(r"v_add_f32_e32 v\d+, 0, v\d+", text)), **meta)


model = W.build_readme_ar(W.native_api(), T=20)
program = lowering.lower(model, model.posterior_model, "pathwise")
os.environ["BSVI_SPEC_TRIM"] = "0"
off = native.specialised_source(program, variant)
os.environ["BSVI_SPEC_TRIM"] = "1"
on = native.specialised_source(program, variant)
rows = [("switch off (BSVI_SPEC_TRIM=0)", off), ("switch on", on)]
rows += [("on, " + d, "#define %s 1\n" % d + on) for d in ITEMS]
rows += [("on, every item off but the one of " + d[len("SPEC_DEBUG_NO_"):], "".join("#define %s 1\n" % e for e in ITEMS if e != d) + on) for d in ITEMS]
rows += [("on, all three items off", "".join("#define %s 1\n" % d for d in ITEMS) + on)]
print("variant %d of README AR T = 20; code objects and disassemblies in %s" % (variant, out))
for i, (name, src) in enumerate(rows):
    print("%-58s %s" % (name, counts(src, "v%d_%d" % (variant, i))))
