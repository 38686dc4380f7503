"""SHA-256 of the generated source of every kernel variant (bsvi_program_source, host only) for programs WITHOUT minibatch
sources: README AR T=20 and T=200 (Pathwise and BlackBox), beta_binomial, and a program with a two-entry parameter — and of
every variant with the gather phase (bsvi_program_source_minibatch) for the linear regression of tests/test_minibatch_loop_cpu.py.
Run once per library build and compare the two outputs: a change that must leave these programs' kernels alone leaves every line
alone.

usage: python3 tools/spec_source_digests.py [path of another libbsvi.so]"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ["BSVI_SPEC_LEAN_CHAIN"] = "1"            # (variant 7, the source before the lean chain, exists only when this is set)
from brancher_amd import lowering, native, workloads as W     # noqa: E402

if len(sys.argv) > 1:
    # another build's library: it may lack entry points this binding knows (only the two source functions are used here)
    import ctypes
    import torch  # noqa: F401  (the HIP runtime the library binds to, as native.load() does)
    native.LIB_PATH = sys.argv[1]
    other = ctypes.CDLL(native.LIB_PATH)
    for name in [n for n in native.EXPORTS if not hasattr(other, n)]:
        del native.EXPORTS[name]
from test_spec_chain_cpu import two_entry_program             # noqa: E402

api = W.native_api()
programs = []
for T in (20, 200):
    for estimator in ("pathwise", "blackbox"):
        model = W.build_readme_ar(api, T=T)
        programs.append(("readme_ar T=%d %s" % (T, estimator), lowering.lower(model, model.posterior_model, estimator)))
model = W.build_beta_binomial(api)
programs.append(("beta_binomial pathwise", lowering.lower(model, model.posterior_model, "pathwise")))
programs.append(("two-entry parameter (readme_ar T=20)", two_entry_program()))
model = W.build_minibatch_linear_regression(api, dataset_size=40, batch_size=8, n_features=3)
minibatched = lowering.lower(model, model.posterior_model, "pathwise")
for name, program in programs + [("minibatch linreg 40/8/3, gather phase", minibatched)]:
    for variant in range(8):
        if program is minibatched:
            src = native.specialised_source_minibatch(program, variant) if "bsvi_program_source_minibatch" in native.EXPORTS else None
        else:
            src = native.specialised_source(program, variant)
        print("%-40s variant %d  %s  %d bytes" % (name, variant, hashlib.sha256((src or "").encode()).hexdigest(), len(src or "")))
