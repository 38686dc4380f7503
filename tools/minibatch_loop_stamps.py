"""Per-role time stamps (tools/spec_role_stamps.py) of the in-kernel loop of the MINIBATCHED linear regression, with the gather
phase and with it compiled out (SPEC_DEBUG_NO_GATHER): where the phase's cycles go.  B = first barrier -> second (bodies; the
gathering wave's index walk and loads), E = second -> next first (the owners' epilogue; the gathering wave's LDS stores).

usage: python3 tools/minibatch_loop_stamps.py [n_samples]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                        # noqa: E402
from brancher_amd import engine, native, workloads as W     # noqa: E402

n_samples = int(sys.argv[1]) if len(sys.argv) > 1 else 300
n_it = 20000
for defines in (["SPEC_DEBUG_STAMPS", "SPEC_DEBUG_NO_GATHER"], ["SPEC_DEBUG_STAMPS"]):
    os.environ["BSVI_SPEC_DEFINES"] = "\n".join("#define %s 1" % d for d in defines)
    c = engine.compile_model(W.build_minibatch_linear_regression(W.native_api()), None, "pathwise")
    print("%d samples, SGD, defines: %s" % (n_samples, " ".join(defines)))
    for rep in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        losses, _ = c.train(n_it, n_samples, "SGD", seed=0, lr=1e-3, minibatch_loop=True)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        assert c.last_mode == "persistent"
        s = losses[:16 + 8 * 8].cpu().numpy()
        print("wall %.3f us/it, kernel variant %d" % (wall * 1e6 / n_it, native.load().bsvi_spec_last_variant()))
        if rep < 2:
            continue
        for w in range(8):
            r = s[16 + 8 * w: 16 + 8 * w + 8]
            if r[0] != 1.0:
                continue
            at2, past2, sums, done, next1, table = r[1:7]
            print("  wave %d: B %6d | E work %6d (sums read %6s, table published %6s) | wait %6d | iteration %6d"
                  % (w, at2, done - past2, "%d" % (sums - past2) if 0 < sums < 1e8 else "-",
                     "%d" % (table - past2) if 0 < table < 1e8 else "-", next1 - done, next1))
