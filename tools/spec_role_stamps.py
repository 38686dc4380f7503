"""Per-ROLE time stamps of one iteration of the specialised kernel's training loop (diagnostic build: BSVI_SPEC_DEFINES adds
SPEC_DEBUG_STAMPS; every wave's lane 0 writes its stamps into the loss curve at 16 + 8 * wave).  Cycles of s_memtime after the
wave leaves the iteration's first barrier (the barrier releases all waves together): at the second barrier, past it, the
owners' sums read (owners only), their new table published (lean chain: what follows is the loss bookkeeping), the
iteration's work done, past the next first barrier; and, counted from the kernel's entry, the launch's first barrier
passed (prologue and first draws).  Roles at the draw service's five
sample waves: 0-4 sample waves (the owners on wave 1 with BSVI_SPEC_OWNER_WAVE=0), 5-7 draw waves (the owners on wave 5
by default).  B = first barrier -> second (bodies, sums, draws beside them), E = second -> next first (epilogue).

usage: python3 tools/spec_role_stamps.py [n_samples] [optimizer] [define ...]"""
import os
import sys
import time

# (further arguments are defines for the diagnostic build, e.g. SPEC_DEBUG_NO_LEAN_CHAIN: the lean body with the previous epilogue;
#  SPEC_DEBUG_NO_DEFER_BOOK, SPEC_DEBUG_NO_PLAIN_SGD: the tail of the lean chain without one item;
#  BSVI_SPEC_TAIL=0 in the environment: without all of them)
os.environ["BSVI_SPEC_DEFINES"] = "\n".join(["#define SPEC_DEBUG_STAMPS 1"] + ["#define %s 1" % d for d in sys.argv[3:]])
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                        # noqa: E402
from brancher_amd import engine, workloads as W     # noqa: E402

n_samples = int(sys.argv[1]) if len(sys.argv) > 1 else 300
optimizer = sys.argv[2] if len(sys.argv) > 2 else "SGD"
kw = dict(lr=1e-3) if optimizer == "SGD" else dict(lr=1e-2)
api = W.native_api()
c = engine.compile_model(W.build_readme_ar(api, T=20), None, "pathwise")
n_it = 20000
print("BSVI_SPEC_OWNER_WAVE=%s BSVI_SPEC_LEAN_CHAIN=%s BSVI_SPEC_LEAN_BODY=%s BSVI_SPEC_TAIL=%s, %d samples, %s"
      % (os.environ.get("BSVI_SPEC_OWNER_WAVE", "1"), os.environ.get("BSVI_SPEC_LEAN_CHAIN", "1"),
         os.environ.get("BSVI_SPEC_LEAN_BODY", "1"), os.environ.get("BSVI_SPEC_TAIL", "1"), n_samples, optimizer)
      + "".join(" " + d for d in sys.argv[3:]))
for rep in range(3):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    losses, _ = c.train(n_it, n_samples, optimizer, seed=0, **kw)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    s = losses[:16 + 8 * 8].cpu().numpy()
    rows = []
    for w in range(8):
        r = s[16 + 8 * w: 16 + 8 * w + 8]
        if r[0] != 1.0:
            continue
        at2, past2, sums, done, next1, table = r[1:7]
        rows.append("  wave %d: B %6d | E work %6d (sums read %6s, table published %6s) | wait %6d | iteration %6d | first barrier %6d from entry"
                    % (w, at2, done - past2, "%d" % (sums - past2) if 0 < sums < 1e8 else "-",
                       "%d" % (table - past2) if 0 < table < 1e8 else "-", next1 - done, next1, r[7]))
    print("wall %.3f us/it" % (wall * 1e6 / n_it))
    print("\n".join(rows))
