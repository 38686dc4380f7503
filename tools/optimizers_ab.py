"""bench.py's headline measurement (BASELINE config 1) under another optimizer, for a tree given by --root: the workload table of
that tree's bench.py gets the optimizer and its options, everything else — warm-up, spin-up, timing, the JSON line — is bench.py's
own.  Used for profiles/r12/optimizers_ab.txt (parent against candidate under Adam; the new kinds beside Adam).

    python tools/optimizers_ab.py --root . --optimizer RMSprop --lr 1e-3 -- --gpus 1 --steps 20000 --warmup 5
"""
import argparse
import os
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--optimizer", default="Adam")
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("rest", nargs=argparse.REMAINDER, help="-- followed by bench.py's own arguments")
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    os.chdir(root)
    sys.path.insert(0, root)
    import bench
    builder, kwargs, n, _, _, desc = bench.WORKLOADS["cfg1"]
    bench.WORKLOADS["cfg1"] = (builder, kwargs, n, args.optimizer, dict(lr=args.lr), "%s [optimizer: %s lr=%g]" % (desc, args.optimizer, args.lr))
    sys.argv = [os.path.join(root, "bench.py")] + [a for a in args.rest if a != "--"]
    bench.main()


if __name__ == "__main__":
    main()
