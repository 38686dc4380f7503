"""The worst err / bound per (form, launch sequence, estimator) of tests/test_gpu_dense_models.py, from the "dense-models ..." lines that
its cases print before they assert (`pytest -m gpu -s tests/test_gpu_dense_models.py > log`; `python tools/dense_models_summary.py log`):
the table of profiles/r22/dense_models.txt."""
import collections
import re
import sys

LINE = re.compile(r"dense-models (\S+) (\S+) (\S+) (.*?)\s*(\S+)\s+err (\S+)\s+oracle32 (\S+)\s+scale (\S+)\s+err/bound (\S+)")


def main(path):
    worst = collections.OrderedDict()
    for line in open(path):
        m = LINE.search(line)
        if not m:
            continue
        form, seq, est, case, tensor = m.group(1, 2, 3, 4, 5)
        err, yard, scale, ratio = (float(v) for v in m.group(6, 7, 8, 9))
        key = (form, seq, est)
        if key not in worst or ratio > worst[key][0]:
            worst[key] = (ratio, case, tensor, err, yard, scale)
    print("%-28s %-12s %-9s %9s  %-28s %-16s %10s %10s %10s" % ("form", "sequence", "estimator", "err/bound", "case", "tensor", "err", "oracle32", "scale"))
    for (form, seq, est), (ratio, case, tensor, err, yard, scale) in worst.items():
        print("%-28s %-12s %-9s %9.3g  %-28s %-16s %10.3g %10.3g %10.3g" % (form, seq, est, ratio, case, tensor, err, yard, scale))


if __name__ == "__main__":
    main(sys.argv[1])
