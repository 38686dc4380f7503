"""The text the LIBRARY writes for its two generated Bayesian-neural-network kernels ($BSVI_BNN_SOURCE_DUMP) has the digests of
tests/golden/bnn_source/digests.json, for four of the cases tests/test_bnn_source_cpu.py runs through the header alone — so the
description bnn_kernel.inc fills (bnn_source_net) is the one that test hands over."""
import pytest

from test_bnn_source_cpu import DIGESTS, dump

pytestmark = pytest.mark.gpu


def test_the_library_dumps_the_recorded_text():
    wanted = {"16-6-3 classifier": "mid", "16-5-1 B512 (pairs)": "mid", "16-5-3 learnable sigma cauchy": "upper", "16-5-4-3 head exp laplace": "upper"}
    got = dump.library_digests(wanted)
    for name, kind in wanted.items():
        assert got[name][kind] == DIGESTS[name][kind], (name, kind)
