"""Which specialised kernel a training launch gets, and in which shape (spec_select.h): the README AR model at
the sizes where the selection changes — one and three sample waves (the single draw wave), four and five (the draw service with
the owners on a draw wave), six (no extra wave), and the first size of the many-workgroup geometry.  The numbers are what the
library reported before the selection became one function (tests/test_spec_select_cpu.py walks the whole table without a GPU)."""
import pytest

from brancher_amd import engine, native, workloads as W

pytestmark = pytest.mark.gpu

# n -> (variant of the launch, workgroups, threads per workgroup)
EXPECTED = {64: (4, 1, 128), 192: (4, 1, 256), 256: (6, 1, 512), 300: (6, 1, 512), 321: (0, 1, 384), 513: (2, 3, 256)}


def launched(n):
    c = engine.compile_model(W.build_readme_ar(W.native_api(), T=20), None, "pathwise")
    losses, finite = c.train(3, n, "SGD", lr=1e-3)
    assert bool(finite.all())
    assert c.last_mode == "persistent"
    shape = c.native.engine(n, 2)
    print("n", n, "variant", native.load().bsvi_spec_last_variant(), shape)
    assert shape["engine"] == "specialised"
    return native.load().bsvi_spec_last_variant(), shape["n_blocks"], shape["n_threads"]


@pytest.mark.parametrize("n", sorted(EXPECTED))
def test_training_launch_gets_the_variant_and_shape_of_the_table(n):
    assert launched(n) == EXPECTED[n]


def test_owners_stay_on_a_sample_wave_when_switched_off(monkeypatch):
    monkeypatch.setenv("BSVI_SPEC_OWNER_WAVE", "0")
    assert launched(256) == (4, 1, 512)
