"""The conv stack's host-side decisions against the recorded table (no GPU):
which kernel family and variant sel_conv_fwd launches for a shape
(sel_conv_fwd_kernel_id), and which kernel the discriminator layers take
(sel_dconv_kernel), under the default and every documented tune setting.  The
table (tests/golden/conv_dispatch.npz) is the library's own recorded answers
from before the decision was gathered into one function."""
import numpy as np
import pytest

import conv_dispatch_cases as C
from conftest import golden


@pytest.fixture(scope="module")
def lib():
    from sel import _lib as L
    return L.load()


@pytest.fixture(scope="module")
def table():
    return golden("conv_dispatch")


def test_case_table_is_the_recorded_one(table):
    cases = C.conv_cases()
    assert np.array_equal(np.array(cases, dtype=np.int64), table["cases"])
    # the shipped generator at the bench batches, the thresholds, both ELU forms
    assert len(cases) > 2000
    assert {f"k{k}_v{v}" for k, v in C.tune_settings()} | {"cases", "dconv"} == set(table)


def test_forward_kernel_ids_match_the_recorded_table(lib, table):
    ids = C.forward_ids(lib)
    cases = C.conv_cases()
    for name, got in ids.items():
        want = table[name]
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (name, [(cases[i // 4], "bf16 f32".split()[i // 2 % 2], i % 2, int(got[i]), int(want[i]))
                                      for i in bad[:5]])
    # the table exercises every family the decision knows
    default = table["k0_v0"]
    for lo, hi in ((-1, -1), (1, 899999999), (900000000, 909999999), (910000000, 919999999),
                   (930000000, 939999999), (940000000, 999999999), (1000000000, 1499999999),
                   (1500000000, 2147483647)):
        assert ((default >= lo) & (default <= hi)).any(), (lo, hi)
    assert ((table["k38_v1"] >= 920000000) & (table["k38_v1"] <= 929999999)).any()


def test_discriminator_kernels_match_the_recorded_table(lib, table):
    assert C.dconv_kernels(lib) == [str(s) for s in table["dconv"]]
