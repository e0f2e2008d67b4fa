"""sel.streamops.SlotTable -- the host-side bookkeeping of a stream pool (no
GPU): which slots are open, and the checks every slot list passes before it
reaches a kernel (the kernels trust the list to be distinct and in range).
Also the pool entry points' argument validation through ctypes: every call
below is refused before any device work, so the pointers are never dereferenced.
"""
import ctypes

import pytest

from sel import SelError
from sel import convops as CO
from sel import streamops as SO


def test_lowest_free_slot_is_reused_after_close():
    t = SO.SlotTable(4)
    assert [t.open() for _ in range(3)] == [0, 1, 2]
    t.close(1)
    assert len(t) == 2 and not t.is_open(1)
    assert t.open() == 1
    assert t.open() == 3
    t.close(0)
    t.close(2)
    assert t.open() == 0 and t.open() == 2


def test_full_pool_raises():
    t = SO.SlotTable(2)
    t.open()
    t.open()
    with pytest.raises(SelError, match="full"):
        t.open()
    t.close(0)
    assert t.open() == 0


def test_check_returns_the_list_in_order():
    t = SO.SlotTable(6)
    for _ in range(6):
        t.open()
    assert t.check([4, 1, 5]) == [4, 1, 5]
    assert t.check([]) == []
    assert t.check(range(5, -1, -1)) == [5, 4, 3, 2, 1, 0]


def test_duplicate_ids_are_rejected():
    t = SO.SlotTable(4)
    for _ in range(4):
        t.open()
    with pytest.raises(SelError, match="duplicate"):
        t.check([2, 0, 2])


def test_closed_ids_are_rejected():
    t = SO.SlotTable(4)
    for _ in range(3):
        t.open()
    t.close(1)
    with pytest.raises(SelError, match="not open"):
        t.check([0, 1])
    with pytest.raises(SelError, match="not open"):
        t.check([3])              # never opened
    with pytest.raises(SelError, match="not open"):
        t.close(1)                # closing twice
    assert t.check([0, 2]) == [0, 2]


def test_out_of_range_ids_are_rejected():
    t = SO.SlotTable(3)
    for _ in range(3):
        t.open()
    for bad in ([3], [-1], [0, 7], [4], [1.5]):   # 3 would be the template row of a pool of 3
        with pytest.raises(SelError, match="out of range"):
            t.check(bad)


def test_over_long_lists_are_rejected():
    t = SO.SlotTable(2)
    t.open()
    t.open()
    with pytest.raises(SelError, match="holds 2"):
        t.check([0, 1, 0])


def test_check_takes_one_shot_iterators():
    """check() reads its argument once: a generator gets every check a list gets."""
    t = SO.SlotTable(3)
    t.open()
    t.open()
    assert t.check(iter([1, 0])) == [1, 0]
    assert t.check(s for s in (0,)) == [0]
    with pytest.raises(SelError, match="not open"):
        t.check(iter([0, 2]))
    with pytest.raises(SelError, match="out of range"):
        t.check(s for s in (0, 3))
    with pytest.raises(SelError, match="duplicate"):
        t.check(iter([1, 1]))


def test_capacity_must_be_positive():
    with pytest.raises(ValueError):
        SO.SlotTable(0)


def test_pool_entry_points_validate_before_device_work():
    from sel import _lib
    from sel import hfgops as HF
    lib = _lib.load()
    p = lambda v: ctypes.c_void_p(v)  # noqa: E731  (never dereferenced: every call below is refused first)
    inp, wp, out, ca, co, sl, na = (p(0x10000 * i) for i in range(1, 8))

    def step(d, carry=ca, carry_out=co, nslots=7, slots=sl, n=na, dt=(CO.F32, CO.F32), o=out):
        rc = lib.sel_conv_step_pool(ctypes.byref(d), dt[0], dt[1], carry, carry_out, nslots, slots, n, inp, wp, None,
                                    None, o, None)
        return rc, lib.sel_last_error().decode()

    def hstep(d, carry=ca, carry_out=co, nslots=7, slots=sl, n=na, dt=(CO.F32, CO.F32), o=out):
        rc = lib.sel_hfg_conv_step_pool(ctypes.byref(d), dt[0], dt[1], carry, carry_out, nslots, slots, n, inp, wp,
                                        None, None, o, None)
        return rc, lib.sel_last_error().decode()

    good = CO.ConvDesc(12, 4, 8, 8, 7, 1, 6, CO.PAD_ZERO, 0, 0)
    hgood = HF.make_desc(12, 4, 8, 8, 7, 1, 6)
    for call, d, name in ((step, good, "sel_conv_step_pool"), (hstep, hgood, "sel_hfg_conv_step_pool")):
        for kw, says in ((dict(slots=None), "null slots"), (dict(n=None), "null slots"), (dict(nslots=0), "nslots"),
                         (dict(nslots=-3), "nslots"), (dict(carry_out=ca), "alias"), (dict(o=ca), "alias"),
                         (dict(o=inp), "aliases in"), (dict(carry=None), "needs carry"),
                         (dict(dt=(CO.F32, CO.BF16)), "dtypes"), (dict(dt=(7, 7)), "dtypes")):
            rc, msg = call(d, **kw)
            assert rc == -1 and says in msg and name in msg, (name, kw, rc, msg)
        rc, msg = call(d.with_(pad=5) if hasattr(d, "with_") else HF.make_desc(12, 4, 8, 8, 7, 1, 5))
        assert rc == -1 and "(K-1)*dil" in msg, (rc, msg)

    job = (SO.CopyJob * 1)(SO.CopyJob(0x10000, 0x20000, 16))
    jp = ctypes.cast(job, ctypes.c_void_p)
    assert lib.sel_stream_copy_slots(None, 0, 7, sl, sl, 6, na, None) == -1
    assert lib.sel_stream_copy_slots(jp, 1, 7, None, sl, 6, na, None) == -1
    assert lib.sel_stream_copy_slots(jp, 1, 7, sl, None, 6, na, None) == -1
    assert lib.sel_stream_copy_slots(jp, 1, 7, sl, sl, 6, None, None) == -1
    assert lib.sel_stream_copy_slots(jp, 1, 0, sl, sl, 6, na, None) == -1
    assert lib.sel_stream_copy_slots(jp, 1, 7, sl, sl, 0, na, None) == -1
    bad = (SO.CopyJob * 1)(SO.CopyJob(0x10000, 0x20000, 0))
    assert lib.sel_stream_copy_slots(ctypes.cast(bad, ctypes.c_void_p), 1, 7, sl, sl, 6, na, None) == -1
