"""sel_conv_step_pool and sel_stream_copy_slots (csrc/stream.hip).

The oracle is existing code: sel_conv_step at B = 1 on the slot's carry and the
sample's input rows.  Every comparison is bitwise, on integer views.  Every
buffer the kernel must not touch holds a NaN sentinel pattern and is compared
with a copy taken before the launch: out rows >= n*T, the slots of carry_out
that are not listed, its template row, and the whole of carry.

Capacity 6 and nslots 7 (row 6 = the template) unless a case says otherwise.
No launch here is given an out-of-range or duplicate slot id.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
IDS = ["fp32", "bf16"]
CAP, NSLOTS = 6, 7
SETS = {"none": [], "one_on_the_last_slot": [5], "all_reversed": [5, 4, 3, 2, 1, 0], "three_mixed_tile": [4, 1, 5]}


def bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16 if t.element_size() == 2
                               else torch.uint8)


def same(a, b):
    return torch.equal(bits(a), bits(b))


def sentinel(shape, dtype, gpu):
    """NaNs of varying payload: a copy, a shift or a partial write all show."""
    n = int(np.prod(shape))
    if dtype == torch.float32:
        raw = (0x7FC00000 + (torch.arange(n, dtype=torch.int64) % 4093 + 1)).to(torch.int32)
    else:
        raw = (0x7FC0 + (torch.arange(n, dtype=torch.int64) % 61 + 1)).to(torch.int16)
    return raw.to(gpu).view(dtype).view(shape)


def staged(slots, cap, gpu):
    s = torch.zeros(cap, dtype=torch.int32)
    s[:len(slots)] = torch.tensor(slots, dtype=torch.int32)
    return s.to(gpu), torch.tensor([len(slots)], dtype=torch.int32, device=gpu)


class Case:
    """One layer: descriptor at any batch, packed weight, operand widths."""

    def __init__(self, gpu, dtype, seed, T, C, N, K, dil, w, kind, stride, elu=False, bias_period=0, res=False,
                 cap=CAP, nslots=NSLOTS):
        from sel import convops as CO
        self.gpu, self.dtype, self.T, self.C, self.N, self.K, self.dil = gpu, dtype, T, C, N, K, dil
        self.P = (K - 1) * dil
        self.cap, self.nslots, self.res = cap, nslots, res
        self.g = torch.Generator().manual_seed(seed)
        self.wp = CO.pack(kind, w(self.g).to(gpu), stride, dtype)
        assert tuple(self.wp.shape) == (N, K, C)
        self.bias = torch.randn(bias_period, generator=self.g).to(gpu) if bias_period else None
        self.mk = lambda B: CO.ConvDesc(B * T, T, C, N, K, dil, self.P, CO.PAD_ZERO, int(elu), bias_period)

    def rnd(self, *shape):
        return torch.randn(*shape, generator=self.g).to(self.dtype).to(self.gpu)

    def operands(self):
        """Random pools and dense buffers at capacity; every row holds data, so
        a row read for a sample that does not exist would change an output."""
        carry = self.rnd(self.nslots, self.P, self.C) if self.P else None
        x = self.rnd(self.cap * self.T, self.C)
        r = self.rnd(self.cap * self.T, self.N) if self.res else None
        return carry, x, r

    def pool(self, carry, x, r, slots, out=None, carry_out=None):
        from sel import streamops as SO
        sl, n = staged(slots, self.cap, self.gpu)
        out = sentinel((self.cap * self.T, self.N), self.dtype, self.gpu) if out is None else out
        if self.P and carry_out is None:
            carry_out = sentinel((self.nslots, self.P, self.C), self.dtype, self.gpu)
        SO.conv_step_pool(self.mk(self.cap), carry, carry_out, sl, n, x, self.wp, self.bias, r, out,
                          nslots=self.nslots)
        return out, carry_out

    def solo(self, carry, x, r, i, slot):
        from sel import streamops as SO
        T = self.T
        return SO.conv_step(self.mk(1), carry[slot:slot + 1].contiguous() if self.P else None,
                            x[i * T:(i + 1) * T].contiguous(), self.wp, self.bias,
                            r[i * T:(i + 1) * T].contiguous() if r is not None else None)

    def check(self, slots):
        carry, x, r = self.operands()
        keep = carry.clone() if self.P else None
        out0 = sentinel((self.cap * self.T, self.N), self.dtype, self.gpu)
        co0 = sentinel((self.nslots, self.P, self.C), self.dtype, self.gpu) if self.P else None
        out, cout = self.pool(carry, x, r, slots, out0.clone(), co0.clone() if self.P else None)
        torch.cuda.synchronize()
        n, T = len(slots), self.T
        for i, slot in enumerate(slots):
            o, c = self.solo(carry, x, r, i, slot)
            assert same(out[i * T:(i + 1) * T], o), ("out", i, slot)
            if self.P:
                assert same(cout[slot], c[0]), ("carry_out", i, slot)
        assert same(out[n * T:], out0[n * T:]), "out rows >= n*T were written"
        if self.P:
            for s in range(self.nslots):
                if s not in slots:
                    assert same(cout[s], co0[s]), f"carry_out slot {s} (not listed) was written"
            assert same(carry, keep), "carry was written"


def fwd(N, C, K):
    return lambda g: torch.randn(N, C, K, generator=g) / (C * K) ** 0.5


def make(name, gpu, dtype):
    from sel import convops as CO
    if name == "C4_N5_elementwise_masked_bias_elu":
        return Case(gpu, dtype, 1, 3, 4, 5, 3, 2, fwd(5, 4, 3), CO.PACK_FWD, 1, elu=True, bias_period=5)
    if name == "T_lt_P_old_rows_survive_res":
        return Case(gpu, dtype, 2, 5, 16, 32, 7, 9, fwd(32, 16, 7), CO.PACK_FWD, 1, res=True)
    if name == "pointwise_null_pools_res":
        return Case(gpu, dtype, 3, 3, 16, 16, 1, 1, fwd(16, 16, 1), CO.PACK_FWD, 1, res=True)
    if name == "strided_pack_cin8_s2":
        return Case(gpu, dtype, 4, 3, 16, 8, 3, 1, lambda g: torch.randn(8, 8, 4, generator=g) / 32 ** 0.5,
                    CO.PACK_FWD_STRIDED, 2, bias_period=8)
    if name == "convt_pack_cin16_cout8_s2":
        return Case(gpu, dtype, 5, 3, 16, 16, 2, 1, lambda g: torch.randn(16, 8, 4, generator=g) / 32 ** 0.5,
                    CO.PACK_CONVT, 2, bias_period=8)
    if name == "eight_wave_reduction":
        return Case(gpu, dtype, 6, 2, 160, 16, 7, 1, fwd(16, 160, 7), CO.PACK_FWD, 1)
    raise KeyError(name)


SHAPES = ["C4_N5_elementwise_masked_bias_elu", "T_lt_P_old_rows_survive_res", "pointwise_null_pools_res",
          "strided_pack_cin8_s2", "convt_pack_cin16_cout8_s2", "eight_wave_reduction"]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("active", list(SETS))
@pytest.mark.parametrize("shape", SHAPES)
def test_pool_step_equals_solo_steps(gpu, shape, active, dtype):
    make(shape, gpu, dtype).check(SETS[active])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", [0, 1, 64, 70])
def test_pool_step_across_the_row_tile_switch(gpu, n, dtype):
    """Capacity 70 x T 16 = 1120 rows = 70 row tiles: the launch takes four row
    tiles per block (from 64 tiles on) whatever n is, each solo launch one."""
    from sel import convops as CO
    c = Case(gpu, dtype, 7, 16, 8, 16, 2, 1, fwd(16, 8, 2), CO.PACK_FWD, 1, cap=70, nslots=71)
    perm = torch.randperm(70, generator=torch.Generator().manual_seed(70)).tolist()
    c.check({0: [], 1: [69], 64: perm[:64], 70: list(range(69, -1, -1))}[n])


def _pools(gpu, dtype, shape, seed):
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.uint8:
        return torch.randint(0, 256, shape, generator=g, dtype=torch.uint8).to(gpu)
    return torch.randn(shape, generator=g).to(dtype).to(gpu)


def _guarded(t, gpu):
    """t between two 64-byte guards; returns (flat uint8 buffer, view shaped like t)."""
    nb = t.numel() * t.element_size()
    flat = torch.full((nb + 128,), 0xA5, dtype=torch.uint8, device=gpu)
    v = flat[64:64 + nb].view(t.dtype).view(t.shape)
    v.copy_(t)
    return flat, v


@pytest.mark.parametrize("slots", [[], [5], [4, 1, 5], [5, 4, 3, 2, 1, 0]], ids=["n0", "n1", "n3", "all"])
def test_copy_slots_commit_form(gpu, slots):
    """carry_out -> carry for the listed slots, three jobs in one launch: an
    aligned pitch (16-byte vectors), an odd bf16 pitch (74 bytes: rows are not
    16-byte aligned, byte copies) and a 37-byte pitch."""
    from sel import streamops as SO
    shapes = [((NSLOTS, 3, 16), torch.float32), ((NSLOTS, 37), torch.bfloat16), ((NSLOTS, 37), torch.uint8)]
    src = [_pools(gpu, dt, sh, 40 + i) for i, (sh, dt) in enumerate(shapes)]
    dst0 = [_pools(gpu, dt, sh, 50 + i) for i, (sh, dt) in enumerate(shapes)]
    guarded = [_guarded(d, gpu) for d in dst0]
    keep = [s.clone() for s in src]
    sl, n = staged(slots, CAP, gpu)
    SO.copy_slots([(s, d) for s, (_, d) in zip(src, guarded)], sl, sl, n)
    torch.cuda.synchronize()
    for s, k, d0, (flat, d) in zip(src, keep, dst0, guarded):
        assert same(s, k)
        assert bool((flat[:64] == 0xA5).all()) and bool((flat[-64:] == 0xA5).all())
        for r in range(NSLOTS):
            assert same(d[r], s[r] if r in slots else d0[r]), (r, slots)


@pytest.mark.parametrize("dtype,pitch", [(torch.float32, (3, 16)), (torch.bfloat16, (37,)), (torch.uint8, (21,))],
                         ids=["aligned", "odd_bf16", "odd_bytes"])
def test_copy_slots_open_form(gpu, dtype, pitch):
    """The template row (6) of a pool -> slot 2 of the SAME pool, n = 1; then n = 0 copies nothing."""
    from sel import streamops as SO
    pool0 = _pools(gpu, dtype, (NSLOTS,) + pitch, 60)
    flat, pool = _guarded(pool0, gpu)
    ctl = torch.tensor([1, NSLOTS - 1, 2], dtype=torch.int32, device=gpu)
    SO.copy_slots([(pool, pool)], ctl[1:2], ctl[2:3], ctl[0:1])
    torch.cuda.synchronize()
    for r in range(NSLOTS):
        assert same(pool[r], pool0[NSLOTS - 1 if r == 2 else r]), r
    assert bool((flat[:64] == 0xA5).all()) and bool((flat[-64:] == 0xA5).all())
    after = pool.clone()
    ctl.copy_(torch.tensor([0, NSLOTS - 1, 4], dtype=torch.int32))
    SO.copy_slots([(pool, pool)], ctl[1:2], ctl[2:3], ctl[0:1])
    torch.cuda.synchronize()
    assert same(pool, after)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_one_graph_serves_every_active_set(gpu, dtype):
    """Step + commit captured once (with n = 0), replayed with three staged
    (slots, n) and fresh inputs: carry, carry_out and out equal the eager
    launches on a twin set of buffers, bitwise, after every replay."""
    from sel import streamops as SO
    c = make("T_lt_P_old_rows_survive_res", gpu, dtype)
    carry0, _, _ = c.operands()
    d = c.mk(CAP)
    sets = []
    for tag in ("g", "e"):
        sets.append(dict(carry=carry0.clone(), cout=sentinel(carry0.shape, dtype, gpu),
                         x=torch.zeros(CAP * c.T, c.C, dtype=dtype, device=gpu),
                         r=torch.zeros(CAP * c.T, c.N, dtype=dtype, device=gpu),
                         out=sentinel((CAP * c.T, c.N), dtype, gpu),
                         ctl=torch.zeros(1 + CAP, dtype=torch.int32, device=gpu)))
    G, E = sets

    def launch(s):
        n, sl = s["ctl"][:1], s["ctl"][1:]
        SO.conv_step_pool(d, s["carry"], s["cout"], sl, n, s["x"], c.wp, c.bias, s["r"], s["out"])
        SO.copy_slots([(s["cout"], s["carry"])], sl, sl, n)

    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        launch(G)                                   # n = 0: nothing happens
    torch.cuda.current_stream(gpu).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch(G)
    torch.cuda.synchronize()
    assert same(G["carry"], carry0) and same(G["out"], E["out"]) and same(G["cout"], E["cout"])
    for slots in ([4, 1, 5], [0], [5, 4, 3, 2, 1, 0]):
        x, r = c.rnd(CAP * c.T, c.C), c.rnd(CAP * c.T, c.N)
        words = torch.tensor([len(slots)] + slots + [0] * (CAP - len(slots)), dtype=torch.int32)
        for s in (G, E):
            s["x"].copy_(x)
            s["r"].copy_(r)
            s["ctl"].copy_(words)
        graph.replay()
        launch(E)
        torch.cuda.synchronize()
        for k in ("out", "carry", "cout"):
            assert same(G[k], E[k]), (slots, k)
        assert not same(G["carry"], carry0)


def test_argument_errors_before_device_work(gpu):
    """SEL_ERR_ARG (-1) for null slots / n_active, nslots <= 0 and the inherited
    aliasing and dtype errors; the operands are sentinel-filled and stay so."""
    import ctypes
    from sel import _lib
    from sel import convops as CO
    lib = _lib.lib()
    c = make("T_lt_P_old_rows_survive_res", gpu, torch.float32)
    carry, x, _ = c.operands()
    out0 = sentinel((CAP * c.T, c.N), torch.float32, gpu)
    co0 = sentinel(carry.shape, torch.float32, gpu)
    out, cout = out0.clone(), co0.clone()
    sl, n = staged([4, 1, 5], CAP, gpu)
    P = _lib.ptr
    d = c.mk(CAP)

    def call(carry_=carry, cout_=cout, nslots=NSLOTS, sl_=sl, n_=n, out_=out, dt=(CO.F32, CO.F32)):
        return lib.sel_conv_step_pool(ctypes.byref(d), dt[0], dt[1], P(carry_), P(cout_), nslots, P(sl_), P(n_),
                                      P(x), P(c.wp), None, None, P(out_), _lib.stream())

    assert call(sl_=None) == -1 and call(n_=None) == -1
    assert call(nslots=0) == -1 and call(nslots=-1) == -1
    assert call(cout_=carry) == -1          # carry_out aliases carry
    assert call(out_=carry) == -1           # out aliases carry
    assert call(out_=x) == -1               # out aliases in
    assert call(cout_=x) == -1              # carry_out aliases in
    assert call(dt=(CO.F32, CO.BF16)) == -1 and call(dt=(9, 9)) == -1
    torch.cuda.synchronize()
    assert same(out, out0) and same(cout, co0)


def test_python_layer_rejects_bad_slot_lists(gpu):
    """Out-of-range and duplicate ids never reach a kernel: SlotTable.check refuses them."""
    from sel import SelError
    from sel import streamops as SO
    t = SO.SlotTable(CAP)
    for _ in range(CAP):
        t.open()
    for bad in ([6], [-1], [2, 2], list(range(6)) + [0]):
        with pytest.raises(SelError):
            t.check(bad)
