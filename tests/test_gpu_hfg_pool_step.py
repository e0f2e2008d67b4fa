"""sel_hfg_conv_step_pool (csrc/hfg_step.hip), in the scheme of
tests/test_gpu_stream_pool_step.py: the oracle is sel_hfg_conv_step at B = 1 on
the slot's carry and the sample's rows, every comparison is bitwise on integer
views, and out rows >= n*T, unlisted slots of carry_out, its template row and
the whole of carry are compared with copies taken before the launch.

Capacity 6 and nslots 7 unless a case says otherwise.  No launch is given an
out-of-range or duplicate slot id.
"""
import pytest
import torch

from test_gpu_stream_pool_step import CAP, DTYPES, IDS, NSLOTS, SETS, same, sentinel, staged

pytestmark = pytest.mark.gpu


class Case:
    def __init__(self, gpu, dtype, seed, T, C, N, K, dil, G=1, slope=0.1, shared_in=False, shared_res=False,
                 bias_period=0, res=False, tanh=False, scale=1.0, accumulate=False, out_dtype=None, convt=0,
                 cap=CAP, nslots=NSLOTS):
        from sel import convops as CO
        from sel import hfgops as HF
        self.gpu, self.dtype, self.odt = gpu, dtype, out_dtype or dtype
        self.T, self.C, self.N, self.G, self.P = T, C, N, G, (K - 1) * dil
        self.cap, self.nslots, self.res, self.accumulate = cap, nslots, res, accumulate
        self.cin = C // G if shared_in else C
        self.nres = N // G if shared_res else N
        self.g = torch.Generator().manual_seed(seed)
        if convt:       # ConvTranspose1d weight (Cin, Cout, 2s): N = s * Cout, K = 2
            w = torch.randn(C, N // convt, 2 * convt, generator=self.g) / (2 * C) ** 0.5
            self.wp = CO.pack(CO.PACK_CONVT, w.to(gpu), convt, dtype)
        else:
            w = torch.randn(N, C // G, K, generator=self.g) / (C // G * K) ** 0.5
            self.wp = CO.pack(CO.PACK_FWD, w.to(gpu), 1, dtype)
        assert tuple(self.wp.shape) == (N, K, C // G)
        self.bias = torch.randn(bias_period, generator=self.g).to(gpu) if bias_period else None
        self.mk = lambda B: HF.make_desc(B * T, T, C, N, K, dil, self.P, groups=G, shared_in=shared_in,
                                         shared_res=shared_res, bias_period=bias_period, tanh=tanh,
                                         accumulate=accumulate, slope=slope, scale=scale)

    def rnd(self, shape, dtype=None):
        dtype = dtype or self.dtype
        return torch.randn(*shape, generator=self.g).to(dtype).to(self.gpu)

    def check(self, slots):
        from sel import streamops as SO
        T, n = self.T, len(slots)
        carry = self.rnd((self.nslots, self.P, self.C)) if self.P else None
        x = self.rnd((self.cap * T, self.cin))
        r = self.rnd((self.cap * T, self.nres), self.odt) if self.res else None
        # accumulate adds into out: pre-filled with data where samples exist, sentinels behind them
        out0 = sentinel((self.cap * T, self.N), self.odt, self.gpu)
        if self.accumulate:
            out0[:n * T] = self.rnd((n * T, self.N), self.odt)
        keep = carry.clone() if self.P else None
        co0 = sentinel((self.nslots, self.P, self.C), self.dtype, self.gpu) if self.P else None
        out, cout = out0.clone(), co0.clone() if self.P else None
        sl, na = staged(slots, self.cap, self.gpu)
        SO.hfg_conv_step_pool(self.mk(self.cap), carry, cout, sl, na, x, self.wp, self.bias, r, out,
                              nslots=self.nslots)
        torch.cuda.synchronize()
        for i, slot in enumerate(slots):
            o = out0[i * T:(i + 1) * T].clone()
            o, c = SO.hfg_conv_step(self.mk(1), carry[slot:slot + 1].contiguous() if self.P else None,
                                    x[i * T:(i + 1) * T].contiguous(), self.wp, self.bias,
                                    r[i * T:(i + 1) * T].contiguous() if r is not None else None, o)
            assert same(out[i * T:(i + 1) * T], o), ("out", i, slot)
            if self.P:
                assert same(cout[slot], c[0]), ("carry_out", i, slot)
        assert same(out[n * T:], out0[n * T:]), "out rows >= n*T were written"
        if self.P:
            for s in range(self.nslots):
                if s not in slots:
                    assert same(cout[s], co0[s]), f"carry_out slot {s} (not listed) was written"
            assert same(carry, keep), "carry was written"


def make(name, gpu, dtype):
    if name == "G3_shared_in_shared_res":         # C/G = 8: 16-byte loads; in / res of pitch C/G, N/G
        return Case(gpu, dtype, 1, 3, 24, 24, 3, 1, G=3, shared_in=True, shared_res=True, bias_period=24, res=True)
    if name == "G2_five_per_group_elementwise":
        return Case(gpu, dtype, 2, 3, 10, 10, 3, 2, G=2, bias_period=10, res=True)
    if name == "K11_dil5_T1_old_rows_survive":
        return Case(gpu, dtype, 3, 1, 16, 16, 11, 5)
    if name == "convt_cin16_cout8_s2":
        return Case(gpu, dtype, 4, 3, 16, 16, 2, 1, bias_period=8, convt=2)
    if name == "tanh_scale_accumulate":
        return Case(gpu, dtype, 5, 3, 16, 8, 7, 1, slope=0.01, bias_period=8, res=True, tanh=True, scale=1.0 / 3,
                    accumulate=True)
    if name == "tanh_fp32_output":
        return Case(gpu, dtype, 6, 5, 16, 1, 7, 1, slope=0.01, bias_period=1, tanh=True, out_dtype=torch.float32)
    raise KeyError(name)


SHAPES = ["G3_shared_in_shared_res", "G2_five_per_group_elementwise", "K11_dil5_T1_old_rows_survive",
          "convt_cin16_cout8_s2", "tanh_scale_accumulate", "tanh_fp32_output"]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("active", list(SETS))
@pytest.mark.parametrize("shape", SHAPES)
def test_hfg_pool_step_equals_solo_steps(gpu, shape, active, dtype):
    make(shape, gpu, dtype).check(SETS[active])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", [0, 1, 64, 70])
def test_hfg_pool_step_across_the_row_tile_switch(gpu, n, dtype):
    """Capacity 70 x T 16 = 1120 rows = 70 row tiles: four row tiles per block
    whatever n is, one per block in every solo launch.  G = 2, 4 channels per group."""
    c = Case(gpu, dtype, 7, 16, 8, 16, 2, 1, G=2, bias_period=16, cap=70, nslots=71)
    perm = torch.randperm(70, generator=torch.Generator().manual_seed(71)).tolist()
    c.check({0: [], 1: [69], 64: perm[:64], 70: list(range(69, -1, -1))}[n])


def test_hfg_argument_errors_before_device_work(gpu):
    import ctypes
    from sel import _lib
    from sel import convops as CO
    lib = _lib.lib()
    c = make("K11_dil5_T1_old_rows_survive", gpu, torch.float32)
    carry, x = c.rnd((NSLOTS, c.P, c.C)), c.rnd((CAP * c.T, c.C))
    out0 = sentinel((CAP * c.T, c.N), torch.float32, gpu)
    co0 = sentinel(carry.shape, torch.float32, gpu)
    out, cout = out0.clone(), co0.clone()
    sl, n = staged([4, 1, 5], CAP, gpu)
    P = _lib.ptr
    d = c.mk(CAP)

    def call(carry_=carry, cout_=cout, nslots=NSLOTS, sl_=sl, n_=n, out_=out, dt=(CO.F32, CO.F32), res_=None):
        return lib.sel_hfg_conv_step_pool(ctypes.byref(d), dt[0], dt[1], P(carry_), P(cout_), nslots, P(sl_), P(n_),
                                          P(x), P(c.wp), None, P(res_), P(out_), _lib.stream())

    assert call(sl_=None) == -1 and call(n_=None) == -1
    assert call(nslots=0) == -1 and call(nslots=-1) == -1
    assert call(cout_=carry) == -1 and call(out_=carry) == -1 and call(out_=x) == -1 and call(cout_=x) == -1
    assert call(res_=cout) == -1            # carry_out aliases res
    assert call(dt=(CO.F32, CO.BF16)) == -1 and call(dt=(9, 9)) == -1
    torch.cuda.synchronize()
    assert same(out, out0) and same(cout, co0)
