"""Host side of the vocoder sessions, on the CPU.

sel.streamops.plan_vocoder() is pure Python: it turns a HiFi-GAN StreamGenerator
into the ordered sel_hfg_conv_step launches of a hop.  Here each plan is
executed by an fp64 torch statement of the step contract (include/sel.h
sel_hfg_conv_step: the virtual input [carry | act(in)], groups, the shared input
and residual, the epilogue order; the two pack forms with the weight-norm fold
g * v / ||v|| restated below) on the weights of the reference goldens
(tests/golden/vocoder_v1.npz MultiGroupConv1d, vocoder_v0.npz
MultiReceptiveField) and must reproduce every streamed chunk and every final
pad_buffer the reference recorded, to 1e-5 norm-wise (the project's fp32 bound;
the goldens are the reference's own fp32 output).  Also: the shape of the
full-width plans, what plan_vocoder() rejects, and sel_hfg_conv_step's argument
validation through ctypes (SEL_ERR_ARG before any device work).
"""
import ctypes

import numpy as np
import pytest
import torch

from conftest import golden
from sel import configs
from sel import convops as CO
from sel import hfgops as HF
from sel import streamops as SO

SCALES = dict(upsample_scales=[5, 5, 4, 3], upsample_kernel_sizes=[10, 10, 8, 6])
V1 = dict(in_channels=64, channels=64, resblock_kernel_sizes=[11], resblock_dilations=[[1, 3, 5]], groups=3, **SCALES)
V0 = dict(in_channels=64, channels=32, resblock_kernel_sizes=[3, 7, 11], resblock_dilations=[[1, 3, 5]] * 3,
          groups=1, **SCALES)
MODELS = [("vocoder_v1", V1), ("vocoder_v0", V0)]
SEL_ERR_ARG = -1


def _generator(params):
    from models.vocoder.HiFiGAN import StreamGenerator
    return StreamGenerator(**params).eval()


def _folded(sd, prefix):
    """g * v / ||v|| (norm over all dims but 0), or the plain weight"""
    if prefix + ".weight_g" in sd:
        g, v = sd[prefix + ".weight_g"], sd[prefix + ".weight_v"]
        return v * (g / v.flatten(1).norm(dim=1).view(-1, 1, 1))
    return sd[prefix + ".weight"]


def _pack(kind, w, s):
    """The packed forms as include/sel.h defines them."""
    if kind == CO.PACK_FWD:                       # W[N][C/G][K] -> Wp[N][K][C/G]
        return w.permute(0, 2, 1).contiguous()
    assert kind == CO.PACK_CONVT
    cin, cout, k2 = w.shape                       # Wt[Cin][Cout][2s] -> Wp[s*Cout][2][Cin]
    assert k2 == 2 * s
    wp = torch.zeros(s * cout, 2, cin, dtype=w.dtype)
    for ph in range(s):
        wp[ph * cout:(ph + 1) * cout, 0] = w[:, :, ph + s].t()   # the previous input row
        wp[ph * cout:(ph + 1) * cout, 1] = w[:, :, ph].t()       # the current one
    return wp


def _step(st, B, x, carry, wp, bias, res, prev):
    """sel_hfg_conv_step's contract in torch: returns (out (B*T, N), carry_out)."""
    G, T, P = st.groups, st.T, st.pad
    Cg, Ng = st.C // G, st.N // G
    x = x.reshape(B, T, Cg if st.shared_in else st.C)
    a = torch.where(x >= 0, x, st.slope * x)
    if st.shared_in:
        a = a.repeat(1, 1, G)                     # the carry has pitch C: once per group
    v = torch.cat((carry, a), 1) if P else a
    out = torch.zeros(B, T, st.N, dtype=x.dtype)
    for g in range(G):
        vg, wg = v[:, :, g * Cg:(g + 1) * Cg], wp[g * Ng:(g + 1) * Ng]
        out[:, :, g * Ng:(g + 1) * Ng] = sum(
            torch.einsum("btc,nc->btn", vg[:, k * st.dil:k * st.dil + T], wg[:, k]) for k in range(st.K))
    if st.bias_period:
        out = out + bias.repeat(st.N // st.bias_period)
    if res is not None:
        r = res.reshape(B, T, Ng if st.shared_res else st.N)
        out = out + (r.repeat(1, 1, G) if st.shared_res else r)
    if st.tanh:
        out = torch.tanh(out)
    out = out * st.scale
    out = out.reshape(B * T, st.N)
    if st.accumulate:
        out = out + prev
    return out, (v[:, v.shape[1] - P:].clone() if P else None)


class _Executor:
    def __init__(self, steps, sd, B):
        self.steps, self.B = steps, B
        self.wp = [_pack(st.kind, _folded(sd, st.conv), st.stride) for st in steps]
        self.bias = [sd[st.conv + ".bias"] if st.bias_period else None for st in steps]
        self.carry = [torch.zeros(st.carry_shape, dtype=torch.float64) if st.carry_shape else None for st in steps]

    def run(self, x):
        outs = {}
        buf = lambda i: x if i == -1 else outs[i]  # noqa: E731
        for i, st in enumerate(self.steps):
            assert st.out == i or (st.accumulate and st.out < i)
            o, c = _step(st, self.B, buf(st.src), self.carry[i], self.wp[i], self.bias[i],
                         None if st.res is None else buf(st.res), outs.get(st.out))
            outs[st.out] = o
            self.carry[i] = c
        return outs[self.steps[-1].out]

    def buffers(self):
        """{state_dict key: (B, C, P)} from the carries."""
        out = {}
        for st, c in zip(self.steps, self.carry):
            if c is not None:
                assert st.buffer == st.name + ".pad_buffer" and tuple(c.shape[1:]) == st.buffer_shape[:0:-1]
                out[st.buffer] = c.transpose(1, 2)
        return out


def _close(a, b, name):
    b = torch.as_tensor(np.asarray(b)).double()
    e = float((a - b).norm() / (b.norm() + 1e-300))
    assert a.shape == b.shape and e <= 1e-5, (name, tuple(a.shape), tuple(b.shape), e)


def _golden_sd(g):
    return {k[3:]: torch.from_numpy(v.astype(np.float64)) for k, v in g.items() if k.startswith("sd.")}


@pytest.mark.parametrize("name,params", MODELS)
def test_plan_executes_to_the_reference_golden(name, params):
    g = golden(name)
    sd = _golden_sd(g)
    pl = SO.plan_vocoder(_generator(params), 1, 1)
    assert (pl.batch, pl.frames, pl.in_channels, pl.out_channels, pl.out_samples) == (1, 1, 64, 1, 300)
    ex = _Executor(pl.steps, sd, 1)
    x = torch.from_numpy(g["x"]).double()
    for c in range(7):
        y = ex.run(x[:1, :, c:c + 1].transpose(2, 1)).reshape(1, 300, 1).transpose(1, 2)
        _close(y, g[f"y.{c}"], f"y.{c}")
    bufs = ex.buffers()
    assert set(bufs) == {k for k in sd if k.endswith("pad_buffer")} == {k[4:] for k in g if k.startswith("buf.")}
    for k, v in bufs.items():
        _close(v, g["buf." + k], k)


@pytest.mark.parametrize("name,params", MODELS)
def test_two_frame_hops_equal_the_golden_chunks(name, params):
    g = golden(name)
    pl = SO.plan_vocoder(_generator(params), 1, 2)
    assert pl.out_samples == 600
    ex = _Executor(pl.steps, _golden_sd(g), 1)
    x = torch.from_numpy(g["x"]).double()
    ys = [ex.run(x[:1, :, 2 * h:2 * h + 2].transpose(2, 1)).reshape(1, 600, 1).transpose(1, 2) for h in range(3)]
    want = np.concatenate([g[f"y.{c}"] for c in range(6)], -1)
    _close(torch.cat(ys, -1), want, "y.0..y.5")


def test_full_width_v1_plan():
    pl = SO.plan_vocoder(_generator(configs.VOCODER_V1), 1, 1)
    st = pl.steps
    assert len(st) == 34 and sum(s.carry_shape is not None for s in st) == 30
    assert pl.out_samples == 300 and pl.in_channels == 64 and pl.out_channels == 1
    assert (st[0].name, st[0].slope, st[0].src, st[0].K, st[0].groups) == ("input_conv", 1.0, -1, 7, 1)
    d5 = next(s for s in st if s.name == "blocks.0.convs1.2")
    assert (d5.T, d5.K, d5.dil, d5.groups, d5.carry_shape) == (5, 11, 5, 3, (1, 50, 768))
    assert d5.buffer == "blocks.0.convs1.2.pad_buffer" and d5.buffer_shape == (1, 768, 50)
    assert d5.conv == "blocks.0.convs1.2.conv" and d5.kind == CO.PACK_FWD
    T = 1
    for i, s in enumerate((5, 5, 4, 3)):
        up = next(j for j, v in enumerate(st) if v.name == f"upsamples.{i}")
        ch = 512 >> (i + 1)
        assert (st[up].kind, st[up].stride, st[up].T, st[up].C, st[up].N, st[up].K, st[up].bias_period,
                st[up].slope, st[up].carry_shape) == (CO.PACK_CONVT, s, T, 2 * ch, s * ch, 2, ch, 0.1, (1, 1, 2 * ch))
        T *= s
        c1, c2 = st[up + 1], st[up + 2]
        assert c1.name == f"blocks.{i}.convs1.0" and c2.name == f"blocks.{i}.convs2.0"
        # the first layer reads the ch-channel upsampling output for every group; no repeat step exists
        assert c1.shared_in and not c1.shared_res and c1.src == up and c1.res is None and c1.C == 3 * ch
        assert c2.shared_res and not c2.shared_in and c2.src == up + 1 and c2.res == up
        assert c1.carry_shape == (1, 10, 3 * ch) and c1.T == T and c1.slope == 0.1
        for later in st[up + 3:up + 7]:
            assert not later.shared_in and not later.shared_res and later.groups == 3
        assert st[up + 4].res == up + 2 and st[up + 6].res == up + 4
        co = st[up + 7]
        assert (co.name, co.conv, co.K, co.groups, co.C, co.N, co.carry_shape, co.slope, co.bias_period) == \
            (f"blocks.{i}.conv_out", f"blocks.{i}.conv_out", 1, 1, 3 * ch, ch, None, 1.0, 0)
        assert co.src == up + 6
    assert all(s.out == i and not s.accumulate and s.scale == 1.0 for i, s in enumerate(st))
    last = st[-1]
    assert last.name == "output_conv" and last.tanh and last.out_float and last.slope == pytest.approx(0.01)
    assert (last.T, last.C, last.N, last.K) == (300, 32, 1, 7) and not any(s.tanh or s.out_float for s in st[:-1])


def test_full_width_v0_plan():
    pl = SO.plan_vocoder(_generator(configs.VOCODER_V0), 1, 1)
    st = pl.steps
    assert len(st) == 78 and sum(s.carry_shape is not None for s in st) == 78
    assert len({s.buffer for s in st}) == 78 and all(s.groups == 1 for s in st)
    for i in range(4):
        up = next(j for j, v in enumerate(st) if v.name == f"upsamples.{i}")
        fused = up + 6                                  # block 0's last conv owns the fusion buffer
        for j in range(3):
            blk = st[up + 1 + 6 * j:up + 7 + 6 * j]
            assert [s.name for s in blk] == [f"blocks.{i}.blocks.{j}.convs{c}.{l}" for l in range(3) for c in (1, 2)]
            assert blk[0].src == up and blk[1].res == up  # every block reads the upsampling output
            assert all(s.K == (3, 7, 11)[j] for s in blk)
            assert all(s.scale == 1.0 and not s.accumulate and s.out == up + 1 + 6 * j + n
                       for n, s in enumerate(blk[:-1]))
            last = blk[-1]
            assert last.scale == pytest.approx(1.0 / 3) and last.out == fused and last.accumulate == (j > 0)
        nxt = st[up + 19]
        assert nxt.src == fused and nxt.name in (f"upsamples.{i + 1}", "output_conv")
    assert st[-1].tanh and st[-1].out_float


def test_single_conv_layers_take_x_as_residual():
    pl = SO.plan_vocoder(_generator(dict(V1, use_additional_convs=False)), 2, 1)
    st = pl.steps
    assert len(st) == 1 + 4 * (1 + 3 + 1) + 1
    up = 1
    assert st[up + 1].shared_in and st[up + 1].shared_res and st[up + 1].src == st[up + 1].res == up
    assert st[up + 2].src == st[up + 2].res == up + 1 and not st[up + 2].shared_in
    assert st[up + 1].carry_shape == (2, 10, 96)


def test_plan_vocoder_rejects_what_a_session_cannot_run():
    from layers.conv_layer import CausalConvTranspose1d
    with pytest.raises(NotImplementedError, match="LeakyReLU"):
        SO.plan_vocoder(_generator(dict(V1, nonlinear_activation="ReLU", nonlinear_activation_params={})), 1, 1)
    G = _generator(V0)
    G.blocks[2].blocks[1].activation = torch.nn.ELU()
    with pytest.raises(NotImplementedError, match="LeakyReLU"):
        SO.plan_vocoder(G, 1, 1)
    G = _generator(V1)
    SO.plan_vocoder(G, 1, 1)
    G.upsamples[1] = CausalConvTranspose1d(32, 16, kernel_size=12, stride=5)
    with pytest.raises(NotImplementedError, match="2 \\* stride"):
        SO.plan_vocoder(G, 1, 1)
    with pytest.raises(ValueError):
        SO.plan_vocoder(_generator(V1), 0, 1)


def test_hfg_conv_step_wrapper_refuses_cpu_tensors():
    from sel import SelError
    d = HF.make_desc(4, 4, 6, 6, 3, 1, 2, groups=3)
    with pytest.raises(SelError, match="device"):
        SO.hfg_conv_step(d, torch.zeros(1, 2, 6), torch.zeros(4, 6), torch.zeros(6, 3, 2))


def test_hfg_conv_step_validates_arguments_before_device_work():
    from sel import _lib
    lib = _lib.load()
    p = lambda v: ctypes.c_void_p(v)  # noqa: E731  (never dereferenced: every call below is refused first)
    inp, wp, out, ca, co = p(0x10000), p(0x20000), p(0x30000), p(0x40000), p(0x50000)

    def call(d, carry=ca, carry_out=co, dt=(CO.F32, CO.F32)):
        rc = lib.sel_hfg_conv_step(ctypes.byref(d) if d is not None else None, dt[0], dt[1], carry, inp, wp, None,
                                   None, out, carry_out, None)
        return rc, lib.sel_last_error().decode()

    def desc(**kw):
        d = HF.make_desc(12, 4, 24, 24, 7, 2, 12, groups=3, slope=0.1)
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    rc, msg = call(None)
    assert rc == SEL_ERR_ARG and "null descriptor" in msg, (rc, msg)
    rc, msg = call(desc(pad=11))
    assert rc == SEL_ERR_ARG and "(K-1)*dil" in msg, (rc, msg)
    rc, msg = call(desc(act_skip=12))
    assert rc == SEL_ERR_ARG and "act_skip" in msg, (rc, msg)
    rc, msg = call(desc(C=25))
    assert rc == SEL_ERR_ARG and "must divide" in msg, (rc, msg)
    rc, msg = call(desc(N=25))
    assert rc == SEL_ERR_ARG and "must divide" in msg, (rc, msg)
    rc, msg = call(desc(in_group_stride=24))
    assert rc == SEL_ERR_ARG and "in_group_stride" in msg, (rc, msg)
    rc, msg = call(desc(res_group_stride=3))
    assert rc == SEL_ERR_ARG and "res_group_stride" in msg, (rc, msg)
    rc, msg = call(desc(), ca, ca)
    assert rc == SEL_ERR_ARG and "alias" in msg, (rc, msg)
    rc, msg = call(desc(), None, co)
    assert rc == SEL_ERR_ARG and "needs carry" in msg, (rc, msg)
    rc, msg = call(desc(), dt=(CO.F32, CO.BF16))
    assert rc == SEL_ERR_ARG and "dtypes" in msg, (rc, msg)
    rc, msg = call(desc(pad_mode=CO.PAD_REPLICATE))
    assert rc == SEL_ERR_ARG and "SEL_PAD_ZERO" in msg, (rc, msg)
    rc, msg = call(desc(T_out=3))
    assert rc == SEL_ERR_ARG and "T_out" in msg, (rc, msg)
    rc, msg = call(desc(rows=10))
    assert rc == SEL_ERR_ARG and "multiple of T" in msg, (rc, msg)
