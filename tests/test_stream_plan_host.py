"""Host side of the streaming sessions, on the CPU.

sel.streamops.plan() is pure Python: it turns a StreamGenerator into the ordered
sel_conv_step launches of a hop.  Here each plan is executed by a torch
statement of the step contract (include/sel.h sel_conv_step: the virtual input
[carry | act(in)], the packed forms of sel_pack_weight restated below) in fp64
and must reproduce oracle.ref_ops.stream_encode / stream_decode over 3 hops,
carries included, to 1e-6 -- which proves the strided (2s-sample phase carry) and
transposed (previous-row carry) bookkeeping without a GPU.  Also: what plan()
rejects, and sel_conv_step's argument validation through ctypes (negative code
before any device work).
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ref_ops as R
from sel import convops as CO
from sel import streamops as SO

GOLDEN_W = dict(encode_channels=4, decode_channels=4, code_dim=64, codebook_num=2, codebook_size=64)
FULL_W = dict(encode_channels=32, decode_channels=32, code_dim=64, codebook_num=8, codebook_size=1024)
NOPQC_W = dict(encode_channels=8, decode_channels=8, code_dim=64, codebook_num=2, codebook_size=64)


def _pack(kind, w, s):
    """The packed forms as include/sel.h defines them."""
    if kind == CO.PACK_FWD:                       # W[Cout][Cin][K] -> Wp[Cout][K][Cin]
        return w.permute(0, 2, 1).contiguous()
    if kind == CO.PACK_FWD_STRIDED:               # -> Wp[Cout][3][s*Cin] over the phase view
        cout, cin, k2 = w.shape
        assert k2 == 2 * s
        wp = torch.zeros(cout, 3, s * cin, dtype=w.dtype)
        for tap in range(3):
            for ph in range(s):
                # phase row t + tap, phase ph is sample (t + tap)*s + ph of the 2s-sample
                # carry + chunk; the reference's cat(buffer, x) starts one sample later
                k = tap * s + ph - 1
                if 0 <= k < 2 * s:
                    wp[:, tap, ph * cin:(ph + 1) * cin] = w[:, :, k]
        return wp
    cin, cout, k2 = w.shape                       # Wt[Cin][Cout][2s] -> Wp[s*Cout][2][Cin]
    assert k2 == 2 * s
    wp = torch.zeros(s * cout, 2, cin, dtype=w.dtype)
    for ph in range(s):
        wp[ph * cout:(ph + 1) * cout, 0] = w[:, :, ph + s].t()   # the previous input row
        wp[ph * cout:(ph + 1) * cout, 1] = w[:, :, ph].t()       # the current one
    return wp


def _step(st, B, x, carry, wp, bias, res):
    """sel_conv_step's contract in torch: returns (out (B*T, N), carry_out)."""
    x = x.reshape(B, st.T, st.C)
    v = F.elu(x) if st.in_elu else x
    P = st.pad
    if P:
        v = torch.cat((carry, v), 1)
    out = sum(torch.einsum("btc,nc->btn", v[:, k * st.dil:k * st.dil + st.T], wp[:, k]) for k in range(st.K))
    if st.bias_period:
        out = out + bias.repeat(st.N // st.bias_period)
    out = out.reshape(B * st.T, st.N)
    if res is not None:
        out = out + res.reshape(B * st.T, st.N)
    return out, (v[:, -P:].clone() if P else None)


class _Executor:
    def __init__(self, steps, sd, B):
        self.steps, self.B = steps, B
        self.wp = [_pack(st.kind, sd[st.weight], st.stride) for st in steps]
        self.bias = [sd[st.bias] if st.bias else None for st in steps]
        self.carry = [torch.zeros(st.carry_shape, dtype=torch.float64) if st.carry_shape else None for st in steps]

    def run(self, x):
        outs = []
        buf = lambda i: x if i == -1 else outs[i]  # noqa: E731
        for i, st in enumerate(self.steps):
            o, c = _step(st, self.B, buf(st.src), self.carry[i], self.wp[i], self.bias[i],
                         None if st.res is None else buf(st.res))
            outs.append(o)
            self.carry[i] = c
        return outs[-1]

    def buffers(self):
        """{oracle state key: (B, Cin, P_ref)} from the carries."""
        out = {}
        for st, c in zip(self.steps, self.carry):
            if c is None:
                continue
            v = c.reshape(self.B, -1, st.buffer_shape[1])
            if st.kind == CO.PACK_FWD_STRIDED:
                assert v.shape[1] == st.buffer_shape[2] + 1
                v = v[:, 1:]
            assert tuple(v.shape[1:]) == (st.buffer_shape[2], st.buffer_shape[1])
            assert st.buffer == st.name + ".pad_buffer"
            out[st.name] = v.transpose(1, 2)
        return out


def _close(a, b, name):
    e = float((a - b).norm() / (b.norm() + 1e-300))
    assert a.shape == b.shape and e <= 1e-6, (name, tuple(a.shape), tuple(b.shape), e)


def _generator(pqc, gp, seed):
    if pqc:
        from models.autoencoder.AudioDec import StreamGenerator
    else:
        from models.autoencoder_without_PQC.AudioDec import StreamGenerator
    torch.manual_seed(seed)
    return StreamGenerator(**gp).eval()


@pytest.mark.parametrize("pqc,gp,B,chunk", [(True, GOLDEN_W, 2, 600), (True, FULL_W, 1, 300), (False, NOPQC_W, 1, 600)],
                         ids=["golden_width", "full_width", "without_pqc"])
def test_plan_executes_to_the_oracle(pqc, gp, B, chunk):
    G = _generator(pqc, gp, 11)
    pl = SO.plan(G, B, chunk)
    sd = {k: v.detach().double() for k, v in G.state_dict().items()}
    geo = R.generator_geometry(**gp)
    assert pl.frames == chunk // 300 and pl.pqc == pqc and pl.out_samples == chunk
    # every carried layer of the generator is in the plan exactly once
    keys = [st.buffer for st in pl.encode + pl.decode if st.buffer]
    want = [k for k in G.state_dict() if k.endswith("pad_buffer")
            and (pqc or not k.startswith(("projector", "decoder.conv1")))]
    assert sorted(keys) == sorted(want)
    enc, dec = _Executor(pl.encode, sd, B), _Executor(pl.decode, sd, B)
    S = {}
    g = torch.Generator().manual_seed(4)
    for hop in range(3):
        x = 0.1 * torch.randn(B, 1, chunk, generator=g, dtype=torch.float64)
        z = enc.run(x.transpose(1, 2)).reshape(B, pl.frames, pl.enc_channels)
        zr = R.stream_encode(sd, S, x, geo, project=pqc)
        _close(z.transpose(1, 2), zr, f"z.{hop}")
        zq = torch.randn(B, pl.frames, pl.dec_in_channels, generator=g, dtype=torch.float64)
        y = dec.run(zq).reshape(B, pl.out_samples, pl.out_channels)
        _close(y.transpose(1, 2), R.stream_decode(sd, S, zq, geo, pqc=pqc), f"y.{hop}")
        bufs = {**enc.buffers(), **dec.buffers()}
        assert set(bufs) == set(S)
        for k, v in bufs.items():
            _close(v, S[k], f"carry {k} hop {hop}")


def test_plan_steps_describe_the_shipped_generator():
    pl = SO.plan(_generator(True, FULL_W, 1), 1, 300)
    assert len(pl.encode) == 1 + 4 * 7 + 1 and len(pl.decode) == 1 + 4 * 7 + 1
    deep = next(st for st in pl.encode if st.name == "encoder.conv_blocks.3.conv")
    assert (deep.kind, deep.T, deep.C, deep.N, deep.K, deep.carry_shape) == (CO.PACK_FWD_STRIDED, 1, 1280, 512, 3,
                                                                           (1, 2, 1280))
    up = next(st for st in pl.decode if st.name == "decoder.conv_blocks.0.conv")
    assert (up.kind, up.T, up.C, up.N, up.K, up.bias_period, up.carry_shape) == (CO.PACK_CONVT, 1, 512, 5 * 256, 2,
                                                                               256, (1, 1, 512))
    ru = next(i for i, st in enumerate(pl.encode) if st.name == "encoder.conv_blocks.0.res_units.2.conv1")
    assert pl.encode[ru].in_elu == 1 and pl.encode[ru].dil == 9 and pl.encode[ru].carry_shape == (1, 54, 32)
    assert pl.encode[ru + 1].K == 1 and pl.encode[ru + 1].src == ru and pl.encode[ru + 1].res == pl.encode[ru].src
    assert pl.encode[-1].out_float and pl.decode[-1].out_float and not pl.encode[0].out_float


def test_plan_rejects_what_a_session_cannot_run():
    from layers.conv_layer import CausalConv1d
    from models.autoencoder.AudioDec import Generator
    with pytest.raises(NotImplementedError, match="causal"):
        SO.plan(Generator(mode="noncausal", **GOLDEN_W), 1, 600)
    G = _generator(True, GOLDEN_W, 1)
    with pytest.raises(NotImplementedError, match="multiple of the encoder's total stride"):
        SO.plan(G, 1, 601)
    SO.plan(G, 1, 300)
    G.encoder.conv_blocks[1].res_units[0].conv1 = CausalConv1d(8, 8, 7, groups=2)
    with pytest.raises(NotImplementedError, match="grouped"):
        SO.plan(G, 1, 600)
    G = _generator(True, GOLDEN_W, 1)
    G.encoder.conv_blocks[0].conv = CausalConv1d(4, 8, kernel_size=7, stride=3)
    with pytest.raises(NotImplementedError, match="2 \\* stride"):
        SO.plan(G, 1, 600)
    from models.autoencoder.AudioDec import StreamGenerator
    with pytest.raises(NotImplementedError, match="conv1d_bn"):
        SO.plan(StreamGenerator(projector="conv1d_bn", **GOLDEN_W), 1, 600)


def test_conv_step_wrapper_refuses_cpu_tensors():
    from sel import SelError
    d = CO.ConvDesc(4, 4, 8, 8, 3, 1, 2, CO.PAD_ZERO, 0, 0)
    with pytest.raises(SelError, match="device"):
        SO.conv_step(d, torch.zeros(1, 2, 8), torch.zeros(4, 8), torch.zeros(8, 3, 8))


def test_conv_step_validates_arguments_before_device_work():
    from sel import _lib
    lib = _lib.load()
    p = lambda v: ctypes.c_void_p(v)  # noqa: E731  (never dereferenced: every call below is refused first)
    inp, wp, out, ca, co = p(0x10000), p(0x20000), p(0x30000), p(0x40000), p(0x50000)

    def call(d, carry, carry_out, i=inp, w=wp, o=out):
        rc = lib.sel_conv_step(ctypes.byref(d), CO.F32, CO.F32, carry, i, w, None, None, o, carry_out, None)
        return rc, lib.sel_last_error().decode()

    good = CO.ConvDesc(12, 4, 8, 8, 7, 1, 6, CO.PAD_ZERO, 0, 0)
    rc, msg = call(good, ca, ca)
    assert rc == -1 and "alias" in msg, (rc, msg)
    rc, msg = call(good.with_(pad=5), ca, co)
    assert rc == -1 and "(K-1)*dil" in msg, (rc, msg)
    rc, msg = call(good.with_(pad=5), None, None, None, None, None)
    assert rc == -1 and "(K-1)*dil" in msg, (rc, msg)
    rc, msg = call(good.with_(pad_mode=CO.PAD_REPLICATE), ca, co)
    assert rc == -1 and "SEL_PAD_ZERO" in msg, (rc, msg)
    rc, msg = call(good.with_(rows=10), ca, co)
    assert rc == -1 and "multiple of T" in msg, (rc, msg)
    rc, msg = call(good, None, co)
    assert rc == -1 and "needs carry" in msg, (rc, msg)
    rc, msg = call(good, None, None, None, None, None)
    assert rc == -1, (rc, msg)
    assert lib.sel_stream_commit(None, 0, None) == -1
    job = (SO.CopyJob * 1)(SO.CopyJob(0x10000, 0x10000, 16))
    assert lib.sel_stream_commit(ctypes.cast(job, ctypes.c_void_p), 1, None) == -1
