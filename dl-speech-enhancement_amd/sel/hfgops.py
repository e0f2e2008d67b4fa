"""Inference ops of the HiFi-GAN vocoder generator over libsel.so's grouped
LeakyReLU-fused conv primitive (csrc/hifigan.hip, include/sel.h sel_hfg_conv_desc).

Reference semantics (file:line under the reference root):
* Generator / StreamGenerator   models/vocoder/HiFiGAN.py:28-305
* HiFiGANResidualBlock          models/vocoder/modules/residual_block.py:23-106
* MultiReceptiveField / MultiGroupConv1d   models/vocoder/modules/multi_fusion.py:23-141

Activations are channels-last (B, T, C) as in sel.convops.  Every LeakyReLU,
residual add, tanh, the MultiReceptiveField average and MultiGroupConv1d's
channel repeat run inside the primitive's prologue / epilogue.

Weight norm: the reference wraps the inner nn.Conv1d / nn.ConvTranspose1d with
torch.nn.utils.weight_norm, whose hook recomputes ``.weight`` only when the
inner module is called.  This package never calls it, so ``weight`` is stale
after load_state_dict; the packs here are built from g * v / ||v|| (norm over
all dims but 0) and cached by the parameters' versions.

Training the vocoder (dgrad, grouped wgrad, weight-norm backward) is not built:
``require_inference`` raises when a gradient would be needed.
"""
import ctypes
import threading
import weakref

import torch
import torch.nn.functional as F

from . import _lib as L
from . import convops as CO


class HfgDesc(ctypes.Structure):
    """include/sel.h sel_hfg_conv_desc"""
    _fields_ = [("rows", ctypes.c_int64), ("T", ctypes.c_int32), ("T_out", ctypes.c_int32),
                ("C", ctypes.c_int32), ("N", ctypes.c_int32), ("K", ctypes.c_int32), ("dil", ctypes.c_int32),
                ("pad", ctypes.c_int32), ("pad_mode", ctypes.c_int32), ("groups", ctypes.c_int32),
                ("in_group_stride", ctypes.c_int32), ("res_group_stride", ctypes.c_int32),
                ("bias_period", ctypes.c_int32), ("act_skip", ctypes.c_int32), ("tanh_out", ctypes.c_int32),
                ("accumulate", ctypes.c_int32), ("act_slope", ctypes.c_float), ("out_scale", ctypes.c_float)]


def make_desc(rows, T, C, N, K, dil=1, pad=0, pad_mode=CO.PAD_ZERO, groups=1, shared_in=False, shared_res=False,
              bias_period=0, act_skip=0, tanh=False, accumulate=False, slope=1.0, scale=1.0, T_out=0):
    return HfgDesc(rows, T, T_out, C, N, K, dil, pad, pad_mode, groups, 0 if shared_in else C // groups,
                   0 if shared_res else N // groups, bias_period, act_skip, int(tanh), int(accumulate), slope, scale)


def require_inference(module, x):
    """The vocoder is inference-only: no silent torch fallback for a training step."""
    if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in module.parameters())):
        raise NotImplementedError(
            "the HiFi-GAN vocoder generator is built for inference only: call it under torch.no_grad() "
            "(or with requires_grad False on the input and every parameter); vocoder training is not implemented")


def slope_of(act):
    """negative slope of the module's activation (the kernels fuse LeakyReLU only)."""
    if not isinstance(act, torch.nn.LeakyReLU):
        raise NotImplementedError(f"the vocoder kernels fuse LeakyReLU only, not {type(act).__name__}")
    return float(act.negative_slope)


# ---- weights: weight-norm fold + pack cache -------------------------------------------------
def effective_weight(m):
    """fp32 weight of an nn.Conv1d / nn.ConvTranspose1d, weight-normed or not."""
    g, v = getattr(m, "weight_g", None), getattr(m, "weight_v", None)
    if g is None or v is None:
        return m.weight.detach()
    g, v = g.detach(), v.detach()
    return v * (g / v.norm(2, dim=tuple(range(1, v.dim())), keepdim=True))


def _signature(m):
    ps = [p for p in (getattr(m, "weight_g", None), getattr(m, "weight_v", None)) if p is not None]
    if len(ps) != 2:
        ps = [m.weight]
    return tuple((p.data_ptr(), p._version, p.device) for p in ps)


_PACKS = weakref.WeakKeyDictionary()   # inner conv module -> {(kind, stride, dtype): (signature, packed)}
_PACK_LOCK = threading.Lock()


def packed(m, kind, stride, dtype):
    """Packed Wp (dtype) of the inner conv module m, refreshed when its
    parameters change (version counters / storage); code that writes a weight
    through ``.data`` must call ``invalidate()``."""
    sig = _signature(m)
    key = (kind, stride, dtype)
    with _PACK_LOCK:
        slot = _PACKS.setdefault(m, {})
        hit = slot.get(key)
        if hit is not None and hit[0] == sig:
            return hit[1]
        w = effective_weight(m)
        L.need_device(w)
        wp = CO.pack(kind, w, stride, dtype)
        slot[key] = (sig, wp)
        return wp


def invalidate():
    with _PACK_LOCK:
        _PACKS.clear()


# ---- the primitive -----------------------------------------------------------------------------
KERNEL_NAMES = {0: "k_hfg_valu", 1: "k_hfg_mfma<1>", 2: "k_hfg_mfma<2>", 4: "k_hfg_mfma<4>"}


def _meta(desc, x, wp, res, out):
    """(kernel tag, algorithmic HBM bytes, flops) of one launch: input, weights,
    res and a previous out read once, out written once."""
    nbytes = x.numel() * x.element_size() + wp.numel() * wp.element_size() + out.numel() * out.element_size()
    if res is not None:
        nbytes += res.numel() * res.element_size()
    if desc.accumulate:
        nbytes += out.numel() * out.element_size()
    flops = 2.0 * desc.rows * desc.N * desc.K * (desc.C // desc.groups)
    kid = L.lib().sel_hfg_conv_kernel(ctypes.byref(desc), CO._code(x.dtype), CO._code(out.dtype))
    return f"{KERNEL_NAMES.get(kid, 'k_hfg')}[{x.dtype}]", nbytes, flops


def prim(desc, x, wp, bias=None, res=None, out=None, out_dtype=None):
    """sel_hfg_conv_fwd; x (B, T, C or C/G) contiguous, returns (rows, N)."""
    L.need_device(x, wp, bias, res, out)
    out_dtype = out_dtype or (out.dtype if out is not None else x.dtype)
    cin = desc.C if desc.in_group_stride else desc.C // desc.groups
    t_out = desc.T_out or desc.T
    assert x.is_contiguous() and x.numel() == desc.rows // t_out * desc.T * cin and wp.dtype == x.dtype
    if out is None:
        assert not desc.accumulate
        out = torch.empty((desc.rows, desc.N), dtype=out_dtype, device=x.device)
    else:
        assert out.is_contiguous() and out.numel() == desc.rows * desc.N and out.dtype == out_dtype
    if res is not None:
        nres = desc.N if desc.res_group_stride else desc.N // desc.groups
        assert res.is_contiguous() and res.dtype == out_dtype and res.numel() == desc.rows * nres
    if bias is not None:
        assert bias.dtype == torch.float32 and bias.is_contiguous()
    L.call("sel_hfg_conv_fwd", ctypes.byref(desc), CO._code(x.dtype), CO._code(out_dtype), L.ptr(x), L.ptr(wp),
           L.ptr(bias), L.ptr(res), L.ptr(out), L.stream(), meta=lambda: _meta(desc, x, wp, res, out))
    return out


def _bias(m):
    return m.bias.detach() if m.bias is not None else None


def enter(x):
    """(B, C, T) module input -> contiguous channels-last (B, T, C) in the compute dtype."""
    L.need_device(x)
    xc = CO.to_cl(x)
    dt = CO.compute_dtype()
    return xc if xc.dtype == dt else CO.cast(xc, dt)


def causal(x, layer, slope=1.0, res=None, shared_in=False, shared_res=False, tanh=False, scale=1.0, out=None,
           out_dtype=None):
    """CausalConv1d.forward (conv_layer.py:139-142) of act(x): left zero pad
    (K-1)*dil in the kernel.  x (B, T, Cin or Cin/G); `out` given: accumulate
    scale * result into it."""
    c = layer.conv
    B, T = x.shape[0], x.shape[1]
    G = c.groups
    d = make_desc(B * T, T, c.in_channels, c.out_channels, c.kernel_size[0], c.dilation[0], layer.pad_length,
                  CO.PAD_ZERO, G, shared_in, shared_res, c.out_channels if c.bias is not None else 0,
                  slope=slope, tanh=tanh, scale=scale, accumulate=out is not None)
    wp = packed(c, CO.PACK_FWD, 1, x.dtype)
    return prim(d, x, wp, _bias(c), res, out, out_dtype).view(B, T, c.out_channels)


def causal_stream(x, layer, slope=1.0, res=None, scale=1.0, out=None, tanh=False, out_dtype=None):
    """CausalConv1d.inference (conv_layer.py:144-147) fed with act(x), as
    HiFiGAN.py:289-295 and residual_block.py:100-106 call it: the valid conv of
    cat(pad_buffer, act(x)); pad_buffer keeps the ACTIVATED tail (it is part of
    the state_dict).  The kernel takes the buffer rows as they are (act_skip)
    and activates the new rows in its prologue."""
    c = layer.conv
    B, T = x.shape[0], x.shape[1]
    P = layer.pad_length
    buf = layer.pad_buffer.transpose(1, 2).expand(B, -1, -1).to(x.dtype)
    xb = torch.cat((buf, x), 1)
    d = make_desc(B * T, T + P, c.in_channels, c.out_channels, c.kernel_size[0], c.dilation[0], 0, CO.PAD_ZERO,
                  c.groups, bias_period=c.out_channels if c.bias is not None else 0, act_skip=P, slope=slope,
                  scale=scale, accumulate=out is not None, tanh=tanh, T_out=T)
    y = prim(d, xb, packed(c, CO.PACK_FWD, 1, x.dtype), _bias(c), res, out, out_dtype).view(B, T, c.out_channels)
    if P:
        # the buffer-sized tail of act(x) (not an activation-sized pass)
        tail = F.leaky_relu(x[:, max(T - P, 0):], slope) if slope != 1.0 else x[:, max(T - P, 0):]
        if T < P:
            tail = torch.cat((buf[:, T:], tail), 1)
        layer.pad_buffer = tail.transpose(1, 2).float().contiguous()
    else:
        layer.pad_buffer = xb.transpose(1, 2).float().contiguous()
    return y


def _convt_desc(layer, rows, T, T_out, pad, act_skip, slope):
    dc = layer.deconv
    s = layer.stride
    return make_desc(rows, T, dc.in_channels, s * dc.out_channels, 2, 1, pad, CO.PAD_REPLICATE,
                     bias_period=dc.out_channels if dc.bias is not None else 0, act_skip=act_skip, slope=slope,
                     T_out=T_out)


def upsample(x, layer, slope):
    """CausalConvTranspose1d.forward (conv_layer.py:180-183) of act(x), k = 2s: a
    2-tap conv with the replicate pad in the kernel producing the s output
    phases of each input step; (B, T, Cin) -> (B, T*s, Cout)."""
    B, T = x.shape[0], x.shape[1]
    dc, s = layer.deconv, layer.stride
    assert layer.kernel_size == 2 * s
    d = _convt_desc(layer, B * T, T, 0, 1, 0, slope)
    return prim(d, x, packed(dc, CO.PACK_CONVT, s, x.dtype), _bias(dc)).view(B, T * s, dc.out_channels)


def upsample_stream(x, layer, slope):
    """CausalConvTranspose1d.inference (conv_layer.py:185-188) fed with act(x):
    output step t reads rows t, t + 1 of cat(pad_buffer, act(x))."""
    B, T = x.shape[0], x.shape[1]
    dc, s = layer.deconv, layer.stride
    assert layer.kernel_size == 2 * s
    buf = layer.pad_buffer.transpose(1, 2).expand(B, -1, -1).to(x.dtype)
    xb = torch.cat((buf, x), 1)
    d = _convt_desc(layer, B * T, T + 1, T, 0, 1, slope)
    y = prim(d, xb, packed(dc, CO.PACK_CONVT, s, x.dtype), _bias(dc)).view(B, T * s, dc.out_channels)
    layer.pad_buffer = F.leaky_relu(x[:, T - 1:], slope).transpose(1, 2).float().contiguous()
    return y


def pointwise(x, conv):
    """bias-free / biased 1x1 conv (Conv1d1x1, conv_layer.py:19-23), weight-norm aware."""
    B, T = x.shape[0], x.shape[1]
    d = make_desc(B * T, T, conv.in_channels, conv.out_channels, 1,
                  bias_period=conv.out_channels if conv.bias is not None else 0)
    return prim(d, x, packed(conv, CO.PACK_FWD, 1, x.dtype), _bias(conv)).view(B, T, conv.out_channels)


TUNE_RESLAYER = 71   # sel_tune key: 1 = two launches per layer, 2 = fused wherever the shape allows
ERR_UNSUPPORTED = -3


def reslayer(x, l1, l2, slope, shared=False, scale=1.0, out=None):
    """One residual layer x + conv2(act(conv1(act(x)))) in one launch
    (sel_hfg_reslayer_fwd), or None where the library keeps two launches."""
    c1, c2 = l1.conv, l2.conv
    if x.dtype != torch.bfloat16 or c2.kernel_size != c1.kernel_size or c2.dilation[0] != 1 \
            or c2.groups != c1.groups or (c1.bias is None) != (c2.bias is None):
        return None
    B, T = x.shape[0], x.shape[1]
    d = make_desc(B * T, T, c1.in_channels, c1.out_channels, c1.kernel_size[0], c1.dilation[0], l1.pad_length,
                  CO.PAD_ZERO, c1.groups, shared, shared, c1.out_channels if c1.bias is not None else 0,
                  slope=slope, scale=scale, accumulate=out is not None)
    w1, w2 = packed(c1, CO.PACK_FWD, 1, x.dtype), packed(c2, CO.PACK_FWD, 1, x.dtype)
    L.need_device(x, out)
    assert x.is_contiguous() and x.numel() == B * T * (d.C // d.groups if shared else d.C)
    y = out if out is not None else torch.empty((B, T, d.N), dtype=x.dtype, device=x.device)
    assert y.is_contiguous() and y.dtype == x.dtype and y.numel() == B * T * d.N
    fn = L.lib().sel_hfg_reslayer_fwd
    args = (ctypes.byref(d), CO.BF16, L.ptr(x), L.ptr(w1), L.ptr(_bias(c1)), L.ptr(w2), L.ptr(_bias(c2)), L.ptr(y),
            L.stream())
    t = L.TIMER
    if t is not None and "sel_hfg_reslayer_fwd" in t.names:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = fn(*args)
        e1.record()
        if rc == 0:
            es = x.element_size()
            nb = (2 * x.numel() + (1 + int(out is not None)) * y.numel() + w1.numel() + w2.numel()) * es
            t.add("sel_hfg_reslayer_fwd",
                  (f"k_hfg_reslayer<{d.C // d.groups}, {d.K}>", nb, 4.0 * d.rows * d.N * d.K * (d.C // d.groups)),
                  e0, e1)
    else:
        rc = fn(*args)
    if rc == ERR_UNSUPPORTED:
        return None
    L.check(rc, "sel_hfg_reslayer_fwd")
    return y.view(B, T, d.N)


def resblock(x, block, slope, stream=False, shared_first=False, scale=1.0, out=None):
    """HiFiGANResidualBlock.forward / .inference (residual_block.py:83-106) on
    channels-last x: per layer x = conv2(act(conv1(act(x)))) + x with both
    activations in the prologues and the add in the epilogue.  shared_first:
    x has C/G channels every group reads (MultiGroupConv1d's repeat).  scale /
    out: the last layer writes scale * x, accumulated into `out` when given
    (the MultiReceptiveField average)."""
    n = block.num_layer
    for idx in range(n):
        last = idx == n - 1
        sh = shared_first and idx == 0
        kw = dict(scale=scale, out=out) if last else {}
        if stream:
            if block.use_additional_convs:
                xt = causal_stream(x, block.convs1[idx], slope)
                x = causal_stream(xt, block.convs2[idx], slope, res=x, **kw)
            else:
                x = causal_stream(x, block.convs1[idx], slope, res=x, **kw)
        elif block.use_additional_convs:
            y = reslayer(x, block.convs1[idx], block.convs2[idx], slope, sh, **kw)
            if y is None:
                xt = causal(x, block.convs1[idx], slope, shared_in=sh)
                y = causal(xt, block.convs2[idx], slope, res=x, shared_res=sh, **kw)
            x = y
        else:
            x = causal(x, block.convs1[idx], slope, res=x, shared_in=sh, shared_res=sh, **kw)
    return x


def mrf(x, blocks, slope, stream=False):
    """MultiReceptiveField (multi_fusion.py:56-79): mean of the blocks' outputs;
    each block's last epilogue adds its share into one buffer."""
    nb = len(blocks)
    out = None
    for blk in blocks:
        y = resblock(x, blk, slope, stream=stream, scale=1.0 / nb, out=out)
        out = y if out is None else out
    return out
