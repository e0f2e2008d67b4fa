"""Ops of the HiFi-GAN vocoder generator over libsel.so's grouped LeakyReLU-fused
conv primitive (csrc/hifigan.hip, include/sel.h sel_hfg_conv_desc) and its
backward (csrc/hifigan_bwd.hip).

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

Training (``generator_train``): the whole generator is ONE autograd node.  Its
forward issues the launches of the no-grad forward (two launches per residual
layer) while a tape records, per conv, the descriptor, the input x and -- for
the tanh output conv only -- the fp32 output.  Its backward walks the tape in
reverse with sel_hfg_conv_bwd_data / sel_hfg_conv_wgrad: LeakyReLU', tanh', the
scales, the skip adds, the MultiReceptiveField fan-in and MultiGroupConv1d's
group sum all run in those kernels' prologues / epilogues, so no
activation-sized elementwise pass and no autograd in-place write exists.  Weight
norm stays in torch on weight-sized tensors: the node's weight inputs are
g * v / ||v|| computed with grad enabled, and its packs are rebuilt from them on
every call (the version-keyed cache below serves inference only: fused Adam does
not bump versions).  Without ``Generator.enable_training()``,
``require_inference`` raises when a gradient would be needed.
"""
import ctypes
import threading
import weakref

import torch
import torch.nn.functional as F
from torch.optim.optimizer import register_optimizer_step_post_hook

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


def needs_grad(module, x):
    return torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in module.parameters()))


def require_inference(module, x):
    """Inference unless training was enabled: no silent torch fallback for a training step."""
    if needs_grad(module, x):
        raise NotImplementedError(
            "the HiFi-GAN vocoder generator is built for inference only: call it under torch.no_grad() "
            "(or with requires_grad False on the input and every parameter), or opt in to the training path "
            "with enable_training()")


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


_TAPE = threading.local()   # .tape: the recorder of a training forward in progress (further down)
_PACKS = weakref.WeakKeyDictionary()   # inner conv module -> {(kind, stride, dtype): (signature, packed)}
_PACK_LOCK = threading.Lock()


def packed(m, kind, stride, dtype):
    """Packed Wp (dtype) of the inner conv module m, refreshed when its
    parameters change (version counters / storage); code that writes a weight
    through ``.data`` must call ``invalidate()``."""
    tape = getattr(_TAPE, "tape", None)
    if tape is not None:
        return tape.pack(m, kind, stride, dtype)
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


def _optimizer_stepped(optimizer, args, kwargs):
    """Global torch.optim post-step hook (as sel.convops has for its packs): a
    fused Adam writes the parameters without bumping their version counters, so
    the inference packs of every conv the optimizer updated are dropped -- the
    no-grad forward of the vocoder trainer's discriminator step follows the
    generator update directly."""
    if not _PACKS:
        return
    stepped = {id(p) for g in optimizer.param_groups for p in g["params"] if p.grad is not None}
    with _PACK_LOCK:
        for m in [m for m in _PACKS if any(id(p) in stepped for p in m.parameters(recurse=False))]:
            del _PACKS[m]


register_optimizer_step_post_hook(_optimizer_stepped)


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
    tape = getattr(_TAPE, "tape", None)
    if tape is not None:
        tape.record(desc, x, wp, res, out)
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
    if getattr(_TAPE, "tape", None) is not None:
        return None   # the training forward stores h: two launches, bit-identical to the fused layer
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


# ---- backward of the primitive ---------------------------------------------------------------
TUNE_WGRAD_SPLIT = 72   # sel_tune key: > 0 forces the row-split count of sel_hfg_conv_wgrad
BWD_DATA_NAMES = {0: "k_bwd_data_valu", 1: "k_bwd_data_mfma<1>", 2: "k_bwd_data_mfma<2>", 4: "k_bwd_data_mfma<4>"}
WGRAD_NAMES = {0: "k_wgrad_valu", 1: "k_wgrad_mfma"}


def dgrad_pack(wp, groups):
    """Wp[N][K][C/G] -> Wd[G][C/G][K][N/G]: the same values with the reduction axis
    of the data gradient contiguous (a weight-sized permute, no rounding)."""
    N, K, Cg = wp.shape
    return wp.view(groups, N // groups, K, Cg).permute(0, 3, 2, 1).contiguous()


def _nbytes(*ts):
    return sum(t.numel() * t.element_size() for t in ts if t is not None)


def bwd_data(desc, gout, wd, x=None, out=None, gskip=None, skip_scale=0.0, gin=None, dtype=None):
    """sel_hfg_conv_bwd_data; returns gin (B, T, C or C/G), accumulated into the
    given `gin` when desc.accumulate."""
    L.need_device(gout, wd, x, out, gskip, gin)
    dtype = dtype or wd.dtype
    cin = desc.C if desc.in_group_stride else desc.C // desc.groups
    B = desc.rows // desc.T
    assert gout.is_contiguous() and gout.numel() == desc.rows * desc.N and wd.dtype == dtype and wd.is_contiguous()
    assert x is None or (x.is_contiguous() and x.dtype == dtype and x.numel() == desc.rows * cin)
    assert out is None or (out.is_contiguous() and out.dtype == gout.dtype and out.numel() == gout.numel())
    assert gskip is None or (gskip.is_contiguous() and gskip.dtype == dtype and gskip.numel() == desc.rows * desc.C)
    if gin is None:
        assert not desc.accumulate
        gin = torch.empty((B, desc.T, cin), dtype=dtype, device=gout.device)
    else:
        assert gin.is_contiguous() and gin.dtype == dtype and gin.numel() == desc.rows * cin

    def meta():
        kid = L.lib().sel_hfg_conv_bwd_kernel(ctypes.byref(desc), CO._code(dtype), CO._code(gout.dtype), 0)
        nb = _nbytes(gout, wd, x if desc.act_slope != 1.0 else None, out if desc.tanh_out else None, gskip, gin,
                     gin if desc.accumulate else None)
        return (f"{BWD_DATA_NAMES.get(kid, 'k_bwd_data')}[{dtype}]", nb,
                2.0 * desc.rows * desc.N * desc.K * (desc.C // desc.groups))

    L.call("sel_hfg_conv_bwd_data", ctypes.byref(desc), CO._code(dtype), CO._code(gout.dtype), L.ptr(gout), L.ptr(out),
           L.ptr(x), L.ptr(wd), L.ptr(gskip), float(skip_scale), L.ptr(gin), L.stream(), meta=meta)
    return gin


def wgrad(desc, gout, x, out=None):
    """sel_hfg_conv_wgrad; returns (gWp fp32 (N, K, C/G), gbias fp32 (bias_period,) or None)."""
    L.need_device(gout, x, out)
    cin = desc.C if desc.in_group_stride else desc.C // desc.groups
    assert gout.is_contiguous() and gout.numel() == desc.rows * desc.N
    assert x.is_contiguous() and x.numel() == desc.rows * cin
    assert out is None or (out.is_contiguous() and out.dtype == gout.dtype and out.numel() == gout.numel())
    codes = (CO._code(x.dtype), CO._code(gout.dtype))
    nbytes = L.lib().sel_hfg_conv_wgrad_workspace(ctypes.byref(desc), *codes)
    ws = L.workspace(nbytes, x.device)
    gwp = torch.empty((desc.N, desc.K, desc.C // desc.groups), dtype=torch.float32, device=x.device)
    gb = torch.empty((desc.bias_period,), dtype=torch.float32, device=x.device) if desc.bias_period else None

    def meta():
        kid = L.lib().sel_hfg_conv_bwd_kernel(ctypes.byref(desc), *codes, 1)
        return (f"{WGRAD_NAMES.get(kid, 'k_wgrad')}[{x.dtype}]",
                _nbytes(gout, x, out if desc.tanh_out else None, gwp, gb) + 2 * nbytes,
                2.0 * desc.rows * desc.N * desc.K * (desc.C // desc.groups))

    L.call("sel_hfg_conv_wgrad", ctypes.byref(desc), *codes, L.ptr(gout), L.ptr(out), L.ptr(x), L.ptr(gwp), L.ptr(gb),
           L.ptr(ws), nbytes, L.stream(), meta=meta)
    return gwp, gb


# ---- training: one autograd node per generator -----------------------------------------------
def effective_weight_train(m):
    """effective_weight with grad enabled: torch's weight-norm formula on the
    weight-sized parameters (g * v / ||v||, norm over all dims but 0), or the
    plain weight after remove_weight_norm()."""
    g, v = getattr(m, "weight_g", None), getattr(m, "weight_v", None)
    if g is None or v is None:
        return m.weight
    return v * (g / v.norm(2, dim=tuple(range(1, v.dim())), keepdim=True))


def inner_convs(module):
    """the nn.Conv1d / nn.ConvTranspose1d modules of a generator, in module order"""
    return [m for m in module.modules() if isinstance(m, (torch.nn.Conv1d, torch.nn.ConvTranspose1d))]


class _Record:
    __slots__ = ("desc", "x", "out", "okey", "reskey", "mod", "wd", "kind", "stride")


class _Tape:
    """Recorder of one training forward: per launch the descriptor, the input x,
    the fp32 output of a tanh conv, and the identities (storage addresses; every
    conv output stays alive as a later conv's saved x) that tie the launches into
    a dataflow graph for the reverse walk."""

    def __init__(self, weights):
        self.weights = weights    # inner conv module -> fp32 effective weight
        self.packs = {}           # (module, kind, stride, dtype) -> (wp, wd)
        self.by_wp = {}           # wp address -> (module, kind, stride, wd)
        self.records = []

    def pack(self, m, kind, stride, dtype):
        key = (m, kind, stride, dtype)
        hit = self.packs.get(key)
        if hit is None:
            wp = CO.pack(kind, self.weights[m], stride, dtype)
            groups = m.groups if kind == CO.PACK_FWD else 1
            hit = self.packs[key] = (wp, dgrad_pack(wp, groups))
            self.by_wp[wp.data_ptr()] = (m, kind, stride, hit[1])
        return hit[0]

    def record(self, desc, x, wp, res, out):
        r = _Record()
        r.desc, r.x, r.okey = desc, x, out.data_ptr()
        r.out = out if desc.tanh_out else None
        r.reskey = res.data_ptr() if res is not None else None
        r.mod, r.kind, r.stride, r.wd = self.by_wp[wp.data_ptr()]
        self.records.append(r)


def _copy_desc(d, **kw):
    c = HfgDesc.from_buffer_copy(d)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def tape_backward(tape, gy, x0, need_x0):
    """Reverse walk of a training forward.  gy: gradient of the last launch's
    output, (rows, N).  Returns ({inner conv module: (gW torch layout, gbias)},
    gradient of x0 or None).  A gradient buffer is keyed by the forward tensor it
    belongs to: every launch that read that tensor accumulates into it in its own
    epilogue, and every launch that accumulated into one output buffer reads the
    same gout."""
    grads = {tape.records[-1].okey: gy}
    gws = {}
    pending = None   # (address of res, gout, out_scale): consumed by the launch that read the same tensor as x
    x0key = x0.data_ptr()
    for r in reversed(tape.records):
        d = r.desc
        gout = grads[r.okey] if d.accumulate else grads.pop(r.okey)
        gwp, gb = wgrad(d, gout, r.x, r.out)
        w = tape.weights[r.mod]
        gw = CO.unpack(r.kind, gwp, tuple(w.shape), r.stride)
        assert r.mod not in gws
        gws[r.mod] = (gw, gb)
        if r.reskey is not None:
            assert pending is None, "a residual is always the input of the layer it closes"
            pending = (r.reskey, gout, d.out_scale)
        xkey = r.x.data_ptr()
        if xkey == x0key and not need_x0:
            continue
        gskip, sscale = None, 0.0
        if pending is not None and pending[0] == xkey:   # else: conv2 of a layer, whose conv1 comes next
            _, gskip, sscale = pending
            pending = None
        gin = grads.get(xkey)
        bd = _copy_desc(d, accumulate=int(gin is not None))
        if gin is None:
            gin = torch.empty(r.x.shape, dtype=r.x.dtype, device=r.x.device)
        grads[xkey] = bwd_data(bd, gout, r.wd, r.x, r.out, gskip, sscale, gin)
    assert pending is None
    return gws, grads.get(x0key)


class _GeneratorFn(torch.autograd.Function):
    """forward(run, mods, c, *tensors): run(x0) is the generator's launch sequence
    on the channels-last input; tensors = per inner conv its effective weight
    and bias (or None), in the order of mods."""

    @staticmethod
    def forward(ctx, run, mods, c, *tensors):
        weights = {m: tensors[2 * i].detach() for i, m in enumerate(mods)}
        tape = _Tape(weights)
        x0 = enter(c)
        _TAPE.tape = tape
        try:
            y = run(x0)            # (B, T, out_channels) fp32
        finally:
            _TAPE.tape = None
        tape.packs, tape.by_wp = {}, {}   # the forward packs are not needed again (Wd lives in the records)
        ctx.tape, ctx.x0, ctx.mods = tape, x0, mods
        ctx.c_dtype = c.dtype
        return y.transpose(1, 2)

    @staticmethod
    def backward(ctx, g):
        tape, mods = ctx.tape, ctx.mods
        last = tape.records[-1].desc
        gy = g.transpose(1, 2).contiguous().view(last.rows, last.N)
        gws, gx0 = tape_backward(tape, gy, ctx.x0, ctx.needs_input_grad[2])
        ctx.tape = None
        out = []
        for i, m in enumerate(mods):
            gw, gb = gws.get(m, (None, None))
            out += [gw if ctx.needs_input_grad[3 + 2 * i] else None, gb if ctx.needs_input_grad[4 + 2 * i] else None]
        gc = gx0.transpose(1, 2).to(ctx.c_dtype) if gx0 is not None else None
        return (None, None, gc, *out)


def generator_train(module, run, c):
    """Differentiable run(enter(c)) for a generator `module` whose convs all go
    through this file's primitive: gradients reach c and every parameter."""
    L.need_device(c)
    mods = inner_convs(module)
    tensors = []
    for m in mods:
        tensors += [effective_weight_train(m), m.bias]
    return _GeneratorFn.apply(run, mods, c, *tensors)
