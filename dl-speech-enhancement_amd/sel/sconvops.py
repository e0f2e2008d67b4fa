"""Autograd ops over the channels-last 2-D conv kernels of libsel.so (sconv2d.hip):
the UnivNet spectral discriminator (models/vocoder/modules/discriminator.py:450-580
of the reference).

A spectral sub-discriminator is |STFT| followed by six weight-normalised Conv2d
with LeakyReLU; like sel.dconvops.ChainFn it runs as ONE autograd Function
(SpecChainFn) whose forward keeps every layer's output in a channels-last
buffer (B, H, W, C) and whose backward walks the chain with the adjoint
primitive, applying the previous layer's LeakyReLU' in the same epilogue.
Only the last layer's output is returned (the reference returns the tensor, not
a list), as the (B, 1, H', W') view of its fp32 (B, H', W', 1) buffer.

Weight norm runs in torch on the weight-sized tensors, both ways: the effective
weight w = g * v / ||v|| is formed and packed here (cached until the parameters
change), and the kernels' gradient of w is turned into (gv, gg) here.
"""
import ctypes
import weakref

import torch
from torch.optim.optimizer import register_optimizer_step_post_hook as _register_optimizer_step_post_hook

from . import _lib as L
from . import spectral as S
from .convops import _code

# power floor of the spectrogram: invisible in fp32 (|X| >= 1e-15 instead of 0)
# and, through the kernels' `p >= floor` test, a zero gradient where the power
# is exactly zero (frame 0 of a Hann-windowed, win/2-padded signal)
MAG_FLOOR = 1e-30


class SConvDesc(ctypes.Structure):
    """include/sel.h sel_sconv_desc"""
    _fields_ = [(n, ctypes.c_int32) for n in ("B", "H", "W", "Cin", "Cout", "kh", "kw", "sh", "sw", "act")] + \
        [("slope", ctypes.c_float)]


class LayerSpec:
    """One Conv2d(cin, cout, (kh, kw), stride (sh, sw)), valid padding, LeakyReLU
    after it when `leaky`."""

    __slots__ = ("cin", "cout", "kh", "kw", "sh", "sw", "leaky")

    def __init__(self, cin, cout, kernel, stride, leaky):
        self.cin, self.cout, self.leaky = int(cin), int(cout), bool(leaky)
        self.kh, self.kw = (int(k) for k in kernel)
        self.sh, self.sw = (int(s) for s in stride)
        check(self.desc(1, self.kh, self.kw, 0.0))

    def desc(self, B, H, W, slope):
        return SConvDesc(B=B, H=H, W=W, Cin=self.cin, Cout=self.cout, kh=self.kh, kw=self.kw, sh=self.sh, sw=self.sw,
                         act=1 if self.leaky else 0, slope=slope)

    def out_hw(self, H, W):
        return (H - self.kh) // self.sh + 1, (W - self.kw) // self.sw + 1


def check(desc):
    """The kernels' limits (include/sel.h), checked by the library without a GPU."""
    lib = L.load()
    if lib.sel_sconv_check(ctypes.byref(desc)) != 0:
        raise NotImplementedError(lib.sel_last_error().decode())


def frames(T, win, hop):
    """Frames of the spectrogram of T samples: zero pad win // 2 on both sides,
    then a centred STFT."""
    return 1 + (T + 2 * (win // 2)) // hop


def geometry(T, n_fft, hop, win, specs):
    """[(H, W)] of the spectrogram and of every layer's output for T samples."""
    H, W = frames(T, win, hop), n_fft // 2 + 1
    out = [(H, W)]
    for sp in specs:
        if H < sp.kh or W < sp.kw:
            raise ValueError(f"{T} samples leave {H} x {W} for a {sp.kh} x {sp.kw} conv (n_fft {n_fft}, hop {hop})")
        H, W = sp.out_hw(H, W)
        out.append((H, W))
    return out


def spectrogram(x, n_fft, hop, win, window):
    """torchaudio.functional.spectrogram(x, pad=win // 2, window, n_fft, hop, win,
    power=1.0, normalized=False) of x (B, T) fp32, transposed: (B, frames, bins).
    The zero pad and its adjoint (a slice) are torch ops on (B, T); |STFT| and its
    backward are sel_stft_mag_fwd / bwd with the power floor MAG_FLOOR."""
    xp = torch.nn.functional.pad(x, (win // 2, win // 2))
    return S.stft_mag(xp, n_fft, hop, win, window, eps=MAG_FLOOR)


# ---------------------------------------------------------------------------
# effective weights and their packed forms
# ---------------------------------------------------------------------------
def _norm(v):
    return v.detach().float().flatten(1).norm(dim=1).view(-1, 1, 1, 1)


def effective_weight(v, g):
    """torch.nn.utils.weight_norm (dim 0): g * v / ||v||, fp32."""
    return g.detach().float() * v.detach().float() / _norm(v)


def _pack_fwd(sp, w, dtype):
    if sp.cin == 1:
        return w[:, 0].permute(1, 2, 0).contiguous()            # [kh][kw][C] fp32
    if sp.cout == 1:
        return w[0].permute(1, 2, 0).contiguous()               # [kh][kw][C] fp32
    wp = w.permute(2, 3, 0, 1).contiguous()                     # [kh][kw][Cout][Cin]
    if dtype == torch.float32:
        return wp
    # bf16: w as two bf16 terms (its rounding and the rounding of the remainder), so
    # that the forward's LeakyReLU masks see the rounding of the activations only
    hi = wp.to(dtype)
    return torch.stack((hi, (wp - hi.float()).to(dtype))).contiguous()


def _pack_adj(sp, w, dtype):
    parts = []
    for p in range(sp.sw):
        ws = w[:, :, :, p::sp.sw].flip(2, 3)                    # taps kw = p (mod sw), flipped
        if sp.cin == 1:
            parts.append(ws[:, 0].permute(1, 2, 0).reshape(-1))
        elif sp.cout == 1:
            parts.append(ws[0].permute(1, 2, 0).reshape(-1))
        else:
            parts.append(ws.permute(2, 3, 1, 0).reshape(-1).to(dtype))  # [kh][Kp][Cin][Cout]
    return torch.cat(parts).contiguous()


class _PackCache:
    """Packed effective weights, reused until weight_v / weight_g change (their
    version counters, or an optimizer step on them: torch's fused Adam does not
    bump the version; the same hook as sel.dconvops)."""

    def __init__(self):
        self._e = {}

    def get(self, sp, v, g, dtype, mode):
        key = (id(v), mode, dtype, sp.sw)
        ver = (v._version, g._version)
        hit = self._e.get(key)
        if hit is not None and hit[0]() is v and hit[1]() is g and hit[2] == ver:
            return hit[3]
        w = effective_weight(v, g)
        out = _pack_fwd(sp, w, dtype) if mode == 0 else _pack_adj(sp, w, dtype)
        self._e[key] = (weakref.ref(v), weakref.ref(g), ver, out)
        return out

    def mark_stale(self, params):
        ids = {id(p) for p in params}
        for k in [k for k, e in self._e.items() if k[0] in ids or id(e[1]()) in ids]:
            del self._e[k]

    def prune(self):
        for k in [k for k, e in self._e.items() if e[0]() is None or e[1]() is None]:
            del self._e[k]


PACKS = _PackCache()


def _optimizer_stepped(optimizer, args, kwargs):
    PACKS.mark_stale([p for g in optimizer.param_groups for p in g["params"] if p.grad is not None])
    PACKS.prune()


_register_optimizer_step_post_hook(_optimizer_stepped)


# ---------------------------------------------------------------------------
# layer primitives
# ---------------------------------------------------------------------------
def _out_dtype(sp, dtype):
    return torch.float32 if sp.cout == 1 else dtype


def _in_dtype(sp, dtype):
    return torch.float32 if sp.cin == 1 else dtype


def conv_fwd(sp, x, wpack, bias, slope, dtype):
    """x (B, H, W, Cin) -> y (B, H', W', Cout); bias fp32 or None."""
    B, H, W, _ = x.shape
    d = sp.desc(B, H, W, slope)
    check(d)
    Ho, Wo = sp.out_hw(H, W)
    y = torch.empty(B, Ho, Wo, sp.cout, dtype=_out_dtype(sp, dtype), device=x.device)
    L.call("sel_sconv_fwd", ctypes.byref(d), _code(dtype), L.ptr(x), L.ptr(wpack), L.ptr(bias), L.ptr(y), L.stream(),
           meta=lambda: (f"sconv_fwd[{sp.cin}->{sp.cout},k{sp.kh}x{sp.kw},s{sp.sw}]",
                         x.numel() * x.element_size() + y.numel() * y.element_size(),
                         2.0 * y.numel() * sp.kh * sp.kw * sp.cin))
    return y


def conv_bwd_data(sp, gy, wadj, aux, in_shape, slope, dtype):
    """gx (B, H, W, Cin) of the layer input from gy (B, H', W', Cout); times
    LeakyReLU'(aux) when aux (the layer input as stored) is given."""
    B, H, W, _ = in_shape
    d = sp.desc(B, H, W, slope)
    gx = torch.empty(B, H, W, sp.cin, dtype=_in_dtype(sp, dtype), device=gy.device)
    L.call("sel_sconv_bwd_data", ctypes.byref(d), _code(dtype), L.ptr(gy), L.ptr(wadj), L.ptr(aux), L.ptr(gx),
           L.stream(),
           meta=lambda: (f"sconv_dgrad[{sp.cin}->{sp.cout},k{sp.kh}x{sp.kw},s{sp.sw}]",
                         gx.numel() * gx.element_size() + gy.numel() * gy.element_size(),
                         2.0 * gy.numel() * sp.kh * sp.kw * sp.cin))
    return gx


def conv_wgrad(sp, gy, x, slope, dtype, want_bias=True):
    """(gw (Cout, Cin, kh, kw), gb (Cout)) fp32 of the effective weight and bias."""
    B, H, W, _ = x.shape
    d = sp.desc(B, H, W, slope)
    ws = L.workspace(L.lib().sel_sconv_wgrad_workspace(ctypes.byref(d), _code(dtype)), x.device)
    gw = torch.empty(sp.cout, sp.cin, sp.kh, sp.kw, dtype=torch.float32, device=x.device)
    gb = torch.empty(sp.cout, dtype=torch.float32, device=x.device) if want_bias else None
    L.call("sel_sconv_wgrad", ctypes.byref(d), _code(dtype), L.ptr(gy), L.ptr(x), L.ptr(gw), L.ptr(gb), L.ptr(ws),
           ws.numel(), L.stream(),
           meta=lambda: (f"sconv_wgrad[{sp.cin}->{sp.cout},k{sp.kh}x{sp.kw},s{sp.sw}]",
                         x.numel() * x.element_size() + gy.numel() * gy.element_size(),
                         2.0 * gy.numel() * sp.kh * sp.kw * sp.cin))
    return gw, gb


def weight_norm_backward(gw, v, g):
    """(gv, gg) of w = g * v / ||v|| from gw (torch, weight-sized fp32 tensors)."""
    vf, gf = v.detach().float(), g.detach().float()
    n = _norm(v)
    dot = (gw * vf).flatten(1).sum(dim=1).view(-1, 1, 1, 1)
    gg = dot / n
    gv = gf / n * (gw - vf * dot / (n * n))
    return gv, gg


# ---------------------------------------------------------------------------
# the chain
# ---------------------------------------------------------------------------
class SpecChainFn(torch.autograd.Function):
    """One spectral sub-discriminator on its spectrogram: mag (B, frames, bins)
    fp32 -> the last layer's output, the (B, 1, H', W') view of an fp32 buffer.

    forward(ctx, mag, specs, slope, dtype, frozen, *params): params per layer are
    (weight_v, weight_g, bias or None); frozen = the parameters are constants
    here (no weight-gradient kernels, no gradient returned for them)."""

    NPRE = 5  # leading non-parameter inputs of forward

    @staticmethod
    def forward(ctx, mag, specs, slope, dtype, frozen, *params):
        L.need_device(mag)
        if specs[-1].leaky or specs[-1].cout != 1:
            raise NotImplementedError("the spectral chain ends in a plain C -> 1 conv")
        x = mag.contiguous().unsqueeze(-1)
        bufs = []
        for li, sp in enumerate(specs):
            v, g, b = params[3 * li:3 * li + 3]
            bias = b.detach().float().contiguous() if b is not None else None
            x = conv_fwd(sp, x, PACKS.get(sp, v, g, dtype, 0), bias, slope, dtype)
            bufs.append(x)
        ctx.save_for_backward(mag, *bufs[:-1], *params)
        ctx.cfg = (specs, slope, dtype, frozen, tuple(bufs[-1].shape))
        return bufs[-1].permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, gout):
        specs, slope, dtype, frozen, oshape = ctx.cfg
        nl = len(specs)
        saved = ctx.saved_tensors
        mag, bufs, params = saved[0], saved[1:nl], saved[nl:]
        pgrads = [None] * len(params)
        # the loss kernels write gradients of batch slices and of the whole view;
        # whatever their strides, the chain takes the dense (B, H', W', 1) form
        gpre = gout.permute(0, 2, 3, 1).float().contiguous()
        assert tuple(gpre.shape) == oshape
        xin0 = mag.contiguous().unsqueeze(-1)
        gmag = None
        for li in range(nl - 1, -1, -1):
            sp = specs[li]
            v, g, b = params[3 * li:3 * li + 3]
            x_in = bufs[li - 1] if li > 0 else xin0
            base = SpecChainFn.NPRE + 3 * li
            need = [ctx.needs_input_grad[base + k] and not frozen for k in range(3)]
            need[2] = need[2] and b is not None
            if any(need):
                gw, gb = conv_wgrad(sp, gpre, x_in, slope, dtype, want_bias=need[2])
                if need[0] or need[1]:
                    gv, gg = weight_norm_backward(gw, v, g)
                    pgrads[3 * li] = gv if need[0] else None
                    pgrads[3 * li + 1] = gg if need[1] else None
                if need[2]:
                    pgrads[3 * li + 2] = gb
            if li == 0 and not ctx.needs_input_grad[0]:
                break
            if li > 0 and not specs[li - 1].leaky:
                raise NotImplementedError("inner spectral discriminator layers are LeakyReLU layers")
            gin = conv_bwd_data(sp, gpre, PACKS.get(sp, v, g, dtype, 1), bufs[li - 1] if li > 0 else None,
                                x_in.shape, slope, dtype)
            if li == 0:
                gmag = gin.squeeze(-1)
            gpre = gin
        return (gmag, None, None, None, None, *pgrads)
