"""Cases, fp64 references and bounds of the 1-D conv primitive (csrc/conv.hip,
csrc/conv_wss.hip, csrc/conv_wgrad.hip: sel_conv_fwd / sel_conv_wgrad) at its
tile and dispatch edges, shared by tests/test_gpu_conv_edges.py, tests/test_conv_cases_host.py
and tests/test_gpu_c3.py (which takes its operands, reference and bf16 checker
from here).  Nothing here needs a GPU: sel_conv_fwd_kernel_id and
sel_conv_wgrad_workspace are host decisions.

What lives here:
  * CASES: forward primitives (B, T, C, N, K, dil, pad, pad_mode, in_elu,
    bias_period), each the smallest shape that reaches one edge of one kernel
    family, with the tune settings it needs (key 0 forces the variant; keys 4
    and 42 switch off the thin / pointwise kernels that would pre-empt it; key
    51 asks for the (16, 128) sample tile without an ELU), its epilogue
    operands, its output dtypes and the kernel name it must reach per output
    dtype, written out, so that a dispatch change cannot move a case onto
    another kernel unnoticed;
  * NOT_WSS: the neighbours of k_conv_wss's legal shapes that must not reach it;
  * WGRAD_CASES: weight-gradient launches with the plan they must get (mode,
    k_wgrad3_bf16 instance, tiles per split, number of splits), and
    wgrad_mode / wgrad_plan / wgrad_workspace: conv_wgrad.hip's plan restated;
  * operands / reference / wgrad_reference: the buffers of a case and the fp64
    primitive on the same rounded operands, with the sums of absolute terms the
    fp32 bounds scale with;
  * the checkers, and the wrong answers (mutations) the host test feeds them.

Bounds.  u = 2^-24, eps = 2 u = 2^-23 (fp32); bf16 has 8 significant bits.

bf16 output: operands are the same bf16 values in kernel and reference, their
products are exact in fp32, the sums run in fp32 and the result is rounded to
bf16 once (2^-9 relative where nothing cancels).  The project's bound for that
(check_bf16, formerly tests/test_gpu_c3.py _check):
    ||a - b|| <= 4e-3 ||b||   and   |a - b| <= 8e-3 |b| + 2e-3 max|b|  per element.

fp32 output: 1e-5 norm-wise (the project's figure) and per element
    |a - b| <= (n + 4) eps S,   S = sum |w| |act(x)| (+ |bias| + |res|),
n = K C products: any order of summing n + 2 terms in fp32 is within
(n + 1) u S (1 + O(u)) of the exact sum, the epilogue multiply adds one
rounding, eps = 2 u leaves a factor 2 (the derivation of tests/dconv_cases.py;
fp32 operands add one rounding per product, which the factor 2 also covers).
With aux the kernel's ELU'(aux) = exp(aux) comes from the hardware exp, a few
fp32 ulp off: (n + 12) eps S.

ELU prologue.  The kernel rounds exp2(x log2e) - 1 (fp32, hardware exp) to
bf16, the reference rounds fp64 expm1(x).  Where the fp64 value lies within
AMBIG = 2^-20 (absolute: 16 fp32 ulp of 1.0, over the "few ulp" conv_common.h
states for v_exp_f32; the subtraction of 1 is exact, so the error of the
operand is the absolute error of the exp) of a bf16 rounding boundary the two
may pick neighbouring bf16 values.  Such an operand is "ambiguous"; the
positive branch is exact and never is.  An fp32 output (and a weight gradient)
of an ELU case is allowed the slack
    sum |w| ulp_bf16(operand) over the ambiguous operands
(one more fp64 conv) per element on top of its bound; the norm-wise 1e-5 is
not widened.  bf16 outputs keep check_bf16.
With x = 0.5 randn rounded to bf16 about 0.1 % of the operands are ambiguous
(a cell of the bf16 grid at |v| ~ 0.25 is 2^-9 wide, the ambiguous band 2^-19);
the host test holds every ELU case below 1 %.

Weight / bias gradients: fp32 sums over n = B T rows of exact products, in
nsplit partials summed afterwards: per element
    |a - b| <= (n + nsplit + 2) eps sum |g| |act(x)|
for any order, and 1e-5 norm-wise (tests/test_gpu_conv.py's figure; every case
here has at most 4.5 k rows).  ELU cases get the ambiguity slack
sum |g| ulp_bf16(operand) the same way.
"""
import zlib

import torch

from sel import convops as CO

EPS32 = 2.0 ** -23
AMBIG = 2.0 ** -20
BF16, F32 = torch.bfloat16, torch.float32
OUT_FILL = 7.0          # prefill of output buffers
GUARD = 4096            # guard elements after an output buffer

# constants of conv_wgrad.hip and conv_tile.h, restated
W2_BM, W2_HALO, WB_BM, WB_BC, WG_BM = 128, 64, 64, 32, 64
C1_TR, C1_NMAX, C1_KMAX, C1_HALO = 256, 64, 8, 64
WF_BM, WF_XR, SPLIT_GROUP = 64, 128, 32
RU_OOB = 0x7FFFFFF0


# ---------------------------------------------------------------------------
# forward cases
# ---------------------------------------------------------------------------
class Case:
    """One forward primitive launch.  pad None: causal ((K - 1) dil).  adjoint:
    the descriptor is d.adjoint() of the fields given (the dgrad launch).
    in32: fp32 operands (the output is fp32 too).  kernel: the name it must
    reach, "{to}" standing for the output type; family: what the name starts
    with where the reporter gives no tile (the generic kernels)."""

    def __init__(self, name, family, shape, kernel, tune=(), pad=None, mode=0, elu=0, bias=0, epi="none",
                 dtypes=("bf16", "f32"), adjoint=False, in32=False, edge=""):
        self.name, self.family, self.kernel, self.tune, self.epi = name, family, kernel, dict(tune), epi
        self.dtypes, self.adjoint, self.in32, self.edge = dtypes, adjoint, in32, edge
        self.B, T, C, N, K, dil = shape
        pad = (K - 1) * dil if pad is None else pad
        d = CO.ConvDesc(self.B * T, T, C, N, K, dil, pad, mode, elu, bias)
        self.d = d.adjoint() if adjoint else d

    @property
    def aux(self):
        return self.epi in ("aux", "both")

    @property
    def res(self):
        return self.epi in ("res", "both")

    def in_dtype(self):
        return F32 if self.in32 else BF16

    def name_for(self, dt):
        return self.kernel.format(to="bf16" if dt == "bf16" else "float")


_F4 = {21: "k_conv_fwd_bf16<256, 32, 4, %d, {to}>", 22: "k_conv_fwd_bf16<128, 32, 4, %d, {to}>",
       23: "k_conv_fwd_bf16<128, 64, 2, %d, {to}>", 24: "k_conv_fwd_bf16<256, 64, 4, %d, {to}>",
       25: "k_conv_fwd_bf16<128, 128, 2, %d, {to}>", 26: "k_conv_fwd_bf16<64, 128, 1, %d, {to}>"}
_OFF = {4: 1, 42: 1}   # the thin and the pointwise kernel off


def _f4(name, v, kmax, shape, edge, tune=(), **kw):
    return Case(name, "f4", shape, _F4[v] % kmax, {0: v, **dict(tune)}, edge=edge, **kw)


def _make_cases():
    c = []
    # ---- k_conv_fwd_bf16 (variants 21-26, KMAX 1 / 3 / 8)
    c.append(_f4("f4_t1_k8", 21, 8, (3, 1, 64, 96, 8, 8), "T = 1 under K = 8 (halo 56 > T), one row of a 256-row tile", bias=32))
    c.append(_f4("f4_n30", 26, 8, (3, 65, 32, 30, 4, 5), "N % 4 != 0 and bias_period % 4 != 0 (scalar epilogue), one chunk, "
                 "BM + 1", bias=6, epi="both"))
    c.append(_f4("f4_halo63", 25, 8, (3, 65, 32, 96, 8, 9), "halo 63", bias=32, epi="aux"))
    c.append(_f4("f4_k1", 23, 1, (3, 129, 32, 32, 1, 1), "KMAX 1, BM + 1", tune=_OFF, epi="res"))
    epis = {21: "none", 22: "aux", 23: "res", 24: "both", 25: "none", 26: "aux"}
    for v in range(21, 27):
        c.append(_f4(f"f4_257_v{v}", v, 3, (2, 257, 32, 96, 3, 1), "T = k BM + 1 for BM 64 / 128 / 256; N no multiple of 64; centred pad on 23 / 25 / 26",
                     bias=96 if v % 2 else 0, epi=epis[v], elu=int(v == 24), pad=1 if v in (23, 25, 26) else None))
    c.append(_f4("f4_255_v24", 24, 3, (2, 255, 32, 96, 3, 1), "T = BM - 1 (256)", epi="res"))
    c.append(_f4("f4_127_v22", 22, 3, (2, 127, 32, 96, 3, 1), "T = BM - 1 (128)", bias=96))
    c.append(_f4("f4_63_v26", 26, 3, (2, 63, 32, 96, 3, 1), "T = BM - 1 (64)", epi="both"))
    c.append(_f4("f4_halo64", 23, 8, (2, 130, 32, 64, 5, 16), "halo exactly F4_HALOMAX = 64", bias=64))
    c.append(_f4("f4_halo_gt_t", 22, 8, (3, 40, 64, 32, 7, 9), "halo 54 > T = 40, ELU prologue", elu=1, bias=32))
    c.append(_f4("f4_centred", 24, 8, (2, 130, 32, 64, 7, 3), "centred zero pad (pad = halo / 2)", pad=9, epi="aux"))
    c.append(_f4("f4_rep1", 25, 3, (2, 130, 64, 160, 2, 1), "replicate pad 1; a 32-column last column tile", pad=1, mode=1,
                 bias=32))
    c.append(_f4("f4_rephalo", 23, 3, (2, 70, 32, 64, 3, 4), "replicate pad = halo", pad=8, mode=1, epi="res"))
    c.append(_f4("f4_adjoint", 22, 8, (2, 257, 96, 32, 7, 3), "the adjoint form (pad 0) with aux + res", adjoint=True,
                 epi="both"))
    c.append(_f4("f4_xcd", 26, 3, (11, 200, 64, 256, 3, 1), "44 row tiles x 2 column tiles: both xcd_tile branches", bias=256))
    # ---- k_conv_ws_bf16 (variant 27)
    ws = lambda name, K, shape, edge, **kw: Case(name, "ws", shape, "k_conv_ws_bf16<%d, {to}>" % K, {0: 27},  # noqa: E731
                                                 edge=edge, **kw)
    c.append(ws("ws_2chunk", 7, (2, 257, 32, 128, 7, 9), "2 chunks < prefetch distance 3; BM + 1", bias=128))
    c.append(ws("ws_2chunk_elu", 7, (2, 257, 32, 128, 7, 9), "the same with the ELU prologue", elu=1, epi="res"))
    c.append(ws("ws_xcd", 3, (11, 200, 160, 256, 3, 32), "10 chunks, halo 64, 11 x 2 tiles: both xcd_tile branches",
                bias=256))
    c.append(ws("ws_rep", 2, (2, 255, 96, 256, 2, 1), "replicate pad 1, K = 2, BM - 1", pad=1, mode=1, bias=128))
    c.append(ws("ws_t1", 3, (1, 1, 32, 128, 3, 1), "T = 1, one sample"))
    c.append(ws("ws_bias4", 3, (2, 130, 96, 128, 3, 2), "bias_period % 8 != 0; 6 chunks", bias=4, epi="aux"))
    c.append(ws("ws_adjoint", 7, (2, 257, 128, 64, 7, 3), "the adjoint form (pad 0) with aux + res; 4 chunks = the ring",
                adjoint=True, epi="both"))
    c.append(ws("ws_c64", 3, (2, 300, 64, 128, 3, 5), "C = 64: 4 chunks = the ring size; centred pad", pad=5, bias=128))
    # ---- k_conv_ws8<7, ..., 512, 128> (variant 28)
    w8 = lambda name, shape, edge, **kw: Case(name, "ws8", shape, "k_conv_ws8<7, {to}, 512, 128>", {0: 28},  # noqa: E731
                                              edge=edge, **kw)
    c.append(w8("ws8_1024", (1, 1024, 32, 128, 7, 9), "T = 1024: exactly two 512-row tiles; 2 chunks < the 3-slot ring",
                bias=128))
    c.append(w8("ws8_1031", (3, 1031, 64, 128, 7, 10), "a 7-row third tile; pad 0; aux + res", pad=0, epi="both"))
    c.append(w8("ws8_1025", (1, 1025, 32, 128, 7, 9), "T = 2 BM + 1: a one-row third tile; centred pad", pad=27, epi="aux"))
    c.append(w8("ws8_elu", (1, 1030, 96, 128, 7, 1), "ELU prologue, causal; 6 chunks: the 3-slot ring twice round", elu=1))
    # ---- k_conv_ws8<K, ..., 256, 128, 64, 2> (variant 29)
    w9 = lambda name, K, shape, edge, **kw: Case(name, "ws8w", shape, "k_conv_ws8<%d, {to}, 256, 128, 64, 2>" % K,  # noqa: E731
                                                 {0: 29}, edge=edge, **kw)
    c.append(w9("ws8w_xcd", 3, (11, 200, 64, 256, 3, 1), "11 x 2 tiles: both xcd_tile branches", bias=256, epi="res"))
    c.append(w9("ws8w_257", 7, (2, 257, 32, 128, 7, 9), "BM + 1, 2 chunks, centred pad", pad=27, epi="aux"))
    c.append(w9("ws8w_halo64_elu", 3, (2, 300, 64, 128, 3, 32), "halo exactly 64, ELU prologue, 4 chunks", elu=1, bias=128))
    # ---- k_conv_wss (variant 30)
    def wss(name, K, S, BN, shape, edge, tune=(), **kw):
        return Case(name, "wss", shape, "k_conv_wss<%d, %d, %d, {to}>" % (K, S, BN), {0: 30, **dict(tune)},
                    edge=edge, dtypes=("bf16", "f32") if S == 25 else ("bf16",), **kw)
    c.append(wss("wss_385", 7, 25, 64, (11, 385, 64, 192, 7, 9), "T = 385: one row in the last strip; 11 row x 3 column tiles "
                 "(both xcd_tile branches)", bias=192))
    c.append(wss("wss_399", 3, 25, 64, (2, 399, 64, 128, 3, 1), "T = 399: ragged last strip; centred pad", pad=1, epi="both"))
    c.append(wss("wss_400_halo64", 3, 25, 64, (2, 400, 64, 64, 3, 32), "halo 64; 2 chunks = the ring", tune=_OFF, epi="aux"))
    c.append(wss("wss_497", 7, 32, 64, (2, 497, 64, 64, 7, 9), "T = 497: the S = 32 interval's lower end", tune=_OFF, bias=64))
    c.append(wss("wss_1009", 3, 32, 64, (2, 1009, 192, 128, 3, 1), "tiles of 505 + 504 rows; pad 0; 6 chunks", pad=0,
                 epi="res"))
    c.append(wss("wss_1000", 2, 32, 64, (1, 1000, 64, 128, 2, 1), "K = 2, pad 0, tiles of 500", pad=0, bias=4))
    c.append(wss("wss_511", 3, 32, 64, (1, 511, 64, 128, 3, 2), "T = 511: one row short of the tallest tile", epi="aux"))
    c.append(wss("wss_512", 3, 32, 64, (2, 512, 64, 128, 3, 2), "T = 512: the S = 32 interval's upper end", epi="both"))
    c.append(wss("wss_241_elu", 7, 16, 128, (2, 241, 64, 256, 7, 9), "(16, 128) tile at T = 241, ELU prologue", elu=1,
                 bias=256))
    c.append(wss("wss_499_elu", 7, 16, 128, (1, 499, 128, 128, 7, 3), "(16, 128) tiles of 250 + 249 rows, 4 chunks", elu=1,
                 epi="res"))
    c.append(wss("wss_499_k51", 7, 16, 128, (2, 499, 64, 128, 7, 3), "(16, 128) tile without ELU (tune key 51 = 1)",
                 tune={51: 1}, epi="aux"))
    c.append(wss("wss_rep", 2, 25, 64, (2, 390, 64, 128, 2, 1), "replicate pad, K = 2, on S = 25", pad=1, mode=1, bias=128))
    # ---- the generic kernels
    for v in range(1, 7):
        c.append(Case(f"gen_tile{v}", "gen", (5, 37, 48, 33, 3, 2), "k_conv_fwd<", {0: v}, bias=33,
                      epi=("none", "aux", "res", "both", "none", "both")[v - 1],
                      edge="flat row tiles across sample boundaries (T = 37); N = 33; C = 48 (a 16-channel last chunk)"))
    c.append(Case("gen_f32", "gen", (5, 37, 48, 33, 3, 2), "k_conv_fwd<", in32=True, dtypes=("f32",), epi="both", bias=33,
                  edge="the generic kernel on fp32 operands"))
    c.append(Case("f32_bm64", "gen", (3, 65, 48, 64, 3, 2), "k_conv_fwd<", in32=True, dtypes=("f32",), epi="both", bias=64,
                  edge="k_conv_fwd_f32<64, 64> (N % 64 == 0) at T = BM + 1"))
    c.append(Case("f32_bm128", "gen", (3, 65, 48, 96, 3, 2), "k_conv_fwd<", in32=True, dtypes=("f32",), epi="aux", pad=1,
                  mode=1, edge="k_conv_fwd_f32<128, 32> (N % 64 != 0), replicate pad"))
    return c


CASES = _make_cases()
BY_NAME = {c.name: c for c in CASES}
FAMILIES = ("f4", "ws", "ws8", "ws8w", "wss", "gen")

# (shape, pad, out dtype, why): forced onto variant 30, these must not reach k_conv_wss
NOT_WSS = [((2, 384, 64, 128, 3, 1), None, "bf16", "T = 384: 24 strips"),
           ((2, 401, 64, 128, 3, 1), None, "bf16", "T = 401: 26 strips"),
           ((2, 513, 64, 128, 3, 1), None, "bf16", "T = 513: tiles of 257 rows"),
           ((2, 400, 64, 128, 3, 1), 3, "bf16", "pad > halo"),
           ((2, 497, 64, 128, 7, 9), None, "f32", "fp32 output takes it at S = 25 only"),
           ((2, 241, 64, 256, 7, 9), None, "bf16", "T = 241 without ELU or key 51: no (16, 128) tile")]


def not_wss_desc(shape, pad):
    B, T, C, N, K, dil = shape
    return CO.ConvDesc(B * T, T, C, N, K, dil, (K - 1) * dil if pad is None else pad, 0, 0, 0)


class tuned:
    """with tuned(lib, {key: value}): the settings applied, the previous ones restored."""

    def __init__(self, lib, settings):
        self.lib, self.settings, self.prev = lib, dict(settings), []

    def __enter__(self):
        for k, v in self.settings.items():
            self.prev.append((k, self.lib.sel_tune(k, v)))
        return self

    def __exit__(self, *exc):
        for k, v in reversed(self.prev):
            self.lib.sel_tune(k, v)
        return False


def kernel_name(case, dt):
    """What the library reports for a case under its tune settings (host only)."""
    from sel import _lib as L
    with tuned(L.load(), case.tune):
        return CO.fwd_kernel_name(case.d, case.in_dtype(), F32 if dt == "f32" else BF16, case.aux or case.res)


# ---------------------------------------------------------------------------
# operands and the fp64 primitive
# ---------------------------------------------------------------------------
def _operands(d, gen, dev, aux, res):
    x = (0.5 * torch.randn(d.rows, d.C, generator=gen, device=dev)).to(torch.bfloat16)
    wp = (torch.randn(d.N, d.K, d.C, generator=gen, device=dev) / (d.K * d.C) ** 0.5).to(torch.bfloat16)
    b = torch.randn(d.bias_period, generator=gen, device=dev) if d.bias_period else None
    a_ = torch.randn(d.rows, d.N, generator=gen, device=dev).to(torch.bfloat16) if aux else None
    r_ = torch.randn(d.rows, d.N, generator=gen, device=dev).to(torch.bfloat16) if res else None
    return x, wp, b, a_, r_


def _seed(name):
    return zlib.crc32(name.encode())


def operands(case, dev):
    """(x, wp, bias, aux, res) of a case, seeded by its name: bf16 (aux / res in
    bf16 too: cast them to the output dtype, which is exact), or fp32 for in32."""
    gen = torch.Generator(device=dev).manual_seed(_seed(case.name))
    x, wp, b, a_, r_ = _operands(case.d, gen, dev, case.aux, case.res)
    if case.in32:   # full-mantissa fp32 operands
        gen2 = torch.Generator(device=dev).manual_seed(_seed(case.name) + 1)
        x = x.float() + 2.0 ** -10 * torch.randn(x.shape, generator=gen2, device=dev)
        wp = wp.float() * (1 + 2.0 ** -10 * torch.randn(wp.shape, generator=gen2, device=dev))
    return x, wp, b, a_, r_


def act_operand(x, d):
    """(fp64 operand the kernels multiply, ulp_bf16 of it where it is ambiguous
    else 0): ELU in fp64 rounded to bf16 for bf16 x (module docstring)."""
    xa = x.double()
    if not d.in_elu:
        return xa, None
    v = torch.where(xa > 0, xa, torch.expm1(xa))
    if x.dtype != torch.bfloat16:
        return v, None
    _m, ex = torch.frexp(v)
    ulp = torch.ldexp(torch.ones_like(v), ex - 8)          # bf16 spacing in v's binade
    mid = torch.floor(v / ulp) * ulp + 0.5 * ulp           # the rounding boundary of v's cell
    amb = (xa < 0) & ((v - mid).abs() <= AMBIG)
    return v.to(torch.bfloat16).double(), torch.where(amb, ulp, torch.zeros_like(ulp))


def _taps(xa, d, B_):
    """xa (B, T, C) fp64 -> the K shifted / padded views the taps multiply."""
    T = d.T
    out = []
    for k in range(d.K):
        idx = torch.arange(T, device=xa.device) + k * d.dil - d.pad
        if d.pad_mode == 0:
            ok = (idx >= 0) & (idx < T)
            xs = torch.zeros(B_, T, xa.shape[2], dtype=torch.float64, device=xa.device)
            xs[:, ok] = xa[:, idx[ok]]
        else:
            xs = xa[:, idx.clamp(0, T - 1)]
        out.append(xs)
    return out


def _conv(xa, w, d, B_):
    out = torch.zeros(B_, d.T, d.N, dtype=torch.float64, device=xa.device)
    for k, xs in enumerate(_taps(xa, d, B_)):
        out += torch.einsum("btc,nc->btn", xs, w[:, k, :])
    return out.view(B_ * d.T, d.N)


def _ref(x, wp, d, B_, bias=None, aux=None, res=None):
    """fp64 primitive on the same (bf16) operands: out[b,t,n] = sum_k,c
    act(x)[b, t + k*dil - pad, c] * wp[n,k,c] (+ bias, * ELU'(aux), + res)."""
    xa, _ = act_operand(x, d)
    out = _conv(xa.view(B_, d.T, d.C), wp.double(), d, B_)
    if bias is not None:
        out += bias.double().repeat(d.N // bias.numel())
    if aux is not None:
        out *= torch.where(aux.double() > 0, 1.0, torch.exp(aux.double()))
    if res is not None:
        out += res.double()
    return out


def reference(case, ops, w=None):
    """dict(y, S, slack) of a case on operands ops = (x, wp, bias, aux, res):
    the fp64 primitive, S = sum |w| |act(x)| + |bias| (times ELU'(aux)) + |res|,
    and the ELU ambiguity slack (None without an ELU prologue).  w: other
    weights (the host test's mutations)."""
    x, wp, b, a_, r_ = ops
    d, B_ = case.d, case.B
    w = wp if w is None else w
    y = _ref(x, w, d, B_, b, a_, r_)
    xa, ulp = act_operand(x, d)
    S = _conv(xa.abs().view(B_, d.T, d.C), w.double().abs(), d, B_)
    slack = _conv(ulp.view(B_, d.T, d.C), w.double().abs(), d, B_) if ulp is not None else None
    if b is not None:
        S += b.double().abs().repeat(d.N // b.numel())
    if a_ is not None:
        g = torch.where(a_.double() > 0, 1.0, torch.exp(a_.double()))
        S *= g
        slack = slack * g if slack is not None else None
    if r_ is not None:
        S += r_.double().abs()
    return dict(y=y, S=S, slack=slack, ambiguous=float((ulp > 0).double().mean()) if ulp is not None else 0.0)


# ---------------------------------------------------------------------------
# bounds
# ---------------------------------------------------------------------------
def _rel(got, ref):
    return ((got.double() - ref).norm() / ref.norm().clamp_min(1e-300)).item()


def _check(got, ref, what):
    g = got.double()
    e = ((g - ref).norm() / ref.norm()).item()
    assert e <= 4e-3, (what, e)
    bad = (g - ref).abs() > 8e-3 * ref.abs() + 2e-3 * ref.abs().max()
    assert not bad.any(), (what, int(bad.sum()), (g - ref).abs().max().item())


def check_bf16(got, ref, what):
    """_check, printing its figures; returns the worst element / allowed."""
    g = got.double()
    allowed = 8e-3 * ref.abs() + 2e-3 * ref.abs().max()
    worst = ((g - ref).abs() / allowed).max().item()
    print(f"{what}: bf16 norm-wise {_rel(g, ref):.3e} (<= 4e-3), worst element / allowed {worst:.3f}")
    _check(got, ref, what)
    return worst


def check_f32(got, ref, S, n, what, slack=None, extra=4):
    """fp32 sums of n products: 1e-5 norm-wise and (n + extra) eps S per element,
    the latter widened by the ELU ambiguity slack where there is one."""
    g = got.double()
    diff = (g - ref).abs()
    allowed = (n + extra) * EPS32 * S
    plain = (diff / allowed.clamp_min(1e-300)).max().item()
    if slack is not None:
        allowed = allowed + slack
    worst = (diff / allowed.clamp_min(1e-300)).max().item()
    e = _rel(g, ref)
    print(f"{what}: fp32 norm-wise {e:.3e} (<= 1e-5), worst element / allowed {worst:.3f} (n = {n})" +
          (f", without the ELU slack {plain:.3f}" if slack is not None else ""))
    assert e <= 1e-5, (what, e)
    assert bool((diff <= allowed).all()), (what, worst, int((diff > allowed).sum()))
    return worst


def check_output(case, dt, got, ref, what):
    """One forward output of a case in dtype dt against reference(case, ...)."""
    if dt == "bf16":
        return check_bf16(got, ref["y"], what)
    return check_f32(got, ref["y"], ref["S"], case.d.K * case.d.C, what, ref["slack"], 12 if case.aux else 4)


def check_wgrad(got, ref, S, n, nsplit, what, slack=None):
    """A weight / bias gradient: (n + nsplit + 2) eps S per element, 1e-5 norm-wise."""
    return check_f32(got, ref, S, n + nsplit, what, slack, 2)


# ---------------------------------------------------------------------------
# wrong answers the checkers must refuse (tests/test_conv_cases_host.py)
# ---------------------------------------------------------------------------
MUTATIONS = ("row_shift", "drop_tap", "drop_chunk", "last_row", "swap_columns")


def mutate(case, ops, ref, how):
    """The fp64 output a kernel with one defect would give."""
    d = case.d
    y = ref["y"]
    if how == "row_shift":          # every output one row late
        return torch.roll(y, 1, 0)
    if how in ("drop_tap", "drop_chunk"):
        w = ops[1].clone()
        if how == "drop_tap":
            w[:, d.K - 1, :] = 0
        else:
            w[:, :, d.C - 16:] = 0
        return reference(case, ops, w)["y"]
    if how == "last_row":           # the last row of the last sample holds its neighbour (or nothing)
        y = y.clone()
        y[-1] = y[-2] if y.shape[0] > 1 else 0
        return y
    wcol = 64 if d.N >= 128 else 32 if d.N >= 64 else 16 if d.N >= 32 else 8
    y = y.clone()
    y[:, :2 * wcol] = torch.cat([ref["y"][:, wcol:2 * wcol], ref["y"][:, :wcol]], 1)
    return y


# ---------------------------------------------------------------------------
# weight gradient: conv_wgrad.hip's wgrad_mode / wgrad_plan restated, cases
# ---------------------------------------------------------------------------
def _cdiv(a, b):
    return -(-a // b)


def wgrad_tr_ok(d):
    return d.C % 32 == 0 and d.N % 32 == 0 and (d.K - 1) * d.dil <= W2_HALO and d.K <= 8 and \
        d.T * max(d.C, d.N) * 2 <= RU_OOB


def wgrad_c1_ok(d):
    return d.C == 1 and d.N % 8 == 0 and d.N <= C1_NMAX and d.K <= C1_KMAX and (d.K - 1) * d.dil <= C1_HALO


def wgrad_mode(d, bf16, tune=None):
    """0 generic, 2 k_wgrad2_bf16, 3 k_wgrad3_bf16, 4 the C = 1 kernel."""
    tune = tune or {}
    if not bf16:
        return 4 if wgrad_c1_ok(d) and tune.get(54, 0) != 1 else 0
    t = tune.get(1, 0)
    if wgrad_c1_ok(d) and t != 1:
        return 4
    if t == 1 or not wgrad_tr_ok(d):
        return 0
    return 2 if t == 2 else 3


def wgrad3_instance(N, C, K):
    """(NT, CT, MAXT) of k_wgrad3_bf16: the widest block whose per-wave tile count stays <= 4."""
    def tiles_per_wave(nt, ct):
        wpn, pairs = 4 // nt, ct * K
        wpp = wpn if pairs >= wpn else pairs
        return _cdiv(pairs, wpp)
    nt = 2 if N % 64 == 0 else 1
    ct = 2 if C % 64 == 0 else 1
    if tiles_per_wave(nt, ct) > 4 and ct == 2:
        ct = 1
    if tiles_per_wave(nt, ct) > 4 and nt == 2:
        nt = 1
    tpw = tiles_per_wave(nt, ct)
    return nt, ct, tpw if tpw <= 4 else 8


def wgrad3_reachable():
    """Every instance wgrad_plan can ask for at K <= 8 (wgrad_tr_ok)."""
    return {wgrad3_instance(N, C, K) for N in (32, 64) for C in (32, 64) for K in range(1, 9)}


def wgrad_plan(d, mode, tune=None):
    """dict(mode, inst, bn, n_tiles, tiles_per_split, nsplit) as conv_wgrad.hip plans it."""
    tune = tune or {}
    B = d.rows // d.T
    if mode == 4:
        n_tiles = B * _cdiv(d.T, C1_TR)
        tps = max(1, _cdiv(n_tiles, 512))
        return dict(mode=4, inst=None, bn=d.N, n_tiles=n_tiles, tiles_per_split=tps, nsplit=_cdiv(n_tiles, tps))
    tr = mode >= 2
    bm = W2_BM if tr else WB_BM
    inst = None
    if mode == 3:
        inst = wgrad3_instance(d.N, d.C, d.K)
        bn, bc = 32 * inst[0], 32 * inst[1]
    else:
        bn = 32 if tr else (16 if d.N <= 16 else 32 if d.N <= 32 else 64)
        bc = 32 if tr else WB_BC
    n_tiles = B * _cdiv(d.T, bm)
    blocks = _cdiv(d.N, bn) * _cdiv(d.C, bc)
    target = tune.get(10, 0) if tune.get(10, 0) > 0 else (512 if mode == 3 else 768)
    want = max(1, _cdiv(target, blocks))
    if mode == 3:
        want = _cdiv(want, 8) * 8
    per_split = (d.N * d.K * d.C + d.N) * 4
    cap_mb = (tune.get(62, 0) if tune.get(62, 0) > 0 else 32) if mode == 3 else 64
    want = min(want, max(1, (cap_mb << 20) // per_split), max(1, n_tiles))
    tps = max(1, _cdiv(n_tiles, want))
    return dict(mode=mode, inst=inst, bn=bn, n_tiles=n_tiles, tiles_per_split=tps, nsplit=max(1, _cdiv(n_tiles, tps)))


def wgrad_workspace(d):
    """sel_conv_wgrad_workspace restated (default tune settings)."""
    if d.rows <= 0:
        return 16
    ns = wgrad_plan(d, 0)["nsplit"]
    if wgrad_tr_ok(d):
        ns = max(ns, wgrad_plan(d, 2)["nsplit"], wgrad_plan(d, 3)["nsplit"])
    if wgrad_c1_ok(d):
        ns = max(ns, wgrad_plan(d, 4)["nsplit"])
    return (ns + _cdiv(ns, SPLIT_GROUP)) * (d.N * d.K * d.C + d.N) * 4


def wgrad_kernel(d, bf16, tune=None):
    """Name of the partial kernel a weight-gradient launch runs (conv_wgrad.hip wgrad_impl)."""
    tune = tune or {}
    p = wgrad_plan(d, wgrad_mode(d, bf16, tune), tune)
    t = "bf16" if bf16 else "float"
    if p["mode"] == 4:
        return f"k_wgrad_c1<{t}, {d.N // 8}>"
    if p["mode"] == 3:
        return "k_wgrad3_bf16<%d, %d, %d>" % p["inst"]
    if p["mode"] == 2:
        return f"k_wgrad2_bf16<{1 if d.K == 1 else 2 if d.K <= 4 else 4}>"
    if bf16:
        return f"k_wgrad_bf16<{p['bn']}>"
    if d.C % 4 == 0 and d.N % 4 == 0 and d.K <= 8 and (d.K - 1) * d.dil <= WF_XR - WF_BM and \
            d.pad <= (d.K - 1) * d.dil and tune.get(54, 0) != 1:
        nb = 32 if d.N <= 32 else 64
        cb = 32 if nb == 64 else (64 if d.C % 64 == 0 else 32)
        return f"k_wgrad_f32<{1 if d.K == 1 else 3 if d.K <= 3 else 8}, {nb}, {cb}>"
    return "k_conv_wgrad<float>"


def generic_f32_splits(d, nsplit):
    """Splits k_conv_wgrad<float> fills of the plan's nsplit (the rest is memset)."""
    rps = _cdiv(_cdiv(d.rows, nsplit), WG_BM) * WG_BM
    return _cdiv(d.rows, rps)


class WCase:
    """One weight-gradient launch: shape (B, T, C, N, K, dil), the plan it must
    get (mode, inst, tiles_per_split, nsplit) and the kernel that runs it.
    unpack: (kind, cout, cin, k, stride) for sel_conv_wgrad_unpacked."""

    def __init__(self, name, shape, kernel, mode_, tps, nsplit, inst=None, dt="bf16", tune=(), pad=None, mode=0, elu=0,
                 bias=0, unpack=None, edge=""):
        self.name, self.kernel, self.dt, self.tune, self.unpack, self.edge = name, kernel, dt, dict(tune), unpack, edge
        self.plan = dict(mode=mode_, inst=inst, tiles_per_split=tps, nsplit=nsplit)
        self.B, T, C, N, K, dil = shape
        pad = (K - 1) * dil if pad is None else pad
        self.d = CO.ConvDesc(self.B * T, T, C, N, K, dil, pad, mode, elu, bias)

    @property
    def bf16(self):
        return self.dt == "bf16"


def _make_wcases():
    w = []
    # every reachable k_wgrad3_bf16 instance (B = 3: mode 3 wants >= 8 splits, so
    # n_tiles < want and every 128-row tile is a split of its own)
    T_OF = {1: 3, 127: 3, 129: 6, 300: 9}     # T -> n_tiles = nsplit at B = 3
    m3 = [((1, 1, 1), 32, 32, 1, 300), ((1, 1, 1), 32, 32, 2, 129), ((1, 1, 2), 32, 32, 5, 127),
          ((1, 2, 1), 64, 32, 1, 129), ((1, 2, 2), 64, 32, 3, 1), ((1, 2, 3), 64, 32, 5, 300), ((1, 2, 4), 64, 32, 7, 127),
          ((2, 1, 1), 32, 64, 1, 127), ((2, 1, 2), 32, 64, 3, 300), ((2, 1, 3), 32, 64, 5, 129), ((2, 1, 4), 32, 64, 7, 1),
          ((2, 2, 1), 64, 64, 1, 1), ((2, 2, 2), 64, 64, 2, 300), ((2, 2, 3), 64, 64, 3, 127), ((2, 2, 4), 64, 64, 4, 129),
          ((2, 1, 3), 64, 64, 5, 300), ((2, 1, 4), 64, 64, 8, 129)]
    for inst, C, N, K, T in m3:
        P = inst[1] * K
        edge = f"instance {inst} at T = {T}" + (f"; P = CT K = {P}: the RG > 1 row-split form" if P <= 2 and inst[0] == 1
                                                else "")
        w.append(WCase(f"wg3_c{C}_n{N}_k{K}_t{T}", (3, T, C, N, K, 2 if K > 1 else 1), "k_wgrad3_bf16<%d, %d, %d>" % inst,
                       3, 1, T_OF[T], inst, bias=N if K % 2 else 0, edge=edge))
    w.append(WCase("wg3_short_last_split", (1, 2176, 256, 256, 7, 1), "k_wgrad3_bf16<2, 1, 4>", 3, 2, 9, (2, 1, 4), bias=256,
                   edge="17 tiles in 9 splits of 2: a one-tile last split"))
    w.append(WCase("wg3_ns42", (7, 641, 32, 32, 3, 1), "k_wgrad3_bf16<1, 1, 1>", 3, 1, 42, (1, 1, 1), bias=32,
                   edge="nsplit > 32: k_split_sum1 / k_split_sum2 with a bias gradient; a one-row last tile"))
    w.append(WCase("wg3_ns42_nobias", (7, 641, 32, 32, 3, 1), "k_wgrad3_bf16<1, 1, 1>", 3, 1, 42, (1, 1, 1),
                   edge="nsplit > 32 without a bias gradient"))
    w.append(WCase("wg3_rep", (3, 129, 64, 64, 2, 1), "k_wgrad3_bf16<2, 2, 2>", 3, 1, 6, (2, 2, 2), pad=1, mode=1, bias=32,
                   edge="replicate pad; bias_period < N"))
    w.append(WCase("wg3_elu", (3, 300, 32, 32, 7, 9), "k_wgrad3_bf16<1, 1, 2>", 3, 1, 9, (1, 1, 2), elu=1,
                   edge="ELU prologue, halo 54"))
    # the two-level reduction through sel_conv_wgrad_unpacked, one per pack kind
    # (generic kernel: 64-row tiles, 8 per 449-row sample, 40 splits)
    w.append(WCase("wg_unpack_fwd", (5, 449, 32, 32, 3, 1), "k_wgrad_bf16<32>", 0, 1, 40, tune={1: 1}, bias=32,
                   unpack=(CO.PACK_FWD, 32, 32, 3, 1), edge="k_split_sum2_unpack, PACK_FWD"))
    w.append(WCase("wg_unpack_strided", (5, 449, 32, 32, 3, 1), "k_wgrad_bf16<32>", 0, 1, 40, tune={1: 1}, pad=2, bias=32,
                   unpack=(CO.PACK_FWD_STRIDED, 32, 16, 4, 2), edge="k_split_sum2_unpack, PACK_FWD_STRIDED"))
    w.append(WCase("wg_unpack_convt", (5, 449, 32, 32, 2, 1), "k_wgrad_bf16<32>", 0, 1, 40, tune={1: 1}, pad=1, mode=1,
                   bias=16, unpack=(CO.PACK_CONVT, 16, 32, 4, 2), edge="k_split_sum2_unpack, PACK_CONVT"))
    # tune key 1 = 1: k_wgrad_bf16 at bn 16 / 32 / 64; 2: k_wgrad2_bf16<1 / 2 / 4>
    for N, T, ns in ((16, 300, 15), (32, 127, 6), (64, 129, 9)):
        w.append(WCase(f"wg_generic_bn{N}", (3, T, 32, N, 3, 2), f"k_wgrad_bf16<{N}>", 0, 1, ns, tune={1: 1}, bias=N,
                       edge=f"tune key 1 = 1 at bn {N}"))
    for K, km, T, ns in ((1, 1, 300, 9), (4, 2, 129, 6), (7, 4, 127, 3)):
        w.append(WCase(f"wg2_k{K}", (3, T, 64, 32, K, 1), f"k_wgrad2_bf16<{km}>", 2, 1, ns, tune={1: 2}, bias=32,
                       edge=f"tune key 1 = 2, KM = {km}"))
    # fp32
    w.append(WCase("wgf_64x32", (3, 129, 32, 64, 3, 2), "k_wgrad_f32<3, 64, 32>", 0, 1, 9, dt="f32", bias=64,
                   edge="k_wgrad_f32 64 x 32 blocks"))
    w.append(WCase("wgf_32x64", (3, 127, 64, 32, 7, 3), "k_wgrad_f32<8, 32, 64>", 0, 1, 6, dt="f32", elu=1,
                   edge="k_wgrad_f32 32 x 64 blocks, ELU prologue (exact in fp32)"))
    w.append(WCase("wgf_32x32", (3, 300, 36, 28, 1, 1), "k_wgrad_f32<1, 32, 32>", 0, 1, 15, dt="f32", bias=28,
                   edge="k_wgrad_f32 32 x 32 blocks, ragged C and N"))
    w.append(WCase("wgf_generic", (3, 65, 6, 10, 3, 2), "k_conv_wgrad<float>", 0, 1, 6, dt="f32", bias=10,
                   edge="C % 4 != 0: k_conv_wgrad<float> fills 4 of the plan's 6 splits (the memset tail)"))
    # the C = 1 kernel
    for N in (8, 16, 32, 64):
        for dt in ("bf16", "f32"):
            t = "bf16" if dt == "bf16" else "float"
            w.append(WCase(f"wgc1_n{N}_{dt}", (3, 300, 1, N, 7, 2), f"k_wgrad_c1<{t}, {N // 8}>", 4, 1, 6, dt=dt,
                           bias=N if N != 16 else 0, edge=f"C = 1 at N = {N}"))
    return w


WGRAD_CASES = _make_wcases()
W_BY_NAME = {c.name: c for c in WGRAD_CASES}


def wgrad_operands(case, dev):
    """(gout (rows, N), x (rows, C)) of a weight-gradient case, seeded by its name."""
    gen = torch.Generator(device=dev).manual_seed(_seed(case.name))
    d = case.d
    x = 0.5 * torch.randn(d.rows, d.C, generator=gen, device=dev)
    g = 0.5 * torch.randn(d.rows, d.N, generator=gen, device=dev)
    if case.bf16:
        return g.to(torch.bfloat16), x.to(torch.bfloat16)
    return g, x


def wgrad_reference(case, g, x):
    """dict(gw (N, K, C), S_gw, gb, S_gb, slack) in fp64: gw[n,k,c] = sum_b,t
    g[b,t,n] act(x)[b, t + k dil - pad, c], gb[j] = sum over rows and n = j mod
    bias_period of g, the same sums of absolute terms, the ELU ambiguity slack."""
    d, B_ = case.d, case.B
    xa, ulp = act_operand(x, d)
    ga = g.double().view(B_, d.T, d.N)

    def corr(gg, xx):
        out = torch.zeros(d.N, d.K, d.C, dtype=torch.float64, device=x.device)
        for k, xs in enumerate(_taps(xx.view(B_, d.T, d.C), d, B_)):
            out[:, k, :] = torch.einsum("btn,btc->nc", gg, xs)
        return out
    r = dict(gw=corr(ga, xa), S_gw=corr(ga.abs(), xa.abs()), slack=corr(ga.abs(), ulp) if ulp is not None else None,
             gb=None, S_gb=None, ambiguous=float((ulp > 0).double().mean()) if ulp is not None else 0.0)
    if d.bias_period:
        r["gb"] = ga.sum((0, 1)).view(-1, d.bias_period).sum(0)
        r["S_gb"] = ga.abs().sum((0, 1)).view(-1, d.bias_period).sum(0)
    return r


def unpack_ref(kind, gwp, cout, cin, k, stride):
    """Packed (N, K, C) gradient -> the torch weight layout, index by index as
    conv_wgrad.hip's pack_dst maps it (structural zeros of the strided form dropped)."""
    flat = gwp.reshape(-1)
    j = torch.arange(flat.numel(), device=flat.device)
    if kind == CO.PACK_FWD:
        ci, kk, co = j % cin, (j // cin) % k, j // (cin * k)
        dst, shape = (co * cin + ci) * k + kk, (cout, cin, k)
    elif kind == CO.PACK_FWD_STRIDED:
        s = stride
        ci, ph, tap, co = j % cin, (j // cin) % s, (j // (s * cin)) % 3, j // (3 * s * cin)
        kk = torch.where(tap == 0, ph - 1, torch.where(tap == 1, ph + s - 1, torch.where(ph == 0, 2 * s - 1, -1)))
        dst, shape = torch.where(kk < 0, -1, (co * cin + ci) * (2 * s) + kk), (cout, cin, 2 * s)
    else:
        s = stride
        ci, tap, r = j % cin, (j // cin) % 2, j // (2 * cin)
        ph, co = r // cout, r % cout
        kk = torch.where(tap == 1, ph, ph + s)
        dst, shape = (ci * cout + co) * (2 * s) + kk, (cin, cout, 2 * s)
    out = torch.full((shape[0] * shape[1] * shape[2],), float("nan"), dtype=flat.dtype, device=flat.device)
    ok = dst >= 0
    out[dst[ok]] = flat[ok]
    return out.view(shape)


WGRAD_MUTATIONS = ("row_shift", "drop_tap", "drop_chunk", "last_row", "swap_columns")


def mutate_wgrad(case, g, x, ref, how):
    """The fp64 weight gradient a kernel with one defect would give."""
    d = case.d
    gw = ref["gw"].clone()
    if how == "row_shift":
        return wgrad_reference(case, g, torch.roll(x, 1, 0))["gw"]
    if how == "drop_tap":
        gw[:, d.K - 1, :] = 0
    elif how == "drop_chunk":
        gw[:, :, d.C - 16:] = 0
    elif how == "last_row":         # the last row of the last sample left out of the sums
        g2 = g.clone()
        g2[-1] = 0
        return wgrad_reference(case, g2, x)["gw"]
    else:
        wcol = 32 if d.N >= 64 else 16 if d.N >= 32 else 4
        gw[:2 * wcol] = torch.cat([ref["gw"][wcol:2 * wcol], ref["gw"][:wcol]], 0)
    return gw
