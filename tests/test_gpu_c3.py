"""Parity of the C3 (BASELINE configs[2]) bf16 path at the bench's own size.

1. Every bf16 tile variant of the MFMA conv primitive (tune key 0 = 21..27,
   conv.hip fwd4_choice; 27 = the warp-specialised k_conv_ws_bf16, 28 / 29 =
   its eight-wave forms k_conv_ws8 (512 x 128 tiles of 128 x 64 wave tiles /
   256 x 128 of 64 x 64), bit-identical to 27 where they apply; 30 = the
   sample-tile kernel k_conv_wss of conv_wss.hip, whole 400-row samples x 64
   channels on 16x16x32 MFMAs: another fp32 summation order, so it is held to
   the fp64 bound only)
   on the real C3 layer shapes in primitive form,
   forward and dgrad (adjoint) forms, against an fp64 reference computed from
   the SAME bf16 operands.  Both accumulate exact bf16 products (fp32 vs fp64
   sums) and the kernel rounds once to bf16, so the bound is bf16 output
   rounding: <= 4e-3 norm-wise, and elementwise |a-b| <= 8e-3|b| + 2e-3 max|b|.
   The variant the dispatcher picks by default (key 0 = 0) must be bit-equal to
   the forced one it names.
   Shapes (B = 64, 1 s @ 24 kHz): RU128 k7 d1/3/9 at T=2000 (128k rows), RU256
   k7 d1/3/9 at T=400 (25.6k rows; the 256-row tiles overrun every sample),
   the 256-wide 1x1, the strided 128->256 s5 / 256->512 s5 layers (phase-packed
   3-tap form), the transposed 512->256 s5 decoder layer (2 taps, replicate
   pad), and their dgrads.  Reference layers: conv_layer.py:139-142, :180-183,
   residual_unit.py:43-46.
2. One full denoise-trainer step at B = 64 x 24000 in bf16 against the fp32
   oracle on the same weights (trainer/denoise.py:52-84): y, z, the loss and
   the encoder gradients, norm-wise (bounds in the test).
"""
import zlib

import pytest
import torch

from conv_cases import _check, _operands, _ref  # the fp64 primitive and the bf16 bound (tests/conv_cases.py)

pytestmark = pytest.mark.gpu

B = 64
# (tag, C, N, K, dil, pad_mode, in_elu, bias_period, T, aux, res)
FWD = [
    ("ru128_k7_d1", 128, 128, 7, 1, 0, 1, 0, 2000, 0, 0),
    ("ru128_k7_d9", 128, 128, 7, 9, 0, 1, 0, 2000, 0, 0),
    ("ru256_k7_d1", 256, 256, 7, 1, 0, 1, 0, 400, 0, 0),
    ("ru256_k7_d3", 256, 256, 7, 3, 0, 1, 0, 400, 0, 0),
    ("ru256_k7_d9", 256, 256, 7, 9, 0, 1, 0, 400, 0, 0),
    ("ru256_1x1", 256, 256, 1, 1, 0, 1, 0, 400, 0, 1),
    ("down128_256_s5", 640, 256, 3, 1, 0, 0, 256, 400, 0, 0),
    ("down256_512_s5", 1280, 512, 3, 1, 0, 0, 512, 80, 0, 0),
    ("up512_256_s5", 512, 1280, 2, 1, 1, 0, 256, 80, 0, 0),
    # the 2-tap phase-view transposed convs at 400 / 2000 rows per sample
    # (warp-specialised kernel since round 4, forward and adjoint forms)
    ("up256_128_s5", 256, 640, 2, 1, 1, 0, 640, 400, 0, 0),
    ("up128_64_s2", 128, 256, 2, 1, 1, 0, 256, 2000, 0, 0),
    # the other T = 80 layers (round 6: five-sample k_conv_wss tiles)
    ("proj512_64", 512, 64, 3, 1, 0, 0, 0, 80, 0, 0),
    ("dec_conv1_64_512", 64, 512, 7, 1, 0, 0, 0, 80, 0, 0),
]


@pytest.mark.parametrize("Bs", [7, 3, 1])
@pytest.mark.parametrize("out32", [0, 1])
def test_sample_tiles_ragged_batches(gpu, Bs, out32):
    """k_conv_wss on five-sample tiles (T = 80) with a batch that leaves the
    last tile short (7 = 5 + 2, 3, 1 samples), a halo of 54 rows (k7, dil 9:
    each sample's segment must stay its own) and replicate padding, bf16 and
    fp32 outputs, against fp64 of the same operands."""
    from sel import _lib as L
    from sel import convops as CO
    prev = L.lib().sel_tune(67, 1)  # the five-sample tiles for every width (default: N >= 512)
    try:
        _ragged(gpu, CO, Bs, out32)
    finally:
        L.lib().sel_tune(67, prev)


def _ragged(gpu, CO, Bs, out32):
    for (C, N, K, dil, mode) in ((64, 128, 7, 9, 0), (128, 320, 2, 1, 1), (256, 64, 3, 1, 0), (128, 512, 3, 1, 0)):
        T = 80
        pad = (K - 1) * dil if mode == 0 else 1
        d = CO.ConvDesc(Bs * T, T, C, N, K, dil, pad, mode, 0, N)
        od = torch.float32 if out32 else torch.bfloat16
        assert CO.fwd_kernel_name(d, torch.bfloat16, od).startswith("k_conv_wss<"), CO.fwd_kernel_name(
            d, torch.bfloat16, od)
        gen = torch.Generator(device=gpu).manual_seed(Bs * 1000 + K)
        x, wp, b, _, _ = _operands(d, gen, gpu, 0, 0)
        ref = _ref(x, wp, d, Bs, b)
        got = CO.prim(d, x, wp, bias=b, out_dtype=od)
        _check(got, ref, (Bs, C, N, K, dil, mode, out32))


@pytest.mark.parametrize("form", ["fwd", "dgrad"])
@pytest.mark.parametrize("shape", FWD, ids=[s[0] for s in FWD])
def test_fwd4_tile_variants_on_c3_shapes(gpu, shape, form):
    from sel import _lib as L
    from sel import convops as CO
    tag, C, N, K, dil, mode, elu, bias, T, aux, res = shape
    pad = (K - 1) * dil if mode == 0 else 1
    d = CO.ConvDesc(B * T, T, C, N, K, dil, pad, mode, elu, bias)
    if form == "dgrad":
        # the backward uses the adjoint primitive on gout (pad' = (K-1)dil - pad,
        # no prologue) with the ELU'(aux) and residual epilogue of a residual unit
        d = d.adjoint()
        aux = res = int(K > 1 and C == N)
    gen = torch.Generator(device=gpu).manual_seed(zlib.crc32(f"{tag}/{form}".encode()))
    x, wp, b, a_, r_ = _operands(d, gen, gpu, aux, res)
    ref = _ref(x, wp, d, B, b, a_, r_)
    lib = L.lib()
    p4 = lib.sel_tune(4, 1)  # the weight-stationary thin kernel would pre-empt the tiled one
    p42 = lib.sel_tune(42, 1)  # and so would the pointwise kernel on the 1x1 shapes
    try:
        default_name = CO.fwd_kernel_name(d, torch.bfloat16, torch.bfloat16)
        assert default_name.startswith(("k_conv_fwd_bf16", "k_conv_ws_bf16", "k_conv_ws8", "k_conv_wss")), default_name
        default = CO.prim(d, x, wp, bias=b, aux=a_, res=r_).clone()
        _check(default, ref, (form, "default", default_name))
        matched = False
        ws = {}
        for v in range(21, 31):
            p0 = lib.sel_tune(0, v)
            try:
                name = CO.fwd_kernel_name(d, torch.bfloat16, torch.bfloat16)
                got = CO.prim(d, x, wp, bias=b, aux=a_, res=r_)
            finally:
                lib.sel_tune(0, p0)
            _check(got, ref, (form, v, name))
            if name.startswith(("k_conv_ws_bf16", "k_conv_ws8")):
                ws[name] = got
            if name == default_name:
                matched = True
                assert torch.equal(got, default), (form, v)
        assert matched, default_name
        # the eight-wave kernel (variant 28, where legal) keeps the 12-wave kernel's
        # (chunk, tap) MFMA order per output: same bits
        first = next(iter(ws.values()), None)
        for name, got in ws.items():
            assert torch.equal(got, first), (form, list(ws), name)
    finally:
        lib.sel_tune(4, p4)
        lib.sel_tune(42, p42)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_c3_denoise_step_vs_fp32_oracle(gpu, dtype):
    """Full C3 step: PQC generator (symAD_libritts_24000_hop300), B = 64 x 1 s,
    loss = lambda_vq * sum(vqloss) + 45 * mel, grads into the encoder/projector
    (decoder + quantizer frozen, codebook eval) — HIP convs (bf16 or the
    exact-fp32 path) vs the fp32 oracle on the same weights.

    Forward: y, z and the mel term norm-wise.  Backward, two ways:
    * same upstream gradient: both sides back-propagate the ORACLE's dL/dy and
      dL/dvqloss, which isolates the conv stack's backward from the mel-L1
      subgradient (sign(mel(y) - mel(x)) flips wherever |diff| is below the
      forward error: measured 9e-2 end-to-end in bf16 on r2a, a property of the
      L1 loss, not of the kernels);
    * end to end (own loss): bounded loosely, for the record.
    Bounds — bf16 (2^-9 operand rounding per layer, ~30 layers): y, z 3e-2,
    mel 5e-3, same-upstream grad 3e-2 concatenated / 6e-2 worst tensor, end to
    end 1.5e-1.  fp32: 1e-4 forward, 2e-3 gradients (summation order only).
    VQ indices are not compared here: z differs at the bf16 level, so near-ties
    may flip (the VQ kernel's exactness is tested on identical z,
    test_gpu_model.py)."""
    from oracle import ref_ops as R
    from oracle.melfilters import mel as melbank
    from losses import MultiMelSpectrogramLoss
    from models.autoencoder.AudioDec import Generator
    from sel import configs
    from sel.convops import precision
    cfg = configs.get("symAD_libritts_24000_hop300")
    mp = cfg["mel_loss_params"]
    torch.manual_seed(93)
    G = Generator(**cfg["generator_params"])
    P = {k: v.clone() for k, v in G.state_dict().items()}
    train = [k for k in P if k.startswith(("encoder.", "projector.")) and k.endswith(("weight", "bias"))]
    for k in train:
        P[k].requires_grad_(True)
    g = torch.Generator().manual_seed(5)
    clean = 0.1 * torch.randn(B, 1, 24000, generator=g)
    noisy = R.add_noise(clean, 0.1 * torch.randn(B, 1, 24000, generator=g), 15)
    mm = torch.from_numpy(melbank(sr=mp["fs"], n_fft=2048, n_mels=80, fmin=mp["fmin"], fmax=mp["fmax"]).T.copy())
    wl = mp["win_lengths"][0] or 2048
    torch.set_num_threads(min(16, torch.get_num_threads()))
    yr, zqr, zr, vqr, _ = R.generator_forward(P, noisy, R.generator_geometry(), pqc=True)
    yr.retain_grad()
    vqr.retain_grad()
    melr = R.multi_mel_loss(yr, clean, [(2048, 300, wl)], [R.hann(wl)], [mm], 1e-10, None)
    lossr = cfg["lambda_vq_loss"] * vqr.sum() + cfg["lambda_mel_loss"] * melr
    lossr.backward()
    gy, gvq = yr.grad.clone(), vqr.grad.clone()

    G = G.to(gpu)
    for p in list(G.quantizer.parameters()) + list(G.decoder.parameters()):
        p.requires_grad_(False)
    G.quantizer.codebook.eval()
    mel = MultiMelSpectrogramLoss(**mp).to(gpu)
    params = dict(G.named_parameters())
    rel = lambda a, b: ((a.detach().double().cpu() - b.detach().double()).norm() / b.detach().double().norm()).item()

    def grad_err():
        num = den = 0.0
        worst = (0.0, "")
        for k in train:
            gd, gr = params[k].grad.double().cpu(), P[k].grad.double()
            num += ((gd - gr) ** 2).sum().item()
            den += (gr ** 2).sum().item()
            worst = max(worst, (rel(gd, gr), k))
            params[k].grad = None
        return (num / den) ** 0.5, worst

    with precision(torch.bfloat16 if dtype == "bf16" else torch.float32):
        xin = noisy.to(gpu)
        y, zq, z, vql, ppl = G(xin)
        meld = mel(y, clean.to(gpu))
        ((y * gy.to(gpu)).sum() + (vql * gvq.to(gpu)).sum()).backward()
        eg_same, worst_same = grad_err()
        y, zq, z, vql, ppl = G(xin)
        meld = mel(y, clean.to(gpu))
        (cfg["lambda_vq_loss"] * vql.sum() + cfg["lambda_mel_loss"] * meld).backward()
        eg_e2e, worst_e2e = grad_err()
    ey, ez = rel(y, yr), rel(z, zr)
    em = abs(meld.item() - melr.item()) / abs(melr.item())
    print(f"C3 {dtype} vs fp32 oracle: y {ey:.2e} z {ez:.2e} mel {em:.2e} | same-upstream grad {eg_same:.2e} "
          f"worst {worst_same} | end-to-end grad {eg_e2e:.2e} worst {worst_e2e}")
    if dtype == "bf16":
        assert ey <= 3e-2 and ez <= 3e-2, (ey, ez)
        assert em <= 5e-3, em
        assert eg_same <= 3e-2 and worst_same[0] <= 6e-2, (eg_same, worst_same)
        assert eg_e2e <= 1.5e-1, eg_e2e
    else:
        assert ey <= 1e-4 and ez <= 1e-4 and em <= 1e-4, (ey, ez, em)
        assert eg_same <= 2e-3 and worst_same[0] <= 5e-3, (eg_same, worst_same)
        assert eg_e2e <= 5e-2, eg_e2e
