"""CPU checks of the HiFi-GAN vocoder generator's drop-in boundary: the classes
import with the reference's names and state_dict keys, the constructor asserts
are the reference's, the settings build the full-width model, and the new C
entry points validate their descriptors before any device work."""
import ctypes

import pytest
import torch

from conftest import golden

SCALES = dict(upsample_scales=[5, 5, 4, 3], upsample_kernel_sizes=[10, 10, 8, 6])
V1 = dict(in_channels=64, channels=64, resblock_kernel_sizes=[11], resblock_dilations=[[1, 3, 5]], groups=3, **SCALES)
V0 = dict(in_channels=64, channels=32, resblock_kernel_sizes=[3, 7, 11], resblock_dilations=[[1, 3, 5]] * 3,
          groups=1, **SCALES)


def test_classes_import():
    from models.vocoder.HiFiGAN import Discriminator, Generator, StreamGenerator
    from models.vocoder.modules.multi_fusion import MultiGroupConv1d, MultiReceptiveField
    from models.vocoder.modules.residual_block import HiFiGANResidualBlock
    assert issubclass(StreamGenerator, Generator) and issubclass(MultiGroupConv1d, HiFiGANResidualBlock)
    assert Discriminator is not None and MultiReceptiveField is not None


@pytest.mark.parametrize("name,params", [("vocoder_v1", V1), ("vocoder_v0", V0)])
def test_state_dict_keys_match_reference(name, params):
    from models.vocoder.HiFiGAN import StreamGenerator
    g = golden(name)
    G = StreamGenerator(**params)
    want = {k[3:]: v.shape for k, v in g.items() if k.startswith("sd.")}
    have = {k: tuple(v.shape) for k, v in G.state_dict().items()}
    assert set(have) == set(want)
    assert all(have[k] == tuple(want[k]) for k in have)
    sd = {k: torch.from_numpy(g["sd." + k].astype("float32")) for k in want}
    G.load_state_dict(sd, strict=True)
    G.remove_weight_norm()
    assert not any(k.endswith("weight_g") for k in G.state_dict())


def test_constructor_asserts_match_reference():
    from models.vocoder.HiFiGAN import Generator
    from models.vocoder.modules.residual_block import HiFiGANResidualBlock
    with pytest.raises(AssertionError):
        Generator(channels=16, kernel_size=6)                     # even kernel size
    with pytest.raises(AssertionError):
        Generator(channels=16, upsample_scales=(8, 8, 2, 2), upsample_kernel_sizes=(16, 16, 4, 5))   # k != 2s
    with pytest.raises(AssertionError):
        Generator(channels=16, upsample_scales=(8, 8), upsample_kernel_sizes=(16, 16, 4, 4))
    with pytest.raises(AssertionError):
        Generator(channels=16, resblock_kernel_sizes=(3, 7), resblock_dilations=[(1, 3, 5)])
    with pytest.raises(AssertionError):
        HiFiGANResidualBlock(kernel_size=4, channels=8)


def test_full_width_parameter_count():
    from models.vocoder.HiFiGAN import StreamGenerator
    from sel import configs
    G = StreamGenerator(**configs.VOCODER_V1)
    assert sum(p.numel() for p in G.parameters()) == int(golden("vocoder_v1")["full_width_param_count"])
    for cfg in (configs.VOCODER_V0, configs.VOCODER_V2):
        assert cfg["in_channels"] == 64 and cfg["channels"] == 512


def test_grad_required_raises_without_gpu():
    """the check comes before any device work"""
    from models.vocoder.HiFiGAN import Generator
    G = Generator(**V1)
    with pytest.raises(NotImplementedError, match="inference only"):
        G(torch.zeros(1, 64, 2))


def test_entry_points_reject_bad_descriptors_without_gpu():
    from sel import _lib
    from sel import hfgops as HF
    lib = _lib.load()
    buf = (ctypes.c_float * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(d, a=p, w=p, o=p, bias=None):
        return lib.sel_hfg_conv_fwd(ctypes.byref(d) if d is not None else None, 1, 1, a, w, bias, None, o, None)

    good = dict(rows=14, T=7, C=96, N=96, K=11, dil=5, pad=50, groups=3)
    bad = [dict(good, groups=5),                 # G divides neither C nor N
           dict(good, N=100),                    # G does not divide N
           dict(good, K=0), dict(good, dil=0), dict(good, T=0), dict(good, K=-3),
           dict(good, rows=15),                  # no whole number of samples
           dict(good, bias_period=96)]           # a bias period without a bias
    for kw in bad:
        rc = call(HF.make_desc(**kw))
        assert rc < 0 and b"sel_hfg_conv_fwd" in lib.sel_last_error(), kw
        assert lib.sel_hfg_conv_kernel(ctypes.byref(HF.make_desc(**kw)), 1, 1) < 0 or "bias_period" in kw
    d = HF.make_desc(**good)
    d.in_group_stride = 16                       # neither 0 nor C/G
    assert call(d) == -1 and b"in_group_stride" in lib.sel_last_error()
    d = HF.make_desc(**good)
    d.res_group_stride = 7
    assert call(d) == -1 and b"res_group_stride" in lib.sel_last_error()
    d = HF.make_desc(**good)
    assert call(None) == -1 and call(d, a=None) == -1 and call(d, w=None) == -1 and call(d, o=None) == -1
    assert b"null pointer" in lib.sel_last_error()
    assert lib.sel_hfg_conv_fwd(ctypes.byref(d), 0, 1, p, p, None, None, p, None) == -1   # fp32 in, bf16 out
    # a valid descriptor names its kernel: the 64 x 32 matrix-core tile in bf16, one thread per output in fp32
    assert lib.sel_hfg_conv_kernel(ctypes.byref(d), 1, 1) == 2
    assert lib.sel_hfg_conv_kernel(ctypes.byref(d), 0, 0) == 0


def test_reslayer_entry_rejects_bad_descriptors_without_gpu():
    from sel import _lib
    from sel import hfgops as HF
    lib = _lib.load()
    buf = (ctypes.c_float * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    good = dict(rows=14, T=7, C=96, N=96, K=11, dil=5, pad=50, groups=3)

    def call(d, x=p, w1=p, w2=p, o=p, b1=None, b2=None):
        return lib.sel_hfg_reslayer_fwd(ctypes.byref(d), 1, x, w1, b1, w2, b2, o, None)

    for kw in (dict(good, groups=5), dict(good, K=0), dict(good, dil=-1), dict(good, T=0)):
        assert call(HF.make_desc(**kw)) == -1 and lib.sel_last_error(), kw
    d = HF.make_desc(**good)
    assert call(d, x=None) == -1 and call(d, w2=None) == -1 and call(d, o=None) == -1
    d.in_group_stride = 5
    assert call(d) == -1
    # a well-formed layer the fused kernel does not serve: C/G = 128, and anything under tune key 71 = 1
    assert call(HF.make_desc(rows=14, T=7, C=128, N=128, K=7, dil=1, pad=6)) == -3
    prev = lib.sel_tune(71, 1)
    try:
        assert call(HF.make_desc(**good)) == -3 and b"two launches" in lib.sel_last_error()
    finally:
        lib.sel_tune(71, prev)
