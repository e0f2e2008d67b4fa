"""CPU checks of the UnivNet discriminator boundary: the reference's classes,
constructor defaults and state_dict keys; the seeded golden parameters; the CPU
restatement tests/univnet_ref.py pinned to the golden; the frame / layer
geometry; and the 2-D conv kernels' limits (checked by the library before any
device work)."""
import copy

import numpy as np
import pytest
import torch

import univnet_ref as U
from conftest import golden


@pytest.fixture(scope="module")
def g():
    return U.load_disc_golden(golden)


def _golden_discriminator():
    from models.vocoder.UnivNet import Discriminator
    torch.manual_seed(U.SEED)
    D = Discriminator(**copy.deepcopy(U.D_PARAMS))
    return D, U.redraw(D)


def test_classes_and_default_state_dict(g):
    from models.vocoder.UnivNet import Discriminator
    from models.vocoder.modules.discriminator import (UnivNetMultiResolutionSpectralDiscriminator,
                                                      UnivNetSpectralDiscriminator)
    D = Discriminator()
    assert isinstance(D.mrsd, UnivNetMultiResolutionSpectralDiscriminator)
    assert isinstance(D.mrsd.discriminators[0], UnivNetSpectralDiscriminator) and D.flat_channel is False
    sd = D.state_dict()
    assert list(sd.keys()) == [str(k) for k in g["keys"]]
    assert [",".join(str(s) for s in v.shape) for v in sd.values()] == [str(s) for s in g["shapes"]]
    for i in range(3):
        for j in range(6):
            pre = f"mrsd.discriminators.{i}.layers.{j}" + (".0" if j < 5 else "")
            assert all(pre + s in sd for s in (".weight_g", ".weight_v", ".bias"))
        assert f"mrsd.discriminators.{i}.window" in sd
    from sel import configs
    cfg = configs.get("symADuniv_vctk_48000_hop300")
    assert list(Discriminator(**cfg["discriminator_params"]).state_dict().keys()) == list(sd.keys())


def test_golden_parameters_load_strict(g):
    from models.vocoder.UnivNet import Discriminator
    D, chk = _golden_discriminator()
    assert chk == float(g["chk"])          # the same draw, in the reference's parameter order
    D2 = Discriminator(**copy.deepcopy(U.D_PARAMS))
    D2.load_state_dict(D.state_dict(), strict=True)
    assert U.checksum(D2) == float(g["chk"])


def test_restatement_reproduces_golden(g):
    D, _ = _golden_discriminator()
    P = {k: v.double().requires_grad_(v.is_floating_point() and not k.endswith("window"))
         for k, v in D.state_dict().items()}
    x = torch.from_numpy(g["x"]).double().requires_grad_(True)
    outs = U.discriminator(P, x, **U.D_PARAMS)
    assert torch.is_tensor(outs[0]) and isinstance(outs[3], list)
    rel = lambda a, b: float((a.detach().double() - torch.from_numpy(b).double()).norm() /  # noqa: E731
                             torch.from_numpy(b).double().norm())
    for k, t in U.flat_outputs(outs).items():
        assert tuple(t.shape) == g[k].shape and rel(t, g[k]) <= 1e-5, (k, rel(t, g[k]))
    U.weighted_sum(outs).backward()
    assert rel(x.grad, g["grad_x"]) <= 1e-4
    n = 0
    for k, p in P.items():
        if p.requires_grad:
            assert rel(p.grad, g["g." + k]) <= 1e-4, (k, rel(p.grad, g["g." + k]))
            n += 1
    assert n == len(list(D.parameters()))


def test_spectrogram_frame0_is_zero_on_the_cpu():
    x = torch.randn(2, 1800, dtype=torch.float64)
    for n, h, w in zip(U.D_PARAMS["fft_sizes"], U.D_PARAMS["hop_sizes"], U.D_PARAMS["win_lengths"]):
        s = U.spectrogram(x, n, h, w, torch.hann_window(w, dtype=torch.float64))
        assert s.shape == (2, n // 2 + 1, U.frames(1800, w, h)) and float(s[..., 0].abs().max()) == 0.0


@pytest.mark.parametrize("T", [1800, 9600])
def test_geometry_matches_golden(g, T):
    from models.vocoder.UnivNet import Discriminator
    from sel import sconvops as SC
    D = Discriminator(**copy.deepcopy(U.D_PARAMS))
    for i, f in enumerate(D.mrsd.discriminators):
        geo = f.geometry(T)
        assert geo == U.geometry(T, f.fft_size, f.hop_size, f.win_length)
        assert geo[0] == (SC.frames(T, f.win_length, f.hop_size), f.fft_size // 2 + 1)
        assert tuple(geo[-1]) == tuple(int(v) for v in g[f"geo.{T}.{i}"]), (i, geo[-1])
    if T == 1800:
        assert [tuple(g[f"out.{i}"].shape[2:]) for i in range(3)] == [(9, 53), (1, 117), (29, 21)]
    with pytest.raises(ValueError):
        D.mrsd.discriminators[1].geometry(1500)      # 12 frames: no output row is left


def test_limits_raise_not_implemented():
    from models.vocoder.modules.discriminator import UnivNetSpectralDiscriminator
    from sel import sconvops as SC
    SC.LayerSpec(32, 32, (3, 9), (1, 2), True)
    SC.LayerSpec(1, 64, (3, 9), (1, 1), True)
    SC.LayerSpec(64, 1, (3, 3), (1, 1), False)
    bad = [((32, 32, (4, 9), (1, 1), True), "kh <= 3"), ((32, 32, (3, 11), (1, 1), True), "kw <= 9"),
           ((32, 32, (3, 9), (2, 1), True), "sh = 1"), ((32, 32, (3, 9), (1, 3), True), "sw in {1, 2}"),
           ((48, 48, (3, 9), (1, 1), True), "C % 32 == 0"), ((1, 16, (3, 9), (1, 1), True), "C % 32 == 0"),
           ((2, 32, (3, 9), (1, 1), True), "1 -> C")]
    for args, limit in bad:
        with pytest.raises(NotImplementedError, match=limit.replace("{", r"\{").replace("}", r"\}")):
            SC.LayerSpec(*args)
    with pytest.raises(NotImplementedError, match="kw <= 9"):
        UnivNetSpectralDiscriminator(1024, 120, 600, kernel_sizes=[(3, 11)] * 6, strides=[(1, 1)] * 6)
    with pytest.raises(NotImplementedError, match="LeakyReLU"):
        UnivNetSpectralDiscriminator(1024, 120, 600, nonlinear_activation="ReLU", nonlinear_activation_params={})


def test_entry_points_validate_before_device_work():
    import ctypes
    from sel import _lib
    from sel import sconvops as SC
    lib = _lib.load()
    buf = (ctypes.c_float * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    d = SC.LayerSpec(32, 32, (3, 9), (1, 2), True).desc(2, 4, 40, 0.2)
    assert lib.sel_sconv_check(ctypes.byref(d)) == 0
    assert lib.sel_sconv_fwd(ctypes.byref(d), 1, None, p, None, p, None) == -1
    d.kw = 10
    for rc in (lib.sel_sconv_fwd(ctypes.byref(d), 1, p, p, None, p, None),
               lib.sel_sconv_bwd_data(ctypes.byref(d), 1, p, p, None, p, None),
               lib.sel_sconv_wgrad(ctypes.byref(d), 1, p, p, p, None, p, 16, None)):
        assert rc == -1 and b"kw <= 9" in lib.sel_last_error()
    assert lib.sel_sconv_wgrad_workspace(ctypes.byref(d), 1) == 0
    d.kw, d.W = 9, 8                                  # input narrower than the kernel
    assert lib.sel_sconv_check(ctypes.byref(d)) == -1


def test_weight_norm_backward_matches_autograd():
    from sel import sconvops as SC
    g0 = torch.Generator().manual_seed(3)
    v = torch.randn(8, 4, 3, 9, generator=g0, dtype=torch.float64).requires_grad_(True)
    gg = torch.rand(8, 1, 1, 1, generator=g0, dtype=torch.float64).requires_grad_(True)
    gw = torch.randn(8, 4, 3, 9, generator=g0, dtype=torch.float64)
    w = gg * v / v.flatten(1).norm(dim=1).view(-1, 1, 1, 1)
    (w * gw).sum().backward()
    gv, ggr = SC.weight_norm_backward(gw.float(), v.detach().float(), gg.detach().float())
    assert float((gv.double() - v.grad).norm() / v.grad.norm()) < 1e-6
    assert float((ggr.double() - gg.grad).norm() / gg.grad.norm()) < 1e-6
    assert np.allclose(SC.effective_weight(v.detach().float(), gg.detach().float()).double(), w.detach(), atol=1e-6)
