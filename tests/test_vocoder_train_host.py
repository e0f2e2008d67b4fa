"""CPU checks of the vocoder training boundary: the backward entry points of the
grouped primitive validate their descriptors before any device work, the
trainer class exists with the reference's interface, and the training opt-in
adds no state."""
import ctypes
import inspect

import torch

V1 = dict(in_channels=64, channels=64, resblock_kernel_sizes=[11], resblock_dilations=[[1, 3, 5]], groups=3,
          upsample_scales=[5, 5, 4, 3], upsample_kernel_sizes=[10, 10, 8, 6])


def test_backward_entry_points_reject_bad_descriptors_without_gpu():
    from sel import _lib
    from sel import hfgops as HF
    lib = _lib.load()
    buf = (ctypes.c_float * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def data(d, g=p, x=p, w=p, o=p):
        return lib.sel_hfg_conv_bwd_data(ctypes.byref(d) if d is not None else None, 1, 1, g, None, x, w, None, 0.0, o,
                                         None)

    def wgrad(d, g=p, x=p, gw=p, gb=None, ws=p):
        return lib.sel_hfg_conv_wgrad(ctypes.byref(d) if d is not None else None, 1, 1, g, None, x, gw, gb, ws, 16,
                                      None)

    good = dict(rows=14, T=7, C=96, N=96, K=11, dil=5, pad=50, groups=3)
    bad = [dict(good, groups=5),                 # G divides neither C nor N
           dict(good, N=100),                    # G does not divide N
           dict(good, K=0), dict(good, dil=0), dict(good, T=0), dict(good, K=-3),
           dict(good, rows=15),                  # no whole number of samples
           dict(good, bias_period=96)]           # a bias period without a bias gradient
    for kw in bad:
        d = HF.make_desc(**kw)
        rc = wgrad(d)
        assert rc < 0 and b"sel_hfg_conv_wgrad" in lib.sel_last_error(), kw
        if "bias_period" in kw:
            continue                             # the data gradient does not read the bias period
        rc = data(d)
        assert rc < 0 and b"sel_hfg_conv_bwd_data" in lib.sel_last_error(), kw
        assert lib.sel_hfg_conv_bwd_kernel(ctypes.byref(d), 1, 1, 0) < 0
        assert lib.sel_hfg_conv_bwd_kernel(ctypes.byref(d), 1, 1, 1) < 0
        assert lib.sel_hfg_conv_wgrad_workspace(ctypes.byref(d), 1, 1) == 0
    for call in (data, wgrad):
        d = HF.make_desc(**good)
        d.in_group_stride = 16                   # neither 0 nor C/G
        assert call(d) == -1 and b"in_group_stride" in lib.sel_last_error()
        d = HF.make_desc(**good)
        d.res_group_stride = 7
        assert call(d) == -1 and b"res_group_stride" in lib.sel_last_error()
        assert call(None) == -1
    d = HF.make_desc(**good)
    assert data(d, g=None) == -1 and data(d, w=None) == -1 and data(d, o=None) == -1
    assert data(HF.make_desc(**dict(good, slope=0.1)), x=None) == -1     # LeakyReLU' needs the saved input
    assert wgrad(d, g=None) == -1 and wgrad(d, x=None) == -1 and wgrad(d, gw=None) == -1 and wgrad(d, ws=None) == -1
    assert wgrad(d, gb=p) == -1                  # a bias gradient without a bias period
    assert wgrad(d) == -1 and b"workspace" in lib.sel_last_error()     # 16 bytes are too few
    assert lib.sel_hfg_conv_bwd_data(ctypes.byref(d), 0, 1, p, None, p, p, None, 0.0, p, None) == -1  # fp32 in, bf16 out
    dt = HF.make_desc(**dict(good, tanh=True))
    assert data(dt) == -1 and b"saved output" in lib.sel_last_error()
    # training never streams
    for kw in (dict(good, rows=10, T_out=5), dict(good, act_skip=3)):
        d = HF.make_desc(**kw)
        assert data(d) == -3 and b"streaming" in lib.sel_last_error(), kw
        assert wgrad(d) == -3, kw
        assert lib.sel_hfg_conv_bwd_kernel(ctypes.byref(d), 1, 1, 0) == -3
    # a valid descriptor names its instances: the matrix-core kernels in bf16, one thread per output in fp32
    d = HF.make_desc(**good)
    assert lib.sel_hfg_conv_bwd_kernel(ctypes.byref(d), 1, 1, 0) == 2
    assert lib.sel_hfg_conv_bwd_kernel(ctypes.byref(d), 1, 1, 1) == 1
    assert lib.sel_hfg_conv_bwd_kernel(ctypes.byref(d), 0, 0, 0) == 0
    assert lib.sel_hfg_conv_bwd_kernel(ctypes.byref(d), 0, 0, 1) == 0
    # T = 7, B = 2: two row tiles, so a forced split count of 3 is clamped to 2
    per = (96 * 11 * 32 + 96) * 4
    prev = lib.sel_tune(72, 3)
    try:
        assert lib.sel_hfg_conv_wgrad_workspace(ctypes.byref(d), 1, 1) == 2 * per
        lib.sel_tune(72, 1)
        assert lib.sel_hfg_conv_wgrad_workspace(ctypes.byref(d), 1, 1) == per
    finally:
        lib.sel_tune(72, prev)


def test_vocoder_trainer_class():
    import trainer.vocoder as TV
    from trainer.trainerGAN import TrainerGAN
    assert issubclass(TV.Trainer, TrainerGAN)
    want = ["self", "steps", "epochs", "data_loader", "model", "criterion", "optimizer", "scheduler", "config", "device"]
    assert list(inspect.signature(TV.Trainer.__init__).parameters) == want
    assert "_train_step" in TV.Trainer.__dict__ and "_eval_step" in TV.Trainer.__dict__

    class Gen(torch.nn.Module):
        enabled = False

        def enable_training(self, flag=True):
            self.enabled = flag

    gen = Gen()
    cfg = {"outdir": None, "generator_train_start_steps": 7, "discriminator_train_start_steps": 11}
    tr = TV.Trainer(steps=0, epochs=0, data_loader={}, model={"generator": gen, "analyzer": torch.nn.Identity()},
                    criterion={}, optimizer={}, scheduler={}, config=cfg)
    assert tr.generator_start == 7 and tr.discriminator_start == 11 and gen.enabled is True
    tr = TV.Trainer(steps=0, epochs=0, data_loader={}, model={"generator": torch.nn.Identity()}, criterion={},
                    optimizer={}, scheduler={}, config={"outdir": None})
    assert tr.generator_start == 0 and tr.discriminator_start == 0


def test_enable_training_adds_no_state():
    from models.vocoder.HiFiGAN import Generator, StreamGenerator
    for cls in (Generator, StreamGenerator):
        G = cls(**V1)
        keys = list(G.state_dict())
        nparam, nbuf = len(list(G.parameters())), len(list(G.buffers()))
        assert G.enable_training() is G and G._training_enabled is True
        assert list(G.state_dict()) == keys
        assert len(list(G.parameters())) == nparam and len(list(G.buffers())) == nbuf
        G.enable_training(False)
        assert G._training_enabled is False and list(G.state_dict()) == keys
    # off (the default): a forward that needs a gradient still raises, and names the opt-in
    G = Generator(**V1)
    try:
        G(torch.zeros(1, 64, 2))
    except NotImplementedError as e:
        assert "inference only" in str(e) and "enable_training()" in str(e)
    else:
        raise AssertionError("forward did not raise")
