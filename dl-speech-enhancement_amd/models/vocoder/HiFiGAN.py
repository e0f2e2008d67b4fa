"""HiFi-GAN modules — drop-in for the reference ``models/vocoder/HiFiGAN.py``.

* ``Generator`` / ``StreamGenerator`` (:28-305): the causal HiFi-GAN vocoder
  generator of the AudioDec baseline (encoder -> projector -> quantizer ->
  vocoder) and of the streaming codec's decoders.  Same constructor arguments,
  defaults, asserts, sub-module names and ``state_dict`` keys.  Every conv runs
  the grouped LeakyReLU-fused HIP primitive of sel.hfgops.  Inference by
  default: ``forward`` raises NotImplementedError when a gradient would be
  required, unless ``enable_training()`` opted in to the training path (the
  backward kernels of the same primitive, trainer/vocoder.py).
* ``Discriminator`` (:308-395): MSD + MPD, outputs concatenated (MSD first).
"""
import logging
import os

import numpy as np
import torch
import torch.nn as nn

from layers.conv_layer import CausalConv1d, CausalConvTranspose1d
from models.vocoder.modules.discriminator import HiFiGANMultiPeriodDiscriminator, HiFiGANMultiScaleDiscriminator
from models.vocoder.modules.multi_fusion import MultiGroupConv1d, MultiReceptiveField
from sel import hfgops as HF
from sel.streams import run_concurrent


class Generator(nn.Module):
    """HiFiGAN causal generator module."""

    _training_enabled = False   # enable_training()

    def __init__(self, in_channels=80, out_channels=1, channels=512, kernel_size=7, upsample_scales=(8, 8, 2, 2),
                 upsample_kernel_sizes=(16, 16, 4, 4), resblock_kernel_sizes=(3, 7, 11),
                 resblock_dilations=[(1, 3, 5), (1, 3, 5), (1, 3, 5)], groups=1, bias=True,
                 use_additional_convs=True, nonlinear_activation="LeakyReLU",
                 nonlinear_activation_params={"negative_slope": 0.1}, use_weight_norm=True, stats=None):
        super().__init__()

        # check hyperparameters are valid
        assert kernel_size % 2 == 1, "Kernel size must be odd number."
        assert len(upsample_scales) == len(upsample_kernel_sizes)
        assert len(resblock_dilations) == len(resblock_kernel_sizes)

        # Group conv or MRF
        if (len(resblock_dilations) == len(resblock_kernel_sizes) == 1) and (groups > 1):
            multi_fusion = MultiGroupConv1d
        else:
            multi_fusion = MultiReceptiveField

        self.num_upsamples = len(upsample_kernel_sizes)
        self.input_conv = CausalConv1d(in_channels, channels, kernel_size, stride=1)
        self.upsamples = nn.ModuleList()
        self.blocks = nn.ModuleList()
        self.activation_upsamples = getattr(torch.nn, nonlinear_activation)(**nonlinear_activation_params)
        for i in range(len(upsample_kernel_sizes)):
            assert upsample_kernel_sizes[i] == 2 * upsample_scales[i]
            self.upsamples += [CausalConvTranspose1d(channels // (2 ** i), channels // (2 ** (i + 1)),
                                                     kernel_size=upsample_kernel_sizes[i],
                                                     stride=upsample_scales[i])]
            self.blocks += [multi_fusion(channels=channels // (2 ** (i + 1)),
                                         resblock_kernel_sizes=resblock_kernel_sizes,
                                         resblock_dilations=resblock_dilations, groups=groups, bias=bias,
                                         use_additional_convs=use_additional_convs,
                                         nonlinear_activation=nonlinear_activation,
                                         nonlinear_activation_params=nonlinear_activation_params)]
        self.activation_output1 = nn.LeakyReLU()
        self.activation_output2 = nn.Tanh()
        self.output_conv = CausalConv1d(channels // (2 ** (i + 1)), out_channels, kernel_size, stride=1)

        # load stats
        if stats is not None:
            self.register_stats(stats)
            self.norm = True
        else:
            self.norm = False
        logging.info(f"Input normalization: {self.norm}")

        # apply weight norm
        if use_weight_norm:
            self.apply_weight_norm()

        # reset parameters
        self.reset_parameters()

    def _block(self, i, x, stream):
        """blocks[i] on channels-last x (the modules' own forward / inference without
        the (B, C, T) round trip)."""
        blk = self.blocks[i]
        if isinstance(blk, MultiGroupConv1d):
            sl = HF.slope_of(blk.activation)
            if stream:
                x = x.repeat(1, 1, blk.groups)
            return HF.pointwise(HF.resblock(x, blk, sl, stream=stream, shared_first=not stream), blk.conv_out)
        return HF.mrf(x, list(blk.blocks), HF.slope_of(blk.blocks[0].activation), stream=stream)

    def forward(self, c):
        """c (B, in_channels, T) -> (B, out_channels, T * prod(upsample_scales)), fp32.

        One primitive launch per conv: LeakyReLU(0.1) before every conv,
        LeakyReLU(0.01) before the output conv and tanh after it run inside
        the kernels (HiFiGAN.py:141-161)."""
        train = self._training_enabled and HF.needs_grad(self, c)
        if not train:
            HF.require_inference(self, c)
        if self.norm:
            c = (c.transpose(2, 1) - self.mean) / self.scale
            c = c.transpose(2, 1)
        if train:
            return HF.generator_train(self, self._run, c)
        return self._run(HF.enter(c)).transpose(1, 2)

    def enable_training(self, flag=True):
        """Opt in to (or out of) the training path: with it on, a ``forward`` that
        needs a gradient runs the backward kernels of sel.hfgops instead of
        raising.  A plain attribute: no parameter, buffer or state_dict key."""
        self._training_enabled = bool(flag)
        return self

    def _run(self, x):
        """the launch sequence of forward on channels-last x (B, T, in_channels) -> (B, T', out_channels) fp32"""
        x = HF.causal(x, self.input_conv)
        up = HF.slope_of(self.activation_upsamples)
        for i in range(self.num_upsamples):
            x = HF.upsample(x, self.upsamples[i], up)
            x = self._block(i, x, False)
        return HF.causal(x, self.output_conv, HF.slope_of(self.activation_output1), tanh=True,
                         out_dtype=torch.float32)

    def reset_parameters(self):
        """Reset parameters (the official implementation's initialisation,
        https://github.com/jik876/hifi-gan/blob/master/models.py)."""

        def _reset_parameters(m):
            if isinstance(m, (nn.Conv1d, nn.ConvTranspose1d)):
                m.weight.data.normal_(0.0, 0.01)
                logging.debug(f"Reset parameters in {m}.")

        self.apply(_reset_parameters)

    def remove_weight_norm(self):
        """Remove weight normalization module from all of the layers."""

        def _remove_weight_norm(m):
            try:
                logging.debug(f"Weight norm is removed from {m}.")
                nn.utils.remove_weight_norm(m)
            except ValueError:  # this module didn't have weight norm
                return

        self.apply(_remove_weight_norm)

    def apply_weight_norm(self):
        """Apply weight normalization module from all of the layers."""

        def _apply_weight_norm(m):
            if isinstance(m, nn.Conv1d) or isinstance(m, nn.ConvTranspose1d):
                nn.utils.weight_norm(m)
                logging.debug(f"Weight norm is applied to {m}.")

        self.apply(_apply_weight_norm)

    def register_stats(self, stats):
        """Register stats for de-normalization as buffer (".npy": rows mean, scale)."""
        assert stats.endswith(".h5") or stats.endswith(".npy")
        assert os.path.exists(stats), f"Stats {stats} does not exist!"
        mean = np.load(stats)[0].reshape(-1)
        scale = np.load(stats)[1].reshape(-1)
        self.register_buffer("mean", torch.from_numpy(mean).float())
        self.register_buffer("scale", torch.from_numpy(scale).float())
        logging.info("Successfully registered stats as buffer.")


class StreamGenerator(Generator):
    """HiFiGAN streaming generator."""

    def __init__(self, in_channels=80, out_channels=1, channels=512, kernel_size=7, upsample_scales=(8, 8, 2, 2),
                 upsample_kernel_sizes=(16, 16, 4, 4), resblock_kernel_sizes=(3, 7, 11),
                 resblock_dilations=[(1, 3, 5), (1, 3, 5), (1, 3, 5)], groups=1, bias=True,
                 use_additional_convs=True, nonlinear_activation="LeakyReLU",
                 nonlinear_activation_params={"negative_slope": 0.1}, use_weight_norm=True, stats=None):
        super().__init__(in_channels=in_channels, out_channels=out_channels, channels=channels,
                         kernel_size=kernel_size, upsample_scales=upsample_scales,
                         upsample_kernel_sizes=upsample_kernel_sizes, resblock_kernel_sizes=resblock_kernel_sizes,
                         resblock_dilations=resblock_dilations, groups=groups, bias=bias,
                         use_additional_convs=use_additional_convs, nonlinear_activation=nonlinear_activation,
                         nonlinear_activation_params=nonlinear_activation_params, use_weight_norm=use_weight_norm,
                         stats=stats)
        self.reset_buffer()

    def initial_decoder(self, c):
        self.decode(c)

    @torch.no_grad()
    def decode(self, c):
        """c (B, T, in_channels) -> (B, out_channels, T * prod(upsample_scales)).  The
        stages hand channels-last tensors on as (B, C, T) views, as forward does."""
        c = self.decode_norm(c)
        c = self.decode_input(c.transpose(2, 1))
        c = self.decode_upsample(c)
        c = self.decode_output(c)
        return c

    def decode_norm(self, c):
        if self.norm:
            c = (c - self.mean) / self.scale
        return c

    @torch.no_grad()
    def decode_input(self, c):
        return HF.causal_stream(HF.enter(c), self.input_conv).transpose(1, 2)

    @torch.no_grad()
    def decode_upsample(self, c):
        x = HF.enter(c)
        up = HF.slope_of(self.activation_upsamples)
        for i in range(self.num_upsamples):
            x = HF.upsample_stream(x, self.upsamples[i], up)
            x = self._block(i, x, True)
        return x.transpose(1, 2)

    @torch.no_grad()
    def decode_output(self, c):
        """output_conv.inference(LeakyReLU(c)) and the tanh in one launch, fp32 out."""
        x = HF.causal_stream(HF.enter(c), self.output_conv, HF.slope_of(self.activation_output1), tanh=True,
                             out_dtype=torch.float32)
        return x.transpose(1, 2)

    def session(self, batch=1, frames=1, graph=True, codes=False, wire=False, datagrams=False):
        """An opt-in sel.streaming.VocoderSession over this generator: fixed state,
        one grouped step launch per conv, each hop of `frames` frames replayed as a graph.
        ``codes=True`` also calls ``enable_codes()``; a vocoder has no codebooks of
        its own, so ``receive`` works once ``enable_codes(lookup_generator)`` has
        been given the encoder's generator.  ``wire=True`` and ``datagrams=True``
        (with ``codes``) are passed on to ``enable_codes``."""
        from sel.streaming import VocoderSession
        s = VocoderSession(self, batch, frames, graph)
        if codes:
            s.enable_codes(wire=wire, datagrams=datagrams)
        return s

    def pool(self, capacity, frames=1, graph=True, dtype=None, codes=False, wire=False, datagrams=False):
        """An opt-in sel.streaming.VocoderPool over this generator: `capacity`
        independent streams, one batched hop per tick over the active ones.
        ``codes=True``, ``wire=True`` and ``datagrams=True`` as in ``session``."""
        from sel.streaming import VocoderPool
        p = VocoderPool(self, capacity, frames, graph, dtype)
        if codes:
            p.enable_codes(wire=wire, datagrams=datagrams)
        return p

    def reset_buffer(self):
        """Zero every streaming pad_buffer."""

        def _reset_buffer(m):
            if isinstance(m, CausalConv1d) or isinstance(m, CausalConvTranspose1d):
                m.reset_buffer()

        self.apply(_reset_buffer)


class Discriminator(nn.Module):
    """HiFi-GAN multi-scale + multi-period discriminator module."""

    def __init__(self, scales=3, scale_downsample_pooling="AvgPool1d",
                 scale_downsample_pooling_params={"kernel_size": 4, "stride": 2, "padding": 2},
                 scale_discriminator_params={"in_channels": 1, "out_channels": 1, "kernel_sizes": [15, 41, 5, 3],
                                             "channels": 128, "max_downsample_channels": 1024, "max_groups": 16,
                                             "bias": True, "downsample_scales": [2, 2, 4, 4, 1],
                                             "nonlinear_activation": "LeakyReLU",
                                             "nonlinear_activation_params": {"negative_slope": 0.1}},
                 follow_official_norm=True, periods=[2, 3, 5, 7, 11],
                 period_discriminator_params={"in_channels": 1, "out_channels": 1, "kernel_sizes": [5, 3],
                                              "channels": 32, "downsample_scales": [3, 3, 3, 3, 1],
                                              "max_downsample_channels": 1024, "bias": True,
                                              "nonlinear_activation": "LeakyReLU",
                                              "nonlinear_activation_params": {"negative_slope": 0.1},
                                              "use_weight_norm": True, "use_spectral_norm": False}):
        super().__init__()
        self.msd = HiFiGANMultiScaleDiscriminator(scales=scales, downsample_pooling=scale_downsample_pooling,
                                                  downsample_pooling_params=scale_downsample_pooling_params,
                                                  discriminator_params=scale_discriminator_params,
                                                  follow_official_norm=follow_official_norm)
        self.mpd = HiFiGANMultiPeriodDiscriminator(periods=periods, discriminator_params=period_discriminator_params)

    def _chains(self, x, pooled, method):
        """The 3 scale and 5 period sub-discriminators on `method` (None = the
        module call), as independent chains on side streams (sel.streams: same
        kernels, same bits); MSD outputs first, as the reference concatenates."""
        fs = list(self.msd.discriminators) + list(self.mpd.discriminators)
        xs = list(pooled) + [x] * len(self.mpd.discriminators)
        calls = [(lambda f=f, v=v: f(v) if method is None else getattr(f, method)(v)) for f, v in zip(fs, xs)]
        return run_concurrent(calls, [x] + list(pooled))

    def _flat(self, x):
        batch, channel, time = x.size()
        return x.reshape(batch * channel, 1, time) if channel != 1 else x

    def forward(self, x):
        """x (B, C, T) -> list of lists of each sub-discriminator's layer outputs
        (MSD then MPD), HiFiGAN.py:380-395."""
        x = self._flat(x)
        return self._chains(x, self.msd._scales(x, lambda f, v: v), None)

    @torch.no_grad()
    def stash_first_half(self, x):
        """No-grad forward of B clips x into per-layer buffers sized for 2B clips,
        kept for forward_second_half (train_denoise.DenoiseStep: the generator
        step's D(target) is the D step's real half); returns x's outputs."""
        x = self._flat(x)
        return self._chains(x, self.msd._scales(x, lambda f, v: v), "stash_first_half")

    def clear_stash(self):
        """Drop every sub-discriminator's stash_first_half buffers (sized for 2B
        clips): called whenever the generator step will not be followed by a
        forward_second_half that consumes them."""
        for f in list(self.msd.discriminators) + list(self.mpd.discriminators):
            f._stash = None

    def forward_second_half(self, x):
        """forward(torch.cat([stashed clips, x])) without recomputing the stashed
        half, as one autograd graph over all 2B clips.  Each output row runs the
        same kernels as in the concatenated pass, but the flat tiling may put a
        clip in another tile: tests/test_gpu_gan.py holds the two paths to 1e-6
        (fp32) / 1e-3 (bf16) norm-wise, not to bit equality."""
        x = self._flat(x)
        with torch.no_grad():  # the waveform (a detached prediction) takes no gradient
            pooled = self.msd._scales(x, lambda f, v: v)
        return self._chains(x, pooled, "forward_second_half")
