"""UnivNet discriminator — drop-in for the reference ``models/vocoder/UnivNet.py``.

``Discriminator`` (:23-103): the multi-resolution spectral discriminator (MRSD)
plus the HiFi-GAN multi-period discriminator, outputs concatenated with the
MRSD's first.  Same constructor arguments, sub-module names and ``state_dict``
keys.  The three spectral chains (sel.sconvops.SpecChainFn on the channels-last
2-D conv kernels) and the five period chains (sel.dconvops.ChainFn) run as
independent chains on side streams, as ``HiFiGAN.Discriminator`` does.

Reference quirk kept: each spectral sub-discriminator contributes its last
layer's TENSOR (B, 1, H', W'), not a list of layer outputs, so the adversarial
losses take the whole tensor and the feature-matching loss iterates over its
batch dimension.
"""
import torch.nn as nn

from models.vocoder.modules.discriminator import HiFiGANMultiPeriodDiscriminator
from models.vocoder.modules.discriminator import UnivNetMultiResolutionSpectralDiscriminator
from sel.streams import run_concurrent


class Discriminator(nn.Module):
    """UnivNet multi-resolution spectrogram + multi-period discriminator module."""

    def __init__(self, fft_sizes=[1024, 2048, 512], hop_sizes=[120, 240, 50], win_lengths=[600, 1200, 240],
                 window="hann_window",
                 spectral_discriminator_params={"channels": 32,
                                                "kernel_sizes": [(3, 9), (3, 9), (3, 9), (3, 9), (3, 3), (3, 3)],
                                                "strides": [(1, 1), (1, 2), (1, 2), (1, 2), (1, 1), (1, 1)],
                                                "bias": True, "nonlinear_activation": "LeakyReLU",
                                                "nonlinear_activation_params": {"negative_slope": 0.2}},
                 periods=[2, 3, 5, 7, 11],
                 period_discriminator_params={"in_channels": 1, "out_channels": 1, "kernel_sizes": [5, 3],
                                              "channels": 32, "downsample_scales": [3, 3, 3, 3, 1],
                                              "max_downsample_channels": 1024, "bias": True,
                                              "nonlinear_activation": "LeakyReLU",
                                              "nonlinear_activation_params": {"negative_slope": 0.1},
                                              "use_weight_norm": True, "use_spectral_norm": False},
                 flat_channel=False):
        super().__init__()
        self.flat_channel = flat_channel
        self.mrsd = UnivNetMultiResolutionSpectralDiscriminator(fft_sizes=fft_sizes, hop_sizes=hop_sizes,
                                                                win_lengths=win_lengths, window=window,
                                                                discriminator_params=spectral_discriminator_params)
        self.mpd = HiFiGANMultiPeriodDiscriminator(periods=periods, discriminator_params=period_discriminator_params)

    def forward(self, x):
        """x (B, C, T) -> [3 spectral tensors (B, 1, H', W')] + [5 lists of the
        period discriminators' layer outputs] (UnivNet.py:86-103)."""
        batch, channel, time = x.size()
        if channel != 1 and self.flat_channel:
            x = x.reshape(batch * channel, 1, time)
        fs = list(self.mrsd.discriminators) + list(self.mpd.discriminators)
        return run_concurrent([(lambda f=f: f(x)) for f in fs], [x])
