"""Residual block of the HiFi-GAN generator — drop-in for the reference
``models/vocoder/modules/residual_block.py`` (:23-106): same constructor
arguments, sub-module names and ``state_dict`` keys.  ``forward`` and
``inference`` run sel.hfgops: both LeakyReLUs of a layer in the conv kernels'
prologues, the residual add in the second conv's epilogue.  Inference only.
"""
import torch
import torch.nn as nn

from layers.conv_layer import CausalConv1d
from sel import hfgops as HF


class HiFiGANResidualBlock(nn.Module):
    """Causal Residual block module in HiFiGAN."""

    def __init__(self, kernel_size=3, channels=512, dilations=(1, 3, 5), groups=1, bias=True,
                 use_additional_convs=True, nonlinear_activation="LeakyReLU",
                 nonlinear_activation_params={"negative_slope": 0.1}):
        super().__init__()
        self.use_additional_convs = use_additional_convs
        self.convs1 = nn.ModuleList()
        if use_additional_convs:
            self.convs2 = nn.ModuleList()
        assert kernel_size % 2 == 1, "Kernel size must be odd number."
        self.activation = getattr(nn, nonlinear_activation)(**nonlinear_activation_params)
        for dilation in dilations:
            self.convs1 += [CausalConv1d(in_channels=channels, out_channels=channels, kernel_size=kernel_size,
                                         stride=1, dilation=dilation, groups=groups, bias=bias)]
            if use_additional_convs:
                self.convs2 += [CausalConv1d(in_channels=channels, out_channels=channels, kernel_size=kernel_size,
                                             stride=1, dilation=1, groups=groups, bias=bias)]
        self.num_layer = len(self.convs1)

    def forward(self, x):
        """x (B, channels, T) -> (B, channels, T)."""
        HF.require_inference(self, x)
        return HF.resblock(HF.enter(x), self, HF.slope_of(self.activation)).transpose(1, 2)

    @torch.no_grad()
    def inference(self, x):
        return HF.resblock(HF.enter(x), self, HF.slope_of(self.activation), stream=True).transpose(1, 2)
