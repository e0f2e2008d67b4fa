"""Multi-fusion modules of the HiFi-GAN generator — drop-in for the reference
``models/vocoder/modules/multi_fusion.py`` (:23-141).

* ``MultiReceptiveField``: the mean over the residual blocks is accumulated by
  each block's last conv epilogue (no add / divide launches).
* ``MultiGroupConv1d``: ``x.repeat(1, groups, 1)`` is never materialised in
  ``forward``: the first layer's grouped conv reads the same channels for every
  group (``in_group_stride`` 0) and its residual likewise.
Inference only (sel.hfgops).
"""
import torch
import torch.nn as nn

from layers.conv_layer import Conv1d1x1
from models.vocoder.modules.residual_block import HiFiGANResidualBlock
from sel import hfgops as HF


class MultiReceptiveField(nn.Module):
    """Multi-receptive field module in HiFiGAN."""

    def __init__(self, channels=512, resblock_kernel_sizes=(3, 7, 11),
                 resblock_dilations=[(1, 3, 5), (1, 3, 5), (1, 3, 5)], groups=1, bias=True,
                 use_additional_convs=True, nonlinear_activation="LeakyReLU",
                 nonlinear_activation_params={"negative_slope": 0.1}):
        assert len(resblock_kernel_sizes) == len(resblock_dilations)
        super().__init__()
        self.num_blocks = len(resblock_kernel_sizes)
        self.blocks = nn.ModuleList()
        for i in range(self.num_blocks):
            self.blocks += [HiFiGANResidualBlock(kernel_size=resblock_kernel_sizes[i], channels=channels,
                                                 dilations=resblock_dilations[i], groups=groups, bias=bias,
                                                 use_additional_convs=use_additional_convs,
                                                 nonlinear_activation=nonlinear_activation,
                                                 nonlinear_activation_params=nonlinear_activation_params)]

    def _run(self, c, stream):
        slope = HF.slope_of(self.blocks[0].activation)
        return HF.mrf(HF.enter(c), list(self.blocks), slope, stream=stream).transpose(1, 2)

    def forward(self, c):
        """c (B, channels, T) -> (B, channels, T)."""
        HF.require_inference(self, c)
        return self._run(c, False)

    @torch.no_grad()
    def inference(self, c):
        return self._run(c, True)


class MultiGroupConv1d(HiFiGANResidualBlock):
    """Multi-group convolution module."""

    def __init__(self, channels=512, resblock_kernel_sizes=(3), resblock_dilations=[(1, 3, 5)], groups=3, bias=True,
                 use_additional_convs=True, nonlinear_activation="LeakyReLU",
                 nonlinear_activation_params={"negative_slope": 0.1}):
        assert len(resblock_kernel_sizes) == len(resblock_dilations) == 1
        super().__init__(kernel_size=resblock_kernel_sizes[0], channels=channels * groups,
                         dilations=resblock_dilations[0], groups=groups, bias=bias,
                         use_additional_convs=use_additional_convs, nonlinear_activation=nonlinear_activation,
                         nonlinear_activation_params=nonlinear_activation_params)
        self.groups = groups
        self.conv_out = Conv1d1x1(in_channels=channels * groups, out_channels=channels, bias=False)

    def forward(self, x):
        """x (B, channels, T) -> (B, channels, T)."""
        HF.require_inference(self, x)
        y = HF.resblock(HF.enter(x), self, HF.slope_of(self.activation), shared_first=True)
        return HF.pointwise(y, self.conv_out).transpose(1, 2)

    @torch.no_grad()
    def inference(self, x):
        # the streaming buffers hold all channels * groups rows of the repeated input (they are
        # state_dict entries), so the repeat is materialised here: a few rows per step
        xr = HF.enter(x).repeat(1, 1, self.groups)
        y = HF.resblock(xr, self, HF.slope_of(self.activation), stream=True)
        return HF.pointwise(y, self.conv_out).transpose(1, 2)
