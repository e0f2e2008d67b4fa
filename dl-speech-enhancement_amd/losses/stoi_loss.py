"""Intelligibility loss (not in the reference): 1 - STOI, or 1 - ESTOI, of the
prediction against the clean target, as the end-to-end STOI-loss papers and
torch_stoi use it, on the sel_stoi / sel_stoi_bwd HIP kernels.
Gradients flow to the prediction only: the target is data and the silent-frame
mask, which comes from the target, is a constant selection."""
import torch

from sel import metrics as M

__all__ = ["STOILoss"]


class STOILoss(torch.nn.Module):
    """forward(pred, target) -> the scalar 1 - mean_b d_b; (B, T) or (B, 1, T) at
    `fs` Hz (resampled to 10 kHz on the device when fs != 10000)."""

    def __init__(self, fs, extended=False):
        super().__init__()
        if int(fs) <= 0:
            raise ValueError("STOILoss: fs must be positive")
        self.fs = int(fs)
        self.extended = bool(extended)

    def forward(self, pred, target):
        if pred.shape != target.shape or pred.dim() not in (2, 3) or (pred.dim() == 3 and pred.shape[1] != 1):
            raise ValueError(f"STOILoss: pred {tuple(pred.shape)} and target {tuple(target.shape)} must both be "
                             f"(B, T) or (B, 1, T)")
        return 1.0 - M._stoi_grad(pred, target, self.fs, self.extended)[1]
