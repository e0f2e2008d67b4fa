"""mel_spectrogram.py drop-in: the eval Mel-L1 metric (reference :38-44) and
the measures of its ``print_measures`` (:47-64).

The reference builds ``mel_spectrogram = torchaudio.transforms.MelSpectrogram(48000)``
and ``Mel_L1(pred, target) = L1(mel(pred), mel(target))``.  ``measures()``
returns what ``print_measures`` prints, for the eight of its nine measures that
exist here (sel.metrics; the BSS-eval SDR on request); its remaining module-level code (soundfile I/O,
plots, :66-118) is not part of the hot path and is not reproduced.

``MelSpectrogram`` mirrors torchaudio's transform signature and defaults
(n_fft 400, hop = win // 2, periodic Hann, center/reflect, onesided, power 2,
HTK mel scale, no norm) and runs the sel_power_mel_fwd HIP kernel (mixed-radix
FFT for n_fft = 400).  Only the defaults' feature set is implemented: other
options raise instead of silently differing.
"""
import torch
from torch import nn

from sel import spectral as S
from sel.melbank import htk_fbanks


class MelSpectrogram(nn.Module):
    """torchaudio.transforms.MelSpectrogram (2.1.1) on the MI355X path."""

    def __init__(self, sample_rate=16000, n_fft=400, win_length=None, hop_length=None, f_min=0.0, f_max=None,
                 pad=0, n_mels=128, window_fn=torch.hann_window, power=2.0, normalized=False, wkwargs=None,
                 center=True, pad_mode="reflect", onesided=None, norm=None, mel_scale="htk"):
        super().__init__()
        unsupported = {"pad": pad != 0, "normalized": bool(normalized), "center": not center,
                       "pad_mode": pad_mode != "reflect", "onesided": onesided is False, "norm": norm is not None,
                       "mel_scale": mel_scale != "htk", "power": power is None}
        bad = [k for k, v in unsupported.items() if v]
        if bad:
            raise NotImplementedError(f"sel MelSpectrogram: options {bad} differ from the reference's defaults")
        self.sample_rate = sample_rate
        self.n_fft = n_fft
        self.win_length = win_length if win_length is not None else n_fft
        self.hop_length = hop_length if hop_length is not None else self.win_length // 2
        self.power = float(power)
        self.n_mels = n_mels
        self.f_min = f_min
        self.f_max = f_max if f_max is not None else float(sample_rate // 2)
        window = window_fn(self.win_length) if wkwargs is None else window_fn(self.win_length, **wkwargs)
        self.register_buffer("window", window.float())
        fb = htk_fbanks(n_fft // 2 + 1, float(f_min), self.f_max, n_mels, sample_rate)
        self.register_buffer("fb", fb)
        kr, _ = S.mel_ranges(fb)
        self.register_buffer("krange", kr, persistent=False)

    def forward(self, waveform, lengths=None):
        """With lengths (not in torchaudio's signature) row b is its
        first lengths[b] samples and the call returns (mel, frames): frames[b] =
        1 + lengths[b] // hop_length (device int64), the frames of mel past them
        are zero.  Host lengths are checked against [n_fft // 2 + 1, time]."""
        shape = waveform.shape
        x = waveform.reshape(-1, shape[-1]).float()
        if lengths is not None:
            out, frames = S.power_mel(x, self.n_fft, self.hop_length, self.win_length, self.window, self.fb,
                                      self.krange, self.power, lengths=lengths)
            return out.reshape(shape[:-1] + out.shape[-2:]), frames.reshape(shape[:-1])
        out = S.power_mel(x, self.n_fft, self.hop_length, self.win_length, self.window, self.fb, self.krange,
                          self.power)
        return out.reshape(shape[:-1] + out.shape[-2:])


mel_spectrogram = MelSpectrogram(48000)
mae = nn.L1Loss()


def Mel_L1(pred, target):
    """reference :40-44; the module buffers follow the input's device."""
    if mel_spectrogram.window.device != pred.device:
        mel_spectrogram.to(pred.device)
    with torch.no_grad():
        return mae(mel_spectrogram(pred), mel_spectrogram(target))


def _measures_var(waveform1, waveform2, sample_rate, sdr, lengths):
    """(per-row values, batch means) of the measures over a ragged batch: every
    measure through its *_var entry point on one device lengths array."""
    from sel import _lib as L
    from sel import metrics as M
    if waveform1.shape != waveform2.shape:
        raise ValueError(f"measures: {tuple(waveform1.shape)} and {tuple(waveform2.shape)} differ in shape")
    T = waveform1.shape[-1]
    B = waveform1.numel() // T if T else 0
    if lengths is None:
        L.need_device(waveform1, waveform2)
        lengths = torch.full((B,), T, dtype=torch.int64, device=waveform1.device)
    lens = L.lengths_arg(lengths, B, T, max(M.stoi_min_length(sample_rate), mel_spectrogram.n_fft // 2 + 1),
                         waveform1.device, "measures")
    L.need_device(waveform1, waveform2)
    if mel_spectrogram.window.device != waveform1.device:
        mel_spectrogram.to(waveform1.device)
    rows, means = {}, {}
    with torch.no_grad():
        w1 = waveform1.detach().reshape(B, T).float().contiguous()
        w2 = waveform2.detach().reshape(B, T).float().contiguous()
        rows["MAE"], rows["MSE"], m = M.rows_l1_l2(w1, w2, lens, means=True)
        means["MAE"], means["MSE"] = m[0], m[1]
        rows["SNR"], means["SNR"] = M._sdr_family(w1, w2, False, False, lens)
        if sdr:
            rows["SDR"], means["SDR"] = M._bss_sdr(w1, w2, 512, False, 0.0, lens)
        rows["SI-SDR(True)"], means["SI-SDR(True)"] = M._sdr_family(w1, w2, True, True, lens)
        rows["SI-SDR(False)"], means["SI-SDR(False)"] = M._sdr_family(w1, w2, True, False, lens)
        rows["STOI"], means["STOI"] = M._stoi(w1, w2, sample_rate, False, lens)
        m1, frames = mel_spectrogram(w1, lengths=lens)
        m2, _ = mel_spectrogram(w2, lengths=lens)
        rows["Mel-L1"], _, m = M.rows_l1_l2(m1, m2, frames, means=True)
        means["Mel-L1"] = m[0]
    return rows, means


def measures_rows(waveform1, waveform2, sample_rate=48000, sdr=False, lengths=None):
    """The keys of measures() with (B,) device tensors: one value per row of the
    (B, T) batch.  With lengths (a device int64 tensor, used as it is, or a host
    sequence, checked) row b is its first lengths[b] samples and nothing past
    them is read; each row's kernel measures have the bits of a call on that row
    alone.  MAE, MSE and Mel-L1 are per-row means accumulated in fp64
    (sel_rows_l1_l2_var); Mel-L1 averages over the row's own 1 + lengths[b] // 200
    frames."""
    return _measures_var(waveform1, waveform2, sample_rate, sdr, lengths)[0]


def measures(waveform1, waveform2, sample_rate=48000, sdr=False, lengths=None):
    """With lengths the batch is ragged: row b is its first
    lengths[b] samples, and EVERY key is the mean over rows of the per-row value
    (measures_rows).  For MAE, MSE and Mel-L1 that is a mean of per-row means, not
    the mean over all elements; for equal lengths the two coincide up to rounding.
    Without lengths:

    The reference's print_measures (:47-64) as a dict of 0-d device tensors:
    every measure is called as measure(waveform1, waveform2), i.e. waveform1 is
    the prediction and waveform2 the target / clean signal.  Keys, as the
    reference names them: MAE, MSE, SNR, SI-SDR(True), SI-SDR(False), STOI,
    Mel-L1.  With sdr=True the dict also has SDR (torchmetrics'
    SignalDistortionRatio with its defaults, a 512-tap BSS-eval filter solve:
    sel.metrics.SignalDistortionRatio) between SNR and SI-SDR(True), where the
    reference prints it.  Absent: PESQ (the ITU-T P.862 reference program, which
    cannot be restated).  Mel-L1 uses the module's 48 kHz mel transform whatever
    sample_rate is, as the reference does."""
    from sel import _lib as L
    from sel import metrics as M
    if lengths is not None:
        return _measures_var(waveform1, waveform2, sample_rate, sdr, lengths)[1]
    L.need_device(waveform1, waveform2)
    with torch.no_grad():
        out = {
            "MAE": mae(waveform1, waveform2),
            "MSE": nn.functional.mse_loss(waveform1, waveform2),
            "SNR": M.SignalNoiseRatio()(waveform1, waveform2),
        }
        if sdr:
            out["SDR"] = M.SignalDistortionRatio()(waveform1, waveform2)
        out.update({
            "SI-SDR(True)": M.ScaleInvariantSignalDistortionRatio(zero_mean=True)(waveform1, waveform2),
            "SI-SDR(False)": M.ScaleInvariantSignalDistortionRatio(zero_mean=False)(waveform1, waveform2),
            "STOI": M.ShortTimeObjectiveIntelligibility(sample_rate)(waveform1, waveform2),
            "Mel-L1": Mel_L1(waveform1, waveform2),
        })
        return out
