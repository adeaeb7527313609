"""SpecAugment — mirror of lcasr/utils/augmentation.py:10-100 (same constructor and forward), masking on the GPU.

The reference applies `n_time_masks` + `n_freq_masks` calls of torchaudio's `mask_along_axis[_iid]`, each a `masked_fill`
pass over the batch with the spectrogram mean (or 0) as fill value, the mean reaching the host in between.  Here the module
is split in two so that the random draw and the kernel can be tested apart:

    draw(shape, generator)                     -> (t_iv, f_iv): int32 half-open [start, end) intervals on the device
    apply(specgram, t_iv, f_iv, mask_value)    -> ops.spec_mask: ONE pass that fills the union of the bands

and the fill value stays a device scalar (ops.mean_f32), so nothing syncs.  All masks fill the same value, hence the union
equals the reference's sequence of masked_fills.

INTERVAL LAW.  torchaudio is not available where this was written; the law below is taken from its documentation of
`mask_along_axis` / `mask_along_axis_iid` and is the specification here.  With `size` the length of the masked axis:

    mask_param' = mask_param                      if p == 1.0
                = min(mask_param, int(size * p))  otherwise
    mask_param' < 1: nothing is masked; else
    value = U[0,1) * mask_param',  min_value = U[0,1) * (size - value),
    interval [floor(min_value), floor(min_value) + floor(value))

so a mask is at most mask_param' wide and lies inside the axis.  Bit-equal random streams with torchaudio are not a goal.

AddGaussianSNR and AddBackgroundNoise are the two waveform corruptions of the reference's noise-robustness drivers
(eval/rev16_gaussian_noise/run.py, eval/rev16_background_noise/run.py), with audiomentations' constructor keywords and call
signature and the mixing on the device (utils/audio_tools.py: add_gaussian_snr, add_background_noise).  What a call draws - whether
it applies, the SNR, the clip and where it starts - comes from a random.Random(seed) on the host, in that order; nothing is read
back from the device.  Bit-equal noise with numpy's generator is not a goal: the normals are the contract of include/sconf_noise.h.
"""
from __future__ import annotations

import random
from typing import Optional, Sequence, Tuple

import torch

from .. import functional as Fn          # Fn.ops: the HIP op layer (tests swap it for the CPU kernel references)
from . import audio_tools


class SpecAugment(torch.nn.Module):
    def __init__(self, n_time_masks: int, n_freq_masks: int, freq_mask_param: int, iid_masks: bool = True, time_mask_param: int = -1,
                 min_p: float = -1, max_p: float = 1.0, zero_masking: bool = False, **kwargs) -> None:
        super().__init__()
        if n_time_masks != 0: assert (min_p != -1 or time_mask_param != -1), 'Either min_p or n_time_masks must be set o:'
        assert min_p == -1 or (min_p >= 0 and min_p <= 1), 'min_p must be within range [0.0, 1.0]'
        assert max_p >= 0 and max_p <= 1, 'max_p must be within range [0.0, 1.0]'
        self.n_time_masks = n_time_masks
        self.time_mask_param = time_mask_param
        self.n_freq_masks = n_freq_masks
        self.freq_mask_param = freq_mask_param
        self.iid_masks = iid_masks
        self.max_p = max_p
        self.zero_masking = zero_masking
        self.min_p = min_p

    def time_mask_width(self, t: int) -> int:
        """augmentation.py:78-81: with min_p the masks together cover int(t * min_p) frames."""
        if self.min_p != -1:
            return int(int(t * self.min_p) / self.n_time_masks) if self.n_time_masks != 0 else 0
        return self.time_mask_param

    def _intervals(self, rows: int, n: int, size: int, mask_param: int, generator, device) -> torch.Tensor:
        mp = mask_param if self.max_p == 1.0 else min(mask_param, int(size * self.max_p))
        if n == 0 or mp < 1:
            return torch.zeros(rows, n, 2, dtype=torch.int32, device=device)
        gdev = generator.device if generator is not None else device
        u = torch.rand(2, rows, n, generator=generator, device=gdev).to(device=device, dtype=torch.float64)
        value = u[0] * mp
        start = torch.floor(u[1] * (size - value))
        end = torch.clamp(start + torch.floor(value), max=size)
        return torch.stack([start, end], dim=-1).to(torch.int32).contiguous()

    def draw(self, shape, generator: Optional[torch.Generator] = None, device=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """Intervals for a spectrogram of `shape` (..., freq, time): t_iv (B, n_time_masks, 2) and f_iv (B, n_freq_masks, 2),
        B = product of the leading axes (1 without one).  One draw per example when iid_masks and there is a batch axis
        (mask_along_axis_iid, augmentation.py:83-93), one shared set otherwise (mask_along_axis, :95-98)."""
        shape = tuple(shape)
        f, t = shape[-2:]
        B = 1
        for s in shape[:-2]: B *= int(s)
        if device is None:
            device = generator.device if generator is not None else ('cuda' if torch.cuda.is_available() else 'cpu')
        rows = B if (len(shape) > 2 and self.iid_masks is True) else 1
        t_iv = self._intervals(rows, self.n_time_masks, t, self.time_mask_width(t), generator, device)
        f_iv = self._intervals(rows, self.n_freq_masks, f, self.freq_mask_param, generator, device)
        if rows != B:
            t_iv, f_iv = t_iv.expand(B, -1, -1).contiguous(), f_iv.expand(B, -1, -1).contiguous()
        return t_iv, f_iv

    def apply(self, specgram: torch.Tensor, t_iv: torch.Tensor, f_iv: torch.Tensor, mask_value, batch: Optional[int] = None) -> torch.Tensor:
        """specgram (..., freq, time) with row b's bands filled with mask_value (a device scalar tensor or a number).
        batch: broadcast a single spectrogram to that many rows (the repeat + clone of dynamic_eval.py:84-86 in the same pass)."""
        f, t = specgram.shape[-2:]
        x = specgram.reshape(-1, f, t).to(torch.float32).contiguous()
        if not torch.is_tensor(mask_value):
            mask_value = torch.full((), float(mask_value), dtype=torch.float32, device=x.device)
        mask_value = mask_value.to(device=x.device, dtype=torch.float32).reshape(())
        out = Fn.ops.spec_mask(x, t_iv.to(x.device), f_iv.to(x.device), mask_value, batch)
        return out if batch is not None else out.reshape(specgram.shape)

    def mask_value(self, specgram: torch.Tensor, audio_lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
        """0, or the mean of the spectrogram (over t < audio_lengths[b] if given), augmentation.py:70-73 - a device scalar."""
        if self.zero_masking:
            return torch.zeros((), dtype=torch.float32, device=specgram.device)
        x = specgram.to(torch.float32).contiguous()
        if audio_lengths is None:
            return Fn.ops.mean_f32(x)
        return Fn.ops.mean_f32(x, audio_lengths.to(device=x.device, dtype=torch.int32).contiguous())

    def forward(self, specgram: torch.Tensor, audio_lengths: Optional[torch.Tensor] = None, generator: Optional[torch.Generator] = None) -> torch.Tensor:
        """specgram (..., freq, time) on the GPU -> masked copy of the same shape (augmentation.py:61-100)."""
        Fn.ops.require_gpu(specgram, 'specgram')
        t_iv, f_iv = self.draw(specgram.shape, generator, specgram.device)
        return self.apply(specgram, t_iv, f_iv, self.mask_value(specgram, audio_lengths))


class _SNRTransform:
    """What the two corruptions share: the keywords, the host generator and the draw of `apply or not` and of the SNR."""

    def __init__(self, min_snr_db: float, max_snr_db: float, p: float, seed: Optional[int]) -> None:
        if min_snr_db > max_snr_db:
            raise ValueError(f'min_snr_db = {min_snr_db} must not exceed max_snr_db = {max_snr_db}')
        if not 0 <= p <= 1:
            raise ValueError(f'p = {p} must be within [0, 1]')
        self.min_snr_db, self.max_snr_db, self.p = float(min_snr_db), float(max_snr_db), float(p)
        self.rng = random.Random(seed)
        self.calls = 0                                                     # applied calls so far: the row id of the next one's normals

    def draw_snr(self) -> Optional[float]:
        """None where this call leaves the waveform alone, else the SNR in dB."""
        if self.rng.random() >= self.p:
            return None
        return self.rng.uniform(self.min_snr_db, self.max_snr_db)


class AddGaussianSNR(_SNRTransform):
    """audiomentations.AddGaussianSNR(min_snr_db, max_snr_db, p) on the device.  The normals' key is `seed` (17925, the reference's
    per-file numpy seed, where None) and the n-th applied call takes row id n of them, so that successive files get different noise
    and a transform rebuilt with the same seed repeats it."""

    def __init__(self, min_snr_db: float = 5.0, max_snr_db: float = 40.0, p: float = 0.5, seed: Optional[int] = None) -> None:
        super().__init__(min_snr_db, max_snr_db, p, seed)
        self.noise_seed = 17925 if seed is None else int(seed)

    def __call__(self, waveform: torch.Tensor, sample_rate: int = 16000) -> torch.Tensor:
        snr = self.draw_snr()
        if snr is None:
            return waveform
        rows = 1 if waveform.dim() == 1 else waveform.shape[0]
        out = audio_tools.add_gaussian_snr(waveform, snr, seed=self.noise_seed, first_row=self.calls)
        self.calls += rows
        return out


class AddBackgroundNoise(_SNRTransform):
    """audiomentations.AddBackgroundNoise(sounds, min_snr_db, max_snr_db, p) on the device.  `sounds`: a list of 1-D float32 device
    tensors at 16 kHz (decoding files stays with the caller).  Per applied call one clip is chosen; where it is longer than the
    waveform it is cropped at a drawn offset in 0 .. len(clip) - len(waveform), where it is not it starts at 0 and repeats."""

    def __init__(self, sounds: Sequence[torch.Tensor], min_snr_db: float = 3.0, max_snr_db: float = 30.0, p: float = 0.5,
                 seed: Optional[int] = None) -> None:
        super().__init__(min_snr_db, max_snr_db, p, seed)
        self.sounds = list(sounds)
        if not self.sounds or any(not torch.is_tensor(s) or s.dim() != 1 or s.shape[0] < 1 for s in self.sounds):
            raise ValueError('sounds must be a non-empty list of non-empty 1-D tensors')

    def draw(self, length: int) -> Optional[Tuple[float, int, int]]:
        """(snr_db, index of the clip, offset into it) of one call on a waveform of `length` samples, or None."""
        snr = self.draw_snr()
        if snr is None:
            return None
        which = self.rng.randrange(len(self.sounds))
        spare = self.sounds[which].shape[0] - length
        return snr, which, self.rng.randint(0, spare) if spare > 0 else 0

    def __call__(self, waveform: torch.Tensor, sample_rate: int = 16000) -> torch.Tensor:
        drawn = self.draw(waveform.shape[-1])
        if drawn is None:
            return waveform
        snr, which, offset = drawn
        rows = 1 if waveform.dim() == 1 else waveform.shape[0]
        self.calls += rows
        return audio_tools.add_background_noise(waveform, self.sounds[which], snr, offsets=[offset] * rows)
