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
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from .. import functional as Fn          # Fn.ops: the HIP op layer (tests swap it for the CPU kernel references)


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
