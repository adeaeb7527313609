"""CTC loss seam: ``ctc_loss_fn(log_probs(T,B,C), targets, input_lengths, target_lengths)`` with
torch.nn.CTCLoss(blank, reduction) semantics (exp/train.py:104,249), computed by csrc/ctc.hip; and the wild-card CTC loss of the
reference's lcasr/losses/wctc.py (``wctc_loss`` / ``WCTCLoss``), computed by csrc/wctc.hip."""
import torch

from . import functional as Fn


class CTCLoss(torch.nn.Module):
    def __init__(self, blank: int = 0, reduction: str = 'mean', zero_infinity: bool = False):
        super().__init__()
        if zero_infinity:
            raise NotImplementedError('zero_infinity=True is not used by the reference training loop')
        if reduction not in ('none', 'sum', 'mean'):
            raise ValueError(f'bad reduction {reduction}')
        self.blank, self.reduction = blank, reduction

    def forward(self, log_probs, targets, input_lengths, target_lengths):
        """log_probs: (T, B, C) f32 log-probabilities — typically ``out['final_posteriors'].transpose(0, 1)``,
        which is a zero-copy view of the batch-major tensor the kernels consume."""
        Fn.ops.require_gpu(log_probs, 'log_probs')
        nll = Fn.ctc_nll(log_probs.transpose(0, 1), targets, input_lengths, target_lengths, self.blank)
        if self.reduction == 'none':
            return nll
        if self.reduction == 'sum':
            return nll.sum()
        tl = target_lengths.to(nll.device).clamp_min(1).to(nll.dtype)
        return (nll / tl).mean()


def wctc_loss(log_probs, targets, input_lengths, target_lengths, blank: int = 0, reduction: str = 'none',
              finfo_min_fp32: float = torch.finfo(torch.float32).min, finfo_min_fp16: float = torch.finfo(torch.float16).min,
              alignment: bool = False, mode: str = 'soft', return_mean: bool = False, zero_infinity: bool = False):
    """The reference's wctc_loss (lcasr/losses/wctc.py:7), its signature kept: log_probs (T, B, C) f32 time-major on the GPU, the
    (B,) vector of losses or, with return_mean, its mean.  `reduction` and `zero_infinity` are accepted and ignored exactly as the
    reference ignores them; `finfo_min_*` and `alignment` are accepted and ignored (unreachable states are exact zeros here).
    Where this departs from the reference - input_lengths is honoured, an infeasible sample gives +inf, an empty transcript is
    refused - is stated in include/sconf_wctc.h."""
    Fn.ops.require_gpu(log_probs, 'log_probs')
    if log_probs.dtype != torch.float32:
        raise TypeError(f'wctc_loss: f32 log-probs only, got {log_probs.dtype}')
    nll = Fn.wctc_nll(log_probs.transpose(0, 1), targets, input_lengths, target_lengths, blank, mode)
    return nll.mean() if return_mean else nll


class WCTCLoss(torch.nn.CTCLoss):
    """The reference's WCTCLoss (lcasr/losses/wctc.py:71) with the mode as a keyword: 'soft' (the reference's default),
    'max_prob' or 'sum_prob'."""

    def __init__(self, blank: int = 0, reduction: str = 'mean', zero_infinity: bool = False, mode: str = 'soft'):
        super().__init__(blank=blank, reduction=reduction, zero_infinity=zero_infinity)
        Fn._wctc.mode_id(mode)
        self.mode = mode

    def forward(self, log_probs, targets, input_lengths, target_lengths):
        return wctc_loss(log_probs, targets, input_lengths, target_lengths, blank=self.blank, reduction=self.reduction,
                         zero_infinity=self.zero_infinity, mode=self.mode)
