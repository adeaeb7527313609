"""Attention (lcasr/components/attention.py:448-551): fused qkv Linear (no bias by default) with the
reference's "(h d qkv)" column order, NeoX rotary on q,k, bidirectional softmax attention with optional
sliding window and key padding, output Linear.  FlashSelfAttention / SDPA are replaced by csrc/attention.hip."""
import os

import torch
import torch.nn as nn

from .. import functional as Fn


def get_window_size(kwargs, direction=None):
    """attention.py:321-328."""
    if direction is None:
        return kwargs.get('attention_window_size', -1)
    if kwargs.get(f'attention_window_size_{direction}', None) is not None:
        return kwargs.get(f'attention_window_size_{direction}')
    return kwargs.get('attention_window_size', -1)


class ReturnAttention(nn.Module):
    """attention.py:424-445.  The reference's module recomputes the attention on the host and returns (out, a_weight); here the
    fused forward has already produced the block's output, and this module only materialises the scaled pre-softmax scores
    (B,H,N,N) on the device (csrc/attn_maps.hip).  Its forward returns (None, scores), so a `register_forward_hook` on
    `Attention.return_attention_module` sees the scores as output[1], as in the reference.  Masked positions - keys and query
    rows past `lengths`, keys outside the module's window - are -inf (the reference has no working masked case).
    `dtype`: torch.float32 (default) or torch.bfloat16 storage of the scores."""

    def __init__(self):
        super().__init__()
        self.dtype = torch.float32

    def forward(self, q, k, lse=None, lengths=None, window=(-1, -1)):
        return None, Fn.ops.attn_scores(q, k, lengths, window, out_dtype=self.dtype)


class ReturnAttentionOffsets(nn.Module):
    """The long-context statistic: forward returns (profile (B,H,2N-1) f32, live_rows (B,) int64), both on the device;
    profile[b, h, delta + N - 1] is the attention probability summed over the diagonal j - i = delta, live_rows the number of
    query rows that are not padding.  No N x N tensor exists at any point (csrc/attn_maps.hip)."""

    def forward(self, q, k, lse, lengths=None, window=(-1, -1)):
        B, N = q.shape[0], q.shape[1]
        live = lengths.to(torch.int64) if lengths is not None else torch.full((B,), N, dtype=torch.int64, device=q.device)
        return Fn.ops.attn_offset_profile(q, k, lse, lengths, window), live


class Attention(nn.Module):
    def __init__(self, n_feats, head_dim, n_heads, dropout=0.0, **kwargs):
        super().__init__()
        if dropout != 0.0:
            raise NotImplementedError('attention dropout is 0 in every SConformerXL config')
        if kwargs.get('causal', False):
            raise NotImplementedError('causal attention is not on the hot path')
        self.layer_idx = kwargs.get('layer_idx', None)
        self.n_feats, self.head_dim, self.n_heads = n_feats, head_dim, n_heads
        self.dropout_p = dropout
        self.left_window, self.right_window = get_window_size(kwargs, 'left'), get_window_size(kwargs, 'right')
        self.causal = False
        self.return_attention_weights = kwargs.get('return_attention_weights', False)
        self.return_attention_offsets = kwargs.get('return_attention_offsets', False)
        self.return_attention_module = ReturnAttention()
        self.return_offsets_module = ReturnAttentionOffsets()
        self.qkv_proj = nn.Linear(n_feats, 3 * n_heads * head_dim, bias=kwargs.get('qkv_bias', False))
        self.out_proj = nn.Linear(n_heads * head_dim, n_feats, bias=kwargs.get('bias', False))

    def forward_prenorm(self, x, norm, residual, lengths=None, rotary=None, **_):
        """x (B,N,d) f32.  lengths: int32 (B,) device tensor or None.  rotary: (cos, sin) compact tables or None.
        norm None: x is already normalised (the module-level `forward`)."""
        B, N, _d = x.shape
        nw, nb = norm.norm_params() if norm is not None else (None, None)
        mode, eps = (norm.mode, norm.eps) if norm is not None else ('none', 0.0)
        cos, sin = rotary if rotary is not None else (None, None)
        if self.return_attention_weights or self.return_attention_offsets:
            return self._forward_observed(x, nw, nb, cos, sin, lengths, mode, eps, residual)
        y = Fn.attn_block(x.reshape(B * N, -1), nw, nb, self.qkv_proj.weight, self.out_proj.weight, self.qkv_proj.bias,
                          self.out_proj.bias, cos, sin, lengths, B, N, self.n_heads, self.head_dim,
                          (self.left_window, self.right_window), mode, eps, residual)
        return y.view(B, N, -1)

    def _forward_observed(self, x, nw, nb, cos, sin, lengths, mode, eps, residual):
        """forward_prenorm with return_attention_weights and / or return_attention_offsets set: the same kernels as the plain path
        (the output is bit-equal), outside autograd, then the observer modules - whose forward hooks are how the collectors below
        read the maps - on the post-rotary q, k and the row log-sum-exp, under the module's CURRENT windows."""
        flag = 'return_attention_weights' if self.return_attention_weights else 'return_attention_offsets'
        if self.training:
            raise RuntimeError(f'Attention.{flag} is an evaluation-time switch: call model.eval() (and run under torch.no_grad()), '
                               f'or clear {flag}.')
        B, N, _d = x.shape

        def observer(q, k, lse, lens, window):
            if self.return_attention_weights:
                self.return_attention_module(q, k, lse, lens, window)
            if self.return_attention_offsets:
                self.return_offsets_module(q, k, lse, lens, window)

        y = Fn.attn_block_observed(x.reshape(B * N, -1), nw, nb, self.qkv_proj.weight, self.out_proj.weight, self.qkv_proj.bias,
                                   self.out_proj.bias, cos, sin, lengths, B, N, self.n_heads, self.head_dim,
                                   (self.left_window, self.right_window), mode, eps, residual, observer, flag)
        return y.view(B, N, -1)

    def forward(self, x, attn_mask=None, length=None, pad_mask=None, flash_attn=True, rotary_emb_fn=None):
        """The reference's module-level call (attention.py:509-551) on an already normalised x (B,N,d).
        pad_mask (B,N) bool, True = padded position: must be the suffix mask sconformer_xl.py:207 builds from `length`;
        attn_mask carries the same information in the reference and is ignored here.  rotary_emb_fn: the reference's
        `apply_rotary` object (.cos/.sin of shape (1,n,1,D)) or a (cos, sin) pair of compact (n, D/2) tables."""
        B, N, _d = x.shape
        lengths = None
        if pad_mask is not None:
            lengths = (~pad_mask).sum(-1).to(dtype=torch.int32).contiguous()
        elif length is not None and int(length.max()) != int(length.min()):
            lengths = length.to(device=x.device, dtype=torch.int32).contiguous()
        rotary = None
        if rotary_emb_fn is not None:
            if isinstance(rotary_emb_fn, (tuple, list)):
                rotary = tuple(rotary_emb_fn)
            else:
                if getattr(rotary_emb_fn, 'learned', False):
                    raise NotImplementedError('learned rotary frequencies are not on the hot path')
                h = self.head_dim // 2
                rotary = (rotary_emb_fn.cos[0, :N, 0, :h].float().contiguous(), rotary_emb_fn.sin[0, :N, 0, :h].float().contiguous())
        return self.forward_prenorm(x, None, False, lengths=lengths, rotary=rotary)


class CollectAttentionProbs:
    """attention.py:556-595, same constructor and methods: pass a list of Attention modules; every model forward after that
    appends one (B,H,N,N) bf16 CPU tensor per module, `collector()` stacks them to (L,B,H,N,N) and clears.  With save_path every
    layer's tensor is also written with torch.save as `{save_prefix}_{idx}.pt` (or `layer_{idx}.pt`); discard=True keeps nothing in
    memory.  As in the reference, and despite the name, what is stored is the SCALED PRE-SOFTMAX SCORES (`a_weight`), not
    probabilities: softmax(-1) of the result gives them.  Masked positions are -inf.  The scores are produced on the device by
    csrc/attn_maps.hip (f32) and rounded to bf16 here, as the reference's hook does."""

    def __init__(self, attn_modules, discard=False, save_path=None, save_prefix=None):
        self.attn_modules = attn_modules
        self.attn_probs = []
        self.save_path = save_path
        self.save_prefix = save_prefix
        self.discard = discard
        self._handles = []
        for idx, module in enumerate(self.attn_modules):
            module.return_attention_weights = True
            self._handles.append(module.return_attention_module.register_forward_hook(self.get_attn_hook(idx)))

    def remove(self):
        """Not in the reference (whose collector stays attached for the life of the model): detach the hooks and clear the flag."""
        for h in self._handles: h.remove()
        self._handles = []
        for module in self.attn_modules: module.return_attention_weights = False

    def collect(self):
        return self.attn_probs

    def clear(self):
        self.attn_probs = []

    def __call__(self):
        probs = self.collect()
        if len(probs) == 0:
            print('No attention probabilities found! Make sure to call the model on some input first!')
        probs = torch.stack(probs, dim=0)
        self.clear()
        return probs

    def get_attn_hook(self, layer_idx):
        def attn_hook(module, input, output):
            out, a_weight = output
            a_weight = a_weight.detach().cpu().to(torch.bfloat16)
            if not self.discard: self.attn_probs.append(a_weight)
            if self.save_path is not None:
                name = f'{self.save_prefix}_{layer_idx}.pt' if self.save_prefix is not None else f'layer_{layer_idx}.pt'
                torch.save(a_weight, os.path.join(self.save_path, name))
            return out, a_weight
        return attn_hook


class CollectAttentionOffsets:
    """The collector for contexts where (B,H,N,N) does not fit anywhere: per module and forward one offset profile (B,H,2N-1) f32
    and the live-row counts (B,), both moved to the CPU.  `collector()` returns (profiles (L,B,H,2N-1), live_rows (B,)) and clears.
    Each (b, h) profile sums to live_rows[b]; `mass_within` and `mean_abs_offset` turn it into the two usual figures."""

    def __init__(self, attn_modules):
        self.attn_modules = attn_modules
        self.profiles, self.live_rows = [], None
        self._handles = []
        for module in self.attn_modules:
            module.return_attention_offsets = True
            self._handles.append(module.return_offsets_module.register_forward_hook(self._hook))

    def remove(self):
        for h in self._handles: h.remove()
        self._handles = []
        for module in self.attn_modules: module.return_attention_offsets = False

    def _hook(self, module, input, output):
        profile, live = output
        self.profiles.append(profile.detach().float().cpu())
        self.live_rows = live.detach().cpu()

    def collect(self):
        return self.profiles

    def clear(self):
        self.profiles, self.live_rows = [], None

    def __call__(self):
        if len(self.profiles) == 0:
            raise RuntimeError('CollectAttentionOffsets: nothing collected - call the model on some input first')
        out = torch.stack(self.profiles, dim=0), self.live_rows
        self.clear()
        return out


def _offsets(profile):
    n = (profile.shape[-1] + 1) // 2
    return torch.arange(-(n - 1), n, device=profile.device)


def mass_within(profile, live_rows, w):
    """Share of the attention mass at |delta| <= w: profile (..., B, H, 2N-1), live_rows (B,) -> (..., B, H)."""
    near = (_offsets(profile).abs() <= w).to(profile.dtype)
    return (profile * near).sum(-1) / live_rows.to(profile.dtype)[:, None]


def mean_abs_offset(profile, live_rows):
    """Mean |delta| under the attention distribution, averaged over live query rows: -> (..., B, H), in tokens."""
    return (profile * _offsets(profile).abs().to(profile.dtype)).sum(-1) / live_rows.to(profile.dtype)[:, None]
