"""Helpers shared by the kernel parity tests (test_kernels_gpu.py, test_kernel_geometry_gpu.py and the CPU self-check of the
references, test_kernel_geometry_refs.py).  TEST INFRASTRUCTURE, plain importable module (no fixtures, no pytest hooks).

Tolerances (the parity contract of test_kernels_gpu.py): the kernels read bf16-rounded operands and accumulate in f32, so against a
reference fed the SAME rounded inputs f32 outputs agree to 2e-3 of the tensor's max magnitude and bf16 outputs to 1.2e-2."""
import contextlib

import torch

import kernel_refs as R

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
TOL_F32, TOL_BF16 = 2e-3, 1.2e-2


def dev(t):
    return t.cuda() if isinstance(t, torch.Tensor) else t


def rel_err(out, ref, floor=0.0):
    """max |out - ref| / max(max |ref|, floor), evaluated in float64."""
    o, r = out.detach().double().cpu(), ref.detach().double().cpu()
    return float((o - r).abs().max()) / (max(float(r.abs().max()), floor) + 1e-12)


def close(out, ref, tol=None, name='', floor=0.0):
    assert out.shape == ref.shape, f'{name}: shape {tuple(out.shape)} vs {tuple(ref.shape)}'
    if tol is None:
        tol = TOL_BF16 if out.dtype == BF else TOL_F32
    o, r = out.detach().float().cpu(), ref.detach().float().cpu()
    assert torch.isfinite(o).all(), f'{name}: non-finite output'
    scale = max(float(r.abs().max()), floor) + 1e-12
    err = float((o - r).abs().max()) / scale
    assert err <= tol, f'{name}: max err {err:.3e} of max|ref|={scale:.3e} > {tol}'


def rnd(*shape, dtype=BF, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


# ---------------------------------------------------------------------------------------------- references at a chosen precision
@contextlib.contextmanager
def ref_precision(prec):
    """kernel_refs does all its math in its module-level `f32` dtype (and allocates a few temporaries in torch's default dtype):
    with both set to float64 the same functions are the high-precision restatement of every op."""
    old, old_default = R.f32, torch.get_default_dtype()
    R.f32 = prec
    torch.set_default_dtype(prec)
    try:
        yield R
    finally:
        R.f32 = old
        torch.set_default_dtype(old_default)


def _to_prec(a, prec):
    if isinstance(a, torch.Tensor):
        return a.detach().cpu().to(prec) if a.is_floating_point() else a.detach().cpu()
    if isinstance(a, torch.dtype):
        return prec if a.is_floating_point else a
    if isinstance(a, (tuple, list)):
        return type(a)(_to_prec(x, prec) for x in a)
    return a


def ref(name, *args, prec=F64, **kw):
    """kernel_refs.<name> evaluated in `prec`: floating tensors (the bf16 / f32 values the kernel reads) are widened exactly,
    floating dtype arguments (output types) become `prec`, so an op that takes its output type as an argument returns an unrounded
    result.  attn_fwd / attn_bwd, glu_dwconv_fwd, convmod_bwd (dg), affine_silu_fwd and sub_silu_transpose round to bf16 by
    themselves, as the kernels store: their float64 result is still one bf16 rounding away from the exact value (which is why the
    float32 and float64 forms of those differ by up to one bf16 flip, ~1e-3; they are compared at TOL_BF16 / 2e-2)."""
    with ref_precision(prec):
        return getattr(R, name)(*_to_prec(args, prec), **{k: _to_prec(v, prec) for k, v in kw.items()})
