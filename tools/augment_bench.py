"""sconf_spec_mask / sconf_mean_f32 / sconf_ctc_collapse at the dynamic-evaluation and training shapes, timed with HIP events
(wrapper calls, output allocation included).  Under `rocprofv3 --kernel-trace --stats -- python tools/augment_bench.py` the
kernel trace gives the per-dispatch times quoted in DESIGN.md section 9."""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import lcasr_amd
from lcasr_amd.hip import ops

def timeit(fn, n=20):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n): fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3     # us

g = torch.Generator().manual_seed(0)
for (B, F, T, bc) in [(3, 80, 16384, True), (128, 80, 16384, False), (128, 80, 16384, True)]:
    src = torch.randn(1 if bc else B, F, T, generator=g).cuda()
    t_iv = torch.tensor([[100, 500], [9000, 9400]], dtype=torch.int32).repeat(B, 1, 1).cuda()
    f_iv = torch.tensor([[3, 20], [40, 41], [70, 75]], dtype=torch.int32).repeat(B, 1, 1).cuda()
    mv = torch.zeros((), device='cuda')
    us = timeit(lambda: ops.spec_mask(src, t_iv, f_iv, mv, batch=B if bc else None))
    wr = B * F * T * 4
    rd = (1 if bc else B) * F * T * 4 * (1 - 23 / 80)        # masked frequency bins are not read
    print(f'spec_mask B={B} F={F} T={T} broadcast={bc}: {us:.1f} us incl. output allocation, write {wr/1e6:.1f} MB + read {rd/1e6:.1f} MB -> {(wr+rd)/us/1e3:.0f} GB/s')
x = torch.randn(128, 80, 16384, generator=g).cuda()
us = timeit(lambda: ops.mean_f32(x)); print(f'mean_f32 {x.numel()*4/1e6:.0f} MB: {us:.1f} us -> {x.numel()*4/us/1e3:.0f} GB/s')
x = torch.randn(1, 80, 16384, generator=g).cuda()
us = timeit(lambda: ops.mean_f32(x)); print(f'mean_f32 {x.numel()*4/1e6:.1f} MB: {us:.1f} us')
lp = torch.randn(1, 2048, 4096, generator=g).cuda()
us = timeit(lambda: ops.ctc_collapse(lp, None, 4095)); print(f'ctc_collapse (1,2048,4096) {lp.numel()*4/1e6:.0f} MB: {us:.1f} us -> {lp.numel()*4/us/1e3:.0f} GB/s')
