"""Micro-benchmark of the attention-map kernels beside the forward they observe: sconf_attn_scores (f32 and bf16 output),
sconf_attn_offset_profile (unbounded and under a (256, 256) window) and sconf_attn_fwd at B=1, N=2048, H=6, D=128 and
B=1, N=16384, H=16, D=128, random data, device events after warm-up, all in one process.
Usage:  python tools/attn_maps_bench.py [B N H D ...]      (REPS=10)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import lcasr_amd.hip.ops as ops
args = [int(x) for x in sys.argv[1:]] or [1, 2048, 6, 128, 1, 16384, 16, 128]
reps = int(os.environ.get('REPS', '10'))
def t(fn):
    for _ in range(2): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps
for B, N, H, D in zip(*[iter(args)] * 4):
    qkv = torch.randn(B, N, 3, H, D, device='cuda').bfloat16()
    q, k, v = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
    _, lse = ops.attn_fwd(q, k, v, None)
    _, lse_w = ops.attn_fwd(q, k, v, None, (256, 256))
    qk = 2.0 * B * H * N * N * D
    print(f'B={B} N={N} H={H} D={D}')
    ms = t(lambda: ops.attn_fwd(q, k, v, None))
    print(f'  attn_fwd                  {ms*1e3:9.1f} us  {2*qk/ms/1e9:7.1f} TF/s (4BHN^2D)')
    ms = t(lambda: ops.attn_offset_profile(q, k, lse, None))
    print(f'  offset_profile            {ms*1e3:9.1f} us  {qk/ms/1e9:7.1f} TF/s (2BHN^2D)')
    ms = t(lambda: ops.attn_fwd(q, k, v, None, (256, 256)))
    print(f'  attn_fwd       w=(256,256){ms*1e3:9.1f} us')
    ms = t(lambda: ops.attn_offset_profile(q, k, lse_w, None, (256, 256)))
    print(f'  offset_profile w=(256,256){ms*1e3:9.1f} us')
    for dt, nb in ((torch.float32, 4), (torch.bfloat16, 2)):
        ms = t(lambda: ops.attn_scores(q, k, None, out_dtype=dt))
        print(f'  scores {str(dt)[6:]:9s}          {ms*1e3:9.1f} us  {B*H*N*N*nb/ms/1e6:7.1f} GB/s written')
