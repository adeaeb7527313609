"""Micro-benchmark of the fused subsampler stage 0->1 kernels at config 3 (B=16, T=16384, C=256)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import lcasr_amd.hip.ops as ops
B, F, T, C = int(os.environ.get("SUB_B", "16")), 80, 16384, 256


def slab_bench():
    """`sub_bench.py slabs`: the fused stage at C = 256 .. 1024, F = 80, B x T = 22 x 16384 (the paper's 4x batch at that length), the
    wide stages with each slab width of SCONF_SUB_SLAB; ms, algorithmic bytes/s (mel in, d1 out / dd1 in) and ns per 1000 outputs."""
    Bs = int(os.environ.get("SUB_B", "22"))
    xs = torch.randn(Bs, F, T, device='cuda')
    def timed(fn, n=10):
        for _ in range(3): fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n): fn()
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n
    for Cc, widths in ((256, (None,)), (512, (None,)), (768, (256, 384, 512)), (1024, (256, 512))):
        w0 = torch.randn(Cc, 9, device='cuda') * 0.3; b0 = torch.randn(Cc, device='cuda') * 0.1
        wd = torch.randn(Cc, 9, device='cuda') * 0.3; bd = torch.randn(Cc, device='cuda') * 0.1
        gr = [torch.zeros(Cc, 9, device='cuda'), torch.zeros(Cc, device='cuda'), torch.zeros(Cc, 9, device='cuda'), torch.zeros(Cc, device='cuda')]
        for wdt in widths:
            if wdt is None: os.environ.pop('SCONF_SUB_SLAB', None)
            else: os.environ['SCONF_SUB_SLAB'] = str(wdt)
            d1 = ops.sub_stage01_fwd(xs, w0, b0, wd, bd)
            dd1 = torch.randn_like(d1)
            nbytes = xs.numel() * 4 + d1.numel() * 2
            tf = timed(lambda: ops.sub_stage01_fwd(xs, w0, b0, wd, bd))
            tb = timed(lambda: ops.sub_stage01_bwd_(dd1, xs, w0, b0, wd, *gr))
            print(f'C {Cc:5d} slabs fwd {ops.sub_stage01_slabs(F, Cc)} bwd {ops.sub_stage01_slabs(F, Cc, True)} (width {wdt or Cc}): '
                  f'fwd {tf:7.3f} ms {nbytes / tf / 1e9:6.2f} TB/s {tf * 1e9 / d1.numel():6.2f} ns/1000 out | '
                  f'bwd {tb:7.3f} ms {nbytes / tb / 1e9:6.2f} TB/s {tb * 1e9 / d1.numel():6.2f} ns/1000 out', flush=True)
            del d1, dd1
    os.environ.pop('SCONF_SUB_SLAB', None)


if sys.argv[1:2] == ['slabs']:
    slab_bench()
    sys.exit(0)
x = torch.randn(B, F, T, device='cuda')
w0 = torch.randn(C, 9, device='cuda') * 0.3; b0 = torch.randn(C, device='cuda') * 0.1
wd = torch.randn(C, 9, device='cuda') * 0.3; bd = torch.randn(C, device='cuda') * 0.1
def t(fn, n=5):
    for _ in range(2): fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n
d1 = ops.sub_stage01_fwd(x, w0, b0, wd, bd)
for nb in (512, 1024, 2048, 4096, 8192):
    os.environ['SCONF_SUB_FWD_BLOCKS'] = str(nb)
    print(f'fwd blocks {nb}: {t(lambda: ops.sub_stage01_fwd(x, w0, b0, wd, bd)):.3f} ms')
dd1 = torch.randn_like(d1.float()).bfloat16()
g = [torch.zeros(C, 9, device='cuda'), torch.zeros(C, device='cuda'), torch.zeros(C, 9, device='cuda'), torch.zeros(C, device='cuda')]
for cfg in sys.argv[1:] or ['2,1024']:
    os.environ['SCONF_SUB_BWD_CFG'] = cfg
    print(f'bwd cfg {cfg:10s}: {t(lambda: ops.sub_stage01_bwd_(dd1, x, w0, b0, wd, *g)):.3f} ms')
Ti, Fi = 4096, 20
pre1 = torch.randn(B, Ti, Fi, C, device='cuda').bfloat16()
dd2 = torch.randn(B, Ti // 2, Fi // 2, C, device='cuda').bfloat16()
gw, gbv = torch.zeros(C, 9, device='cuda'), torch.zeros(C, device='cuda')
print(f'dwconv fwd: {t(lambda: ops.sub_dwconv_fwd(pre1, wd, bd)):.3f} ms')
for thr in ('256', '512'):
    os.environ['SCONF_SUB_DWBWD_THREADS'] = thr
    for cfg in ('4,512', '4,1024', '8,256', '8,512', '8,1024', '8,2048'):
        os.environ['SCONF_SUB_DWBWD_CFG'] = cfg
        print(f'dwconv bwd threads {thr} cfg {cfg}: {t(lambda: ops.sub_dwconv_bwd(dd2, wd, pre1, gw, gbv)):.3f} ms')
