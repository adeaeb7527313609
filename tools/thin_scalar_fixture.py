"""Shrink a scalar fixture written by oracle/make_golden.py::run_case (save_weights=False, strided_grads=True) below the
1 MiB limit of a committed file.  usage: python tools/thin_scalar_fixture.py TAG [TAG ...]   (tests/golden/TAG.npz, in place)

* `x` (B x 80 x T f32 noise, 1.2 MB compressed at T = 2048) is dropped: oracle/make_golden.py::synth regenerates it from its
  seed; `x_sum` / `x_sq_sum` (f64) let the tests check that the regenerated input is the one the fixture was made from.
* every `gs.` entry (a strided sample of a gradient tensor, <= gs_cap elements) is strided once more down to <= gs_cap2
  elements with the same rule (flatten, every ceil(n / cap)-th element): the tests sample the HIP gradient in the same two steps."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GS_CAP2 = 1024


def strided(v, cap):
    flat = v.reshape(-1)
    return flat[::max(1, -(-flat.size // cap))]


def thin(path):
    fx = dict(np.load(path, allow_pickle=False))
    if 'x' in fx:
        x = fx.pop('x').astype(np.float64)
        fx['x_sum'], fx['x_sq_sum'] = np.float64(x.sum()), np.float64((x * x).sum())
    if 'gs_cap2' not in fx:
        for k in [k for k in fx if k.startswith('gs.')]:
            fx[k] = strided(fx[k], GS_CAP2).copy()
        fx['gs_cap2'] = np.array(GS_CAP2)
    np.savez_compressed(path, **fx)
    print(f'{path}: {os.path.getsize(path)} bytes')


if __name__ == '__main__':
    for tag in sys.argv[1:]:
        thin(os.path.join(ROOT, 'tests', 'golden', tag + '.npz'))
