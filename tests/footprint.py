"""Write-footprint harness: where does an entry point of include/sconf.h write, does it write everything it claims to, and does it
read any of its outputs or scratch before writing them?  TEST INFRASTRUCTURE, plain importable module (no fixtures, no pytest hooks),
device-agnostic: tests/test_footprint.py drives it with CPU tensors and small Python "kernels", the GPU tests of every ABI unit with
the library's entry points (run_on_device: raw pointers through lcasr_amd.hip._lib.call, as ops._p passes them).

Every buffer of one call - inputs, outputs, workspaces, length vectors - is carved out of ONE uint8 arena at 16-byte granularity (the
flat gradient buffer guarantees no more, so offsets are deliberately NOT rounded to 256 or 512) with a guard band of at least GUARD
bytes before and after each region; the bytes between the rows of a strided region are guards too.  Each region has a class:

  IN       bit-unchanged after the call
  OUT      every byte of its elements overwritten, from the inputs alone (order='atomic': a sum whose order the header leaves open)
  ACC      accumulated (+=) onto an initial content that is an input; 'fixed' summation order (bit-reproducible) or 'atomic'
  INOUT    updated in place
  SCRATCH  any content afterwards, nothing outside it

A case runs twice from identical inputs and identical initial ACC / INOUT content: run A fills everything else with 0xFF bytes (NaN
as bf16 / f32 / f64, -1 as an integer), run B with seeded pseudo-random bytes.  The arena is snapshotted right before each call.

  confinement    in both runs every byte outside the elements of OUT / ACC / INOUT / SCRATCH regions equals the snapshot
  completeness   OUT, ACC fixed and INOUT regions are bit-identical between the runs and hold no NaN of run A's fill
                 (ACC atomic: equal between the runs at the op's value tolerance)
  values         run B's outputs agree with the float64 restatement at the op's existing tolerance
"""
import ctypes
import math

import pytest
import torch

from kernel_test_utils import TOL_BF16, TOL_F32

GRAIN = 16          # carving granularity in bytes
GUARD = 256         # least number of guard bytes before and after every region
IN, OUT, ACC, INOUT, SCRATCH = 'IN', 'OUT', 'ACC', 'INOUT', 'SCRATCH'
WRITABLE = (OUT, ACC, INOUT, SCRATCH)
_INT_OF_SIZE = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


class FootprintError(AssertionError):
    pass


class Region:
    """`shape` elements of `dtype` at element strides `strides`, starting `offset` bytes into the arena."""

    def __init__(self, name, shape, dtype, cls, strides, offset, init=None, order=None, tol=None, unspecified=None, produced=False):
        self.name, self.shape, self.dtype, self.cls, self.strides, self.offset = name, tuple(shape), dtype, cls, tuple(strides), offset
        self.init, self.order, self.tol, self.unspecified, self.produced = init, order, tol, unspecified, produced
        self.itemsize = torch.empty(0, dtype=dtype).element_size()
        n = 1 + sum((s - 1) * st for s, st in zip(self.shape, self.strides)) if all(self.shape) else 0
        self.extent = n * self.itemsize                                  # bytes from the first to one past the last element

    @property
    def numel(self):
        return math.prod(self.shape)

    def view(self, buf, raw=False):
        """The region inside arena tensor `buf`; raw=True: as the integer type of the same width (bit comparisons)."""
        dt = _INT_OF_SIZE[self.itemsize] if raw else self.dtype
        flat = buf[self.offset:self.offset + self.extent].view(dt)
        return flat.as_strided(self.shape, self.strides)

    def __repr__(self):
        return f'{self.cls} {self.name}{list(self.shape)}'


class Arena:
    """Lays regions out first (take), then materialises the bytes for one run (build)."""

    def __init__(self):
        self.regions = {}
        self.cursor = GUARD + GRAIN

    def take(self, name, shape, dtype, cls=IN, ld=None, strides=None, init=None, order=None, tol=None, unspecified=None, produced=False):
        """Carve a region.  ld: row stride of a 2-D region; strides: element strides of any view (attention operands); default
        contiguous.  init: the content of IN / ACC / INOUT regions, a tensor of `shape` (or a callable taking the function that
        maps a region to its address, for tables of raw pointers).  order ('fixed' | 'atomic'): required for ACC; an OUT region may be
        'atomic' where the header says its sums are not bit-reproducible.  tol: value
        tolerance override (default TOL_BF16 / TOL_F32 by dtype).  unspecified: bool tensor of `shape`, True where include/sconf.h
        says in words that the content is unspecified: excluded from completeness and values, still confined.  produced: an IN region
        whose content a `before` call of the case writes (a forward's outputs handed to its backward) instead of `init`."""
        if isinstance(shape, int): shape = (shape,)
        assert name not in self.regions, name
        assert cls in (IN,) + WRITABLE, cls
        assert not (ld is not None and strides is not None)
        if ld is not None:
            assert len(shape) == 2 and ld >= shape[1], (name, shape, ld)
            strides = (ld, 1)
        if strides is None:
            strides = [1] * len(shape)
            for i in range(len(shape) - 2, -1, -1): strides[i] = strides[i + 1] * shape[i + 1]
        assert (order is not None) == (cls == ACC) or (cls == OUT and order == 'atomic'), (name, cls, order)
        assert order in (None, 'fixed', 'atomic'), order
        assert (init is not None) == (cls in (IN, ACC, INOUT) and not produced), f'{name}: {cls} regions {"need" if init is None else "take no"} initial content'
        if torch.is_tensor(init):
            assert tuple(init.shape) == tuple(shape) and init.dtype == dtype, (name, tuple(init.shape), shape, init.dtype, dtype)
        r = Region(name, shape, dtype, cls, strides, self.cursor, init, order, tol, unspecified, produced)
        self.regions[name] = r
        self.cursor = -(-(r.offset + max(r.extent, 1)) // GRAIN) * GRAIN + GUARD
        if self.cursor % (2 * GRAIN) == 0: self.cursor += GRAIN          # keep the offsets odd multiples of 16: nothing rides on 32+
        return r

    @property
    def nbytes(self):
        return self.cursor

    def validate(self):
        """Regions disjoint, 16-byte aligned, and at least GUARD bytes of guard before and after each."""
        end = 0
        for r in sorted(self.regions.values(), key=lambda r: r.offset):
            assert r.offset % GRAIN == 0, f'{r}: offset {r.offset} is not 16-byte aligned'
            assert r.offset - end >= GUARD or (end == 0 and r.offset >= GUARD), f'{r}: only {r.offset - end} guard bytes before it'
            end = r.offset + r.extent
        assert self.nbytes - end >= GUARD, 'no guard behind the last region'

    def build(self, device, fill, seed=0):
        """The arena bytes for one run: fill 'ff' or 'rand' everywhere, then the initial content of IN / ACC / INOUT regions."""
        if fill == 'ff':
            buf = torch.full((self.nbytes,), 0xFF, dtype=torch.uint8)
        else:
            buf = torch.randint(0, 256, (self.nbytes,), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed + 1))
        buf = buf.to(device)
        base = buf.data_ptr()
        assert base % GRAIN == 0
        addr = lambda r: base + r.offset
        for r in self.regions.values():
            if r.init is not None:
                t = r.init(addr) if callable(r.init) else r.init
                r.view(buf).copy_(t.to(device))
        return buf

    def writable_mask(self, device):
        """uint8 (nbytes): non-zero at the bytes of elements of OUT / ACC / INOUT / SCRATCH regions."""
        m = torch.zeros(self.nbytes, dtype=torch.uint8, device=device)
        for r in self.regions.values():
            if r.cls in WRITABLE and r.numel: r.view(m, raw=True).fill_(-1 if r.itemsize > 1 else 255)
        return m

    def guard_bytes(self):
        return self.nbytes - sum(r.numel * r.itemsize for r in self.regions.values() if r.cls in WRITABLE)

    def locate(self, off):
        """Describe arena byte `off` relative to the nearest region."""
        best = None
        for r in self.regions.values():
            d = 0 if r.offset <= off < r.offset + r.extent else min(abs(off - r.offset), abs(off - (r.offset + r.extent - 1)))
            if best is None or d < best[0]: best = (d, r)
        r = best[1]
        rel = off - r.offset
        if 0 <= rel < r.extent:
            where = f'inside the {r.cls} region {r.name!r}' if r.cls == IN else f'in a stride gap of the {r.cls} region {r.name!r}'
            return f'{where}, byte {rel} of its extent (element offset {rel // r.itemsize})'
        if rel < 0: return f'{-rel} byte(s) BEFORE the {r.cls} region {r.name!r}'
        return f'{rel - r.extent + 1} byte(s) PAST the end of the {r.cls} region {r.name!r}'


class Case:
    """One call: the entry point, its arena, its argument list and its float64 restatement.

    args: the C argument list; a Region stands for its address, None for NULL, everything else is passed as given.
    ref_name: the kernel_refs function that restates the call; ref(views) -> {region name: expected tensor} evaluates it, with
    views[name] the initial content of every IN / ACC / INOUT region (of `before`'s outputs too once they have run).  A value may be
    a pair (tensor, fn) where the header defines only fn(region) - the sum over slab lines, say - and not each element.
    before: calls [(entry point, args)] that produce the content of some regions before the snapshot (a forward feeding its backward).
    variant: what the routing query reported (printed by the GPU tests).  unvalued: writable regions the restatement has no value
    for (bit checks only).  indirect: regions reached through a table of addresses instead of an argument."""

    def __init__(self, id, name, arena, args, ref_name, ref, before=(), variant='', unvalued=(), indirect=()):
        self.id, self.name, self.arena, self.args, self.ref_name, self.ref = id, name, arena, list(args), ref_name, ref
        self.before, self.variant, self.unvalued, self.indirect = list(before), variant, set(unvalued), set(indirect)

    def __repr__(self):
        return self.id


def resolve(args, buf):
    base = buf.data_ptr()
    return [ctypes.c_void_p(base + a.offset) if isinstance(a, Region) else a for a in args]


def lib_launch(name, args, buf, views):
    """The real thing: lcasr_amd.hip._lib.call with raw pointers into the arena, on torch's current stream."""
    from lcasr_amd.hip import _lib
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.call(name, *resolve(args, buf), stream)
    torch.cuda.synchronize()


def _value_close(out, ref, tol, what, mask=None):
    assert tuple(out.shape) == tuple(ref.shape), f'{what}: shape {tuple(out.shape)}, the restatement gives {tuple(ref.shape)}'
    o, r = out.detach().double().cpu(), ref.detach().double().cpu()
    if mask is not None:
        keep = ~mask.cpu()
        o, r = o[keep], r[keep]
    if not o.numel(): return 0.0
    same_inf = torch.isinf(r) & (o == r)                                 # -inf scores / +inf lse are values, compared exactly
    if not bool(torch.isfinite(o[~same_inf]).all() and torch.isfinite(r[~same_inf]).all()):
        raise FootprintError(f'{what}: non-finite output where the restatement is finite (or the reverse)')
    o, r = o[~same_inf], r[~same_inf]
    if not o.numel(): return 0.0
    scale = float(r.abs().max()) + 1e-12
    err = float((o - r).abs().max()) / scale
    if err > tol: raise FootprintError(f'{what}: max err {err:.3e} of max|ref| = {scale:.3e} > {tol}')
    return err


def default_tol(r):
    if r.tol is not None: return r.tol
    return TOL_BF16 if r.dtype == torch.bfloat16 else TOL_F32


def run_case(case, device, launch=lib_launch, seed=0):
    """Both runs and all three checks.  Every finding of the case is collected and raised as one FootprintError that names the regions.
    Returns the figures of the report line."""
    A = case.arena
    A.validate()
    mask = A.writable_mask(device)
    fails, results = [], {}
    head = f'{case.id} [{case.name}]'
    for fill in ('ff', 'rand'):
        buf = A.build(device, fill, seed)
        views = {n: r.view(buf) for n, r in A.regions.items()}
        for name, args in case.before: launch(name, args, buf, views)
        snap = buf.clone()
        launch(case.name, case.args, buf, views)
        bad = ((buf != snap) & (mask == 0)).nonzero()
        if bad.numel():
            first = int(bad[0])
            fails.append(f'confinement, fill {fill}: {bad.numel()} byte(s) changed outside the writable regions; the first is '
                         f'{A.locate(first)} (arena byte {first})')
        results[fill] = (buf, snap)
    (bufA, _), (bufB, snapB) = results['ff'], results['rand']
    inputs = {n: r.view(snapB).clone().cpu() for n, r in A.regions.items() if r.cls in (IN, ACC, INOUT)}
    expected = case.ref(inputs)
    checked = []
    for n, r in A.regions.items():
        if r.cls not in (OUT, ACC, INOUT) or not r.numel: continue
        what = f'{r.cls} region {n!r}'
        keep = ~r.unspecified.to(device) if r.unspecified is not None else torch.ones(r.shape, dtype=torch.bool, device=device)
        a, b = r.view(bufA), r.view(bufB)
        if r.dtype.is_floating_point:
            nan = torch.isnan(a) & keep
            if bool(nan.any()):
                fails.append(f'{what} completeness: {int(nan.sum())} element(s) are NaN after the 0xFF-filled run, first at '
                             f'{nan.nonzero()[0].tolist()}: left unwritten, or computed from bytes the call never wrote')
        try:
            if r.order == 'atomic':
                _value_close(b, a, default_tol(r), what + ' between the two fills (atomic order)', ~keep)
            else:
                diff = (r.view(bufA, raw=True) != r.view(bufB, raw=True)) & keep
                if bool(diff.any()):
                    fails.append(f'{what} completeness: {int(diff.sum())} element(s) differ between the 0xFF-filled and the random-filled '
                                 f'run, first at {diff.nonzero()[0].tolist()}: left unwritten, or the result depends on output / scratch / '
                                 f'guard content')
            if n in expected and isinstance(expected[n], tuple):            # (value, fn): the header defines fn(region), not each element
                err = _value_close(expected[n][1](b), expected[n][0], default_tol(r), what + ' values')
                checked.append(f'{n}={err:.1e}')
            elif n in expected:
                err = _value_close(b, expected[n], default_tol(r), what + ' values', ~keep)
                checked.append(f'{n}={err:.1e}')
            else:
                assert n in case.unvalued, f'{head} {what}: the restatement returns no value for it'
        except FootprintError as e:
            fails.append(str(e))
    if fails:
        raise FootprintError(f'{head}: ' + '\n  '.join(fails))
    return {'arena_bytes': A.nbytes, 'guard_bytes': A.guard_bytes(), 'valued': checked}


def report_line(case, figures):
    return (f'[footprint] {case.id}: {case.name} variant={case.variant or "-"} arena={figures["arena_bytes"]} B '
            f'guard={figures["guard_bytes"]} B checked, max err {" ".join(figures["valued"]) or "-"}')


def run_on_device(case, prototypes):
    """One case of a GPU test: run_case on 'cuda' through lib_launch, every call a launcher of `prototypes`, the report line printed.
    A launch refused on the host is a failure of this case; a device fault ends the session: nothing more runs on a faulted GPU."""
    assert {case.name} | {name for name, _ in case.before} <= set(prototypes)
    try:
        figures = run_case(case, 'cuda')
    except RuntimeError as e:
        if 'HIP error' in str(e) or 'illegal memory access' in str(e):
            pytest.exit(f'{case.id}: device fault, no further case is launched: {e}', returncode=3)
        raise
    print(report_line(case, figures))


# ------------------------------------------------------------------------------------------------ layout checks that need no device
def check_layout(case, prototypes):
    """CPU check of one case: regions disjoint, aligned and guarded; the argument list as long as the prototype (less the stream);
    the declared OUT / ACC / INOUT shapes are the shapes the kernel_refs restatement returns."""
    A = case.arena
    A.validate()
    for name, args in list(case.before) + [(case.name, case.args)]:
        assert len(args) + 1 == len(prototypes[name]), f'{case.id}: {name} takes {len(prototypes[name])} arguments, the case passes {len(args)} + stream'
        for i, (a, t) in enumerate(zip(args, prototypes[name])):
            if isinstance(a, Region): assert A.regions.get(a.name) is a, f'{case.id}: {a} is not a region of this arena'
            kind = 'pointer' if isinstance(a, (Region, ctypes.Array, type(None))) else 'float' if isinstance(a, float) else 'int'
            want = {ctypes.c_void_p: 'pointer', ctypes.c_float: 'float', ctypes.c_double: 'float'}.get(t, 'int')
            assert isinstance(a, (Region, ctypes.Array, type(None), float, int)) and kind == want, \
                f'{case.id}: {name} argument {i} is a {want} in the prototype, the case passes {a!r}'
    used = {a.name for _, args in list(case.before) + [(case.name, case.args)] for a in args if isinstance(a, Region)}
    used |= case.indirect
    assert used == set(A.regions), f'{case.id}: regions never passed: {set(A.regions) - used}'
    inputs = {n: r.init.clone() for n, r in A.regions.items() if torch.is_tensor(r.init)}
    expected = case.ref(inputs)
    outs = {n for n, r in A.regions.items() if r.cls in (OUT, ACC, INOUT) and r.numel}
    assert set(expected) | case.unvalued == outs, f'{case.id}: restated {sorted(expected)}, declared {sorted(outs)}'
    for n, t in expected.items():
        if isinstance(t, tuple): t = torch.zeros(A.regions[n].shape) if tuple(t[1](torch.zeros(A.regions[n].shape)).shape) == tuple(t[0].shape) else t[0]
        assert tuple(t.shape) == A.regions[n].shape, f'{case.id}: {n} is declared {A.regions[n].shape}, {case.ref_name} returns {tuple(t.shape)}'
