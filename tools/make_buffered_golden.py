"""TEST INFRASTRUCTURE ONLY (development container only): the fixture of the buffered evaluation mode, taken straight from the
imported reference's lcasr/eval/buffered_transcription.py::fetch_logits (fp32, CPU).  The reference is imported at run time
through oracle.make_golden.load_reference(), with the stand-in audio_tools module of tools/make_subsample4_golden.py; only
numbers are written.

Writes tests/golden/buffered_tiny.npz with two parts:
  (a) tiny.*   the reference function on the model and spectrogram of infer_tiny.npz for ten (seq_len, overlap) settings;
  (b) place.*  the same function on a stub model (tests/eval_refs.py::StubModel) whose posteriors are exact integers naming the
               window and the row they came from, swept over recording lengths and (seq_len, overlap); only the settings the
               reference completes are kept (the others end in its own assertion or slice assignment).
Usage:  python tools/make_buffered_golden.py
"""
import contextlib
import io
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from oracle.make_golden import GOLD, REF, load_reference   # noqa: E402
from eval_refs import Args, StubModel, StubTok, stub_spec  # noqa: E402

LIMIT = 1 << 20
TINY_CASES = [(256, 64), (256, 0), (2048, 0), (-1, -1), (320, 160), (1000, 0), (500, 0), (504, 248), (256, 192), (264, 16)]
SPEC_NS = [1000, 1001, 1023, 4096]
SEQ_LENS = [-1, 64, 256, 264, 320, 504, 512, 1000, 1024, 2048, 5000]
OVERLAPS = [-1, 0, 8, 16, 64, 128, 192, 248, 256]


def quiet(fn, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **kw)


def main():
    assert os.path.isdir(REF), 'reference not present: this script only runs in the development container'
    SC, _, _ = load_reference()
    at = types.ModuleType('lcasr.utils.audio_tools'); at.total_frames = lambda s: int(s * 100); at.total_seconds = lambda f: f / 100
    sys.modules['lcasr.utils.audio_tools'] = at
    for name, path in [('lcasr.eval', REF + '/lcasr/eval'), ('lcasr.decoding', REF + '/lcasr/decoding')]:
        m = types.ModuleType(name); m.__path__ = [path]; sys.modules[name] = m
    from lcasr.eval.buffered_transcription import fetch_logits
    torch.set_num_threads(8)

    src = np.load(os.path.join(GOLD, 'infer_tiny.npz'))
    kw = {k[4:]: (src[k].item() if src[k].shape == () else src[k].tolist()) for k in src.files if k.startswith('cfg.')}
    model = SC(**kw)
    model.load_state_dict({k[2:]: torch.from_numpy(src[k].copy()) for k in src.files if k.startswith('w.')})
    model.eval(); model.device = 'cpu'
    spec = torch.from_numpy(src['spec'].copy())

    class Tok:
        def vocab_size(self): return kw['vocab_size']

    fx = {'tiny.cases': np.array(TINY_CASES)}
    for ci, (sl, ov) in enumerate(TINY_CASES):
        ref = quiet(fetch_logits, Args, model, spec.clone(), sl, ov, Tok(), use_tqdm=False)
        print(f'[tiny seq_len={sl} overlap={ov}] rows={ref.shape[0]}')
        fx[f'tiny.logits.{ci}'] = ref.astype(np.float32)

    stub = StubModel(); stub.device = 'cpu'
    kept, dropped = [], 0
    for spec_n in SPEC_NS:
        for sl in SEQ_LENS:
            for ov in OVERLAPS:
                sl_r = min(512 if sl == -1 else sl, spec_n)
                if (sl == -1 or sl <= spec_n) and (128 if ov == -1 else ov) >= sl_r:
                    continue                                   # a chunk of no frames: the reference never leaves its loop
                try:
                    ref = quiet(fetch_logits, Args, stub, stub_spec(spec_n), sl, ov, StubTok(), use_tqdm=False)
                except Exception:                              # its own assertion or slice assignment: not a case
                    dropped += 1
                    continue
                assert ref.ndim == 2 and ref.shape[1] == 4 and (ref == ref[:, :1]).all() and (ref == np.round(ref)).all()
                fx[f'place.rows.{len(kept)}'] = ref[:, 0].astype(np.int64)
                kept.append((spec_n, sl, ov))
    fx['place.cases'] = np.array(kept)
    print(f'[place] {len(kept)} settings kept, {dropped} the reference does not complete')
    path = os.path.join(GOLD, 'buffered_tiny.npz')
    np.savez_compressed(path, **fx)
    size = os.path.getsize(path)
    print(f'[buffered_tiny] {len(fx)} arrays, {size} bytes')
    assert size < LIMIT, size


if __name__ == '__main__':
    main()
