"""Write-footprint tests of the audio ABI unit on the device: every case of tests/audio_footprint_cases.py runs twice out of one
guarded arena (0xFF fill, random fill) through tests/footprint.py - guards intact, only the declared outputs written, every output
element written from the inputs alone (bit-equal between the fills, so the fixed-order statistics are covered), values against the
float64 restatement, the workspace carved at exactly the queried size with a guard right behind."""
import ctypes

import pytest
import torch

import audio_footprint_cases as AC
import footprint as FP

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def audio():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from lcasr_amd.hip import audio as a
    a.load()
    return a


def test_every_audio_entry_point_has_a_case(audio):
    assert {entry for entry, _ in AC.CASES.values()} | AC.NO_LAUNCH == set(audio.PROTOTYPES) | set(audio.PLAIN)
    assert not {entry for entry, _ in AC.CASES.values()} & AC.NO_LAUNCH


@pytest.mark.parametrize('id', list(AC.CASES))
def test_audio_front_end(audio, id):
    from lcasr_amd.hip import _lib

    def launch(name, args, buf, views):
        assert name in audio.PROTOTYPES
        audio.load()
        _lib.call(name, *FP.resolve(args, buf), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()

    case = AC.build(id, audio.load())
    try:
        figures = FP.run_case(case, 'cuda', launch=launch)
    except RuntimeError as e:                        # a device fault ends the session: nothing more runs on a faulted GPU
        if 'HIP error' in str(e) or 'illegal memory access' in str(e):
            pytest.exit(f'{id}: device fault, no further case is launched: {e}', returncode=3)
        raise
    print(FP.report_line(case, figures))
