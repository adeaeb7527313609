"""Write-footprint tests of the audio ABI unit on the device: every case of tests/audio_footprint_cases.py runs twice out of one
guarded arena (0xFF fill, random fill) through tests/footprint.py - guards intact, only the declared outputs written, every output
element written from the inputs alone (bit-equal between the fills, so the fixed-order statistics are covered), values against the
float64 restatement, the workspace carved at exactly the queried size with a guard right behind."""
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


@pytest.mark.parametrize('id', list(AC.CASES))
def test_audio_front_end(audio, id):
    FP.run_on_device(AC.build(id, audio.load()), audio.PROTOTYPES)
