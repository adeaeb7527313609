"""Write-footprint tests of the hotword beam search's unit on the device: every case of tests/hot_footprint_cases.py runs twice out
of one guarded arena (0xFF fill, random fill) through tests/footprint.py - guards intact, the two images and the log-probs unchanged,
only the seven outputs and the workspace written, every element of the outputs written from the inputs alone (bit-equal between the
fills), and every value at the restatement of tests/hot_refs.py."""
import pytest
import torch

import footprint as FP
import hot_footprint_cases as HC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def hot():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from lcasr_amd.hip import hot as h
    h.load()
    return h


@pytest.mark.parametrize('id', list(HC.CASES))
def test_hot_footprint(hot, id):
    FP.run_on_device(HC.build(id, hot.load()), hot.PROTOTYPES)
