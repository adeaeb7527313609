"""Write-footprint tests of the resampler's ABI unit on the device: every case of tests/resample_footprint_cases.py runs twice out
of one guarded arena (0xFF fill, random fill) through tests/footprint.py - guards intact (the NaN behind every row's length and in
the channel that may not be read never reach an output), only `out` written, every element of it written from the inputs alone
(bit-equal between the fills), and every sample within resample_refs.bound of the float64 restatement."""
import pytest
import torch

import footprint as FP
import resample_footprint_cases as RC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def resample():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from lcasr_amd.hip import resample as r
    r.load()
    return r


@pytest.mark.parametrize('id', list(RC.CASES))
def test_resampler(resample, id):
    FP.run_on_device(RC.build(id, resample.load()), resample.PROTOTYPES)
