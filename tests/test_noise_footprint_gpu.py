"""Write-footprint tests of the noise unit on the device: every case of tests/noise_footprint_cases.py runs twice out of one guarded
arena (0xFF fill, random fill) through tests/footprint.py - guards intact (the NaN behind every row's length and behind every clip's
noise_lengths never reach an output), only `power` and `ws`, or `out`, written, every element of them written from the inputs alone
(bit-equal between the fills), and every value within the bounds of tests/noise_refs.py of its float64 restatement."""
import pytest
import torch

import footprint as FP
import noise_footprint_cases as NC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def noise():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from lcasr_amd.hip import noise as n
    n.load()
    return n


@pytest.mark.parametrize('id', list(NC.CASES))
def test_noise(noise, id):
    FP.run_on_device(NC.build(id, noise.load()), noise.PROTOTYPES)
