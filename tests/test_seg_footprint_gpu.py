"""Write-footprint tests of the segmentation unit on the device: every case of tests/seg_footprint_cases.py runs twice out of one
guarded arena (0xFF fill, random fill) through tests/footprint.py - guards intact, only the six outputs and the workspace of
sconf_seg_align, or the three outputs of sconf_seg_score, written, the workspace at exactly the queried size, every element of the
outputs written from the inputs alone (bit-equal between the fills), the alignment equal to the float64 restatement's and the
utterance scores within seg_refs.score_bound of it."""
import pytest
import torch

import footprint as FP
import seg_footprint_cases as SC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def seg():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from lcasr_amd.hip import seg as s
    s.load()
    return s


@pytest.mark.parametrize('id', list(SC.CASES))
def test_seg(seg, id):
    FP.run_on_device(SC.build(id, seg.load()), seg.PROTOTYPES)
