"""Write-footprint tests of the posterior unit on the device: every case of tests/post_footprint_cases.py runs twice out of one
guarded arena (0xFF fill, random fill) through tests/footprint.py - guards intact, only the outputs and the lattice's workspace
written, the workspace at exactly sconf_post_workspace bytes, every element of the outputs written from the inputs alone (bit-equal
between the fills, whatever the columns behind C, the frames behind input_lengths, the slots behind target_lengths and the
unwritten part of the workspace held), NaN and -inf where the numpy restatement has them and the rest within the header's
tolerances of it."""
import pytest
import torch

import footprint as FP
import post_footprint_cases as KC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def post():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from lcasr_amd.hip import post as k
    k.load()
    return k


@pytest.mark.parametrize('id', list(KC.CASES))
def test_post(post, id):
    FP.run_on_device(KC.build(id, post.load()), post.PROTOTYPES)
