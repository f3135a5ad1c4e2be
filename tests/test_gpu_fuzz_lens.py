"""A slice of tests/fuzz_lens.py: seeds 1000 .. 1399 -- the scenes and cameras of tests/test_gpu_fuzz_features.py's slice -- through
the lens, shutter and temporal libraries and DeviceScene.guides: sub-rays, dense frames in one call, in two ranges and in several
batches, listed frames, the guides and temporal steps, each against the restatements tests/test_fuzz_lens.py pins, bit for bit."""
import pytest

import fuzz_features as FF
import fuzz_lens as FL

pytestmark = pytest.mark.gpu
BLOCK = 20
BLOCKS = [FL.SLICE[first:first + BLOCK] for first in range(0, len(FL.SLICE), BLOCK)]


@pytest.mark.parametrize("seeds", BLOCKS, ids=[f"{b[0]}-{b[-1]}" for b in BLOCKS])
def test_a_block_of_seeds_equals_the_restatements(sqt, seeds):
    assert not FF.DEVICE_ERROR, FF.DEVICE_ERROR
    failures = [(seed, msg) for seed in seeds for msg in FL.run_case(seed)]
    assert not failures, failures


# Seeds the campaign finds, with one sentence each on the cause.  python tests/fuzz_lens.py 240 60000000 found none.  (One test over
# the tuple, as tests/test_gpu_fuzz_level1.py has it: pytest turns a parametrised test over an empty tuple into a skipped one.)
REGRESSIONS = ()


def test_the_seeds_the_campaign_found(sqt):
    assert not FF.DEVICE_ERROR, FF.DEVICE_ERROR
    assert [(seed, msg) for seed in REGRESSIONS for msg in FL.run_case(seed)] == []
