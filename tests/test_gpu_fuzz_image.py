"""A slice of tests/fuzz_image.py: seeds 1000 .. 1399 -- the scenes and cameras of tests/test_gpu_fuzz_features.py's slice -- through
the denoiser's variance and filter, the sparse mask and upsample, the glare pyramid, the film library and the drivers that chain them
(Temporal, denoise_frame, render_sparse), each against the restatements tests/test_fuzz_image.py pins, bit for bit, and each kernel
family's forms against each other.

Measured on an MI355X: a block of 20 seeds takes 0.85 to 2.1 s (the first block, which loads the libraries, the longest), the module
23 s."""
import pytest

import fuzz_features as FF
import fuzz_image as FI

pytestmark = pytest.mark.gpu
BLOCK = 20
BLOCKS = [FI.SLICE[first:first + BLOCK] for first in range(0, len(FI.SLICE), BLOCK)]


@pytest.mark.parametrize("seeds", BLOCKS, ids=[f"{b[0]}-{b[-1]}" for b in BLOCKS])
def test_a_block_of_seeds_equals_the_restatements(sqt, seeds):
    assert not FF.DEVICE_ERROR, FF.DEVICE_ERROR
    failures = [(seed, msg) for seed in seeds for msg in FI.run_case(seed)]
    assert not failures, failures


# Seeds the campaign finds, with one sentence each on the cause.  python tests/fuzz_image.py 240 70000000 found none: 4709 cases,
# 0 mismatches.  (One test over the tuple, as tests/test_gpu_fuzz_lens.py has it:
# pytest turns a parametrised test over an empty tuple into a skipped one.)
REGRESSIONS = ()


def test_the_seeds_the_campaign_found(sqt):
    assert not FF.DEVICE_ERROR, FF.DEVICE_ERROR
    assert [(seed, msg) for seed in REGRESSIONS for msg in FI.run_case(seed)] == []
