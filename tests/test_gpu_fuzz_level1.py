"""The pytest slice of tests/fuzz_level1.py on the GPU: seeds 3000 .. 3199 -- mirror rooms, soups with planar mirrors, lattices and
the edge scenes at the records' limits (tests/test_fuzz_level1.py judges what they cover) -- through render_rows, render_rows_range
one sample index at a time, render_rows_masked under a mask and its complement, render_views and raytrace, with level1_cull at 1 and
at 0: every frame bit-equal to the oracle's, and sq_get_stats slots 28, 29 and 30 equal to the restatements' counts after every call."""
import pytest

import fuzz_level1 as FL

pytestmark = pytest.mark.gpu
BLOCK = 25
BLOCKS = [range(first, first + BLOCK) for first in range(3000, 3200, BLOCK)]


@pytest.mark.parametrize("seeds", BLOCKS, ids=[f"{b[0]}-{b[-1]}" for b in BLOCKS])
def test_a_block_of_seeds_equals_the_oracle_and_the_predicted_counts(sqt, seeds):
    failures = [(seed, msg) for seed in seeds for msg in FL.run_case(seed)]
    assert not failures, failures


# Seeds the campaign finds, with one sentence each on the cause.  python tests/fuzz_level1.py 240 70000000 found none.
REGRESSIONS = ()


def test_the_seeds_the_campaign_found(sqt):
    assert [(seed, msg) for seed in REGRESSIONS for msg in FL.run_case(seed)] == []
