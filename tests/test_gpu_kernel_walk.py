"""Every case of tests/kernel_walk.py on the GPU: small calls whose union launches every kernel of the library that a call can reach
(tests/golden/kernel_walk.json records which case dispatched which, tests/test_kernel_walk.py holds the library's kernel list to it),
each asserting the plan it was written for and its whole output, bit for bit, against the oracle or its pinned restatements.

One DeviceScene per scene serves that scene's cases, the option tables are restored after each, and after the first HIP error no further
case touches the device (fuzz_features.DEVICE_ERROR's rule): the rest fail as "not run"."""
import pytest

import kernel_walk as KW

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def walk(sqt, O):
    w = KW.Walk()
    yield w
    if not w.device_error:
        w.close()


@pytest.mark.parametrize("index", range(len(KW.CASES)), ids=KW.NAMES)
def test_a_case_of_the_walk_takes_its_plan_and_equals_the_oracle(walk, index):
    walk.run(index)


def test_the_big_frames_have_more_pixels_than_one_accumulate_launch_has_threads(walk):
    assert not walk.device_error, walk.device_error
    w, h, _ = walk.big_frame()
    assert w * h > walk.n_cu * 256 and w * h == (walk.n_cu + 1) * KW.BIG_COLUMNS
