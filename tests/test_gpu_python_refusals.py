"""The Python layer's tensor and frame-state refusals on a real scene and device, held to the transcript of
tests/golden/python_refusals.json (tests/python_refusals.py has the cases and says how the file was recorded).  One scene is
uploaded; all that the cases render is one 8 x 8 range of 2 samples and one 8 x 8 step of one sub-ray."""
import pytest

import python_refusals as PR

pytestmark = pytest.mark.gpu


def test_gpu_refusals_are_the_recorded_ones(sqt):
    env = PR.gpu_env(sqt)
    try:
        assert PR.check("gpu", env) == len(PR.CASES["gpu"]) > 425
        assert env.ds.depth == 3 and env.ds.sky is None              # the cases that change the scene under a frame put it back
    finally:
        env.torch.cuda.synchronize()
        env.ds.close()
