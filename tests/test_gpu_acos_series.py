"""Device sq::facos (debug_eval "acos") against the oracle's sqo_acosf(., TRIG_CRD), bit for bit, on the arguments of
tests/acos_cases.py: the one evaluation of the arcsine series that both ranges of crd::acos_ share must give every lane the value the
oracle's two-armed form gives, whichever range its neighbours in the wave fall into (the arguments of a wave are mixed: the words'
2v - 1 alternate between the ranges at random, and the runs around +-0.5 cross the edge inside a wave)."""
import pytest

import acos_cases as AC

pytestmark = pytest.mark.gpu


def test_device_facos_equals_the_oracle_bit_for_bit(sqt):
    AC.assert_bit_equal(sqt.debug_eval("acos", AC.arguments()), "device sq::facos")
