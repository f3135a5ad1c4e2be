"""The Python layer's refusals that need no GPU, held to the transcript of tests/golden/python_refusals.json: the same exception
type and the same message as before the layer's rules were gathered in one place, and the same refusal when two things are wrong
(tests/python_refusals.py has the cases and says how the file was recorded)."""
import json

import python_refusals as PR


def test_the_file_holds_the_cases_of_both_groups_and_no_others():
    with open(PR.GOLDEN_FILE) as f:
        held = json.load(f)
    names = {n for g in PR.CASES.values() for n, _ in g}
    assert set(held) == names, sorted(set(held) ^ names)
    assert all(isinstance(v, list) and len(v) == 2 and all(isinstance(s, str) for s in v) for v in held.values())


def test_cpu_refusals_are_the_recorded_ones(sqt):
    assert PR.check("cpu", PR.Env(sqt)) == len(PR.CASES["cpu"]) > 745
