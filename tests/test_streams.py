"""CPU test that keeps the stream tests complete: every declaration of include/squigly_hip.h that takes a `void* hip_stream` is in
tests/stream_harness.STREAM_ENTRY_POINTS, which that module's parametrisation is built from, so an entry point with a stream
cannot be added without a test on a gated side stream."""
import os
import re

from conftest import ROOT


def _stream_declarations():
    text = open(os.path.join(ROOT, "include", "squigly_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    found = []
    for name, params in re.findall(r"\b(sq_\w+)\s*\(([^()]*)\)\s*;", text):
        if any(re.fullmatch(r"void\s*\*\s*hip_stream", p.strip()) for p in params.split(",")):
            found.append(name)
    return found


def test_every_entry_point_with_a_stream_has_a_stream_test():
    import stream_harness as S                                    # importing it must not need a device
    declared = _stream_declarations()
    assert len(declared) == len(set(declared)) and len(declared) >= 10, declared
    assert len(S.STREAM_ENTRY_POINTS) == len(set(S.STREAM_ENTRY_POINTS))
    assert set(declared) == set(S.STREAM_ENTRY_POINTS), sorted(set(declared) ^ set(S.STREAM_ENTRY_POINTS))
    # every listed entry point is driven: it has a job under at least one schedule, and the job exists
    driven = {ep for ep, _, _ in S.PARAMS}
    assert driven == set(S.STREAM_ENTRY_POINTS)
    for ep, job, form in S.PARAMS:
        assert callable(getattr(S, "job_" + job)) and form in S.FORMS, (ep, job, form)


def test_the_parser_sees_a_stream_parameter_only_where_there_is_one():
    declared = _stream_declarations()
    assert "sq_render_rows_device" in declared and "sq_scene_set_lights" in declared
    for name in ("sq_scene_get_lights", "sq_scene_upload", "sq_set_option", "sq_render_rgb8", "sq_scene_rng_table"):
        assert name not in declared
