"""What the wavefront form of lit cast frames (option "cast_wavefront") is worth: the 1920 x 1080 cast frame of data/camera at 1 spp.

Sides, alternating in one process (device events around each call, best and median of --reps after a warm-up):
    unset        the light never set: the per-pixel kernel with the built-in light, as before sq_scene_set_lights existed
    lane_1       the reference's light set explicitly: the per-lane kernel for caller-given lights (sq_cast_pixels)
    wave_1       the same light, cast_wavefront = 1
    lane_8       eight lights, per-lane
    wave_8       eight lights, cast_wavefront = 1
Every timed frame is first checked bit-equal between the forms (unset = lane_1 = wave_1; lane_8 = wave_8).

Copied into the tools/ of a checkout that has no sq_scene_set_lights yet, the script runs the `unset` side only: that is how the
parent commit's figure is taken, by the same code, alternating with this one in one job.

    python tools/gpu_lights.py [--reps 20]
"""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 1920, 1080
EIGHT = [((0, 3, -1), (2, 2, 2)), ((0, 0, 0), (1.5, 0.5, 0.25)), ((1.5, -2, 0.5), (0.25, 2, 1)), ((-2, 1, 2), (3, 0.75, 0.5)),
         ((0, 0, 4), (0.5, 1, 4)), ((100, 100, 100), (50, 80, 20)), ((-1.5, 2, 1), (1, 1, 2)), ((0.5, 0.5, 1.5), (2, 1, 0.5))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    import torch
    sqt = importlib.import_module("squigly-trace_amd")
    data = os.path.join(ROOT, "data")
    ds = sqt.DeviceScene(sqt.BIH(sqt.Mesh.from_obj(os.path.join(data, "scene.obj"), data)), 0)
    cam = sqt.load_camera(os.path.join(data, "camera"))
    has_lights = hasattr(sqt.lib(), "sq_scene_set_lights") and hasattr(ds, "set_lights")
    avg = torch.empty((W, H, 3), dtype=torch.float32, device="cuda:0")
    rgb = torch.empty((W, H, 3), dtype=torch.uint8, device="cuda:0")

    def side(lights, wave):
        def prepare():
            if has_lights:
                ds.set_lights(lights)
                ds.set_option("cast_wavefront", wave)
        return prepare

    sides = {"unset": side(None, 0)}
    if has_lights:
        sides.update({"lane_1": side([sqt.REFERENCE_LIGHT], 0), "wave_1": side([sqt.REFERENCE_LIGHT], 1),
                      "lane_8": side(EIGHT, 0), "wave_8": side(EIGHT, 1)})
    frames, forms = {}, {}
    for k, prepare in sides.items():                                  # warm-up (workspace, code objects) and the frames to compare
        prepare()
        ds.render_rows(cam, 1, W, H, cast=True, out_avg=avg, out_rgb=rgb)
        torch.cuda.synchronize()
        frames[k] = (avg.clone(), rgb.clone())
        forms[k] = ds.last_plan()["trace_form"]
    same = lambda x, y: bool(torch.equal(frames[x][0].view(torch.int32), frames[y][0].view(torch.int32)) and torch.equal(frames[x][1], frames[y][1]))  # noqa: E731
    equal = {"lane_1": same("unset", "lane_1"), "wave_1": same("unset", "wave_1"), "wave_8": same("lane_8", "wave_8")} if has_lights else {}
    if not all(equal.values()):
        print(json.dumps({"error": "the forms differ", "bit_equal": equal}), flush=True)
        return 1
    ms = {k: [] for k in sides}
    for _ in range(a.reps):
        for k, prepare in sides.items():                              # alternating: a drift of the machine hits every side alike
            prepare()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ds.render_rows(cam, 1, W, H, cast=True, out_avg=avg, out_rgb=rgb)
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    row = {"cast_frame": f"{W}x{H}@1", "reps": a.reps, "build": sqt.build_id(), "bit_equal": equal, "forms": forms}
    for k, v in ms.items():
        v.sort()
        row[k + "_best_ms"], row[k + "_median_ms"] = round(v[0], 4), round(v[len(v) // 2], 4)
    if has_lights:
        row["wave_1_over_lane_1"] = round(row["wave_1_best_ms"] / row["lane_1_best_ms"], 4)
        row["wave_8_over_lane_8"] = round(row["wave_8_best_ms"] / row["lane_8_best_ms"], 4)
        row["lane_1_over_unset"] = round(row["lane_1_best_ms"] / row["unset_best_ms"], 4)
    print(json.dumps(row), flush=True)
    ds.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
