"""What a sky costs: a frame under a sky against the same frame without one, both through the generic-depth pipeline, timed by
bench.py's own loop -- dist.render_frame on a resident scene, a warm-up frame, then `--steps` frames between two device synchronises.

Sides, alternating in one process (--reps rounds; best and median of the per-frame times):
    d3_deep      depth 3, no sky, option "deep" = 1: the generic-depth pipeline with its exact shortcuts
    d3_sky       depth 3 under the sky: no absorbing-surface shortcut, no emitter pre-test for the last ray, 4 more bytes per slot
    d5, d5_sky   the same pair at depth 5
The sky sides have no frame to be equal to (tests/test_gpu_sky.py holds them); the script only checks that they differ from theirs.

    python tools/gpu_sky.py [--scene obj|hf] [--reps 3] [--steps 3] [--spp 256] [--size 1920x1080] [--hf 708] [--variant 2]

--scene obj is the headline frame (data/scene.obj under data/camera); --scene hf is the height field of tools/gen_scenes.py (--hf N).
"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

SKY = ((0.25, 0.5, 1.0), (0.75, 0.625, 0.5))


def deep_slot_bytes(depth, sky):
    """Bytes per slot of the generic pipeline's own block (csrc/sq_device.hip: deep_slot_bytes)."""
    return 0 if depth < 2 else 4 * (depth - 1) + (8 if depth >= 4 else 0) + (4 if sky else 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="obj", choices=("obj", "hf"))
    ap.add_argument("--hf", type=int, default=708)
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--variant", type=int, default=2)
    ap.add_argument("--only", default="", help="comma-separated sides (default: all)")
    a = ap.parse_args()
    w, h = (int(v) for v in a.size.split("x"))
    import torch
    sqt = importlib.import_module("squigly-trace_amd")
    d = importlib.import_module("squigly-trace_amd.dist")
    if a.scene == "obj":
        data = os.path.join(ROOT, "data")
        bih = sqt.BIH(sqt.Mesh.from_obj(os.path.join(data, "scene.obj"), data))
        cam = sqt.load_camera(os.path.join(data, "camera"))
    else:
        import gen_scenes as G
        obj, sq, camt = G.heightfield_scene(a.hf)
        bih = sqt.BIH(sqt.Mesh.from_text(obj, sq), device=0)
        cam = sqt.camera_from_text(camt)
    ds = sqt.DeviceScene(bih, 0)
    ds.set_option("variant", a.variant)
    ds.set_option("deep", 1)

    def side(depth, sky):
        def prepare():
            ds.set_depth(depth)
            if sky:
                ds.set_sky(*SKY)
            else:
                ds.set_sky(None)
        return prepare

    sides = {"d3_deep": side(3, False), "d3_sky": side(3, True), "d5": side(5, False), "d5_sky": side(5, True)}
    if a.only:
        sides = {k: v for k, v in sides.items() if k in a.only.split(",")}
    frames, forms = {}, {}
    for k, prepare in sides.items():                                  # warm-up (workspace, the depth's block, code objects)
        prepare()
        frames[k] = d.render_frame(ds, cam, a.spp, w, h, want="rgb").clone()
        torch.cuda.synchronize()
        forms[k] = ds.last_plan()["trace_form"]
    for plain, sky in (("d3_deep", "d3_sky"), ("d5", "d5_sky")):
        if plain in frames and sky in frames and torch.equal(frames[plain], frames[sky]):
            print(json.dumps({"error": f"{sky} equals {plain}: the sky did not show"}), flush=True)
            return 1
    ms = {k: [] for k in sides}
    for _ in range(a.reps):
        for k, prepare in sides.items():                              # alternating: a drift of the machine hits every side alike
            prepare()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                d.render_frame(ds, cam, a.spp, w, h, want="rgb")
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3 / a.steps)
    row = {"scene": a.scene if a.scene == "obj" else f"hf{a.hf}", "tris": len(bih.tris), "frame": f"{w}x{h}@{a.spp}", "variant": a.variant,
           "reps": a.reps, "steps": a.steps, "build": sqt.build_id(), "forms": forms,
           "nonblack": {k: int((f.sum(-1) > 0).sum().item()) for k, f in frames.items()}}
    for k, v in ms.items():
        v.sort()
        row[k + "_best_ms"], row[k + "_median_ms"] = round(v[0], 3), round(v[len(v) // 2], 3)
        row[k + "_slot_bytes"] = deep_slot_bytes(int(k[1]), k.endswith("_sky"))
    for plain, sky in (("d3_deep", "d3_sky"), ("d5", "d5_sky")):
        if plain in ms and sky in ms:
            row[sky + "_over_" + plain] = round(row[sky + "_best_ms"] / row[plain + "_best_ms"], 3)
    print(json.dumps(row), flush=True)
    ds.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
