"""What a path depth costs: the headline frame (data/scene.obj, 1920 x 1080 at 256 spp, data/camera) under every depth, timed by
bench.py's own loop -- dist.render_frame on a resident scene, a warm-up frame, then `--steps` frames between two device synchronises.

Sides, alternating in one process (--reps rounds; best and median of the per-frame times):
    d3           depth 3, option "deep" = 0: the three-level pipeline, what a scene ran before sq_scene_set_depth existed
    d3_deep      depth 3 through the generic-depth pipeline ("deep" = 1)
    d1 ... d8    depths 1, 2, 4, 5 and 8
d3_deep is first checked bit-equal to d3.  The other depths have no frame to be equal to; tests/test_gpu_depth.py holds them.

Copied into the tools/ of a checkout that has no sq_scene_set_depth yet, the script runs the `d3` side only: that is how the parent
commit's figure is taken, by the same code, in the same job.

    python tools/gpu_depth.py [--reps 3] [--steps 3] [--spp 256] [--variant 2]
"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 1920, 1080


def deep_slot_bytes(depth):
    """Bytes per slot of the generic pipeline's own block (csrc/sq_device.hip: deep_slot_bytes)."""
    return 0 if depth < 2 else 4 * (depth - 1) + (8 if depth >= 4 else 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--variant", type=int, default=2)
    ap.add_argument("--only", default="", help="comma-separated sides (default: all)")
    a = ap.parse_args()
    import torch
    sqt = importlib.import_module("squigly-trace_amd")
    d = importlib.import_module("squigly-trace_amd.dist")
    data = os.path.join(ROOT, "data")
    ds = sqt.DeviceScene(sqt.BIH(sqt.Mesh.from_obj(os.path.join(data, "scene.obj"), data)), 0)
    cam = sqt.load_camera(os.path.join(data, "camera"))
    ds.set_option("variant", a.variant)
    has_depth = hasattr(ds, "set_depth")

    def side(depth, deep):
        def prepare():
            if has_depth:
                ds.set_depth(depth)
                ds.set_option("deep", deep)
        return prepare

    sides = {"d3": side(3, 0)}
    if has_depth:
        sides["d3_deep"] = side(3, 1)
        sides.update({f"d{k}": side(k, 0) for k in (1, 2, 4, 5, 8)})
    if a.only:
        sides = {k: v for k, v in sides.items() if k in a.only.split(",")}
    frames, forms = {}, {}
    for k, prepare in sides.items():                                  # warm-up (workspace, the depth's block, code objects)
        prepare()
        frames[k] = d.render_frame(ds, cam, a.spp, W, H, want="rgb").clone()
        torch.cuda.synchronize()
        forms[k] = ds.last_plan()["trace_form"]
    if "d3_deep" in frames and "d3" in frames and not torch.equal(frames["d3"], frames["d3_deep"]):
        print(json.dumps({"error": "depth 3 differs between the pipelines"}), flush=True)
        return 1
    ms = {k: [] for k in sides}
    for _ in range(a.reps):
        for k, prepare in sides.items():                              # alternating: a drift of the machine hits every side alike
            prepare()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                d.render_frame(ds, cam, a.spp, W, H, want="rgb")
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3 / a.steps)
    row = {"frame": f"{W}x{H}@{a.spp}", "variant": a.variant, "reps": a.reps, "steps": a.steps, "build": sqt.build_id(), "forms": forms,
           "nonblack": {k: int((f.sum(-1) > 0).sum().item()) for k, f in frames.items()}}
    for k, v in ms.items():
        v.sort()
        row[k + "_best_ms"], row[k + "_median_ms"] = round(v[0], 3), round(v[len(v) // 2], 3)
        if k != "d3":
            row[k + "_slot_bytes"] = deep_slot_bytes(3 if k == "d3_deep" else int(k[1:]))
    if "d3" in ms:
        for k in ms:
            if k != "d3":
                row[k + "_over_d3"] = round(row[k + "_best_ms"] / row["d3_best_ms"], 3)
    print(json.dumps(row), flush=True)
    ds.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
