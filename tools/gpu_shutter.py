"""What motion blur costs: the headline lens frame through DeviceScene.render_lens under the open pose against the same frame
through DeviceScene.render_shutter (libsquigly_shutter.so: every lane computes the pose of its own instant) under a camera that
moves during the exposure; one warm-up frame per side, then `--steps` frames between two device synchronises.

Sides, alternating in one process (--reps rounds; best and median of the per-frame times), jitter 1 throughout:
    lens_r16, lens_r256              render_lens under motion.pose(0)
    shutter_r16_t0, shutter_r16_t1   render_shutter, R = 16, time_jitter 0 and 1
    shutter_r256_t0, shutter_r256_t1 render_shutter, R = 256
    mlens_f100, mlens_f5             one masked step over all R = 16 sub-rays at live fractions 1 and 0.05: live_pixels + render_lens_masked
    mshutter_f100, mshutter_f5       the same step through render_shutter_masked
The motion is the tests' (tests/shutter_restatement.py: MOTION).  The script checks that render_shutter under equal poses gives
render_lens' RGB8 and that the moving frame does not.

    python tools/gpu_shutter.py [--reps 3] [--steps 3] [--spp 256] [--size 1920x1080] [--work-mb 1024] [--only lens_r16,shutter_r16_t1]

--kernels FILE.csv: instead of timing, read the kernel statistics of a `rocprofv3 --kernel-trace --stats` run of this script (a run
of its own: `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/gpu_shutter.py --only
lens_r16,shutter_r16_t1 --reps 1 --steps 1`) and print the average times of the static and the moving ray kernel.
"""
import argparse
import csv
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OPEN = ((0.0, 7.0, 0.75), (1.5707963267948966, 0.0, -0.09817477042468103))
CLOSE = ((1.0, 6.0, 1.25), (1.5707963267948966 + 0.25, 0.0, -0.09817477042468103 + 0.1))


def kernels(path):
    out = {"stats": os.path.basename(path)}
    for r in csv.DictReader(open(path)):
        for name in ("sq_lens_rays", "sq_shutter_rays", "sq_lens_fold", "sq_shutter_fold"):
            if name in r["Name"] and "listed" not in r["Name"]:
                out[name] = {"calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 1)}
    print(json.dumps(out), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--work-mb", type=float, default=1024)
    ap.add_argument("--only", default="", help="comma-separated sides (default: all)")
    ap.add_argument("--kernels", default="", help="a kernel_stats.csv of a rocprofv3 run of this script")
    a = ap.parse_args()
    if a.kernels:
        return kernels(a.kernels)
    w, h = (int(v) for v in a.size.split("x"))
    import torch
    sqt = importlib.import_module("squigly-trace_amd")
    lens = importlib.import_module("squigly-trace_amd.lens")
    mlens = importlib.import_module("squigly-trace_amd.mlens")
    shutter = importlib.import_module("squigly-trace_amd.shutter")
    data = os.path.join(ROOT, "data")
    bih = sqt.BIH(sqt.Mesh.from_obj(os.path.join(data, "scene.obj"), data))
    ds = sqt.DeviceScene(bih, 0)
    ln = sqt.Lens(jitter=1.0)
    moving = {t: sqt.Motion(OPEN, CLOSE, t) for t in (0.0, 1.0)}
    cam = moving[1.0].pose(0)
    dev = torch.device("cuda", 0)

    def lens_side(R):
        return lambda: ds.render_lens(cam, ln, a.spp, R, w, h, want_avg=False, work_mb=a.work_mb).rgb

    def shutter_side(R, m):
        return lambda: ds.render_shutter(m, ln, a.spp, R, w, h, want_avg=False, work_mb=a.work_mb).rgb

    state = {k: torch.zeros(shape, dtype=dt, device=dev) for k, shape, dt in
             (("sums", (w, h, 3), torch.float32), ("sums2", (w, h, 3), torch.float32), ("counts", (w, h), torch.int32),
              ("rgb", (w, h, 3), torch.uint8))}
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    masks = {100: torch.ones((w, h), dtype=torch.uint8, device=dev),
             5: (torch.rand((w, h), generator=gen, device=dev) < 0.05).to(torch.uint8)}

    def masked_side(fraction, m):
        def step():
            index, n_live = ds.live_pixels(masks[fraction], None, 0)
            n = int(n_live.item())
            if m is None:
                ds.render_lens_masked(cam, ln, a.spp, 16, w, h, 0, 16, state["sums"], index, n, sums2=state["sums2"], counts=state["counts"],
                                      work_mb=a.work_mb, out_rgb=state["rgb"])
            else:
                ds.render_shutter_masked(m, ln, a.spp, 16, w, h, 0, 16, state["sums"], index, n, sums2=state["sums2"], counts=state["counts"],
                                         work_mb=a.work_mb, out_rgb=state["rgb"])
            return state["rgb"]
        return step

    sides = {}
    for R in (16, 256):
        if a.spp % R == 0:
            sides[f"lens_r{R}"] = lens_side(R)
            sides[f"shutter_r{R}_t0"] = shutter_side(R, moving[0.0])
            sides[f"shutter_r{R}_t1"] = shutter_side(R, moving[1.0])
    if a.spp % 16 == 0:
        for fraction in (100, 5):
            sides[f"mlens_f{fraction}"] = masked_side(fraction, None)
            sides[f"mshutter_f{fraction}"] = masked_side(fraction, moving[1.0])
    if a.only:
        sides = {k: v for k, v in sides.items() if k in a.only.split(",")}
    frames = {}
    for k, render in sides.items():                                   # warm-up (workspace, table of generator words, code objects)
        frames[k] = render().clone()
        torch.cuda.synchronize()
    if "lens_r16" in frames:
        still = ds.render_shutter(sqt.Motion(OPEN, OPEN, 1.0), ln, a.spp, 16, w, h, want_avg=False, work_mb=a.work_mb).rgb
        if not torch.equal(still, frames["lens_r16"]):
            print(json.dumps({"error": "render_shutter under equal poses differs from render_lens"}), flush=True)
            return 1
        for k in ("shutter_r16_t0", "shutter_r16_t1"):
            if k in frames and torch.equal(frames[k], frames["lens_r16"]):
                print(json.dumps({"error": k + " equals lens_r16: the motion did not show"}), flush=True)
                return 1
    ms = {k: [] for k in sides}
    for _ in range(a.reps):
        for k, render in sides.items():                               # alternating: a drift of the machine hits every side alike
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                render()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3 / a.steps)
    row = {"frame": f"{w}x{h}@{a.spp}", "reps": a.reps, "steps": a.steps, "work_mb": a.work_mb, "build": sqt.build_id(), "lens_build": lens.build_id(),
           "mlens_build": mlens.build_id(), "shutter_build": shutter.build_id(), "live_f5": int(masks[5].sum().item()),
           "nonblack": {k: int((f.sum(-1) > 0).sum().item()) for k, f in frames.items() if not k.startswith("m")}}     # (the masked sides share one state)
    for k, v in ms.items():
        v.sort()
        row[k + "_best_ms"], row[k + "_median_ms"] = round(v[0], 3), round(v[len(v) // 2], 3)
    for k in sides:
        base = {"shutter_r16": "lens_r16", "shutter_r256": "lens_r256", "mshutter_f100": "mlens_f100", "mshutter_f5": "mlens_f5"}.get(k.rsplit("_t", 1)[0])
        if base in ms:
            row[k + "_over_" + base] = round(row[k + "_best_ms"] / row[base + "_best_ms"], 3)
    print(json.dumps(row), flush=True)
    ds.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
