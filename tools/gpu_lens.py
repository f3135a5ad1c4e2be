"""What anti-aliasing and depth of field cost: the headline frame through DeviceScene.render_rows against the same frame through
DeviceScene.render_lens (libsquigly_lens.so: ray kernel -> sq_raytrace_rays_device -> fold kernel), one warm-up frame per side, then
`--steps` frames between two device synchronises.

Sides, alternating in one process (--reps rounds; best and median of the per-frame times):
    rows         render_rows: one primary pass per frame inside the main library
    lens_r1      render_lens, R = 1, no jitter: the same bits by the query route -- the cost of that route and of the two new kernels
    lens_r16     render_lens, R = 16, jitter 1: 16 stratified primary rays per pixel, 16 samples on each
    lens_r256    render_lens, R = 256, jitter 1: a primary ray per sample
The script checks that lens_r1 gives render_rows' RGB8 and that lens_r16 does not.

    python tools/gpu_lens.py [--reps 3] [--steps 3] [--spp 256] [--size 1920x1080] [--work-mb 1024] [--only rows,lens_r16]

--kernels FILE.csv: instead of timing, read the kernel statistics of a `rocprofv3 --kernel-trace --stats` run of this script
(a run of its own: `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/gpu_lens.py --only lens_r16
--reps 1 --steps 1`) and print the two lens kernels' average times and their achieved bytes per second against the HBM peak.
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

HBM_PEAK = 8.0e12          # bytes per second, MI355X (specification)
SUBRAYS = {"lens_r1": 1, "lens_r16": 16, "lens_r256": 256}


def kernel_bytes(pixels, nb, carry, want_rgb=True):
    """Bytes the two kernels move for a batch of nb sub-rays of `pixels` pixels: the ray kernel writes 32 bytes per slot (origin,
    direction, seed); the fold reads 12 per slot, writes the sum (reads it too when it carries) and, on the last batch, the RGB8."""
    rays = 32 * pixels * nb
    fold = 12 * pixels * nb + 12 * pixels * (2 if carry else 1) + (3 * pixels if want_rgb else 0)
    return rays, fold


def kernels(path, pixels, spp, work_mb, subrays):
    lens = importlib.import_module("squigly-trace_amd.lens")
    plan = lens.plan(pixels, 0, subrays, int(work_mb * 2 ** 20))
    rays_b = sum(kernel_bytes(pixels, b - a, a > 0)[0] for a, b in plan) / len(plan)
    fold_b = sum(kernel_bytes(pixels, b - a, a > 0, b == subrays)[1] for a, b in plan) / len(plan)
    out = {"stats": os.path.basename(path), "batches": len(plan), "subrays_per_batch": plan[0][1] - plan[0][0]}
    for r in csv.DictReader(open(path)):
        for name, nbytes in (("sq_lens_rays", rays_b), ("sq_lens_fold", fold_b)):
            if name in r["Name"]:
                us = float(r["AverageNs"]) / 1e3
                out[name] = {"calls": int(r["Calls"]), "avg_us": round(us, 1), "avg_bytes": int(nbytes), "TB_per_s": round(nbytes / us / 1e6, 3),
                             "of_hbm_peak": round(nbytes / (us * 1e-6) / HBM_PEAK, 3)}
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
    ap.add_argument("--kernels-subrays", type=int, default=16)
    a = ap.parse_args()
    w, h = (int(v) for v in a.size.split("x"))
    if a.kernels:
        return kernels(a.kernels, w * h, a.spp, a.work_mb, a.kernels_subrays)
    import torch
    sqt = importlib.import_module("squigly-trace_amd")
    lens = importlib.import_module("squigly-trace_amd.lens")
    data = os.path.join(ROOT, "data")
    bih = sqt.BIH(sqt.Mesh.from_obj(os.path.join(data, "scene.obj"), data))
    cam = sqt.load_camera(os.path.join(data, "camera"))
    ds = sqt.DeviceScene(bih, 0)

    def lens_side(subrays, jitter):
        ln = sqt.Lens(jitter=jitter)
        return lambda: ds.render_lens(cam, ln, a.spp, subrays, w, h, want_avg=False, work_mb=a.work_mb).rgb

    sides = {"rows": lambda: ds.render_rows(cam, a.spp, w, h, want_avg=False)[1], "lens_r1": lens_side(1, 0.0)}
    for name in ("lens_r16", "lens_r256"):
        if a.spp % SUBRAYS[name] == 0:
            sides[name] = lens_side(SUBRAYS[name], 1.0)
    if a.only:
        sides = {k: v for k, v in sides.items() if k in a.only.split(",")}
    frames = {}
    for k, render in sides.items():                                   # warm-up (workspace, table of generator words, code objects)
        frames[k] = render().clone()
        torch.cuda.synchronize()
    if "rows" in frames and "lens_r1" in frames and not torch.equal(frames["rows"], frames["lens_r1"]):
        print(json.dumps({"error": "lens_r1 differs from rows"}), flush=True)
        return 1
    if "rows" in frames and "lens_r16" in frames and torch.equal(frames["rows"], frames["lens_r16"]):
        print(json.dumps({"error": "lens_r16 equals rows: the jitter did not show"}), flush=True)
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
           "batches": {k: len(lens.plan(w * h, 0, SUBRAYS[k], int(a.work_mb * 2 ** 20))) for k in sides if k in SUBRAYS},
           "nonblack": {k: int((f.sum(-1) > 0).sum().item()) for k, f in frames.items()}}
    for k, v in ms.items():
        v.sort()
        row[k + "_best_ms"], row[k + "_median_ms"] = round(v[0], 3), round(v[len(v) // 2], 3)
    for k in sides:
        if k != "rows" and "rows" in ms:
            row[k + "_over_rows"] = round(row[k + "_best_ms"] / row["rows_best_ms"], 3)
    print(json.dumps(row), flush=True)
    ds.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
