"""Cost of splitting a frame into progressive sample ranges (Progressive / sq_render_rows_device_range).

Renders the headline frame (data/scene.obj, 1920 x 1080 @ 256 spp) in 1, 8, 32 and 256 equal steps and prints, per schedule,
the total time (device events around the whole schedule, after one warm-up frame of that schedule; best of --reps), the cost
per extra call against the one-step schedule, and whether the final avg / RGB8 / sums are bit-equal to the one-call frame
(render_rows).  Every step is one range call that re-traces the primary rays and ends with the ramp-down of its trace launches.

    python tools/gpu_progressive.py [--steps 1,8,32,256] [--reps 3] [--dims 1920,1080] [--spp 256] [--no-warmup]

Under `rocprofv3 --kernel-trace --stats` run one schedule at a time (e.g. --steps 256 --reps 1) to see where its time goes.
"""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", default="1,8,32,256", help="comma-separated numbers of steps per frame")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dims", default="1920,1080")
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--no-warmup", action="store_true")
    a = ap.parse_args()
    sqt = importlib.import_module("squigly-trace_amd")
    import torch
    data = os.path.join(ROOT, "data")
    bih = sqt.BIH(sqt.Mesh.from_obj(os.path.join(data, "scene.obj"), data))
    cam = sqt.load_camera(os.path.join(data, "camera"))
    w, h = (int(v) for v in a.dims.split(","))
    n = a.spp
    ds = sqt.DeviceScene(bih, 0)
    ref_avg, ref_rgb = ds.render_rows(cam, n, w, h)
    ref_sums = torch.empty_like(ref_avg)
    ds.render_rows_range(cam, n, w, h, 0, n, ref_sums, want_avg=False, want_rgb=False)
    torch.cuda.synchronize()
    print(f"build {sqt.build_id()}  frame {w}x{h} @ {n} spp", flush=True)

    def schedule(k):
        p = sqt.Progressive(ds, cam, n, w, h)
        per = -(-n // k)
        while not p.finished:
            avg, rgb = p.step(per)
        return avg, rgb, p.sums

    rows = []
    base = None
    for k in (int(v) for v in a.steps.split(",")):
        if not a.no_warmup:
            schedule(k)
            torch.cuda.synchronize()
        best = float("inf")
        for _ in range(max(1, a.reps)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            avg, rgb, sums = schedule(k)
            e1.record()
            torch.cuda.synchronize()
            best = min(best, e0.elapsed_time(e1))
        same = (torch.equal(avg.view(torch.int32), ref_avg.view(torch.int32)) and torch.equal(rgb, ref_rgb)
                and torch.equal(sums.view(torch.int32), ref_sums.view(torch.int32)))
        if base is None and k == 1:
            base = best
        extra = (best - base) / (k - 1) if base is not None and k > 1 else None
        row = {"steps": k, "ms": round(best, 3), "ms_per_extra_call": None if extra is None else round(extra, 4),
               "bit_equal_to_one_call": bool(same)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    ds.close()
    if not all(r["bit_equal_to_one_call"] for r in rows):
        sys.exit(1)


if __name__ == "__main__":
    main()
