"""What adaptive sampling costs and buys (Adaptive / sq_render_rows_device_masked / sq_adaptive_update_device).

On the headline frame (data/scene.obj, 1920 x 1080 @ 256 spp), device events around each call, best of --reps after a warm-up:

  --mode range     one range call [--k0, --k1) through render_rows_range.  Uses nothing but the range call, so the same file times
                   a checkout that does not have the masked call yet (run it from that checkout's tools/ for an A/B in one job).
  --mode masked    the same range through render_rows_masked: with all three optional buffers None (must equal the range call,
                   bits and time), with every pixel live and the second moments on (what the moments cost), and under seeded
                   random masks at the live fractions --fractions (what a dead pixel costs: nothing, if the time follows the
                   fraction down to the call's fixed cost).
  --mode frame     the whole adaptive frame (--tol, --eps, --first, --step) against the one-call frame: milliseconds, samples
                   spent, steps, and per step the live fraction and the time.

    python tools/gpu_adaptive.py --mode masked [--reps 5] [--dims 1920,1080] [--spp 256] [--k0 16 --k1 32]

One JSON line per measurement.
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
    ap.add_argument("--mode", choices=["range", "masked", "frame"], default="masked")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dims", default="1920,1080")
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--k0", type=int, default=16)
    ap.add_argument("--k1", type=int, default=32)
    ap.add_argument("--fractions", default="1,0.5,0.125,0.015625")
    ap.add_argument("--tol", type=float, default=0.5)
    ap.add_argument("--eps", type=float, default=1.0)
    ap.add_argument("--first", type=int, default=16)
    ap.add_argument("--step", type=int, default=16)
    a = ap.parse_args()
    sqt = importlib.import_module("squigly-trace_amd")
    import torch
    data = os.path.join(ROOT, "data")
    bih = sqt.BIH(sqt.Mesh.from_obj(os.path.join(data, "scene.obj"), data))
    cam = sqt.load_camera(os.path.join(data, "camera"))
    w, h = (int(v) for v in a.dims.split(","))
    n, k0, k1 = a.spp, a.k0, a.k1
    ds = sqt.DeviceScene(bih, 0)
    dev = torch.device("cuda", 0)
    print(json.dumps({"build": sqt.build_id(), "mode": a.mode, "frame": [w, h, n], "range": [k0, k1]}), flush=True)

    def timed(fn, before=None):
        """Best of --reps device-event times of fn(), after one untimed warm-up; before() runs outside the timed window."""
        best = float("inf")
        for rep in range(max(1, a.reps) + 1):
            if before is not None:
                before()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if rep:
                best = min(best, e0.elapsed_time(e1))
        return round(best, 3)

    # the fold over [0, k0) that every timed call continues
    base_sums = torch.empty((w, h, 3), dtype=torch.float32, device=dev)
    avg = torch.empty((w, h, 3), dtype=torch.float32, device=dev)
    rgb = torch.empty((w, h, 3), dtype=torch.uint8, device=dev)
    if k0 > 0:
        ds.render_rows_range(cam, n, w, h, 0, k0, base_sums, out_avg=avg, out_rgb=rgb)
    sums = base_sums.clone()
    torch.cuda.synchronize()

    if a.mode == "range":
        ms = timed(lambda: ds.render_rows_range(cam, n, w, h, k0, k1, sums, out_avg=avg, out_rgb=rgb), before=lambda: sums.copy_(base_sums))
        print(json.dumps({"call": "render_rows_range", "ms": ms}), flush=True)
        ds.close()
        return

    if a.mode == "masked":
        ms = timed(lambda: ds.render_rows_range(cam, n, w, h, k0, k1, sums, out_avg=avg, out_rgb=rgb), before=lambda: sums.copy_(base_sums))
        ref = (sums.clone(), avg.clone(), rgb.clone())
        print(json.dumps({"call": "render_rows_range", "ms": ms}), flush=True)
        ms = timed(lambda: ds.render_rows_masked(cam, n, w, h, k0, k1, sums, out_avg=avg, out_rgb=rgb), before=lambda: sums.copy_(base_sums))
        same = all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(ref, (sums, avg, rgb)))
        print(json.dumps({"call": "render_rows_masked, no optional buffer", "ms": ms, "bit_equal_to_range_call": bool(same)}), flush=True)
        # second moments: their fold over [0, k0) first
        base_sums2 = torch.zeros_like(base_sums)
        base_counts = torch.zeros((w, h), dtype=torch.int32, device=dev)
        if k0 > 0:
            ds.render_rows_masked(cam, n, w, h, 0, k0, sums, sums2=base_sums2, counts=base_counts, out_avg=avg, out_rgb=rgb)
        sums2, counts = base_sums2.clone(), base_counts.clone()

        def reset():
            sums.copy_(base_sums); sums2.copy_(base_sums2); counts.copy_(base_counts)
        ms = timed(lambda: ds.render_rows_masked(cam, n, w, h, k0, k1, sums, sums2=sums2, counts=counts, out_avg=avg, out_rgb=rgb), before=reset)
        same = torch.equal(sums.view(torch.int32), ref[0].view(torch.int32)) and torch.equal(rgb, ref[2])
        print(json.dumps({"call": "render_rows_masked, every pixel live, moments and counts", "ms": ms, "sums_rgb_bit_equal_to_range_call": bool(same)}), flush=True)
        g = torch.Generator(device="cpu").manual_seed(1)
        u = torch.rand((w, h), generator=g)
        for f in (float(v) for v in a.fractions.split(",")):
            mask = (u < f).to(torch.uint8).to(dev)
            live = int(mask.sum().item())
            ms = timed(lambda: ds.render_rows_masked(cam, n, w, h, k0, k1, sums, mask=mask, sums2=sums2, counts=counts, out_avg=avg, out_rgb=rgb), before=reset)
            on = mask.bool()
            same = (torch.equal(sums.view(torch.int32)[on], ref[0].view(torch.int32)[on]) and torch.equal(sums.view(torch.int32)[~on], base_sums.view(torch.int32)[~on])
                    and bool((counts[on] == k1).all()) and bool((counts[~on] == k0).all()))
            print(json.dumps({"call": "render_rows_masked, random mask", "live_fraction": round(live / (w * h), 5), "live": live, "ms": ms,
                              "live_equal_to_range_call_dead_untouched": bool(same)}), flush=True)
        ds.close()
        return

    # ---- the whole adaptive frame against the one-call frame
    one = timed(lambda: ds.render_rows(cam, n, w, h, out_avg=avg, out_rgb=rgb))
    print(json.dumps({"call": "render_rows (one call)", "ms": one, "samples": w * h * n}), flush=True)
    best, log = float("inf"), None
    for rep in range(max(1, a.reps) + 1):
        ad = sqt.Adaptive(ds, cam, n, w, h, a.tol, eps=a.eps, first=a.first, step=a.step)
        steps = []
        torch.cuda.synchronize()
        f0 = torch.cuda.Event(enable_timing=True)
        f0.record()
        while not ad.finished:
            live_before, done_before = ad.live, ad.done
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ad.step()                                                   # waits for the live count
            e1.record()
            torch.cuda.synchronize()
            steps.append({"range": [done_before, ad.done], "live_fraction": round(live_before / (w * h), 5), "ms": round(e0.elapsed_time(e1), 3)})
        f1 = torch.cuda.Event(enable_timing=True)
        f1.record()
        torch.cuda.synchronize()
        ms = f0.elapsed_time(f1)
        if rep and ms < best:
            best, log = ms, {"call": "Adaptive", "tol": a.tol, "eps": a.eps, "first": a.first, "step": a.step, "ms": round(ms, 3),
                             "steps": len(steps), "samples_spent": ad.samples_spent, "of": w * h * n, "per_step": steps}
    print(json.dumps(log), flush=True)
    ds.close()


if __name__ == "__main__":
    main()
