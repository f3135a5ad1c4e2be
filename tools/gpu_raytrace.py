"""Radiance queries (DeviceScene.raytrace / sq_raytrace_rays_device) against the frame call, and their throughput on incoherent rays.

1. The frame as a query: the headline 1920 x 1080 frame of data/camera at --frame-spp samples, once through render_rows_range and once
   through raytrace of its camera rays with its seeds (rays and seeds already on the device), alternating in one process; also the
   frame call with option primary_tiles = 0 (the untiled primary pass, which is how a query walks its primary rays).  Device events
   around each call, best and median of --reps after a warm-up, ratio query / frame, and whether sum, avg and rgb are bit-equal.
2. Incoherent rays: for every scene (data/scene.obj and the C3 / C5 stand-ins of tools/gen_scenes.py), N of --ns and spp of --spps,
   two families of N rays with random 64-bit seeds:
     free     : origins uniform in the root box grown by 20 %, uniform unit directions
     to_light : origins uniform in the root box, aimed at a random point of a random emissive triangle
   Msamples/s of the default form and of variant 1 (best of --reps after a warm-up) and whether their sums are bit-equal.

    python tools/gpu_raytrace.py [--scenes scene,blob,heightfield] [--ns 1048576,16777216] [--spps 1,16] [--reps 3] [--frame-spp 256]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/gpu_raytrace.py --profile-one query|frame   # one side at a time
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from gpu_rays import load_scene   # noqa: E402

W, H = 1920, 1080


def timed(fn, torch):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def frame_as_query(sqt, ds, spp, reps, torch):
    cam = sqt.load_camera(os.path.join(ROOT, "data", "camera"))
    o, d = ds.camera_rays(cam, W, H)
    seeds = sqt.frame_seeds(spp, W, H, device="cuda:0")
    fs, qs = torch.empty_like(o), torch.empty_like(o)
    out = {}

    def frame(tiles):
        ds.set_option("primary_tiles", tiles)
        out["frame"] = ds.render_rows_range(cam, spp, W, H, 0, spp, fs)
        ds.set_option("primary_tiles", 1)

    def query():
        out["query"] = ds.raytrace(o, d, seeds=seeds, samples=spp, sums=qs, want_rgb=True)

    sides = {"frame": lambda: frame(1), "query": query, "frame_untiled": lambda: frame(0)}
    for fn in sides.values():                                        # warm-up: workspace, code objects
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in sides}
    for _ in range(reps):
        for k, fn in sides.items():                                  # alternating: a drift of the machine hits every side alike
            ms[k].append(timed(fn, torch))
    frame(1)
    torch.cuda.synchronize()
    (favg, frgb), q = out["frame"], out["query"]
    equal = bool(torch.equal(fs.view(torch.int32), qs.view(torch.int32)) and torch.equal(favg.view(torch.int32), q.avg.view(torch.int32))
                 and torch.equal(frgb, q.rgb))
    row = {"frame_as_query": f"{W}x{H}@{spp}", "reps": reps, "bit_equal": equal, "form": ds.last_plan()["trace_form"]}
    for k, v in ms.items():
        v.sort()
        row[k + "_best_ms"], row[k + "_median_ms"] = round(v[0], 3), round(v[len(v) // 2], 3)
    row["query_over_frame"] = round(row["query_best_ms"] / row["frame_best_ms"], 4)
    row["untiled_over_frame"] = round(row["frame_untiled_best_ms"] / row["frame_best_ms"], 4)
    print(json.dumps(row), flush=True)


def families(bih, n, rng, torch):
    b = bih.bounds.astype(np.float64)
    c, half = (b[:3] + b[3:]) / 2, (b[3:] - b[:3]) / 2
    dirs = rng.normal(size=(n, 3))
    fo = (c + rng.uniform(-1, 1, (n, 3)) * half * 1.2).astype(np.float32)
    fd = (dirs / np.linalg.norm(dirs, axis=1, keepdims=True)).astype(np.float32)
    mats = bih.materials
    lit = np.nonzero(((mats["emit"] * mats["emissive"][:, None]) != 0).any(-1)[bih.tris["mat"]])[0]
    t = bih.tris[lit[rng.integers(0, len(lit), n)]]
    u, v = rng.uniform(0, 1, (2, n, 1)).astype(np.float32)
    flip = (u + v) > 1
    u, v = np.where(flip, 1 - u, u), np.where(flip, 1 - v, v)
    lo = (c + rng.uniform(-1, 1, (n, 3)) * half).astype(np.float32)
    ld = ((t["v0"] + u * (t["v1"] - t["v0"]) + v * (t["v2"] - t["v0"])) - lo).astype(np.float32)
    seeds = torch.from_numpy(rng.integers(-(1 << 60), 1 << 60, n)).cuda()
    g = lambda a: torch.from_numpy(a).cuda()                           # noqa: E731
    return {"free": (g(fo), g(fd)), "to_light": (g(lo), g(ld))}, seeds


def incoherent(sqt, name, ns, spps, reps, torch):
    bih, _ = load_scene(sqt, name)
    ds = sqt.DeviceScene(bih, 0)
    fam, seeds = families(bih, max(ns), np.random.default_rng(1), torch)
    for fname, (o_all, d_all) in fam.items():
        for n in ns:
            o, d, s = o_all[:n], d_all[:n], seeds[:n]
            sums = torch.empty_like(o)
            for spp in spps:
                row = {"scene": name, "family": fname, "n": n, "spp": spp}
                res = {}
                for variant in (2, 1):
                    ds.set_option("variant", variant)
                    call = lambda: ds.raytrace(o, d, seeds=s, samples=spp, sums=sums, want_avg=False)   # noqa: E731
                    call()
                    best = min(timed(call, torch) for _ in range(reps))
                    key = "default" if variant == 2 else "variant1"
                    row[key + "_ms"] = round(best, 3)
                    row[key + "_msamples_s"] = round(n * spp / (best * 1e3), 1)
                    if variant == 2:
                        row["form"] = ds.last_plan()["trace_form"]
                    res[variant] = sums.view(torch.int32).clone()
                ds.set_option("variant", 2)
                row["bit_equal"] = bool(torch.equal(res[1], res[2]))
                row["lit_fraction"] = round((sums != 0).any(-1).float().mean().item(), 3)
                print(json.dumps(row), flush=True)
    ds.close()
    del bih
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="scene,blob,heightfield")
    ap.add_argument("--ns", default="1048576,16777216")
    ap.add_argument("--spps", default="1,16")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--frame-spp", type=int, default=256)
    ap.add_argument("--skip-frame", action="store_true", help="only the incoherent rays")
    ap.add_argument("--profile-one", choices=("query", "frame"), help="one warm-up and one call of that side (for rocprofv3)")
    args = ap.parse_args()
    import torch
    sqt = importlib.import_module("squigly-trace_amd")
    if args.profile_one or not args.skip_frame:
        bih, _ = load_scene(sqt, "scene")
        ds = sqt.DeviceScene(bih, 0)
        if args.profile_one:
            cam = sqt.load_camera(os.path.join(ROOT, "data", "camera"))
            o, d = ds.camera_rays(cam, W, H)
            seeds = sqt.frame_seeds(args.frame_spp, W, H, device="cuda:0")
            sums = torch.empty_like(o)
            for _ in range(2):
                if args.profile_one == "query":
                    ds.raytrace(o, d, seeds=seeds, samples=args.frame_spp, sums=sums, want_rgb=True)
                else:
                    ds.render_rows_range(cam, args.frame_spp, W, H, 0, args.frame_spp, sums)
                torch.cuda.synchronize()
            print(json.dumps({"profile_one": args.profile_one, "frame": f"{W}x{H}@{args.frame_spp}", "plan": ds.last_plan()}))
            return
        frame_as_query(sqt, ds, args.frame_spp, max(args.reps, 5), torch)
        ds.close()
    for name in [s for s in args.scenes.split(",") if s]:
        incoherent(sqt, name, [int(x) for x in args.ns.split(",")], [int(x) for x in args.spps.split(",")], args.reps, torch)


if __name__ == "__main__":
    main()
