"""Throughput of ray queries (DeviceScene.intersect / sq_intersect_rays_device) in the default form and in variant 1, against the
trace rate of the headline frame itself.

For every scene (data/scene.obj and the C3 / C5 stand-ins of tools/gen_scenes.py) and every N of --ns, three families of N rays:
  camera : the primary rays of the headline 1920 x 1080 frame of data/camera (sq_camera_rays_device), repeated to N
  bounce : from barycentric points on random triangles, uniform directions, |d|^2 in [1, 1.5] (like the frames' bounce rays)
  free   : origins uniform in the root box grown by 20 %, uniform unit directions
Each query is timed with device events around the call, after one warm-up, best of --reps; the line gives Mrays/s of both forms and
whether their (tri, dist, point) are bit-equal.  The headline frame's own rate is rays traced (stats()[0]) over the summed time of
its trace launches (option "timing").

    python tools/gpu_rays.py [--scenes scene,blob,heightfield] [--ns 65536,1048576,16777216] [--reps 5] [--frame-spp 256]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/gpu_rays.py --profile-one   # one 16 Mi call: stage / trace / store split
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


def load_scene(sqt, name):
    data = os.path.join(ROOT, "data")
    if name == "scene":
        mesh = sqt.Mesh.from_obj(os.path.join(data, "scene.obj"), data)
    else:
        import gen_scenes as G
        obj, sq, _ = G.blob_scene(6) if name == "blob" else G.heightfield_scene(708)
        enc = lambda t: t.encode() if isinstance(t, str) else t          # noqa: E731
        mesh = sqt.Mesh.from_text(enc(obj), enc(sq))
    return sqt.BIH(mesh, device=0 if len(mesh) >= 50000 else None), mesh


def families(sqt, ds, bih, n, rng, torch):
    cam = sqt.load_camera(os.path.join(ROOT, "data", "camera"))
    co, cd = ds.camera_rays(cam, 1920, 1080)
    rep = (n + co.numel() // 3 - 1) // (co.numel() // 3)
    cam_o, cam_d = co.reshape(-1, 3).repeat(rep, 1)[:n].contiguous(), cd.reshape(-1, 3).repeat(rep, 1)[:n].contiguous()
    tris = bih.tris
    t = tris[rng.integers(0, len(tris), n)]
    u, v = rng.uniform(0, 1, (2, n, 1)).astype(np.float32)
    flip = (u + v) > 1
    u, v = np.where(flip, 1 - u, u), np.where(flip, 1 - v, v)
    bo = (t["v0"] + u * (t["v1"] - t["v0"]) + v * (t["v2"] - t["v0"])).astype(np.float32)
    dirs = rng.normal(size=(n, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    bd = (dirs * np.sqrt(rng.uniform(1.0, 1.5, (n, 1)))).astype(np.float32)
    b = bih.bounds.astype(np.float64)
    c, half = (b[:3] + b[3:]) / 2, (b[3:] - b[:3]) / 2 * 1.2
    fo = (c + rng.uniform(-1, 1, (n, 3)) * half).astype(np.float32)
    dirs = rng.normal(size=(n, 3))
    fd = (dirs / np.linalg.norm(dirs, axis=1, keepdims=True)).astype(np.float32)
    dev = torch.device("cuda", 0)
    return {"camera": (cam_o, cam_d), "bounce": (torch.from_numpy(bo).to(dev), torch.from_numpy(bd).to(dev)),
            "free": (torch.from_numpy(fo).to(dev), torch.from_numpy(fd).to(dev))}


def time_query(ds, o, d, out, reps, torch):
    """Best of reps, ms, of one intersect call into preallocated outputs (after one warm-up)."""
    ds.intersect(o, d, out=out)
    best = float("inf")
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ds.intersect(o, d, out=out)
        e1.record()
        e1.synchronize()
        best = min(best, e0.elapsed_time(e1))
    return best


def frame_rate(sqt, ds, spp, torch):
    """Rays traced per second by the trace launches of the headline frame (1920 x 1080 @ spp, data/camera)."""
    cam = sqt.load_camera(os.path.join(ROOT, "data", "camera"))
    ds.render_rows(cam, spp, 1920, 1080)                                # warm-up (workspace)
    torch.cuda.synchronize()
    ds.stats(reset=True)
    ds.reset_timing()
    ds.enable_timing(True)
    ds.render_rows(cam, spp, 1920, 1080)
    torch.cuda.synchronize()
    ms, launches, _ = ds.kernel_timing()
    rays = ds.stats(reset=True)[0]
    ds.enable_timing(False)
    ds.reset_timing()
    return rays, ms * launches, rays / (ms * launches * 1e3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="scene,blob,heightfield")
    ap.add_argument("--ns", default="65536,1048576,16777216")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frame-spp", type=int, default=256)
    ap.add_argument("--profile-one", action="store_true", help="one warm-up and one 16 Mi incoherent query (for rocprofv3)")
    args = ap.parse_args()
    import torch
    sqt = importlib.import_module("squigly-trace_amd")
    if args.profile_one:
        bih, _ = load_scene(sqt, "scene")
        ds = sqt.DeviceScene(bih, 0)
        f = families(sqt, ds, bih, 1 << 24, np.random.default_rng(3), torch)
        o, d = f["bounce"]
        ds.intersect(o[:65536], d[:65536])
        torch.cuda.synchronize()
        ds.intersect(o, d)
        torch.cuda.synchronize()
        print(json.dumps({"profile_one": "scene", "family": "bounce", "n": 1 << 24, "plan": ds.last_plan()}))
        return
    ns = [int(x) for x in args.ns.split(",")]
    for name in args.scenes.split(","):
        bih, _ = load_scene(sqt, name)
        ds = sqt.DeviceScene(bih, 0)
        rays, ms, rate = frame_rate(sqt, ds, args.frame_spp, torch)
        print(json.dumps({"scene": name, "frame": f"1920x1080@{args.frame_spp}", "rays_traced": rays, "trace_ms": round(ms, 3),
                          "frame_trace_mrays_s": round(rate, 1), "trace_form": ds.last_plan()["trace_form"]}), flush=True)
        fam = families(sqt, ds, bih, max(ns), np.random.default_rng(1), torch)
        for fname, (o_all, d_all) in fam.items():
            for n in ns:
                o, d = o_all[:n], d_all[:n]
                row = {"scene": name, "family": fname, "n": n}
                res = {}
                for variant in (2, 1):
                    ds.set_option("variant", variant)
                    out = sqt.Hits(torch.empty(n, dtype=torch.int32, device="cuda:0"), torch.empty(n, device="cuda:0"),
                                   torch.empty(n, 3, device="cuda:0"))
                    best = time_query(ds, o, d, out, args.reps, torch)
                    key = "default" if variant == 2 else "variant1"
                    row[key + "_ms"] = round(best, 3)
                    row[key + "_mrays_s"] = round(n / (best * 1e3), 1)
                    if variant == 2:
                        row["form"] = ds.last_plan()["trace_form"]
                    res[variant] = [t.view(torch.int32).cpu() for t in out]
                ds.set_option("variant", 2)
                row["bit_equal"] = all(torch.equal(a, b) for a, b in zip(res[2], res[1]))
                hit = (res[2][0] >= 0).float().mean().item()
                row["hit_fraction"] = round(hit, 3)
                print(json.dumps(row), flush=True)
        ds.close()
        del bih
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
