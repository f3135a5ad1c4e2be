"""What a masked lens frame costs: the headline frame through DeviceScene.render_lens (the yardstick, libsquigly_lens.so) against
AdaptiveLens, Adaptive without a lens, one masked lens step (DeviceScene.live_pixels + render_lens_masked) at live fractions 1, 0.25
and 0.05, and the live-list call alone.  One process, the sides alternating, --reps rounds; best and median per side.

    lens          render_lens whole: R sub-rays for every pixel
    adaptive_lens AdaptiveLens at --tol from scratch to finished (its host waits included); reports the fraction of sub-rays spent
    adaptive      Adaptive (no lens) at the same tol, first = step = samples / R samples
    step_f        one masked lens step over all R sub-rays for a random mask of live fraction f (list + render)
                  (step_f_over_f_lens: its time over f times lens' -- 1 would be a step that costs the live fraction and nothing else)
    live          DeviceScene.live_pixels alone at the 0.25 mask with the gap guard on (5 bytes a pixel read, 4 * L written)

    python tools/gpu_mlens.py [--reps 3] [--spp 256] [--subrays 16] [--size 1920x1080] [--tol 0.5] [--only lens,step_1.0]
"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRACTIONS = (1.0, 0.25, 0.05)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--subrays", type=int, default=16)
    ap.add_argument("--tol", type=float, default=0.5)
    ap.add_argument("--eps", type=float, default=1.0)
    ap.add_argument("--first", type=int, default=2, help="sub-rays of AdaptiveLens' first step")
    ap.add_argument("--step", type=int, default=2, help="sub-rays of its later steps")
    ap.add_argument("--live-calls", type=int, default=20)
    ap.add_argument("--only", default="", help="comma-separated sides (default: all)")
    a = ap.parse_args()
    w, h = (int(v) for v in a.size.split("x"))
    S, R = a.spp, a.subrays
    n = S // R
    import torch
    sqt = importlib.import_module("squigly-trace_amd")
    lens_mod = importlib.import_module("squigly-trace_amd.lens")
    mlens = importlib.import_module("squigly-trace_amd.mlens")
    data = os.path.join(ROOT, "data")
    bih = sqt.BIH(sqt.Mesh.from_obj(os.path.join(data, "scene.obj"), data))
    cam = sqt.load_camera(os.path.join(data, "camera"))
    ds = sqt.DeviceScene(bih, 0)
    ln = sqt.Lens(jitter=1.0)
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(1)
    masks = {f: (torch.rand((w, h), device=dev, generator=gen) < f).to(torch.uint8) for f in FRACTIONS}
    state = {k: torch.zeros((w, h) + tail, dtype=dt, device=dev) for k, tail, dt in
             (("sums", (3,), torch.float32), ("sums2", (3,), torch.float32), ("counts", (), torch.int32), ("avg", (3,), torch.float32),
              ("rgb", (3,), torch.uint8))}
    threes = torch.full((w, h), 3, dtype=torch.int32, device=dev)
    info = {}

    def lens_side():
        ds.render_lens(cam, ln, S, R, w, h, want_avg=False)

    def adaptive_lens_side():
        ad = sqt.AdaptiveLens(ds, cam, ln, S, R, w, h, a.tol, eps=a.eps, first=a.first, step=a.step)
        steps = 0
        while not ad.finished:
            ad.step()
            steps += 1
        info["adaptive_lens"] = {"steps": steps, "sub_rays_spent_fraction": round(ad.samples_spent / (w * h * S), 4)}

    def adaptive_side():
        ad = sqt.Adaptive(ds, cam, S, w, h, a.tol, eps=a.eps, first=a.first * n, step=a.step * n)
        steps = 0
        while not ad.finished:
            ad.step()
            steps += 1
        info["adaptive"] = {"steps": steps, "samples_spent_fraction": round(ad.samples_spent / (w * h * S), 4)}

    def step_side(f):
        def run():
            index, n_live = ds.live_pixels(masks[f], state["counts"], 0)
            L = int(n_live.item())                                        # the wait an adaptive loop has anyway
            ds.render_lens_masked(cam, ln, S, R, w, h, 0, R, state["sums"], index, L, sums2=state["sums2"], counts=state["counts"],
                                  out_avg=state["avg"], out_rgb=state["rgb"])
            info[f"step_{f}"] = {"live": L}
        return run

    def live_side():
        for _ in range(a.live_calls):
            ds.live_pixels(masks[0.25], threes, 3)

    sides = {"lens": lens_side, "adaptive_lens": adaptive_lens_side, "adaptive": adaptive_side}
    sides.update({f"step_{f}": step_side(f) for f in FRACTIONS})
    sides["live"] = live_side
    if a.only:
        sides = {k: v for k, v in sides.items() if k in a.only.split(",")}
    for run in sides.values():                                            # warm-up (workspace, table of generator words, code objects)
        run()
        torch.cuda.synchronize()
    ms = {k: [] for k in sides}
    for _ in range(a.reps):
        for k, run in sides.items():                                      # alternating: a drift of the machine hits every side alike
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3 / (a.live_calls if k == "live" else 1))
    row = {"frame": f"{w}x{h}@{S}", "subrays": R, "tol": a.tol, "eps": a.eps, "first": a.first, "step": a.step, "reps": a.reps,
           "build": sqt.build_id(), "lens_build": lens_mod.build_id(), "mlens_build": mlens.build_id(), **info}
    for k, v in ms.items():
        v.sort()
        row[k + "_best_ms"], row[k + "_median_ms"] = round(v[0], 3), round(v[len(v) // 2], 3)
    if "lens" in ms:
        for f in FRACTIONS:
            if f"step_{f}" in ms:
                row[f"step_{f}_over_f_lens"] = round(row[f"step_{f}_best_ms"] / (f * row["lens_best_ms"]), 3)
    if "live" in ms:
        nbytes = 5 * w * h + 4 * int(masks[0.25].sum().item())
        row["live_GB_per_s"] = round(nbytes / (row["live_best_ms"] * 1e-3) / 1e9, 1)
    print(json.dumps(row), flush=True)
    ds.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
