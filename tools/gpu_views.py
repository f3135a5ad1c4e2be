"""Cost of many views of one scene: one batched call (DeviceScene.render_views / sq_render_views_device) against one render_rows
call per view on the same stream.

For every N of --views: N deterministic cameras derived from data/camera (yaw swept over +-0.1 rad, position jittered by a few
hundredths, so that every view sees the scene), one frame size.  Times both ways with device events around the whole work, after
one warm-up of each shape, best of --reps, and prints batched ms, sequential ms, Msamples/s of each and whether every view of the
batched call is bit-equal (avg and RGB8) to its single call.

    python tools/gpu_views.py [--dims 256,256] [--spp 4] [--views 1,8,64] [--reps 5] [--set primary_pooled=1]

Under `rocprofv3 --kernel-trace --stats` run one N at a time (e.g. --views 64 --reps 1) to see where the batched call's time goes.
"""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def view_cameras(sqt, n):
    """n cameras of data/camera with the yaw swept and the position jittered (deterministic)."""
    pos, ang = (list(map(float, ln.split())) for ln in open(os.path.join(ROOT, "data", "camera")).read().split("\n") if ln.strip())
    cams = []
    for i in range(n):
        f = i / max(1, n - 1) - 0.5                                   # -0.5 .. 0.5
        p = (pos[0] + 0.04 * f, pos[1] - 0.02 * (i % 3), pos[2] + 0.01 * (i % 5))
        a = (ang[0] + 0.2 * f, ang[1], ang[2])
        cams.append(sqt.camera_from_text(f"{p[0]!r} {p[1]!r} {p[2]!r}\n{a[0]!r} {a[1]!r} {a[2]!r}\n".encode()))
    return cams


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", default="256,256")
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--views", default="1,8,64", help="comma-separated view counts")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--set", action="append", default=[], metavar="KEY=VALUE", help="sq_set_option before timing (repeatable)")
    ap.add_argument("--batched-only", action="store_true", help="skip the sequential calls and the comparison (for a kernel trace)")
    a = ap.parse_args()
    sqt = importlib.import_module("squigly-trace_amd")
    import torch
    data = os.path.join(ROOT, "data")
    bih = sqt.BIH(sqt.Mesh.from_obj(os.path.join(data, "scene.obj"), data))
    w, h = (int(v) for v in a.dims.split(","))
    n = a.spp
    ds = sqt.DeviceScene(bih, 0)
    for kv in a.set:
        k, v = kv.split("=", 1)
        ds.set_option(k, int(v))
    print(f"build {sqt.build_id()}  frames {w}x{h} @ {n} spp  options {a.set}", flush=True)

    def best_of(fn):
        fn()                                                          # warm-up of this shape (workspace, camera table)
        torch.cuda.synchronize()
        best, out = float("inf"), None
        for _ in range(max(1, a.reps)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn()
            e1.record()
            torch.cuda.synchronize()
            best = min(best, e0.elapsed_time(e1))
        return best, out

    ok = True
    for nv in (int(v) for v in a.views.split(",")):
        cams = view_cameras(sqt, nv)
        out_avg = torch.empty((nv, w, h, 3), dtype=torch.float32, device="cuda:0")
        out_rgb = torch.empty((nv, w, h, 3), dtype=torch.uint8, device="cuda:0")
        if a.batched_only:
            t_bat, _ = best_of(lambda: ds.render_views(cams, n, w, h, out_avg=out_avg, out_rgb=out_rgb))
            print(json.dumps({"views": nv, "dims": [w, h], "spp": n, "batched_ms": round(t_bat, 3)}), flush=True)
            continue
        t_seq, _ = best_of(lambda: [ds.render_rows(c, n, w, h, out_avg=out_avg[i], out_rgb=out_rgb[i]) for i, c in enumerate(cams)])
        seq_avg, seq_rgb = out_avg.clone(), out_rgb.clone()
        t_bat, (avg, rgb) = best_of(lambda: ds.render_views(cams, n, w, h))
        same = torch.equal(avg.view(torch.int32), seq_avg.view(torch.int32)) and torch.equal(rgb, seq_rgb)
        msamples = nv * w * h * n / 1e6
        row = {"views": nv, "dims": [w, h], "spp": n, "batched_ms": round(t_bat, 3), "sequential_ms": round(t_seq, 3),
               "batched_msamples_s": round(msamples / t_bat * 1e3, 1), "sequential_msamples_s": round(msamples / t_seq * 1e3, 1),
               "speedup": round(t_seq / t_bat, 2), "bit_equal_every_view": bool(same)}
        ok = ok and same
        print(json.dumps(row), flush=True)
    ds.close()
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
