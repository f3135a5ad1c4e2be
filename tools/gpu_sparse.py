"""Times sparse frames (libsquigly_denoise.so: sq_denoise_sparse_mask_device, sq_denoise_upsample_device) on the GPU at 1920 x 1080 on
data/scene.obj: the two calls between two device events (warm, median of repeated runs, spread) with their achieved bytes per second
against a device copy of the same compulsory bytes in the same job; a step of sqt.Temporal at 16 spp with sparse=None, 2 and 4, one
step of each in turn, round after round, so that a drift of the machine falls on all three alike -- sparse=None's own spread is the
yardstick the differences are read against; the parts of a sparse step; and the fraction of the pixels each stride traces.

    python tools/gpu_sparse.py [--rows 1080 --cols 1920 --spp 16 --reps 30 --rounds 12 --no-step --out FILE.json]

Prints one JSON object; every time is in milliseconds.  Needs a GPU: there is no fallback."""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GUIDES = 28                    # bytes of a pixel's guides: triangle 4, normal 12, point 12


MASK_BYTES = GUIDES + 1        # compulsory bytes per pixel of the mask call: the guides in (a tap's are among them), a byte out


def upsample_bytes(s):
    """Compulsory bytes per pixel of the fill: every pixel's guides and mask byte in, colour and variance out (16), and one pixel in
    s * s read as a tap or copied through (its guides are counted already)."""
    return GUIDES + 1 + 16 + 16.0 / (s * s)


def timed(torch, fn, reps, warm=3):
    """(median, min, max) milliseconds of fn() between two device events, after `warm` untimed runs."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        ms.append(once(torch, fn))
    return spread(ms)


def once(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def spread(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4), "reps": len(ms)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1080)
    ap.add_argument("--cols", type=int, default=1920)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--no-step", action="store_true", help="leave out the Temporal.step measurements: the two calls alone")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/gpu_sparse.py needs a GPU: nothing is measured without one")
    sqt = importlib.import_module("squigly-trace_amd")
    dn = importlib.import_module("squigly-trace_amd.denoise")
    rows, cols, n, spp, period = a.rows, a.cols, a.rows * a.cols, a.spp, 64
    data = os.path.join(ROOT, "data")
    bih = sqt.BIH(sqt.Mesh.from_obj(os.path.join(data, "scene.obj"), data))
    cams = [sqt.camera_from_text(b"%.3f 7 0.75\n1.5707963267948966 0 -0.09817477042468103\n" % (0.01 * i)) for i in range(a.rounds + 4)]
    ds = sqt.DeviceScene(bih, 0)
    res = {"rows": rows, "cols": cols, "pixels": n, "spp": spp, "device": torch.cuda.get_device_name(0), "denoise_build_id": dn.build_id(),
           "main_build_id": sqt.build_id()}
    try:
        sp = dn.default_sigma_p(ds.bih.bounds)
        g = ds.guides(cams[0], rows, cols)
        res["hit"] = round(float((g.tri >= 0).float().mean()), 4)
        color = torch.rand((rows, cols, 3), device="cuda")
        var = torch.rand((rows, cols), device="cuda")
        out = (torch.empty_like(color), torch.empty_like(var))
        # what a call costs that moves nothing: the same call on the guides' first pixel alone
        one = type(g)(*(t[:1, :1].contiguous() for t in g))
        res["mask_of_one_pixel"] = timed(torch, lambda: dn.sparse_mask(one, 2, (0, 0), sigma_p=sp), a.reps)
        # a device copy reads and writes each of its bytes: a copy of B / 2 bytes moves B
        gbs = lambda b, ms: round(b * n / (ms * 1e-3) / 1e9, 1)      # noqa: E731
        for s in (2, 4):
            r = res["stride_%d" % s] = {}
            mask = dn.sparse_mask(g, s, (0, 0), sigma_p=sp)
            r["live_pixels"] = int((mask != 0).sum())
            r["lattice_pixels"] = len(range(0, rows, s)) * len(range(0, cols, s))
            r["holes"] = r["live_pixels"] - r["lattice_pixels"]
            r["live"] = round(r["live_pixels"] / n, 5)
            for name, fn, b in (("mask", lambda: dn.sparse_mask(g, s, (0, 0), sigma_p=sp), MASK_BYTES),
                                ("upsample", lambda: dn.upsample(color, g, mask, s, (0, 0), var=var, out=out, sigma_p=sp), upsample_bytes(s))):
                r[name] = timed(torch, fn, a.reps)
                src = torch.empty(int(b * n / 2), dtype=torch.uint8, device="cuda").fill_(1)
                dst = torch.empty_like(src)
                r[name + "_copy_of_the_same_bytes"] = timed(torch, lambda: dst.copy_(src), a.reps)
                r[name + "_bytes_per_pixel"] = round(b, 2)
                r[name + "_gb_per_s"], r[name + "_copy_gb_per_s"] = gbs(b, r[name]["median"]), gbs(b, r[name + "_copy_of_the_same_bytes"]["median"])
                del src, dst
        # the step: one of each variant in turn, round after round
        variants = () if a.no_step else (None, 2, 4)
        seqs = {v: sqt.Temporal(ds, rows, cols, spp, period=period, sparse=v) for v in variants}
        for v in variants:                                            # warm: the first frame has no history
            for cam in cams[:2]:
                seqs[v].step(cam)
        torch.cuda.synchronize()
        ms = {v: [] for v in variants}
        for i in range(a.rounds):
            for v in variants:
                ms[v].append(once(torch, lambda: seqs[v].step(cams[2 + i])))
        res["step"] = {("dense" if v is None else "sparse_%d" % v): spread(ms[v]) for v in variants}
        res["step"]["live_of_the_last_frame"] = {"sparse_%d" % v: round(float((seqs[v].live != 0).float().mean()), 5) for v in variants if v}
        # the parts of a sparse step that a dense step does not have, or has at another size
        sums, sums2 = torch.zeros((rows, cols, 3), device="cuda"), torch.zeros((rows, cols, 3), device="cuda")
        parts = res["parts"] = {} if a.no_step else {"guides": timed(torch, lambda: ds.guides(cams[1], rows, cols), max(3, a.reps // 3))}
        for v in variants:
            mask = None if v is None else dn.sparse_mask(g, v, (0, 0), sigma_p=sp)

            def render():
                sums.zero_()
                sums2.zero_()
                ds.render_rows_masked(cams[0], spp * period, rows, cols, spp, 2 * spp, sums, mask=mask, sums2=sums2, want_avg=False, want_rgb=False)
            parts["render_" + ("dense" if v is None else "sparse_%d" % v)] = timed(torch, render, max(3, a.reps // 3))
    finally:
        torch.cuda.synchronize()
        ds.close()
    text = json.dumps(res)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
