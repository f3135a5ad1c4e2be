"""Times the glare stage (sq_denoise_glare_device, libsquigly_denoise.so) on the GPU at 1080 x 1920 and 4320 x 7680, every figure between
two device events (warm, median of repeated runs, min and max): the whole call at levels = 5 in its direct, tiled and chosen forms, three
rounds in turn, so that the direct form's own spread stands beside the difference; the same at levels = 1 (bright-and-down and the
composite alone: the forms differ in bright-and-down only) and the coarse levels as the difference of the two; levels = 0; and, in the
same job, what the call stands beside: a device copy of its compulsory bytes (24 B a pixel plus the pyramid's records, written once and
read once) and the same pyramid written in torch ops.  Then Temporal.step at 16 spp and 1080 x 1920 under Film(curve="filmic") with and
without glare=Glare(), three rounds in turn.

    python tools/gpu_glare.py [--reps 30 --rounds 3 --spp 16 --out FILE.json] [--calls-only]

--calls-only runs each form's call a few times and nothing else: the run to put under `rocprofv3 --kernel-trace --stats` for the
per-kernel times (the kernels are sq_gl_down_direct / sq_gl_down_tiled <true: bright-and-down, false: down>, sq_gl_up_add,
sq_gl_composite4 / sq_gl_composite1).  Prints one JSON object; every time is in milliseconds.  Needs a GPU: there is no fallback."""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = ((1080, 1920), (4320, 7680))
LEVELS = 5
FORMS = {"direct": 1, "tiled": 2, "chosen": 0}


def timed(torch, fn, reps, warm=3):
    """(median, min, max) milliseconds of fn() between two device events, after `warm` untimed runs."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4), "reps": reps}


def frame(torch, rows, cols, seed):
    """Radiances over four decades around 1, a third of the pixels black: generated on the device from a seed."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    px = 10.0 ** (torch.rand((rows, cols, 3), generator=g, device="cuda") * 4.0 - 2.0)
    px[torch.rand((rows, cols), generator=g, device="cuda") < 0.33] = 0.0
    return px.contiguous()


def rounds_of(torch, calls, reps, rounds):
    """calls: name -> fn.  `rounds` rounds in turn; per name the rounds' medians, their median, and their spread (max - min)."""
    res = {k: [] for k in calls}
    for _ in range(rounds):
        for name, fn in calls.items():
            res[name].append(timed(torch, fn, reps)["median"])
    return {k: {"medians": v, "median": round(statistics.median(v), 4), "spread": round(max(v) - min(v), 4)} for k, v in res.items()}


def torch_pyramid(torch, px, threshold=1.0, ceiling=16.0, levels=LEVELS, spread=0.5, strength=0.1):
    """The same pyramid in torch ops (a stand-in for the time, not for the bits): bright pass, four-tap separable stride-2 down steps
    over replicate padding, bilinear up steps."""
    F = torch.nn.functional
    L = 0.25 * px[..., 0] + 0.5 * px[..., 1] + 0.25 * px[..., 2]
    s = torch.where(L > threshold, (L.clamp(max=ceiling) - threshold) / L, torch.zeros_like(L))
    b = (s[..., None] * px).nan_to_num(0.0).clamp(0.0, ceiling).permute(2, 0, 1)[None]
    k = torch.tensor([0.125, 0.375, 0.375, 0.125], device=px.device)
    kx, ky = k.view(1, 1, 1, 4).repeat(3, 1, 1, 1), k.view(1, 1, 4, 1).repeat(3, 1, 1, 1)
    Bs = []
    for _ in range(levels):
        r, c = b.shape[-2:]
        b = F.pad(b, (1, 2 + (c & 1), 1, 2 + (r & 1)), mode="replicate")
        b = F.conv2d(F.conv2d(b, kx, stride=(1, 2), groups=3), ky, stride=(2, 1), groups=3)[..., :(r + 1) // 2, :(c + 1) // 2]
        Bs.append(b)
    a = Bs[-1]
    for lvl in range(levels - 2, -1, -1):
        a = Bs[lvl] + spread * F.interpolate(a, size=Bs[lvl].shape[-2:], mode="bilinear", align_corners=False)
    return px + strength * F.interpolate(a, size=px.shape[:2], mode="bilinear", align_corners=False)[0].permute(1, 2, 0)


def steps(torch, sqt, rows, cols, spp, reps, rounds):
    """Temporal.step under Film(curve="filmic") and the same film with glare=Glare(), `rounds` rounds in turn."""
    data = os.path.join(ROOT, "data")
    ds = sqt.DeviceScene(sqt.BIH(sqt.Mesh.from_obj(os.path.join(data, "scene.obj"), data)), 0)
    try:
        cams = [sqt.camera_from_text(b"%.3f 7 0.75\n1.5707963267948966 0 -0.09817477042468103\n" % (0.01 * i)) for i in range(2)]
        films = {"film": lambda: sqt.Film(curve="filmic"), "film + glare": lambda: sqt.Film(curve="filmic", glare=sqt.Glare())}
        res = {k: [] for k in films}
        for _ in range(rounds):
            for name, make in films.items():
                t = sqt.Temporal(ds, rows, cols, spp, film=make())
                t.step(cams[0])
                res[name].append(timed(torch, lambda: t.step(cams[1]), reps)["median"])
        out = {k: {"medians": v, "median": round(statistics.median(v), 4)} for k, v in res.items()}
        out["spread_of_film"] = round(max(res["film"]) - min(res["film"]), 4)
        out["glare_over_film"] = round(out["film + glare"]["median"] - out["film"]["median"], 4)
        return out
    finally:
        torch.cuda.synchronize()
        ds.close()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--step-reps", type=int, default=7)
    ap.add_argument("--no-step", action="store_true", help="leave out the Temporal.step measurement")
    ap.add_argument("--calls-only", action="store_true", help="run every form's call five times and nothing else (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/gpu_glare.py needs a GPU: nothing is measured without one")
    sqt = importlib.import_module("squigly-trace_amd")
    dn = importlib.import_module("squigly-trace_amd.denoise")
    fm = importlib.import_module("squigly-trace_amd.film")
    res = {"device": torch.cuda.get_device_name(0), "levels": LEVELS, "build_ids": {"denoise": dn.build_id(), "film": fm.build_id(), "main": sqt.build_id()},
           "sizes": {}}
    for rows, cols in SIZES:
        n = rows * cols
        px = frame(torch, rows, cols, rows)
        out = torch.empty_like(px)
        need = dn.glare_work_bytes(rows, cols, LEVELS)
        work = torch.empty(need, dtype=torch.uint8, device="cuda")
        e = torch.ones(1, device="cuda")
        call = lambda levels, form: (lambda: dn.glare(px, exposure=e, gain=(1.1, 1.0, 0.9), levels=levels, form=form, out=out, work=work))   # noqa: E731
        if a.calls_only:
            for _ in range(5):
                for form in (1, 2):
                    call(LEVELS, form)()
            torch.cuda.synchronize()
            continue
        r = {"pixels": n, "work_bytes": need}
        r["levels=5"] = rounds_of(torch, {k: call(LEVELS, f) for k, f in FORMS.items()}, a.reps, a.rounds)
        r["levels=1"] = rounds_of(torch, {k: call(1, f) for k, f in FORMS.items() if f}, a.reps, a.rounds)
        r["coarse levels (levels=5 - levels=1)"] = {k: round(r["levels=5"][k]["median"] - r["levels=1"][k]["median"], 4) for k in ("direct", "tiled")}
        r["levels=0"] = timed(torch, call(0, 0), a.reps)
        ref = dn.glare(px, exposure=e, levels=LEVELS, form=1)
        r["forms_agree"] = bool(torch.equal(ref.view(torch.int32), dn.glare(px, exposure=e, levels=LEVELS, form=2).view(torch.int32)))
        moved = 24 * n + 2 * need                                # colour in, result out, every record written once and read once
        src = torch.empty(moved // 2, dtype=torch.uint8, device="cuda").fill_(1)
        dst = torch.empty_like(src)
        r["compulsory_bytes"] = moved
        r["copy_of_the_same_bytes"] = timed(torch, lambda: dst.copy_(src), a.reps)
        r["copy_gb_per_s"] = round(moved / (r["copy_of_the_same_bytes"]["median"] * 1e-3) / 1e9, 1)
        r["call_gb_per_s"] = {k: round(moved / (r["levels=5"][k]["median"] * 1e-3) / 1e9, 1) for k in FORMS}
        del src, dst
        r["torch_ops_pyramid"] = timed(torch, lambda: torch_pyramid(torch, px), max(3, a.reps // 3))
        res["sizes"][f"{rows}x{cols}"] = r
        del px, out, work
        torch.cuda.empty_cache()
    if not a.calls_only and not a.no_step:
        res["step"] = steps(torch, sqt, SIZES[0][0], SIZES[0][1], a.spp, a.step_reps, a.rounds)
    text = json.dumps(res)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
