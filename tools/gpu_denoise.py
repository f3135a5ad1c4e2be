"""Times the denoiser (libsquigly_denoise.so) on the GPU at 1920 x 1080 with 5 passes: per stage and per kernel form with device
events (warm, median of repeated runs, spread), the variance kernel, whole calls, and -- as the baseline, in the same process on the
same device -- the same filter written with torch ops.

    python tools/gpu_denoise.py [--rows 1080 --cols 1920 --passes 5 --reps 30 --out FILE.json]

The baseline is not pinned to the bit and is never the code under test; it is what a user without the library would write.  The
inputs are seeded and made on the device: normals from a handful of planes plus noise, points on them, about 30 % background,
heavy-tailed colours, variances with exact zeros.  Prints one JSON object; every time is in milliseconds.  Needs a GPU: there is no
fallback."""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_inputs(torch, rows, cols, seed=1, device="cuda"):
    g = torch.Generator(device=device).manual_seed(seed)
    rnd = lambda *s: torch.rand(*s, generator=g, device=device)            # noqa: E731
    rndn = lambda *s: torch.randn(*s, generator=g, device=device)          # noqa: E731
    n_planes = 6
    base = torch.nn.functional.normalize(rndn(n_planes, 3), dim=-1)
    yy, xx = torch.meshgrid(torch.arange(rows, device=device), torch.arange(cols, device=device), indexing="ij")
    which = ((yy // 97 + xx // 131) % n_planes).long()
    normal = torch.nn.functional.normalize(base[which] + 0.02 * rndn(rows, cols, 3), dim=-1).contiguous()
    u = torch.nn.functional.normalize(torch.cross(base, base.roll(1, 0), dim=-1), dim=-1)
    v = torch.cross(base, u, dim=-1)
    point = (0.003 * xx.float()[..., None] * u[which] + 0.003 * yy.float()[..., None] * v[which] + 0.0005 * rndn(rows, cols, 3)).contiguous()
    # background: coarse blobs (a low-resolution mask blown up) and single pixels
    coarse = (rnd(rows // 16 + 1, cols // 16 + 1) < 0.25).repeat_interleave(16, 0).repeat_interleave(16, 1)[:rows, :cols]
    tri = torch.where(coarse | (rnd(rows, cols) < 0.07), -1, 5).to(torch.int32).contiguous()
    color = (rndn(rows, cols, 3) / rndn(rows, cols, 3).abs().clamp_min(1e-3)).abs() * (rnd(rows, cols, 1) < 0.7)
    var = -torch.log(rnd(rows, cols).clamp_min(1e-6)) * (rnd(rows, cols) < 0.8)
    return color.float().contiguous(), var.float().contiguous(), tri, normal.float(), point.float()


def torch_filter(torch, color, var, tri, normal, point, passes, sigma_l, eps_l, sigma_p, squarings):
    """The filter of include/squigly_denoise.h with torch ops: one rolled copy of every image per tap, masked where it wrapped."""
    rows, cols = tri.shape
    valid = tri >= 0
    yy, xx = torch.meshgrid(torch.arange(rows, device=tri.device), torch.arange(cols, device=tri.device), indexing="ij")
    K, G = (0.375, 0.25, 0.0625), (0.5, 0.25)
    lum = lambda c: 0.25 * c[..., 0] + 0.5 * c[..., 1] + 0.25 * c[..., 2]      # noqa: E731

    def tap(a, oy, ox):
        return torch.roll(a, shifts=(-oy, -ox), dims=(0, 1))

    def usable(oy, ox):
        return (yy + oy >= 0) & (yy + oy < rows) & (xx + ox >= 0) & (xx + ox < cols) & tap(valid, oy, ox)
    C_, V = color, var
    for i in range(passes):
        s = 1 << i
        gs, gw = torch.zeros_like(V), torch.zeros_like(V)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                ok = usable(dy, dx)
                g = G[abs(dy)] * G[abs(dx)]
                gs = torch.where(ok, gs + g * tap(V, dy, dx), gs)
                gw = torch.where(ok, gw + g, gw)
        sd = sigma_l * torch.sqrt(gs / gw) + eps_l
        lp = lum(C_)
        sw, sc, sv = torch.zeros_like(V), torch.zeros_like(C_), torch.zeros_like(V)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                oy, ox = dy * s, dx * s
                ok = usable(oy, ox)
                t = (normal * tap(normal, oy, ox)).sum(-1).clamp_min(0.0)
                for _ in range(squarings):
                    t = t * t
                a = (normal * (tap(point, oy, ox) - point)).sum(-1) / sigma_p
                Cq = tap(C_, oy, ox)
                b = (lum(Cq) - lp) / sd
                w = K[abs(dy)] * K[abs(dx)] * t / (1 + a * a) / (1 + b * b)
                sw = torch.where(ok, sw + w, sw)
                sc = torch.where(ok[..., None], sc + w[..., None] * Cq, sc)
                sv = torch.where(ok, sv + w * w * tap(V, oy, ox), sv)
        take = valid & (sw > 0)
        C_ = torch.where(take[..., None], sc / sw[..., None], C_)
        V = torch.where(take, sv / (sw * sw), V)
    return C_, V


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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1080)
    ap.add_argument("--cols", type=int, default=1920)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--baseline-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/gpu_denoise.py needs a GPU: nothing is measured without one")
    dn = importlib.import_module("squigly-trace_amd.denoise")
    L = dn.lib()
    rows, cols, passes = a.rows, a.cols, a.passes
    color, var, tri, normal, point = make_inputs(torch, rows, cols)
    out, out_var = torch.empty_like(color), torch.empty_like(var)
    need = dn.workspace_bytes(rows, cols)
    work = torch.empty(need, dtype=torch.uint8, device="cuda")
    sigma_p = 0.05
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def args(form):
        P = dn.make_params(sigma_p=sigma_p, passes=passes, form=form)
        return (0, rows, cols, color.data_ptr(), var.data_ptr(), tri.data_ptr(), normal.data_ptr(), point.data_ptr(), C.byref(P),
                out.data_ptr(), out_var.data_ptr(), work.data_ptr(), need, st)
    res = {"rows": rows, "cols": cols, "passes": passes, "pixels": rows * cols, "background": round(float((tri < 0).float().mean()), 3),
           "device": torch.cuda.get_device_name(0), "build_id": dn.build_id(), "workspace_bytes": need,
           "auto_forms": [L.sq_denoise_pass_form(i) for i in range(passes)], "forms": {}}
    dn.check(L.sq_denoise_device(*args(0)))                      # the workspace holds a whole call's records from here on
    torch.cuda.synchronize()
    res["pack"] = timed(torch, lambda: dn.check(L.sq_denoise_stage_device(*args(1), -1)), a.reps)
    for name, form in (("direct", 1), ("tiled", 2)):
        per = []
        for i in range(passes):
            per.append(timed(torch, lambda: dn.check(L.sq_denoise_stage_device(*args(form), i)), a.reps))
        res["forms"][name] = {"pass": per, "call": timed(torch, lambda: dn.check(L.sq_denoise_device(*args(form))), a.reps)}
    res["auto_call"] = timed(torch, lambda: dn.check(L.sq_denoise_device(*args(0))), a.reps)
    sums, sums2 = torch.rand(rows, cols, 3, device="cuda") * 16, torch.rand(rows, cols, 3, device="cuda") * 64
    counts = torch.randint(0, 17, (rows, cols), device="cuda", dtype=torch.int32)
    res["variance"] = timed(torch, lambda: dn.denoise_variance(sums, sums2, counts), a.reps)
    # every form gives the same bits, at the size that is timed
    outs = []
    for form in (1, 2, 0):
        dn.check(L.sq_denoise_device(*args(form)))
        torch.cuda.synchronize()
        outs.append((out.clone(), out_var.clone()))
    res["forms_agree_on_bits"] = all(torch.equal(o[0].view(torch.int32), outs[0][0].view(torch.int32)) and
                                     torch.equal(o[1].view(torch.int32), outs[0][1].view(torch.int32)) for o in outs[1:])
    base = lambda: torch_filter(torch, color, var, tri, normal, point, passes, 4.0, 1e-3, sigma_p, 3)      # noqa: E731
    res["torch_baseline_call"] = timed(torch, base, a.baseline_reps, warm=1)
    b_out, _ = base()
    torch.cuda.synchronize()
    hit = tri >= 0
    d = (b_out - outs[0][0])[hit].abs()
    res["baseline_max_abs_difference"] = float(torch.nan_to_num(d, nan=0.0, posinf=0.0).max())
    text = json.dumps(res)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
