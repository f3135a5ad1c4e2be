"""Times the temporal accumulation (libsquigly_temporal.so) on the GPU at 1920 x 1080: the accumulate call between two device events
(warm, median of repeated runs, spread) with its achieved bytes per second against a device copy of the same compulsory bytes in the
same job; the same accumulation written with torch ops, as the baseline; and a step of sqt.Temporal at 16 spp on data/scene.obj split
into its parts.

    python tools/gpu_temporal.py [--rows 1080 --cols 1920 --spp 16 --reps 30 --out FILE.json]

The baseline is not pinned to the bit and is never the code under test; it is what a user without the library would write.  The
inputs of the first two measurements are seeded and made on the device: a wall and a strip in front of it seen by two cameras a
fraction of a pixel apart, about 8 % background, heavy-tailed colours.  Prints one JSON object; every time is in milliseconds.  Needs
a GPU: there is no fallback."""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# What one pixel must move, in bytes: the frame's plain images (colour 12, variance 4, triangle 4, normal 12, point 12, alpha 4), a
# record of each plane of the previous block (48; the four taps of neighbouring pixels share them), the next block (48) and the plain
# outputs (colour 12, variance 4, length 4).
BYTES_PER_PIXEL = 48 + 48 + 48 + 20


def make_frame(torch, rows, cols, pos, seed, device):
    """(color, var, tri, normal, point) of the frame a camera at `pos` looking down +x sees of a wall at x = 4 and a strip at x = 2."""
    g = torch.Generator(device=device).manual_seed(seed)
    rnd = lambda *s: torch.rand(*s, generator=g, device=device)            # noqa: E731
    yy, xx = torch.meshgrid(torch.arange(rows, device=device, dtype=torch.float32), torch.arange(cols, device=device, dtype=torch.float32),
                            indexing="ij")
    d = torch.stack([torch.ones_like(xx), (xx - rows / 2) / rows, (cols / 2 - yy) / cols], -1)     # makeRay, src/Lib.hs:107-114
    p = torch.tensor(pos, device=device, dtype=torch.float32)
    far = p + ((4.0 - p[0]) / d[..., :1]) * d
    near = p + ((2.0 - p[0]) / d[..., :1]) * d
    strip = (near[..., 1] >= -0.3) & (near[..., 1] <= 0.1)
    point = torch.where(strip[..., None], near, far)
    point[..., 0] = torch.where(strip, 2.0, 4.0)
    coarse = (rnd(rows // 16 + 1, cols // 16 + 1) < 0.05).repeat_interleave(16, 0).repeat_interleave(16, 1)[:rows, :cols]
    bg = coarse | (rnd(rows, cols) < 0.03)
    tri = torch.where(bg, -1, torch.where(strip, 20, 10)).to(torch.int32).contiguous()
    point = torch.where(bg[..., None], torch.zeros_like(point), point).contiguous()
    normal = torch.where(bg[..., None], torch.zeros_like(point), torch.tensor([-1.0, 0.0, 0.0], device=device)).contiguous()
    color = (torch.randn(rows, cols, 3, generator=g, device=device) / rnd(rows, cols, 3).clamp_min(1e-3)).abs() * (rnd(rows, cols, 1) < 0.8)
    var = -torch.log(rnd(rows, cols).clamp_min(1e-6)) * (rnd(rows, cols) < 0.8)
    return color.float().contiguous(), var.float().contiguous(), tri, normal, point


def torch_accumulate(torch, color, var, tri, normal, point, alpha, prev_pos, prev, alpha_min, max_history, sigma_p, cos_n):
    """The accumulation of include/squigly_temporal.h with torch ops (the previous camera looks down +x: rot is the identity); prev =
    (color, var, len, tri, normal, point) as plain images.  Returns (out, out_var, out_len)."""
    rows, cols = tri.shape
    e = point - torch.tensor(prev_pos, device=tri.device, dtype=torch.float32)
    k0 = e[..., 0]
    fx = e[..., 1] / k0 * rows + rows / 2
    fy = cols / 2 - e[..., 2] / k0 * cols
    ok = (tri >= 0) & (k0 > 0) & (fx >= -1) & (fx < cols) & (fy >= -1) & (fy < rows)
    fx, fy = torch.where(ok, fx, torch.zeros_like(fx)), torch.where(ok, fy, torch.zeros_like(fy))
    x0, y0 = torch.floor(fx), torch.floor(fy)
    tx, ty = fx - x0, fy - y0
    ix, iy = x0.long(), y0.long()
    p_color, p_var, p_len, p_tri, p_normal, p_point = prev
    sw, sc, sv = torch.zeros_like(var), torch.zeros_like(color), torch.zeros_like(var)
    m = torch.full_like(tri, 0x7fffffff, dtype=torch.int64)
    for j in (0, 1):
        for i in (0, 1):
            qy, qx = iy + j, ix + i
            inside = ok & (qy >= 0) & (qy < rows) & (qx >= 0) & (qx < cols)
            q = qy.clamp(0, rows - 1) * cols + qx.clamp(0, cols - 1)
            take = lambda t: t.reshape(rows * cols, -1)[q].reshape(q.shape + t.shape[2:])       # noqa: E731
            acc = inside & (take(p_tri) >= 0)
            bw = (tx if i else 1 - tx) * (ty if j else 1 - ty)
            acc &= (normal * take(p_normal)).sum(-1) >= cos_n
            acc &= (normal * (take(p_point) - point)).sum(-1).abs() <= sigma_p
            sw = torch.where(acc, sw + bw, sw)
            sc = torch.where(acc[..., None], sc + bw[..., None] * take(p_color), sc)
            sv = torch.where(acc, sv + bw * take(p_var), sv)
            m = torch.where(acc, torch.minimum(m, take(p_len).long()), m)
    blend = sw > 0
    hc, hv = sc / sw[..., None], sv / sw
    m1 = torch.where(blend, m + 1, torch.ones_like(m))
    a = torch.maximum(torch.maximum(1.0 / m1.float(), torch.full_like(var, alpha_min)), alpha)
    out = torch.where(blend[..., None], hc + a[..., None] * (color - hc), color)
    out_var = torch.where(blend, (1 - a) ** 2 * hv + a * a * var, var)
    return out, out_var, torch.where(blend, m1.clamp_max(max_history), torch.ones_like(m1)).to(torch.int32)


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


def step_parts(torch, sqt, tp, rows, cols, spp, reps):
    """A Temporal.step on data/scene.obj written out in its parts, each timed on its own with the inputs the part before it left, and
    the whole step."""
    denoise = importlib.import_module("squigly-trace_amd.denoise")
    data = os.path.join(ROOT, "data")
    bih = sqt.BIH(sqt.Mesh.from_obj(os.path.join(data, "scene.obj"), data))
    cams = [sqt.camera_from_text(b"%.3f 7 0.75\n1.5707963267948966 0 -0.09817477042468103\n" % (0.01 * i)) for i in range(2)]
    ds = sqt.DeviceScene(bih, 0)
    res = {}
    try:
        period = 64
        t = sqt.Temporal(ds, rows, cols, spp, period=period)
        t.step(cams[0])
        prev, prev_cam = t.history.clone(), cams[0]
        sums, sums2 = torch.zeros((rows, cols, 3), device="cuda"), torch.zeros((rows, cols, 3), device="cuda")
        counts = torch.full((rows, cols), spp, dtype=torch.int32, device="cuda")
        cam, k0 = cams[1], spp

        def render():
            sums.zero_()
            sums2.zero_()
            ds.render_rows_masked(cam, spp * period, rows, cols, k0, k0 + spp, sums, sums2=sums2, want_avg=False, want_rgb=False)
        res["render"] = timed(torch, render, reps)
        res["variance"] = timed(torch, lambda: denoise.denoise_variance(sums, sums2, counts), reps)
        res["guides"] = timed(torch, lambda: ds.guides(cam, rows, cols), reps)
        noisy, var, g = sums / float(spp), denoise.denoise_variance(sums, sums2, counts), ds.guides(cam, rows, cols)

        def demodulate():
            ok = ((g.tri >= 0) & (g.surf > 0).all(-1))[..., None]
            x = torch.where(ok, (noisy - g.emit) / torch.where(ok, g.surf, torch.ones_like(g.surf)), noisy)
            ls = (0.25 * g.surf[..., 0] + 0.5 * g.surf[..., 1]) + 0.25 * g.surf[..., 2]
            scale = torch.where(ok[..., 0], ls * ls, torch.ones_like(ls))
            return ok, x, var / scale, scale, tp.frame_alpha(ds, g.tri)
        res["demodulate_and_alpha"] = timed(torch, demodulate, reps)
        ok, x, v, scale, alpha = demodulate()
        nxt = tp.history(rows, cols, 0)
        outs = (torch.empty_like(x), torch.empty_like(v), torch.empty((rows, cols), dtype=torch.int32, device="cuda"))
        acc = lambda: tp.accumulate(x, v, g, prev_cam, prev, nxt, alpha=alpha, out=outs, **t.params)      # noqa: E731
        res["accumulate"] = timed(torch, acc, reps)
        out, out_var, length = acc()
        res["remodulate_and_tonemap"] = timed(torch, lambda: (tp.tonemap(torch.where(ok, out * g.surf + g.emit, out)), out_var * scale), reps)
        res["filter_5_passes"] = timed(torch, lambda: denoise.denoise(out, g.tri, g.normal, g.point, var=out_var, sigma_p=t.params["sigma_p"]), reps)
        res["whole_step"] = timed(torch, lambda: t.step(cam), reps)
        torch.cuda.synchronize()
        res["history_2_or_more"] = round(float((length >= 2).float().mean()), 4)
        res["hit"] = round(float((g.tri >= 0).float().mean()), 4)
        res["samples_of_the_sequence"] = spp * period
        res["main_build_id"] = sqt.build_id()
    finally:
        torch.cuda.synchronize()
        ds.close()
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1080)
    ap.add_argument("--cols", type=int, default=1920)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--baseline-reps", type=int, default=5)
    ap.add_argument("--no-step", action="store_true", help="leave out the Temporal.step measurement (no scene is uploaded)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/gpu_temporal.py needs a GPU: nothing is measured without one")
    sqt = importlib.import_module("squigly-trace_amd")
    tp = importlib.import_module("squigly-trace_amd.temporal")
    rows, cols, n = a.rows, a.cols, a.rows * a.cols
    G = __import__("collections").namedtuple("G", ["tri", "normal", "point"])
    pos0, pos1 = (0.0, 0.0, 0.0), (0.0, 0.37 * 4.0 / rows, -0.21 * 4.0 / cols)
    prev_frame, cur = make_frame(torch, rows, cols, pos0, 1, "cuda"), make_frame(torch, rows, cols, pos1, 2, "cuda")
    alpha = (torch.rand(rows, cols, device="cuda") * 0.3).contiguous()
    params = dict(sigma_p=0.05, **tp.DEFAULTS)
    prev_cam = sqt.Camera()
    prev_cam.pos[:], prev_cam.rot[:] = pos0, (1, 0, 0, 0, 1, 0, 0, 0, 1)
    blocks = [tp.history(rows, cols, 0), tp.history(rows, cols, 0)]
    tp.accumulate(prev_frame[0], prev_frame[1], G(*prev_frame[2:]), None, None, blocks[0], **params)
    outs = (torch.empty_like(cur[0]), torch.empty_like(cur[1]), torch.empty((rows, cols), dtype=torch.int32, device="cuda"))
    call = lambda: tp.accumulate(cur[0], cur[1], G(*cur[2:]), prev_cam, blocks[0], blocks[1], alpha=alpha, out=outs, **params)      # noqa: E731
    res = {"rows": rows, "cols": cols, "pixels": n, "device": torch.cuda.get_device_name(0), "build_id": tp.build_id(),
           "history_bytes": tp.history_bytes(rows, cols), "bytes_per_pixel": BYTES_PER_PIXEL}
    res["accumulate"] = timed(torch, call, a.reps)
    res["first_frame"] = timed(torch, lambda: tp.accumulate(cur[0], cur[1], G(*cur[2:]), None, None, blocks[1], alpha=alpha, out=outs, **params), a.reps)
    res["unpack"] = timed(torch, lambda: tp.unpack(blocks[0], rows, cols), a.reps)
    # a device copy that moves the same bytes (it reads and writes each of its own)
    src = torch.empty(BYTES_PER_PIXEL * n // 2, dtype=torch.uint8, device="cuda").fill_(1)
    dst = torch.empty_like(src)
    res["copy_of_the_same_bytes"] = timed(torch, lambda: dst.copy_(src), a.reps)
    gbs = lambda ms: round(BYTES_PER_PIXEL * n / (ms * 1e-3) / 1e9, 1)      # noqa: E731
    res["accumulate_gb_per_s"], res["copy_gb_per_s"] = gbs(res["accumulate"]["median"]), gbs(res["copy_of_the_same_bytes"]["median"])
    got = [o.clone() for o in call()]
    h = tp.unpack(blocks[0], rows, cols)
    base = lambda: torch_accumulate(torch, *cur, alpha, pos0, tuple(h), params["alpha_min"], params["max_history"], params["sigma_p"],      # noqa: E731
                                    params["cos_n"])
    res["torch_baseline_call"] = timed(torch, base, a.baseline_reps, warm=1)
    b = base()
    torch.cuda.synchronize()
    hit = cur[2] >= 0
    res["history_2_or_more"] = round(float((got[2] >= 2).float().mean()), 4)
    res["baseline_lengths_agree"] = round(float((b[2] == got[2]).float().mean()), 6)
    res["baseline_max_abs_difference"] = float(torch.nan_to_num((b[0] - got[0])[hit].abs(), nan=0.0, posinf=0.0).max())
    if not a.no_step:
        res["step"] = step_parts(torch, sqt, tp, rows, cols, a.spp, max(3, a.reps // 3))
    text = json.dumps(res)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
