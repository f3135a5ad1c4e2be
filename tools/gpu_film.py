"""Times the display stage (libsquigly_film.so) on the GPU at 1080 x 1920, every figure between two device events (warm, median of
repeated runs, spread): develop per curve, in its four-pixel form (aligned pointers) and its one-pixel form (d_color one float and
d_rgb one byte into their allocations); histogram in its folding forms -- the product's and the variant builds beside it -- on a
room frame and on a frame whose pixels share one slot; expose; and, in the same job, what the stage stands in for: temporal.tonemap
(torch ops), the debug_eval host round trip, and a device copy of the same 15 bytes a pixel.  Then Temporal.step at 16 spp with
film=None, Film() and Film(auto=...), each measured several times over so that film=None's own run-to-run spread stands beside the
differences.

    python tools/gpu_film.py [--rows 1080 --cols 1920 --spp 16 --reps 30 --out FILE.json]

The variant builds are made with squigly-trace_amd/build.py when they are missing (compile_lib(LIBS["film"], ["-DSQ_FILM_HIST_FOLD=k"], out)).
Prints one JSON object; every time is in milliseconds.  Needs a GPU: there is no fallback."""
import argparse
import ctypes as C
import importlib
import importlib.util
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = os.path.join(ROOT, "squigly-trace_amd")
FOLDS = {0: "plain", 1: "slot 0 by ballot", 2: "the first lane's slot by ballot"}
BYTES_PER_PIXEL = 12 + 3


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


def variant_libs(fm):
    """fold form -> the library built with it: the product's own form is the product, the others are built beside it when missing."""
    spec = importlib.util.spec_from_file_location("sq_build_for_gpu_film", os.path.join(PKG, "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    libs = {}
    for k in FOLDS:
        path = os.path.join(PKG, f"libsquigly_film_fold{k}.so")
        extra = [f"-DSQ_FILM_HIST_FOLD={k}"]
        want = b.lib_source_id(b.LIBS["film"], extra).encode()
        if not os.path.exists(path) or want not in open(path, "rb").read():
            b.compile_lib(b.LIBS["film"], extra, path)
        libs[k] = fm.load(path)
    return libs


def room_frame(torch, sqt, rows, cols, spp):
    data = os.path.join(ROOT, "data")
    bih = sqt.BIH(sqt.Mesh.from_obj(os.path.join(data, "scene.obj"), data))
    ds = sqt.DeviceScene(bih, 0)
    avg, _ = ds.render_rows(sqt.load_camera(os.path.join(data, "camera")), spp, rows, cols, want_rgb=False)
    torch.cuda.synchronize()
    return bih, ds, avg


def offset(torch, t, skip):
    out = torch.empty(t.numel() + skip, dtype=t.dtype, device=t.device)[skip:].view(*t.shape)
    out.copy_(t)
    return out


def steps(torch, sqt, ds, rows, cols, spp, reps, rounds):
    """Temporal.step under three films, `rounds` times over in turn: per film the medians of the rounds."""
    cams = [sqt.camera_from_text(b"%.3f 7 0.75\n1.5707963267948966 0 -0.09817477042468103\n" % (0.01 * i)) for i in range(2)]
    films = {"film=None": lambda: None, "Film()": lambda: sqt.Film(), "Film(auto)": lambda: sqt.Film(curve="filmic", auto=dict(rate=0.25))}
    res = {k: [] for k in films}
    for _ in range(rounds):
        for name, make in films.items():
            t = sqt.Temporal(ds, rows, cols, spp, film=make())
            t.step(cams[0])
            res[name].append(timed(torch, lambda: t.step(cams[1]), reps)["median"])
    base = res["film=None"]
    out = {k: {"medians": v, "median": round(statistics.median(v), 4)} for k, v in res.items()}
    out["spread_of_film=None"] = round(max(base) - min(base), 4)
    for k in ("Film()", "Film(auto)"):
        out[k]["over_film=None"] = round(out[k]["median"] - out["film=None"]["median"], 4)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1080)
    ap.add_argument("--cols", type=int, default=1920)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--step-reps", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-step", action="store_true", help="leave out the Temporal.step measurement")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/gpu_film.py needs a GPU: nothing is measured without one")
    sqt = importlib.import_module("squigly-trace_amd")
    fm = importlib.import_module("squigly-trace_amd.film")
    tp = importlib.import_module("squigly-trace_amd.temporal")
    libs = variant_libs(fm)                                  # built before the GPU is touched
    rows, cols, n = a.rows, a.cols, a.rows * a.cols
    bih, ds, room = room_frame(torch, sqt, rows, cols, 4)
    res = {"rows": rows, "cols": cols, "pixels": n, "device": torch.cuda.get_device_name(0), "bytes_per_pixel": BYTES_PER_PIXEL,
           "build_ids": {"main": sqt.build_id(), "film": fm.build_id(),
                         **{m: importlib.import_module("squigly-trace_amd." + m).build_id() for m in ("denoise", "lens", "mlens", "shutter", "temporal")}}}
    try:
        black = float((room.amax(-1) == 0).float().mean())
        res["room_black_share"] = round(black, 4)
        one_slot = torch.full_like(room, 0.18)
        gbs = lambda ms: round(BYTES_PER_PIXEL * n / (ms * 1e-3) / 1e9, 1)      # noqa: E731
        # develop
        lut = torch.from_numpy(fm.srgb_lut()).cuda()
        rgb = torch.empty(room.shape, dtype=torch.uint8, device="cuda")
        room1, rgb1 = offset(torch, room, 1), offset(torch, rgb, 1)
        assert room.data_ptr() % 16 == 0 and room1.data_ptr() % 16 == 4 and rgb1.data_ptr() % 4 == 1
        res["develop"] = {}
        for curve in fm.CURVES:
            r = {"four_pixels": timed(torch, lambda: fm.develop(room, 1.0, curve, out=rgb), a.reps),
                 "one_pixel": timed(torch, lambda: fm.develop(room1, 1.0, curve, out=rgb1), a.reps)}
            r["four_pixels_gb_per_s"] = gbs(r["four_pixels"]["median"])
            res["develop"][curve] = r
        disp = torch.empty_like(room)
        e = torch.ones(1, device="cuda")
        res["develop"]["filmic + srgb table + dither + device exposure"] = timed(
            torch, lambda: fm.develop(room, e, "filmic", lut=lut, dither=True, out=rgb), a.reps)
        res["develop"]["filmic + display"] = timed(torch, lambda: fm.develop(room, 1.0, "filmic", out=(rgb, disp), want_display=True), a.reps)
        # histogram, every folding form
        hist = torch.empty(fm.SLOTS, dtype=torch.int32, device="cuda")
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        res["histogram"], counts = {}, {}
        for k, L in libs.items():
            r = {}
            for name, img in (("room", room), ("one_slot", one_slot)):
                r[name] = timed(torch, lambda: L.sq_film_histogram_device(0, rows, cols, img.data_ptr(), hist.data_ptr(), st), a.reps)
                counts[(k, name)] = hist.clone()
            res["histogram"][f"fold {k}: {FOLDS[k]}"] = r
        res["histogram"]["product"] = {"room": timed(torch, lambda: fm.histogram(room, out=hist), a.reps),
                                       "one_slot": timed(torch, lambda: fm.histogram(one_slot, out=hist), a.reps)}
        res["histogram_forms_agree"] = all(torch.equal(counts[(0, nm)], counts[(k, nm)]) for k in libs for nm in ("room", "one_slot"))
        fm.histogram(room, out=hist)
        state = torch.zeros(1, device="cuda")
        res["expose"] = timed(torch, lambda: fm.expose(hist, prev=state, out=state, rate=0.25), a.reps)
        res["histogram + expose + develop"] = timed(
            torch, lambda: fm.develop(room, fm.expose(fm.histogram(room, out=hist), prev=state, out=state, rate=0.25), "filmic", out=rgb), a.reps)
        # what it stands in for
        res["temporal.tonemap (torch ops)"] = timed(torch, lambda: tp.tonemap(room), a.reps)
        res["debug_eval host round trip"] = timed(
            torch, lambda: sqt.debug_eval("tonemap", room.cpu().numpy().reshape(-1, 3), device=0), max(3, a.reps // 6), warm=1)
        src = torch.empty(BYTES_PER_PIXEL * n // 2, dtype=torch.uint8, device="cuda").fill_(1)
        dst = torch.empty_like(src)
        res["copy_of_the_same_bytes"] = timed(torch, lambda: dst.copy_(src), a.reps)
        res["copy_gb_per_s"] = gbs(res["copy_of_the_same_bytes"]["median"])
        same = torch.equal(fm.develop(room), tp.tonemap(room))
        res["temporal.tonemap_equals_develop_on_the_room"] = bool(same)
        if not a.no_step:
            res["step"] = steps(torch, sqt, ds, rows, cols, a.spp, a.step_reps, a.rounds)
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
