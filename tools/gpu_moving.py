"""Times sq_temporal_accumulate_moving_device (libsquigly_temporal.so) on the GPU at 1920 x 1080, and what a scene that changes every
frame costs around it.  One job, every case interleaved over `--rounds` rounds so that the spread is the job's own:

  calls     the old call, the new call with d_out_flags alone (the moving kernel without a clamp), with tables, with each clamp radius in each kernel form, through the
            C-ABI, ten calls between two device events (warm, median of --reps; the median, least and greatest of the rounds'
            medians), beside a device copy of the call's compulsory bytes; with --parent-lib, the old call of another build of
            the library (the parent commit's) on the same buffers in the same rounds; and two calls through the Python layer, one
            call an event pair, whose checks take longer than the kernel.
  per_frame moved_mesh, the tree's build on the host and on the device, and the upload (DeviceScene) for the moving room
            (tests/moving_room.py) and for the 82k-triangle stand-in (tools/gen_scenes.py: the blob turns about z), in host
            milliseconds with the device drained.
  step      one Temporal.step of the moving room at --spp: the constructor's scene; a scene of its own with the box's move; the
            same under a clamp.

    python tools/gpu_moving.py [--rows 1080 --cols 1920 --spp 16 --reps 20 --rounds 5 --parent-lib FILE.so --out FILE.json]

Prints one JSON object; every time is in milliseconds.  Needs a GPU: there is no fallback."""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import gpu_temporal as GT      # noqa: E402  (make_frame, timed, BYTES_PER_PIXEL)

N_TRIS, N_OBJECTS = 32, 3
BATCH = 10            # calls between two device events


def spread(values):
    return {"median": round(statistics.median(values), 4), "min": round(min(values), 4), "max": round(max(values), 4), "rounds": len(values)}


def call_cases(torch, sqt, tp, a):
    rows, cols, n = a.rows, a.cols, a.rows * a.cols
    G = __import__("collections").namedtuple("G", ["tri", "normal", "point"])
    pos0, pos1 = (0.0, 0.0, 0.0), (0.0, 0.37 * 4.0 / rows, -0.21 * 4.0 / cols)
    prev_frame, cur = GT.make_frame(torch, rows, cols, pos0, 1, "cuda"), GT.make_frame(torch, rows, cols, pos1, 2, "cuda")
    alpha = (torch.rand(rows, cols, device="cuda") * 0.3).contiguous()
    params = dict(sigma_p=0.05, **tp.DEFAULTS)
    prev_cam = sqt.Camera()
    prev_cam.pos[:], prev_cam.rot[:] = pos0, (1, 0, 0, 0, 1, 0, 0, 0, 1)
    blocks = [tp.history(rows, cols, 0), tp.history(rows, cols, 0)]
    g = G(*cur[2:])
    tp.accumulate(prev_frame[0], prev_frame[1], G(*prev_frame[2:]), None, None, blocks[0], **params)
    outs = (torch.empty_like(cur[0]), torch.empty_like(cur[1]), torch.empty((rows, cols), dtype=torch.int32, device="cuda"))
    # the wall (triangle 10) is object 1 and moves by a fraction of a pixel, the strip (20) object 0 and stands still
    objects = torch.full((N_TRIS,), -1, dtype=torch.int32, device="cuda")
    objects[10], objects[20] = 1, 0
    back = torch.tensor([[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], [1, 0, 0, 0, 0, 1, 0, 0.3 * 4.0 / rows, 0, 0, 1, 0], [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]],
                        dtype=torch.float32, device="cuda")
    par, L = tp.make_params(**params), tp.lib()
    flags = torch.empty((rows, cols), dtype=torch.uint8, device="cuda")
    ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)      # noqa: E731
    head = lambda: (0, rows, cols, cur[0].data_ptr(), cur[1].data_ptr(), g.tri.data_ptr(), g.normal.data_ptr(), g.point.data_ptr(),      # noqa: E731
                    alpha.data_ptr(), C.byref(prev_cam), blocks[0].data_ptr(), C.byref(par))
    tail = lambda: (blocks[1].data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr())      # noqa: E731

    def old(lib):
        def call():
            assert lib.sq_temporal_accumulate_device(*head(), *tail(), stream()) == 0
        return call

    def moving(objects=None, back=None, clamp=None, form="auto"):
        cl = None if clamp is None else tp.Clamp(clamp[1], clamp[0])

        def call():
            assert L.sq_temporal_accumulate_moving_device(*head(), ptr(objects), 0 if objects is None else N_TRIS, ptr(back),
                                                          0 if back is None else N_OBJECTS, None if cl is None else C.byref(cl),
                                                          tp.FORMS[form], *tail(), flags.data_ptr(), stream()) == 0
        return call
    # Through the C-ABI, BATCH calls between two device events: a call of a tenth of a millisecond is shorter than the Python
    # layer's checks in front of it, and one call between two events measures the host.
    # (every moving() case gives d_out_flags: with nothing at all given the new call runs the old call's kernel)
    cases = {"old_call": old(L), "new_call_flags_only": moving(), "objects": moving(objects=objects, back=back)}
    for radius in (1, 2, 3):
        for form in ("direct", "tiled"):
            cases[f"clamp_r{radius}_{form}"] = moving(clamp=(1.0, radius), form=form)
    cases["objects_clamp_r1_auto"] = moving(objects=objects, back=back, clamp=(1.0, 1))
    if a.parent_lib:
        parent = C.CDLL(os.path.abspath(a.parent_lib))
        parent.sq_temporal_build_id.restype = C.c_char_p
        parent.sq_temporal_accumulate_device.argtypes = L.sq_temporal_accumulate_device.argtypes
        cases["old_call_parent_build"] = old(parent)
    python_layer = {"python_old_call": lambda: tp.accumulate(cur[0], cur[1], g, prev_cam, blocks[0], blocks[1], alpha=alpha, out=outs, **params),
                    "python_new_call_clamp_r1": lambda: tp.accumulate(cur[0], cur[1], g, prev_cam, blocks[0], blocks[1], alpha=alpha, out=outs,
                                                                      clamp=1.0, want_flags=True, **params)}
    src = torch.empty(GT.BYTES_PER_PIXEL * n // 2, dtype=torch.uint8, device="cuda").fill_(1)
    dst = torch.empty_like(src)
    cases["copy_of_the_old_calls_bytes"] = lambda: dst.copy_(src)
    medians = {name: [] for name in list(cases) + list(python_layer)}
    for _ in range(a.rounds):
        for name, fn in cases.items():
            medians[name].append(GT.timed(torch, lambda: [fn() for _ in range(BATCH)], a.reps)["median"] / BATCH)
        for name, fn in python_layer.items():
            medians[name].append(GT.timed(torch, fn, a.reps)["median"])
    res = {name: spread(v) for name, v in medians.items()}
    res["calls_per_event_pair"] = BATCH
    # the forms agree on these inputs too
    cases["clamp_r3_direct"]()
    ref = [o.clone() for o in outs + (flags,)]
    cases["clamp_r3_tiled"]()
    til = outs + (flags,)
    torch.cuda.synchronize()
    res["forms_agree"] = all(bool((x.view(torch.uint8) == y.view(torch.uint8)).all()) for x, y in zip(ref, til))
    res["clamped_share"] = round(float(((ref[3] & tp.FLAG_CLAMPED) != 0).float().mean()), 4)
    res["blended_share"] = round(float(((ref[3] & tp.FLAG_BLENDED) != 0).float().mean()), 4)
    res["bytes_per_pixel_old_call"] = GT.BYTES_PER_PIXEL
    if a.parent_lib:
        res["parent_build_id"] = parent.sq_temporal_build_id().decode()
    return res


def host_ms(torch, fn, reps):
    """(median, min, max) host milliseconds of fn() with the device drained before and after; its last result."""
    ms, out = [], None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3), "reps": reps}, out


def per_frame(torch, sqt, name, mesh, poses, reps):
    res = {"scene": name, "triangles": len(mesh), "materials": len(mesh.materials)}
    res["moved_mesh"], moved = host_ms(torch, lambda: sqt.moved_mesh(mesh, poses), reps)
    res["bih_host"], bih = host_ms(torch, lambda: sqt.BIH(moved), reps)
    res["bih_device"], _ = host_ms(torch, lambda: sqt.BIH(moved, device=0), reps)

    def upload():
        ds = sqt.DeviceScene(bih, 0)
        torch.cuda.synchronize()
        return ds
    scenes = []
    res["upload"], _ = host_ms(torch, lambda: scenes.append(upload()), reps)
    for ds in scenes:
        ds.close()
    return res


def steps(torch, sqt, tp, a):
    import moving_room as MR
    import numpy as np
    data = os.path.join(ROOT, "data")
    mesh, poses, box = MR.product_mesh(sqt, sqt.Mesh.from_obj(os.path.join(data, "scene.obj"), data))
    cam = sqt.camera_from_text(MR.CAMERA_TEXT)
    scenes = [sqt.DeviceScene(sqt.BIH(sqt.moved_mesh(mesh, poses[f])), 0) for f in range(2)]
    back = torch.from_numpy(tp.back_transforms(poses[0], poses[1])).cuda()
    res, reps = {}, max(3, a.reps // 4)
    try:
        for name, clamp, kw in (("constructors_scene", None, {}), ("scene_and_back", None, dict(scene=scenes[1], back=back)),
                                ("scene_back_and_clamp_r1", 1.0, dict(scene=scenes[1], back=back)),
                                ("scene_back_and_clamp_r3", (1.0, 3), dict(scene=scenes[1], back=back))):
            t = sqt.Temporal(scenes[0], a.rows, a.cols, a.spp, clamp=clamp)
            t.step(cam, scene=scenes[0])
            saved = (t.history.clone(), t.camera, t.frames)

            def one(t=t, kw=kw, saved=saved):
                t._blocks[0].copy_(saved[0])               # every timed step is the second frame of the sequence
                t._cur, t.frames = 0, saved[2]
                return t.step(cam, **kw)
            res[name] = GT.timed(torch, one, reps, warm=2)
            if t.flags is not None:
                res[name]["moved_share"] = round(float(((t.flags & tp.FLAG_MOVED) != 0).float().mean()), 4)
                res[name]["clamped_share"] = round(float(((t.flags & tp.FLAG_CLAMPED) != 0).float().mean()), 4)
        res["history_copy_inside_every_timed_step"] = GT.timed(torch, lambda: t._blocks[0].copy_(saved[0]), reps)
    finally:
        torch.cuda.synchronize()
        for ds in scenes:
            ds.close()
    frame = [per_frame(torch, sqt, "moving room", mesh, poses[1], 5)]
    if not a.no_blob:
        import gen_scenes
        obj, sq, _ = gen_scenes.blob_scene(6)
        blob = sqt.Mesh.from_text(obj, sq)
        turn = np.tile(np.eye(3, 4), (len(blob.materials), 1, 1))
        most = int(np.bincount(blob.tris["mat"]).argmax())
        c, s = np.cos(0.05), np.sin(0.05)
        turn[most, :2, :2] = ((c, -s), (s, c))
        frame.append(per_frame(torch, sqt, "82k-triangle stand-in (blob)", blob, turn, 3))
    return res, frame


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1080)
    ap.add_argument("--cols", type=int, default=1920)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="another build of libsquigly_temporal.so whose old call is timed in the same rounds")
    ap.add_argument("--no-step", action="store_true", help="leave out the Temporal.step and per-frame measurements (no scene is uploaded)")
    ap.add_argument("--no-blob", action="store_true", help="leave out the 82k-triangle stand-in")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/gpu_moving.py needs a GPU: nothing is measured without one")
    sqt = importlib.import_module("squigly-trace_amd")
    tp = importlib.import_module("squigly-trace_amd.temporal")
    res = {"rows": a.rows, "cols": a.cols, "device": torch.cuda.get_device_name(0), "build_id": tp.build_id(), "reps": a.reps}
    res["calls"] = call_cases(torch, sqt, tp, a)
    if not a.no_step:
        res["step"], res["per_frame"] = steps(torch, sqt, tp, a)
    text = json.dumps(res)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
