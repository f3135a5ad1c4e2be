"""The rig of tests/test_gpu_streams.py, which the depth and sky tests drive too.  Belongs here: the gate, the jobs (one per family
of stream-taking entry points), the forms they run under and the comparison of their results; no test.

The stream promise of include/squigly_hip.h -- "the call only enqueues work on hip_stream" -- held on a stream where it can fail:
a non-blocking side stream (torch.cuda.Stream()) with work pending in front of the call.  On the null stream, where every other GPU
test runs, a launch on the wrong stream, a missing event edge to the scene's internal stream, an unordered fill of the generator-word
table and a host buffer read after the call returned all give the bit-exact frame.

The rig (one process, at most three user streams besides the scene's internal one):

  gate       a bounded delay (torch.cuda._sleep, calibrated once per module with two events) enqueued on the side stream before
             anything else.  It is sized per case to at least 20 x the measured host time of the warm call, and at least 100 ms.
             Right after every library call `side.query() is False`, and the host clock reads less than 0.8 gate lengths since the
             gate was enqueued: the gate was still closed while the call enqueued, and a warm call does not block the host.
  poison in  every device input of the call is pre-filled with poison (NaN, -1, an all-zero mask) and synchronised; its true
             contents arrive only behind the gate, on the side stream.  A piece of the call that runs anywhere but behind the side
             stream's earlier work reads poison.
  poison out every output is filled with a second poison on the side stream, behind the gate and before the call: a memset or a
             store that the library issues early is overwritten.
  consumer   behind the call, on the side stream, every output is copied away and then poisoned again; the copy is compared.
  host       every host argument (sq_camera, the camera array of a views call, the lights table) is overwritten as soon as the
             call returns, with the gate still closed.
  control    the same intersect query issued on the null stream while its inputs are gated on the side stream must NOT give the
             expected result: this proves on the machine at hand that a gate on the side stream holds back that stream only (two
             HIP streams can share a hardware queue, which would make the rig blind).

What the rig sees: work that runs TOO EARLY (on another stream, or before an edge that is missing) is caught deterministically --
the gate is still closed when it runs, `side.query() is False` right after every call shows that.  Work that runs TOO LATE (a tail
that is not joined back into the caller's stream) is caught only with some likelihood: the consumer races with it.

Expected values come from the same call on the null stream with plain synchronisation, which the other GPU modules tie bit for bit
to the oracle; the 64 x 64 frames are compared with tests/golden as well, and the ray queries with the oracle's intersectBIH.  All
comparisons are on bits (any two NaNs are equal)."""
import ctypes as C
import os
import time

import numpy as np

import render_options as RO
from bitcmp import bits, same as same_f32
from conftest import DATA, GOLDEN
from ray_oracle import check_hits, family_free, family_surface, oracle_hits
from scenes import ROTATED

f32 = np.float32

# Every declaration of include/squigly_hip.h with a `void* hip_stream` parameter (tests/test_streams.py keeps the list complete).
STREAM_ENTRY_POINTS = (
    "sq_render_rows_device",
    "sq_render_rows_device_range",
    "sq_render_rows_device_masked",
    "sq_adaptive_update_device",
    "sq_render_views_device",
    "sq_intersect_rays_device",
    "sq_camera_rays_device",
    "sq_raytrace_rays_device",
    "sq_raycast_rays_device",
    "sq_scene_set_lights",
)

# (w rows, h columns, samples, shard)
FRAMES = ((64, 64, 4, (None, 0, 1)), (40, 72, 3, (2, 1, 3)))
GROWN = (96, 96, 4, (None, 0, 1))                    # a larger shape: the table of generator words grows
N_VIEWS, N_RAYS = 3, 4096
THIRD = b"0.5 6 1\n1.4 0.15 0.2\n"
# a third light between two makes the order of the fold visible (tests/test_gpu_lights.py)
LIGHTS_A = np.array([[0, 0, 0, 1.5, 0.5, 0.25], [100, 100, 100, 50, 80, 20], [0, 3, -1, 2, 2, 2]], f32)
LIGHTS_B = np.array([[0, 3, -1, 2, 2, 2], [100, 100, 100, 50, 80, 20], [0, 0, 0, 1.5, 0.5, 0.25]], f32)
SMALL_SLOTS = 2 * 4096                               # two tracks of one sample of the largest call: several batches in flight
FORMS = {"default": {}, "overlap1": {"overlap": 1}, "overlap2": {"overlap": 2}, "variant1": {"variant": 1}, "resident0": {"resident": 0},
         "cast_wavefront": {"cast_wavefront": 1}}
FRAME_FORMS = ("default", "overlap1", "overlap2", "variant1", "resident0")
RAY_FORMS = ("default", "variant1", "overlap2")
# the cast computations: "overlap" is ignored by them today, which is a fact about launch_frame and not a promise, so they run under
# every form of their shape, and under cast_wavefront in addition
CAST_FRAME_FORMS = FRAME_FORMS + ("cast_wavefront",)
CAST_RAY_FORMS = RAY_FORMS + ("cast_wavefront",)
# entry point -> ((job, the forms it runs under), ...): job_<name> below drives the entry point
CASES = {
    "sq_render_rows_device": (("frames", FRAME_FORMS), ("cast_frames", CAST_FRAME_FORMS)),
    "sq_render_rows_device_range": (("range", FRAME_FORMS),),
    "sq_render_rows_device_masked": (("masked", FRAME_FORMS),),
    "sq_adaptive_update_device": (("adaptive_update", ("default",)),),
    "sq_render_views_device": (("views", FRAME_FORMS),),
    "sq_intersect_rays_device": (("intersect", RAY_FORMS),),
    "sq_camera_rays_device": (("camera_rays", RAY_FORMS),),
    "sq_raytrace_rays_device": (("raytrace", RAY_FORMS),),
    "sq_raycast_rays_device": (("raycast", CAST_RAY_FORMS),),
    "sq_scene_set_lights": (("lights", CAST_FRAME_FORMS),),
}
PARAMS = [(ep, job, form) for ep in STREAM_ENTRY_POINTS for job, forms in CASES[ep] for form in forms]
MIN_GATE_MS, GATE_FACTOR, MAX_GATE_MS = 100.0, 20.0, 3000.0
GATE_MARGIN = 0.8                                    # a call has returned within this share of the gate's length, by the host clock
HIP_STREAM_NON_BLOCKING = 0x01
# the second poison, by dtype name; tri = -1 is a result (a miss), so the integer poison is not -1
POISON_OUT = {"float32": -777.0, "int32": 0x5A5A5A5A, "uint8": 0xA5, "int64": 0x5A5A5A5A5A5A5A5A}


def same_result(a, b):
    """Two results of one type and shape: float32 on bits with NaN = NaN (bitcmp.same), anything else exactly."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return same_f32(a, b) if a.dtype == f32 else bool(np.array_equal(a, b))


def scrub(h):
    """Overwrites a host argument: floats become NaN, integers -1."""
    if isinstance(h, np.ndarray):
        h.fill(np.nan if h.dtype.kind == "f" else -1)
    else:
        C.memset(C.addressof(h), 0xFF, C.sizeof(h))


class Recorder:
    """The library, remembering which functions were looked up: a job has to call the entry point it stands for."""

    def __init__(self, lib):
        self._lib, self.names = lib, []

    def __getattr__(self, name):
        self.names.append(name)
        return getattr(self._lib, name)


class Env:
    """The module's scenes, streams, rays and the calibrated gate."""

    def __init__(self, sqt, torch, O, bih, ob):
        self.sqt, self.torch, self.O, self.bih, self.ob = sqt, torch, O, bih, ob
        self.dev = torch.device("cuda", 0)
        self.L = Recorder(sqt.lib())
        self.cam_text = open(os.path.join(DATA, "camera"), "rb").read()
        self.ds = sqt.DeviceScene(bih, 0)
        self.ds_small = sqt.DeviceScene(bih, 0)         # its workspace never holds more than SMALL_SLOTS: the overlapped forms batch
        rng = np.random.default_rng(11)
        _, limits = bih.cull_boxes()
        fo, fd = family_free(rng, bih.bounds, N_RAYS // 2)
        so, sd = family_surface(rng, bih.tris, limits, N_RAYS // 2)
        self.rays = (np.ascontiguousarray(np.concatenate([fo, so]), f32), np.ascontiguousarray(np.concatenate([fd, sd]), f32))
        self.ray_seeds = (np.arange(N_RAYS, dtype=np.int64) * 7919 + 5) * 4
        self.oracle = None
        self._calibrate()
        self.streams = [torch.cuda.Stream(device=self.dev) for _ in range(3)]
        self.side, self.side2 = self.streams[0], self.streams[1]

    # -- the gate ---------------------------------------------------------------------------------------------------------
    def _timed(self, fn):
        torch = self.torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def _calibrate(self):
        """cycles of torch.cuda._sleep per millisecond, from two timed sleeps (the second about 20 ms long); a chain of large
        elementwise operations stands in when _sleep does not delay the device."""
        torch = self.torch
        self.sleep_cycles_per_ms, self.chain, self.chain_ms = None, None, None
        sleep = getattr(torch.cuda, "_sleep", None)
        if sleep is not None:
            sleep(1000)
            torch.cuda.synchronize()
            probe = 2_000_000
            ms = self._timed(lambda: sleep(probe))
            if ms >= 0.2:
                probe = int(probe * 20.0 / ms)
                ms = self._timed(lambda: sleep(probe))
                self.sleep_cycles_per_ms = probe / ms
        if self.sleep_cycles_per_ms is None:
            self.chain = torch.zeros(64 << 20, dtype=torch.float32, device=self.dev)
            self.chain.add_(1.0)
            torch.cuda.synchronize()
            self.chain_ms = self._timed(lambda: [self.chain.add_(1.0) for _ in range(16)]) / 16
        print(f"[streams] gate calibration: {'_sleep, %.0f cycles per ms' % self.sleep_cycles_per_ms if self.chain is None else 'elementwise chain, %.3f ms per link' % self.chain_ms}")

    def gate(self, stream, ms):
        """Enqueues a delay of about `ms` milliseconds on `stream`; bounded, nothing waits for anything."""
        assert 0 < ms <= MAX_GATE_MS, ms
        with self.torch.cuda.stream(stream):
            if self.chain is None:
                self.torch.cuda._sleep(int(ms * self.sleep_cycles_per_ms))
            else:
                for _ in range(int(ms / self.chain_ms) + 1):
                    self.chain.add_(1.0)

    def new_cam(self, text=None):
        return self.sqt.camera_from_text(self.cam_text if text is None else text)

    def shard(self, w, shard):
        rb, si, ns = shard
        sh = self.sqt.Shard(w if rb is None else rb, si, ns)
        return sh, self.L._lib.sq_shard_rows(w, sh)

    def scene_for(self, form):
        return self.ds_small if form.startswith("overlap") else self.ds

    def set_options(self, ds, **opts):
        RO.set_options(ds, RO.CAST, **{**({"slots": SMALL_SLOTS} if ds is self.ds_small else {}), **opts})

    def oracle_hits(self):
        if self.oracle is None:
            self.oracle = oracle_hits(self.ob, *self.rays)
        return self.oracle

    def close(self):
        self.torch.cuda.synchronize()
        self.ds.close()
        self.ds_small.close()


# ---- the rig --------------------------------------------------------------------------------------------------------
# A job is (bufs, steps).  bufs: (name, role, value) with role "in" (a device input: value = its true contents), "inout" (an input
# that the call also writes) or "out" (value = (shape, dtype)).  steps: callables (B, stream pointer, called) that enqueue one or
# more library calls on the buffers B and report every call with called(*host arguments).
def _np_dtype(torch, t):
    return str(t.dtype).replace("torch.", "")


def _poison_in(torch, t, name):
    if t.dtype == torch.float32:
        t.fill_(float("nan"))
    elif t.dtype == torch.uint8:
        t.fill_(0 if "mask" in name else 0x5A)
    else:
        t.fill_(-1)


def _poison_out(torch, t):
    t.fill_(POISON_OUT[_np_dtype(torch, t)])


def _alloc(env, value):
    torch = env.torch
    if isinstance(value, np.ndarray):
        return torch.empty(value.shape, dtype=getattr(torch, str(value.dtype)), device=env.dev)
    shape, dtype = value
    return torch.empty(shape, dtype=getattr(torch, np.dtype(dtype).name), device=env.dev)


def plain(env, job):
    """The job on the null stream with plain synchronisation: ({name: numpy} of its outputs, host milliseconds of its calls)."""
    torch = env.torch
    bufs, steps = job
    B = {}
    for name, role, value in bufs:
        B[name] = _alloc(env, value)
        if role == "out":
            _poison_out(torch, B[name])
        else:
            B[name].copy_(torch.from_numpy(value))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for step in steps:
        step(B, None, lambda *host, waits=None: [scrub(h) for h in host])
    host_ms = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    return {name: B[name].cpu().numpy() for name, role, _ in bufs if role != "in"}, host_ms


class Gated:
    """A job's buffers on a side stream: poisoned before the gate, filled behind it, snapshotted behind the calls."""

    def __init__(self, env, job, side, label):
        torch = env.torch
        self.env, self.side, self.label = env, side, label
        self.bufs, self.steps = job
        self.B, self.src, self.snap = {}, {}, {}
        for name, role, value in self.bufs:
            t = self.B[name] = _alloc(env, value)
            _poison_in(torch, t, name)
            if role != "out":
                self.src[name] = torch.from_numpy(value).to(env.dev)
            if role != "in":
                self.snap[name] = torch.empty_like(t)
        self.sp = C.c_void_p(side.cuda_stream)
        self.calls = 0

    def arm(self, gate_ms):
        """The gate, then -- behind it -- the true inputs and the poison of the outputs.  Call after a device synchronise."""
        torch = self.env.torch
        self.gate_ms, self.t_gate = gate_ms, time.perf_counter()     # the gate cannot open before t_gate + gate_ms
        self.env.gate(self.side, gate_ms)
        with torch.cuda.stream(self.side):
            for name, role, _ in self.bufs:
                if role == "out":
                    _poison_out(torch, self.B[name])
                else:
                    self.B[name].copy_(self.src[name])

    def called(self, *host, waits=None):
        """After every library call: the gate is still closed (unless the call waits by design: waits = the reason), and the host
        arguments are overwritten."""
        self.calls += 1
        pending = self.side.query() is False
        host_ms = (time.perf_counter() - self.t_gate) * 1e3
        if waits is None:
            assert pending, f"{self.label}: the side stream was idle after call {self.calls}: the call blocked the host, or the gate was too short"
            # pending alone could be the call's own kernels; the host clock shows that the gate itself cannot have opened yet
            assert host_ms < GATE_MARGIN * self.gate_ms, f"{self.label}: {host_ms:.1f} ms of host time since the {self.gate_ms:.0f} ms gate was enqueued"
        else:
            print(f"[streams] {self.label}: call {self.calls} may wait ({waits}); the side stream still has work after it: {pending}; "
                  f"{host_ms:.1f} ms of host time since the {self.gate_ms:.0f} ms gate was enqueued")
        for h in host:
            scrub(h)

    def run(self, which=None):
        for i, step in enumerate(self.steps):
            if which is None or i in which:
                step(self.B, self.sp, self.called)

    def finish(self):
        torch = self.env.torch
        with torch.cuda.stream(self.side):
            for name, t in self.snap.items():
                t.copy_(self.B[name])
                _poison_out(torch, self.B[name])

    def results(self):
        return {name: t.cpu().numpy() for name, t in self.snap.items()}


def gate_ms_for(host_ms):
    return min(MAX_GATE_MS, max(MIN_GATE_MS, GATE_FACTOR * host_ms))


def assert_results(got, want, label):
    assert set(got) == set(want)
    for name in want:
        assert same_result(got[name], want[name]), (label, name, int((bits(got[name]) != bits(want[name])).sum()), got[name].reshape(-1)[:6])


def expected_of(env, job, label):
    """The job's null-stream results (twice: the second, warm run is timed and must repeat the first) and the gate for it."""
    want, _ = plain(env, job)
    again, host_ms = plain(env, job)
    assert_results(again, want, label + " (null stream, repeated)")
    gate_ms = gate_ms_for(host_ms)
    print(f"[streams] {label}: warm host time {host_ms:.3f} ms, gate {gate_ms:.0f} ms")
    return want, gate_ms


def drive(env, job, side, label):
    """The whole rig for one job: expected values, then the gated run on `side`; returns the expected values."""
    torch = env.torch
    want, gate_ms = expected_of(env, job, label)
    g = Gated(env, job, side, label)
    torch.cuda.synchronize()
    del env.L.names[:]                                           # what the gated run itself calls, not the null-stream runs before it
    g.arm(gate_ms)
    g.run()
    g.finish()
    torch.cuda.synchronize()
    assert g.calls >= 1
    assert_results(g.results(), want, label)
    return want


# ---- jobs -----------------------------------------------------------------------------------------------------------
def _ok(env, rc):
    env.sqt._native.check(rc)


def _p(t):
    return t.data_ptr()


def job_frames(env, ds, frames=FRAMES, cam_text=None, cast=0, tag=""):
    bufs, steps = [], []
    for i, (w, h, spp, shard) in enumerate(frames):
        sh, rows = env.shard(w, shard)
        a, r = f"{tag}avg{i}", f"{tag}rgb{i}"
        bufs += [(a, "out", ((rows, h, 3), f32)), (r, "out", ((rows, h, 3), np.uint8))]

        def step(B, sp, called, w=w, h=h, spp=spp, sh=sh, a=a, r=r):
            cam = env.new_cam(cam_text)
            _ok(env, env.L.sq_render_rows_device(ds._h, C.byref(cam), spp, w, h, cast, sh, _p(B[a]), _p(B[r]), sp))
            called(cam)
        steps.append(step)
    return bufs, steps


def job_cast_frames(env, ds, **kw):
    return job_frames(env, ds, cast=1, **kw)


def job_range(env, ds, tag=""):
    """Per frame: [0, 2) and [2, samples) on one fold, and [2, samples) on a fold that arrives behind the gate."""
    torch = env.torch
    bufs, steps = [], []
    for i, (w, h, spp, shard) in enumerate(FRAMES):
        sh, rows = env.shard(w, shard)
        mid = torch.empty((rows, h, 3), dtype=torch.float32, device=env.dev)
        cam = env.new_cam()
        _ok(env, env.L.sq_render_rows_device_range(ds._h, C.byref(cam), spp, w, h, 0, sh, 0, 2, _p(mid), None, None, None))
        torch.cuda.synchronize()
        shape = (rows, h, 3)
        n = [f"{tag}{k}{i}" for k in ("sum", "carry", "avgA", "rgbA", "avgB", "rgbB")]
        bufs += [(n[0], "out", (shape, f32)), (n[1], "inout", mid.cpu().numpy()), (n[2], "out", (shape, f32)), (n[3], "out", (shape, np.uint8)),
                 (n[4], "out", (shape, f32)), (n[5], "out", (shape, np.uint8))]

        def step(B, sp, called, w=w, h=h, spp=spp, sh=sh, n=n):
            for k0, k1, s, a, r in ((0, 2, n[0], n[2], n[3]), (2, spp, n[0], n[2], n[3]), (2, spp, n[1], n[4], n[5])):
                cam = env.new_cam()
                _ok(env, env.L.sq_render_rows_device_range(ds._h, C.byref(cam), spp, w, h, 0, sh, k0, k1, _p(B[s]), _p(B[a]), _p(B[r]), sp))
                called(cam)
        steps.append(step)
    return bufs, steps


def job_masked(env, ds, tag=""):
    """Per frame: [0, 2) and [2, samples) for the pixels of a checkerboard that arrives behind the gate; the dead pixels keep what
    the five buffers hold."""
    bufs, steps = [], []
    for i, (w, h, spp, shard) in enumerate(FRAMES):
        sh, rows = env.shard(w, shard)
        y, x = np.indices((rows, h))
        n = [f"{tag}{k}{i}" for k in ("mask", "sums", "sums2", "counts", "avg", "rgb")]
        bufs += [(n[0], "in", ((y + x) & 1).astype(np.uint8)), (n[1], "inout", np.full((rows, h, 3), 7.25, f32)),
                 (n[2], "inout", np.full((rows, h, 3), 5.5, f32)), (n[3], "inout", np.full((rows, h), 77, np.int32)),
                 (n[4], "out", ((rows, h, 3), f32)), (n[5], "out", ((rows, h, 3), np.uint8))]

        def step(B, sp, called, w=w, h=h, spp=spp, sh=sh, n=n):
            for k0, k1 in ((0, 2), (2, spp)):
                cam = env.new_cam()
                _ok(env, env.L.sq_render_rows_device_masked(ds._h, C.byref(cam), spp, w, h, 0, sh, k0, k1, *(_p(B[k]) for k in n), sp))
                called(cam)
        steps.append(step)
    return bufs, steps


ADAPTIVE_TOL, ADAPTIVE_EPS = 0.1, 1.0


def job_adaptive_update(env, ds, tag=""):
    """The stopping rule on the moments of the 64 x 64 frame; sums, sums2, counts and the mask arrive behind the gate."""
    torch = env.torch
    w, h, spp, shard = FRAMES[0]
    sh, rows = env.shard(w, shard)
    s, q = (torch.empty((rows, h, 3), dtype=torch.float32, device=env.dev) for _ in range(2))
    c = torch.zeros((rows, h), dtype=torch.int32, device=env.dev)
    cam = env.new_cam()
    _ok(env, env.L.sq_render_rows_device_masked(ds._h, C.byref(cam), spp, w, h, 0, sh, 0, spp, None, _p(s), _p(q), _p(c), None, None, None))
    torch.cuda.synchronize()
    n = [tag + k for k in ("sums", "sums2", "counts", "mask", "live")]
    bufs = [(n[0], "in", s.cpu().numpy()), (n[1], "in", q.cpu().numpy()), (n[2], "in", c.cpu().numpy()),
            (n[3], "inout", np.ones((rows, h), np.uint8)), (n[4], "out", ((1,), np.int32))]

    def step(B, sp, called):
        _ok(env, env.L.sq_adaptive_update_device(ds._h, rows * h, _p(B[n[0]]), _p(B[n[1]]), _p(B[n[2]]), ADAPTIVE_TOL, ADAPTIVE_EPS,
                                                 _p(B[n[3]]), _p(B[n[4]]), sp))
        called()                                   # through the C-ABI the call does not wait (DeviceScene.adaptive_update does, by design)
    return bufs, [step]


def job_views(env, ds, tag=""):
    w, h, spp, shard = FRAMES[1]
    sh, rows = env.shard(w, shard)
    shape = (N_VIEWS, rows, h, 3)
    n = [tag + k for k in ("vsum", "vavg", "vrgb")]
    bufs = [(n[0], "out", (shape, f32)), (n[1], "out", (shape, f32)), (n[2], "out", (shape, np.uint8))]

    def step(B, sp, called):
        table = (env.sqt.Camera * N_VIEWS)(env.new_cam(), env.new_cam(ROTATED), env.new_cam(THIRD))
        _ok(env, env.L.sq_render_views_device(ds._h, table, N_VIEWS, spp, w, h, 0, sh, 0, spp, _p(B[n[0]]), _p(B[n[1]]), _p(B[n[2]]), sp))
        called(table)
    return bufs, [step]


def _ray_inputs(env, tag):
    return [(tag + "org", "in", env.rays[0]), (tag + "dir", "in", env.rays[1])]


def job_intersect(env, ds, tag=""):
    bufs = _ray_inputs(env, tag) + [(tag + "tri", "out", ((N_RAYS,), np.int32)), (tag + "dist", "out", ((N_RAYS,), f32)),
                                    (tag + "point", "out", ((N_RAYS, 3), f32))]

    def step(B, sp, called):
        _ok(env, env.L.sq_intersect_rays_device(ds._h, _p(B[tag + "org"]), _p(B[tag + "dir"]), N_RAYS, _p(B[tag + "tri"]), _p(B[tag + "dist"]),
                                                _p(B[tag + "point"]), sp))
        called()
    return bufs, [step]


def job_camera_rays(env, ds, tag=""):
    """The primary rays of a shard, then their intersect, with no host wait in between."""
    w, h, _, shard = FRAMES[1]
    sh, rows = env.shard(w, shard)
    n = [tag + k for k in ("corg", "cdir", "ctri", "cdist", "cpoint")]
    bufs = [(n[0], "out", ((rows, h, 3), f32)), (n[1], "out", ((rows, h, 3), f32)), (n[2], "out", ((rows, h), np.int32)),
            (n[3], "out", ((rows, h), f32)), (n[4], "out", ((rows, h, 3), f32))]

    def step(B, sp, called):
        cam = env.new_cam(ROTATED)
        _ok(env, env.L.sq_camera_rays_device(ds._h, C.byref(cam), w, h, sh, _p(B[n[0]]), _p(B[n[1]]), sp))
        called(cam)
        _ok(env, env.L.sq_intersect_rays_device(ds._h, _p(B[n[0]]), _p(B[n[1]]), rows * h, _p(B[n[2]]), _p(B[n[3]]), _p(B[n[4]]), sp))
        called()
    return bufs, [step]


def job_raytrace(env, ds, tag=""):
    """One call [0, 4), and the same fold in two calls [0, 2) [2, 4)."""
    spp = 4
    n = [tag + k for k in ("org", "dir", "seed", "rsum", "ravg", "rrgb", "rsum2", "ravg2", "rrgb2")]
    bufs = _ray_inputs(env, tag) + [(n[2], "in", env.ray_seeds)]
    for k in (3, 6):
        bufs += [(n[k], "out", ((N_RAYS, 3), f32)), (n[k + 1], "out", ((N_RAYS, 3), f32)), (n[k + 2], "out", ((N_RAYS, 3), np.uint8))]

    def step(B, sp, called):
        for k0, k1, k in ((0, spp, 3), (0, 2, 6), (2, spp, 6)):
            _ok(env, env.L.sq_raytrace_rays_device(ds._h, _p(B[n[0]]), _p(B[n[1]]), _p(B[n[2]]), N_RAYS, k0, k1, _p(B[n[k]]), _p(B[n[k + 1]]),
                                                   _p(B[n[k + 2]]), sp))
            called()
    return bufs, [step]


def job_raycast(env, ds, tag=""):
    bufs = _ray_inputs(env, tag) + [(tag + "rad", "out", ((N_RAYS, 3), f32))]

    def step(B, sp, called):
        _ok(env, env.L.sq_raycast_rays_device(ds._h, _p(B[tag + "org"]), _p(B[tag + "dir"]), N_RAYS, _p(B[tag + "rad"]), sp))
        called()
    return bufs, [step]


def job_lights(env, ds, tag=""):
    """Lights A, a cast frame, lights B enqueued behind that frame, a second frame: the first frame shows A, the second B."""
    w, h, _, shard = FRAMES[0]
    sh, rows = env.shard(w, shard)
    n = [tag + k for k in ("avgA", "rgbA", "avgB", "rgbB")]
    bufs = [(n[0], "out", ((rows, h, 3), f32)), (n[1], "out", ((rows, h, 3), np.uint8)), (n[2], "out", ((rows, h, 3), f32)),
            (n[3], "out", ((rows, h, 3), np.uint8))]

    def step(B, sp, called):
        for lights, a, r in ((LIGHTS_A, n[0], n[1]), (LIGHTS_B, n[2], n[3])):
            table = lights.copy()
            _ok(env, env.L.sq_scene_set_lights(ds._h, table.ctypes.data, len(table), sp))
            called(table)
            cam = env.new_cam()
            _ok(env, env.L.sq_render_rows_device(ds._h, C.byref(cam), 1, w, h, 1, sh, _p(B[a]), _p(B[r]), sp))
            called(cam)
    return bufs, [step]


def golden(name):
    return np.load(os.path.join(GOLDEN, name))


def check_outside(env, job, want):
    """One expectation per family from outside the library: tests/golden, the oracle's intersectBIH, the rule restated in numpy."""
    if job in ("frames", "range", "masked"):
        avg = want["avgA0"] if job == "range" else want["avg0"]
        gold = golden("scene_64x64_4spp_avg.npy")
        if job == "masked":                                     # the live pixels of the checkerboard
            y, x = np.indices(avg.shape[:2])
            live = ((y + x) & 1) == 1
            assert same_result(avg[live], gold[live]) and (bits(avg[~live]) == bits(np.full(3, POISON_OUT["float32"], f32))).all()
            assert (want["counts0"][live] == 4).all() and (want["counts0"][~live] == 77).all()
        else:
            assert same_result(avg, gold)
        if job == "frames":
            assert np.array_equal(want["rgb0"], golden("scene_64x64_4spp_rgb8.npy"))
        if job == "range":
            assert same_result(want["sum0"], want["carry0"]) and same_result(want["avgA1"], want["avgB1"]) and same_result(want["avgA0"], want["avgB0"])
    elif job == "cast_frames":
        assert same_result(want["avg0"], golden("scene_64x64_cast_avg.npy"))
    elif job == "intersect":
        check_hits((want["tri"], want["dist"], want["point"]), env.oracle_hits(), ("streams", "intersect"))
        assert (want["tri"] >= 0).any() and (want["tri"] < 0).any()      # mixed hits and misses
    elif job == "adaptive_update":
        live = int(want["live"][0])
        assert 0 < live < want["mask"].size and live == int(want["mask"].sum())
    elif job == "raytrace":
        assert same_result(want["rsum"], want["rsum2"]) and same_result(want["ravg"], want["ravg2"]) and np.array_equal(want["rrgb"], want["rrgb2"])
        assert want["rsum"].any()
    elif job == "raycast":
        assert want["rad"].any()
    elif job == "lights":
        assert not same_result(want["avgA"], want["avgB"]) and want["avgA"].any()      # the fold is ordered: A and B differ
    elif job == "camera_rays":
        assert (want["ctri"] >= 0).any()
    elif job == "views":
        assert not same_result(want["vavg"][0], want["vavg"][1]) and want["vavg"].any()

