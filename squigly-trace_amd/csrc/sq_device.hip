// sq_device.hip — the host runtime of the renderer and the render half of the C-ABI (include/squigly_hip.h): scene upload, the
// workspace, what a call enqueues (launch_frame) and every extern "C" entry point.  The device code is in the headers included below.
//
// What runs on the GPU (hand-written for CDNA4, wave64; per-ray primitives: sq_scene.h; what a kernel is handed: sq_frame.h) and where: W = sq_kernels_wave.h, T = sq_kernels_trace.h, L = sq_kernels_lane.h
//   camera-ray generation            src/Lib.hs:107-114                      sq_primary (W), sq_primary_resident (T)
//   RNG + bounce (scatter / mirror)  src/Lib.hs:133-134,155-198              sq_gen_bounce1, sq_shade1 (W)
//   BIH traversal + Moller-Trumbore  src/BIH.hs:101-141, Geometry.hs:117-177 sq_trace_rays (T; the dominant kernel)
//   emissive shade, radiance fold    src/Lib.hs:135-137                      sq_shade1, sq_accumulate (W)
//   ordered per-pixel accumulation   src/Lib.hs:85-88                        sq_accumulate (W)
//   atan tonemap                     src/Lib.hs:93-104                       sq_accumulate (W)
//   raycast under caller-given lights src/Lib.hs:141-151                     sq_cast_pixels (L); sq_cast_gen, sq_cast_fold (W: wavefront form)
//   paths of a caller-given depth    src/Lib.hs:127-137                      sq_deep_gen, sq_deep_bounce, sq_deep_fold (W); sq_render_pixels_deep (L)
//   ray queries                      src/BIH.hs:101-141                      sq_rays_stage, sq_rays_store (W); sq_intersect_lanes (L)
//
// Pipeline ("wavefront" form of renderPixel):  every sample of a pixel shoots the same primary ray
// (src/Lib.hs:81-87), so it is traced once per pixel and the pixels that hit are compacted (wave ballot +
// prefix rank).  Then, per batch of samples, every sample owns one slot: its first bounce ray is generated
// into the slot, traced by a persistent kernel (which compacts live slots on the fly and lets a lane pull
// its next ray as soon as the previous one finishes), shaded, replaced in place by the second bounce ray,
// traced again, and folded into a per-sample radiance; radiances are summed per pixel in sample order.
// Every value is computed by the same fp32 expression tree as the reference.
// The one-lane-per-pixel kernel sq_render_pixels serves raycast mode and is a cross-check variant.
// Radiance queries (sq_raytrace_rays_device, sq_raycast_rays_device: Lib.raytrace / Lib.raycast of caller-given rays, src/Lib.hs:127-151)
// run the same pipeline from a third ray source: the kernels' kSrcRays instantiations read origin, direction and seed base from the caller's
// arrays where the frames' instantiations read the camera.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <chrono>
#include <thread>
#include <vector>

#include "../../include/squigly_hip.h"
#include "../../include/squigly_host.h"
#include "sq_call_checks.h"
#include "sq_pack.h"
#include "sq_kernels_lane.h"
#include "sq_kernels_wave.h"
#include "sq_kernels_trace.h"

constexpr int kOneshotRowBlock = 2; // rows per block when a one-shot call shards a frame over devices (balance: squigly-trace_amd/dist.py)

// ----------------------------------------------------------------------------------------------
// Host: scene upload (validation and packing: sq_pack_scene.h, sq_pack.h)
// ----------------------------------------------------------------------------------------------
// A filled table of generator words: entries [0, cover) (RngView), kRngPad bytes of padding behind them.  Nothing writes to a block
// once it is filled, so a scene that adopts one only has to be ordered after `filled`, the event recorded behind the fill.
struct RngTable { uint32_t* words = nullptr; size_t bytes = 0; int64_t cover = 0; hipEvent_t filled = nullptr; };
struct sq_device_scene {
    int device = 0;
    SceneView view{};
    void* d_arena = nullptr;      // every array of `view` lives in this one allocation
    int height = 0; bool small_index = false; int n_cu = 256;
    Level1Cull level1{};          // PackedScene's: the first-bounce reduction's tables (sq_gen_bounce1)
    int shortcut_depth = 0;       // PackedScene's: a launch at a greater depth runs with the s == 0 shortcuts off (launch_frame)
    // workspace (grow-only)
    Work work{}; void* d_work = nullptr; size_t work_bytes = 0; int64_t work_pixels = 0, work_slots = 0;
    // timing of the dominant kernel
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
    double total_ms = 0; int64_t launches = 0;
    Options opt;                  // sq_set_option (sq_plan.h)
    const char* last_kernel = "sq_trace_rays";
    sq_plan plan{}; bool has_plan = false;   // what the last frame's launch_frame chose (sq_last_plan)
    // second stream of the overlapped schedule (launch_frame) and its event pool
    hipStream_t aux = nullptr; std::vector<hipEvent_t> events;
    // multi-view frames: the camera table (kCamWords floats per view, grow-only), filled on the call's stream
    float* d_cams = nullptr; int64_t cams_cap = 0;
    // masked calls with second moments: Work::px_sum2, 3 floats per pixel (grow-only; no other call allocates or reads it)
    float* d_px_sum2 = nullptr; int64_t px_sum2_cap = 0;
    // the table of generator words (grow-only, allocated after the workspace; ensure_rng_table; its budget: option "rng_table_mb")
    RngTable rng{};
    // caller-given lights (sq_scene_set_lights): the host copy (the reference's light until set, and after a reset), whether it was set,
    // the device table (kMaxLights entries, allocated on first need, filled in stream order) and whether it holds the host copy;
    // cast_carry = the wavefront form's carry of T, 3 floats per pixel at the end of the workspace block
    std::vector<sq_light> lights{ sq_light{ { 0.0f, 3.0f, -1.0f }, { 2.0f, 2.0f, 2.0f } } };
    bool lights_set = false, lights_staged = false;
    float* d_lights = nullptr; float* cast_carry = nullptr;
    // caller-given path depth (sq_scene_set_depth) and option "deep"; d_deep = the wavefront form's per-slot state beyond the three-level
    // pipeline's (Deep: trail, oxy), allocated by the first deep call that needs it (grow-only; a scene that stays at depth 3 has none)
    int32_t depth = 3;
    void* d_deep = nullptr; size_t deep_bytes = 0;
    // caller-given sky (sq_scene_set_sky): host state read by the next call's planning, like the depth; it travels by value (Sky)
    sq_sky sky{}; bool sky_set = false;
};

extern "C" int sq_scene_upload(const sq_scene* sc, int32_t device, sq_device_scene** out) {
    if (sq_check_scene_args(sc, out)) return 1;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return sq_set_error("no HIP device available (this library has no CPU fallback)");
    if (device < 0 || device >= ndev) return sq_set_error("device %d outside 0..%d", device, ndev - 1);
    PackedScene P;
    if (sq_pack_scene(*sc, P)) return 1;
    SQ_HIP(hipSetDevice(device));
    sq_device_scene* s = new sq_device_scene;
    s->device = device; s->height = P.height; s->small_index = P.small_index; s->shortcut_depth = P.shortcut_depth; s->level1 = P.level1;
    // SQ_AUTO_OVERLAP=0 / 1: the scene's default of option "auto_overlap", read once per scene (a profiling run of a program that sets
    // no options pins the serial schedule with it: per-kernel times and counters are those of launches that run alone)
    if (const char* env = std::getenv("SQ_AUTO_OVERLAP")) s->opt.auto_overlap = std::atoi(env) != 0;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) s->n_cu = prop.multiProcessorCount;
    // One arena for every array of the scene: one hipMalloc, one host-packed hipMemcpy and (sq_scene_free) one hipFree
    // instead of thirteen of each -- the one-shot calls upload and free a scene per frame, and at the CLI's default frame
    // (540 x 540 at 10 samples) those calls were a third of the call's time.  Every array starts on a 256-byte boundary.
    // The table: each SceneView member and its vector, in arena order; an empty optional array takes no room and stays nullptr.
    SceneView& v = s->view;
    std::vector<unsigned char> tail;                       // level-1 culling's cover and, directly behind it, its mirror record
    if (!P.level1_cover.empty()) {
        tail.resize(sizeof(Level1Cover) + sizeof(Level1Mirror));
        std::memcpy(tail.data(), P.level1_cover.data(), sizeof(Level1Cover));
        std::memcpy(tail.data() + sizeof(Level1Cover), P.level1_mirror.data(), sizeof(Level1Mirror));
    }
    auto arrays = [&](auto&& f) {
        f(v.branches, P.branches, false); f(v.leaves, P.leaves, false); f(v.tris, P.tris, false); f(v.tri_mat, P.tri_mat, false);
        f(v.surfs, P.surfs, false); f(v.mats, P.mats, false); f(v.verts4, P.verts4, false); f(v.trix, P.trix, false);
        f(v.rbranch, P.rbranch, false); f(v.emitters, P.emitters, false);
        f(v.cull_child, P.cull_child, true); f(v.cull_child16, P.cull_child16, true); f(v.branches_m, P.branches_m, true);
        f(v.rtail, tail, true);
    };
    auto slot = [](size_t bytes) { return ((bytes ? bytes : 16) + 255) & ~(size_t)255; };
    size_t arena_bytes = 0;
    arrays([&](auto&, const auto& vec, bool optional) { if (!optional || !vec.empty()) arena_bytes += slot(vec.size() * sizeof(vec[0])); });
    if (hipMalloc(&s->d_arena, arena_bytes) != hipSuccess) { sq_scene_free(s); return sq_set_error("hipMalloc(%zu) for the scene failed", arena_bytes); }
    std::vector<unsigned char> staging(arena_bytes, 0);
    size_t off = 0;
    arrays([&](auto& member, const auto& vec, bool optional) {
        if (optional && vec.empty()) return;
        const size_t bytes = vec.size() * sizeof(vec[0]);
        if (bytes) std::memcpy(staging.data() + off, vec.data(), bytes);
        member = reinterpret_cast<std::remove_reference_t<decltype(member)>>((const char*)s->d_arena + off);
        off += slot(bytes);
    });
    if (hipMemcpy(s->d_arena, staging.data(), arena_bytes, hipMemcpyHostToDevice) != hipSuccess) { sq_scene_free(s); return sq_set_error("hipMemcpy H2D of the scene failed"); }
    if (P.trix.empty()) v.trix = nullptr;                  // "not encodable" (the slot stays, so that later arrays keep their offsets)
    for (int c = 0; c < 3; ++c) { v.root_lo[c] = sc->root.lo[c]; v.root_hi[c] = sc->root.hi[c]; }
    v.root_ref = P.root_ref; v.packed_leaves = P.packed_leaves; v.rroot = P.rroot;
    v.n_branches = P.nb; v.n_leaves = P.nl; v.n_tris = sc->n_tris; v.n_mats = sc->n_mats; v.n_verts = P.n_verts; v.n_emitters = P.n_emitters;
    v.height = P.height; v.nonneg_materials = P.nonneg_materials; v.finite_geometry = P.finite_geometry;
    v.cull_o2max = P.cull_limits[0]; v.cull_d2min = P.cull_limits[1]; v.cull_d2max = P.cull_limits[2];
    v.incremental_ok = 0;                                  // unread by every kernel (sq_scene.h)
    *out = s;
    return 0;
}

// Frame workspaces outlive the scene that allocated them: one block per device is kept for the next scene
// (sq_release_cached_memory() returns it).  The one-shot calls create and free a scene per frame, and a
// hipMalloc that follows the hipFree of a 32 GB block can wait seconds for the driver to scrub it.
namespace {
struct CachedBlock { void* ptr = nullptr; size_t bytes = 0; };
std::mutex g_cache_mutex;
CachedBlock g_cache[64];
void* cache_take(int device, size_t bytes, size_t* got) {   // a block of at least `bytes` (its size in *got), or nullptr
    std::lock_guard<std::mutex> lock(g_cache_mutex);
    CachedBlock& c = g_cache[device & 63];
    if (!c.ptr || c.bytes < bytes) return nullptr;
    void* p = c.ptr; *got = c.bytes; c = CachedBlock{};
    return p;
}
void cache_give(int device, void* ptr, size_t bytes) { // keeps the larger block, frees the other
    void* drop = ptr;
    {
        std::lock_guard<std::mutex> lock(g_cache_mutex);
        CachedBlock& c = g_cache[device & 63];
        if (bytes > c.bytes) { drop = c.ptr; c.ptr = ptr; c.bytes = bytes; }
    }
    if (drop) (void)hipFree(drop);
}
// ... and so do the tables of generator words, whose entries do not depend on the scene: the next scene that needs no more
// seeds than the kept block holds takes it as it is, filled.
RngTable g_rng_cache[64];
void rng_free(RngTable& t) {                            // hipFree waits for the device: no kernel still reads the block
    if (t.words) (void)hipFree(t.words);
    if (t.filled) (void)hipEventDestroy(t.filled);
    t = RngTable{};
}
bool rng_cache_take(int device, int64_t cover, RngTable* out) {   // a block that holds at least `cover` seeds
    std::lock_guard<std::mutex> lock(g_cache_mutex);
    RngTable& c = g_rng_cache[device & 63];
    if (!c.words || c.cover < cover) return false;
    *out = c; c = RngTable{};
    return true;
}
void rng_cache_give(int device, RngTable& t) {          // keeps the block with more seeds, frees the other
    RngTable drop = t;
    t = RngTable{};
    {
        std::lock_guard<std::mutex> lock(g_cache_mutex);
        RngTable& c = g_rng_cache[device & 63];
        if (drop.cover > c.cover) std::swap(drop, c);
    }
    rng_free(drop);
}
}  // namespace
extern "C" void sq_release_cached_memory(void) {
    for (int d = 0; d < 64; ++d) {
        size_t got = 0;
        void* p = cache_take(d, 0, &got);
        RngTable t;
        const bool have_table = rng_cache_take(d, 0, &t);
        if ((p || have_table) && hipSetDevice(d) == hipSuccess) { (void)hipFree(p); rng_free(t); }
    }
}

extern "C" void sq_scene_free(sq_device_scene* s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    for (auto& p : s->pending) { (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second); }
    (void)hipFree(s->d_arena);
    if (s->d_work) cache_give(s->device, s->d_work, s->work_bytes);
    if (s->rng.words) rng_cache_give(s->device, s->rng);
    for (hipEvent_t e : s->events) (void)hipEventDestroy(e);
    if (s->aux) (void)hipStreamDestroy(s->aux);
    (void)hipFree(s->d_cams);
    (void)hipFree(s->d_px_sum2);
    (void)hipFree(s->d_lights);
    (void)hipFree(s->d_deep);
    delete s;
}

extern "C" int32_t sq_shard_rows(int32_t w, sq_shard sh) {
    if (w <= 0 || sh.row_block <= 0 || sh.n_shards <= 0 || sh.shard < 0 || sh.shard >= sh.n_shards) return -1;
    const int64_t nblocks = ((int64_t)w + sh.row_block - 1) / sh.row_block;
    int64_t rows = 0;
    for (int64_t b = sh.shard; b < nblocks; b += sh.n_shards) {
        const int64_t y0 = b * sh.row_block, y1 = (y0 + sh.row_block < w) ? y0 + sh.row_block : w;
        rows += y1 - y0;
    }
    return (int32_t)rows;
}
extern "C" int32_t sq_shard_global_row(int32_t j, sq_shard sh) { return sq::shard_global_row(j, sh.row_block, sh.shard, sh.n_shards); }

namespace {

// Carves the frame workspace out of one allocation (grow-only; allocation happens outside timed steps after warm-up), by
// workspace_layout's offsets (sq_plan.h).
// If the device cannot give `slots` sample slots the request is halved (down to one sample per pixel): the frame
// then simply runs in more batches.  A new block's statistics are cleared on `stream`, the call's own: in front of every kernel of the
// call that counts into them, whichever stream the caller gave (a non-blocking one is not ordered against the null stream).
int ensure_workspace(sq_device_scene* s, int64_t pixels, int64_t slots, hipStream_t stream) {
    if (pixels <= s->work_pixels && slots <= s->work_slots && s->d_work) return 0;
    pixels = std::max(pixels, s->work_pixels); slots = std::max(slots, s->work_slots);
    if (s->d_work) { cache_give(s->device, s->d_work, s->work_bytes); s->d_work = nullptr; s->work_pixels = s->work_slots = 0; }
    size_t block_bytes = 0;
    WorkLayout L{};
    for (;;) {
        if (workspace_layout(pixels, slots, L)) return 1;
        const size_t off = L.total;
        block_bytes = off;
        if ((s->d_work = cache_take(s->device, off, &block_bytes)) != nullptr) break;
        if (hipMalloc(&s->d_work, off) == hipSuccess) break;
        (void)hipGetLastError();
        s->d_work = nullptr;
        // the workspace comes first: the tables of generator words (this scene's, the kept one) go before the slots are halved
        RngTable kept;
        const bool have_kept = rng_cache_take(s->device, 0, &kept);
        if (s->rng.words || have_kept) { rng_free(s->rng); rng_free(kept); continue; }
        if (slots <= pixels) return sq_set_error("hipMalloc(%zu B) for the frame workspace failed", off);
        slots = std::max<int64_t>(pixels, slots / 2);
    }
    char* base = (char*)s->d_work;
    Work& W = s->work;
    int32_t* cnt = (int32_t*)(base + L.cnt);
    W.n_active = cnt; W.head[0] = cnt + 16; W.head[1] = cnt + 32;      // separate cache lines
    W.stats = (unsigned long long*)(base + L.stats);
    if (hipMemsetAsync(W.stats, 0, kStatSlots * sizeof(unsigned long long), stream) != hipSuccess) return sq_set_error("hipMemsetAsync failed");
    W.px_pixel = (int32_t*)(base + L.pix); W.px_t0 = (float*)(base + L.t0); W.px_tri0 = (int32_t*)(base + L.tri0); W.px_sum = (float*)(base + L.sum);
    W.px_mt = (float*)(base + L.mt); W.px_mtri = (int32_t*)(base + L.mtri);
    W.state = (uint8_t*)(base + L.state); W.org = (float4*)(base + L.org); W.dir = (float4*)(base + L.dir); W.tri1 = (int32_t*)(base + L.tri1);
    W.slot_capacity = slots;
    s->cast_carry = (float*)(base + L.carry);
    s->work_bytes = block_bytes; s->work_pixels = pixels; s->work_slots = slots;
    return 0;
}

// The table of generator words a frame of F's shape reads on `stream`: the scene's table, grown first -- behind the workspace, so it
// never takes memory the workspace wanted -- when the frame can use more seeds than it holds (sq_rng_table_cover).  A larger table
// is a new block filled from seed 0: keeping the old entries would need a copy as long as both blocks live, a fill costs about
// 2 ms per 100 M seeds, and a scene grows its table once per larger frame shape.  Failing to allocate is not an error: the scene
// keeps the table it has (or none), and the lanes it does not cover compute their words.  grow = false (a radiance query, whose
// seeds the host does not know) takes the table as it is.
RngView ensure_rng_table(sq_device_scene* s, const Frame& F, hipStream_t stream, bool grow) {
    const int64_t budget = s->opt.rng_table_mb << 20;
    if (budget <= 0) return RngView{ nullptr, 0 };
    RngTable& T = s->rng;
    const int64_t want = grow ? sq_rng_table_cover(F.w, F.h, F.samples, budget) : 0;
    if (want > T.cover) {
        RngTable N;
        if (!rng_cache_take(s->device, want, &N)) {
            N.cover = want;
            N.bytes = (size_t)want * 12 + kRngPad;
            const long long quads = (want + kRngRun - 1) / kRngRun;
            static_assert(kRngPad >= 12 * kRngRun, "the last run of a table is filled and read whole");
            if (hipMalloc((void**)&N.words, N.bytes) != hipSuccess || hipEventCreateWithFlags(&N.filled, hipEventDisableTiming) != hipSuccess) {
                (void)hipGetLastError();
                rng_free(N);
            } else {
                const long long blocks = std::min<long long>((quads + kBlock - 1) / kBlock, (long long)s->n_cu * 64);
                hipLaunchKernelGGL(sq_rng_fill, dim3((unsigned)blocks), dim3(kBlock), 0, stream, N.words, 0ll, quads);
                if (hipGetLastError() != hipSuccess || hipEventRecord(N.filled, stream) != hipSuccess) { (void)hipGetLastError(); rng_free(N); }
            }
        }
        if (N.words) { rng_free(T); T = N; }        // the old block: freed once the device is idle, so no earlier frame still reads it
    }
    if (!T.words) return RngView{ nullptr, 0 };
    // whichever stream filled the block (this scene's earlier frame, another scene's): this frame's reads come after the fill
    if (hipStreamWaitEvent(stream, T.filled, 0) != hipSuccess) { (void)hipGetLastError(); return RngView{ nullptr, 0 }; }
    return RngView{ T.words, (long long)std::min<int64_t>(T.cover, budget / 12) };
}

// The camera table of a multi-view frame: room for n views (grow-only).  Growing frees the old table, which waits for the
// device, so the table a previous frame still reads is not freed under it.
int ensure_cam_table(sq_device_scene* s, int64_t n) {
    if (n <= s->cams_cap) return 0;
    const int64_t cap = std::max<int64_t>((n + 63) / 64 * 64, 2 * s->cams_cap);
    if (s->d_cams) { SQ_HIP(hipFree(s->d_cams)); s->d_cams = nullptr; s->cams_cap = 0; }
    SQ_HIP(hipMalloc(&s->d_cams, (size_t)cap * kCamWords * sizeof(float)));
    s->cams_cap = cap;
    return 0;
}
// Work::px_sum2 of a masked call that carries second moments: room for `pixels` pixels (grow-only, freed as the camera table is).
int ensure_px_sum2(sq_device_scene* s, int64_t pixels) {
    if (pixels <= s->px_sum2_cap) return 0;
    if (s->d_px_sum2) { SQ_HIP(hipFree(s->d_px_sum2)); s->d_px_sum2 = nullptr; s->px_sum2_cap = 0; }
    SQ_HIP(hipMalloc(&s->d_px_sum2, (size_t)pixels * 3 * sizeof(float)));
    s->px_sum2_cap = pixels;
    return 0;
}
// The scene's Deep block: room for `slots` slots of slot_bytes each (deep_slot_bytes, sq_plan.h; grow-only, freed as the camera table is: hipFree waits for the device,
// so a block an enqueued frame still uses is not freed under it).
int ensure_deep(sq_device_scene* s, int64_t slots, size_t slot_bytes, int depth) {
    const size_t need = (size_t)slots * slot_bytes;
    if (need <= s->deep_bytes) return 0;
    if (s->d_deep) { SQ_HIP(hipFree(s->d_deep)); s->d_deep = nullptr; s->deep_bytes = 0; }
    if (hipMalloc(&s->d_deep, need) != hipSuccess) { (void)hipGetLastError(); s->d_deep = nullptr; return sq_set_error("hipMalloc(%zu B) for the path trails of depth %d failed", need, depth); }
    s->deep_bytes = need;
    return 0;
}
// Enqueues the copy of a multi-view frame's cameras into its table F.cams (nothing for a single-view frame: cams = nullptr).
int stage_cams(sq_device_scene* s, const Frame& F, const sq_camera* cams, hipStream_t stream) {
    (void)s;
    if (!cams) return 0;
    static_assert(sizeof(sq_camera) == kCamWords * sizeof(float), "sq_camera is one camera-table entry");
    for (int i0 = 0; i0 < F.n_views; i0 += kCamChunk) {
        const int n = std::min(kCamChunk, F.n_views - i0);
        CamChunk c{};
        std::memcpy(c.v, cams + i0, (size_t)n * sizeof(sq_camera));
        hipLaunchKernelGGL(sq_stage_cams, dim3(1), dim3(kBlock), 0, stream, const_cast<float*>(F.cams) + (long long)kCamWords * i0, n, c);
        SQ_HIP(hipGetLastError());
    }
    return 0;
}

// The scene's light table: room for kMaxLights lights, allocated once (96 KB), so a later sq_scene_set_lights never frees a table that
// an enqueued frame still reads.
int ensure_light_table(sq_device_scene* s) {
    if (s->d_lights) return 0;
    SQ_HIP(hipMalloc((void**)&s->d_lights, (size_t)kMaxLights * kLightWords * sizeof(float)));
    return 0;
}
// Enqueues the copy of `lights` into the scene's light table on `stream`.  The lights travel as kernel arguments, captured when the
// launch is enqueued: the table changes in stream order, and the host array is not read after the call.
int stage_lights(sq_device_scene* s, const std::vector<sq_light>& lights, hipStream_t stream) {
    static_assert(sizeof(sq_light) == kLightWords * sizeof(float), "sq_light is one light-table entry");
    const int n_all = (int)lights.size();
    for (int i0 = 0; i0 < n_all; i0 += kLightChunk) {
        const int n = std::min(kLightChunk, n_all - i0);
        LightChunk c{};
        std::memcpy(c.v, lights.data() + i0, (size_t)n * sizeof(sq_light));
        hipLaunchKernelGGL(sq_stage_lights, dim3(1), dim3(kBlock), 0, stream, s->d_lights + (long long)kLightWords * i0, n, c);
        SQ_HIP(hipGetLastError());
    }
    return 0;
}

// Enqueues fn's launch; with option "timing" brackets it with hipEvents for sq_kernel_timing.
template <typename Fn>
int timed_launch(sq_device_scene* s, Fn&& fn, const char* name, hipStream_t on) {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (s->opt.timing) { SQ_HIP(hipEventCreate(&e0)); SQ_HIP(hipEventCreate(&e1)); SQ_HIP(hipEventRecord(e0, on)); }
    fn();
    SQ_HIP(hipGetLastError());
    if (s->opt.timing) {
        SQ_HIP(hipEventRecord(e1, on)); s->pending.emplace_back(e0, e1); s->last_kernel = name;
        if (s->pending.size() > 8192) SQ_HIP(sq_kernel_timing(s, nullptr, nullptr, nullptr) ? hipErrorUnknown : hipSuccess);   // fold, bounded memory
    }
    return 0;
}

// A call's run-time choices as the kernels' compile-time ones, where it launches (every family is one template: sq_shade1<SRC>, ...).
// with_ad: fn(std::bool_constant<ad>); only single-view frames (CAN_AD) have masked calls, so nothing else instantiates AD kernels.
// with_sky: fn(k) under a sky, fn() without: the kernel's trailing argument pack.  with_ad_sky: fn(ad, k) or fn(ad).
template <bool CAN_AD, typename Fn>
int with_ad(bool ad, Fn&& fn) {
    if constexpr (CAN_AD) if (ad) return fn(std::true_type{});
    return fn(std::false_type{});
}
template <typename SkyT, typename Fn>
int with_sky(bool sky, const SkyT& k, Fn&& fn) { return sky ? fn(k) : fn(); }
template <bool CAN_AD, typename SkyT, typename Fn>
int with_ad_sky(bool ad, bool sky, const SkyT& k, Fn&& fn) {
    return with_ad<CAN_AD>(ad, [&](auto AD) { return sky ? fn(AD, k) : fn(AD); });
}

// What the planner (sq_plan.h, sq_plan_call.h) reads of a scene for `call`: its packed scalars, options, device and state.
PlanInputs plan_inputs(const sq_device_scene* s, const Call& call, int stack_word) {
    PlanInputs in;
    const SceneView& v = s->view;
    in.opt = s->opt;
    in.scene.n_branches = v.n_branches; in.scene.n_verts = v.n_verts; in.scene.n_tris = v.n_tris; in.scene.height = v.height;
    in.scene.has_trix = v.trix != nullptr; in.scene.stack_word = stack_word;
    in.scene.packed_leaves = v.packed_leaves; in.scene.n_emitters = v.n_emitters; in.scene.nonneg_materials = v.nonneg_materials;
    in.scene.finite_geometry = v.finite_geometry; in.scene.shortcut_depth = s->shortcut_depth; in.scene.level1_on = s->level1.on;
    in.device.n_cu = s->n_cu;
    in.state.depth = s->depth; in.state.sky_set = s->sky_set; in.state.lights_set = s->lights_set; in.state.n_lights = (int32_t)s->lights.size();
    in.call = call;
    return in;
}
// Plans the call (nothing here touches the device) and stores the public part as the scene's last plan: after a refusal what was planned
// up to it, otherwise launched = 0 until the caller has ensured its buffers.
int begin_call(sq_device_scene* s, const PlanInputs& in, CallPlan& C) {
    const int rc = plan_call(in, C);
    if (!C.planned) return rc;
    s->plan = C.plan; s->plan.launched = 0; s->has_plan = true;
    return rc;
}
// The scene view with the call's overrides applied.
SceneView call_view(const sq_device_scene* s, const CallPlan& C) {
    SceneView S = s->view;
    if (C.cull_off) S.cull_o2max = -1.0f;                              // no ray is inside the culling limits: every leaf is tested
    S.nonneg_materials = C.nonneg_materials; S.n_emitters = C.n_emitters;
    return S;
}

// The planned trace kernel: (form, pool, profile) -> entry point.
template <typename StackT>
const void* trace_kernel(const CallPlan& C) {
    if (C.dense) return (const void*)sq_trace_rays_dense<StackT>;
    if (C.resident)
        return C.pool ? (C.profile ? (const void*)sq_trace_rays<StackT, true, kResidentBlock, true, true> : (const void*)sq_trace_rays<StackT, true, kResidentBlock, false, true>)
                      : (C.profile ? (const void*)sq_trace_rays<StackT, true, kResidentBlock, true, false> : (const void*)sq_trace_rays<StackT, true, kResidentBlock, false, false>);
    return C.pool ? (C.profile ? (const void*)sq_trace_rays<StackT, false, kTraceBlock, true, true> : (const void*)sq_trace_rays<StackT, false, kTraceBlock, false, true>)
                  : (C.profile ? (const void*)sq_trace_rays<StackT, false, kTraceBlock, true, false> : (const void*)sq_trace_rays<StackT, false, kTraceBlock, false, false>);
}
// What the trace kernel needs of the runtime before its first launch: its dynamic LDS above 64 KB, and the static-LDS check of the
// resident kernels.  SRC: the frame's resident primary-ray kernels, checked with the trace kernels' (an intersection query: kSrcCamera).
template <typename StackT, int SRC>
int prepare_trace(const CallPlan& C, const void* trace_fn) {
    if (C.tr_lds > 64 * 1024) SQ_HIP(hipFuncSetAttribute(trace_fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)C.tr_lds));
    static std::atomic<bool> static_lds_checked{false};               // once per process is enough; the one-shot path's per-device threads may both check
    if (C.resident && !static_lds_checked.load(std::memory_order_relaxed)) {
        // ResidentTris takes a vertex's byte offset for its LDS address: the vertex table must sit at LDS address 0, i.e. the
        // kernels that stage a resident scene must own no static __shared__ (their dynamic LDS then starts at 0).  Checked here,
        // where a violation is an error code, rather than by the device-side trap, where it would be a GPU abort.
        const void* fns[6] = { (const void*)sq_trace_rays<StackT, true, kResidentBlock, false, true>, (const void*)sq_trace_rays<StackT, true, kResidentBlock, true, true>,
                               (const void*)sq_trace_rays<StackT, true, kResidentBlock, false, false>, (const void*)sq_trace_rays<StackT, true, kResidentBlock, true, false>,
                               (const void*)sq_primary_resident<StackT, SRC, false>, (const void*)sq_primary_resident<StackT, SRC, false, Sky> };
        for (const void* fn : fns) {
            hipFuncAttributes attr{};
            SQ_HIP(hipFuncGetAttributes(&attr, fn));
            if (attr.sharedSizeBytes != 0)
                return sq_set_error("internal error: a resident-scene kernel has %zu B of static LDS; its vertex table would not start at LDS address 0", (size_t)attr.sharedSizeBytes);
        }
        static_lds_checked.store(true, std::memory_order_relaxed);
    }
    return 0;
}

// One launch of the planned trace kernel over the queue of W: *W.n_active x kc slots (+ *W.n_active front slots with the mirror
// rays).  queue_rays x kc sizes its reservations (trace_launch, sq_plan.h): a frame's pixels (every pixel may be active), a query chunk's rays.
int launch_trace_kernel(sq_device_scene* s, const SceneView& S, const CallPlan& C, const void* trace_fn, const Work& W, int64_t queue_rays, int kc, int level,
                        hipStream_t on, bool with_mirror_rays) {
    const Options& o = s->opt;
    const TraceLaunch T = trace_launch(C, queue_rays, kc, level);
    TraceArgs A{ W.org, W.dir, W.state, level == 0 ? (int32_t)kRay1 : (int32_t)kRay2, (long long)s->work.slot_capacity, with_mirror_rays ? 1 : 0,
                 W.n_active, kc, W.head[level], C.n_lds, C.stack_cap, (int32_t)o.straggler_lanes, T.chunk, T.guide_shift,
                 (int32_t)o.refill_min, (int32_t)o.flush_min, (int32_t)o.descend_extra, (int32_t)o.descend_lanes,
                 (int32_t)(o.coresidency ? 1 : 0), (int32_t)o.trace_prio, (int32_t)T.pixel_major, W.stats };
    SceneView Sv = S;
    return timed_launch(s, [&] {
        void* kargs[] = { (void*)&Sv, (void*)&A };
        (void)hipLaunchKernel(trace_fn, dim3(C.trace_blocks), dim3(C.trace_threads), kargs, C.tr_lds, on);
    }, "sq_trace_rays", on);
}

// A frame: plan (plan_call), ensure its buffers, schedule for the slots the workspace got (plan_schedule), enqueue.  Every size, grid
// and threshold comes from the plan; what is decided here needs HIP or the template arguments.
// kSrcViews: a multi-view frame; `cams` (host, F.n_views of them) are staged into the scene's camera table F.cams once the frame is planned.
// kSrcRays: a chunk of a radiance query (radiance_rays): a frame of one row whose "pixels" are the caller's rays F.ray_org / ray_dir / ray_seed.
template <typename StackT, int SRC>
int launch_frame(sq_device_scene* s, const FrameOf<SRC>& F, hipStream_t stream, const sq_camera* cams) {
    Call call;
    call.src = SRC; call.cast = F.cast != 0; call.masked = F.mask || F.sum2 || F.count; call.mom2 = F.sum2 != nullptr;
    call.n_views = F.n_views; call.local_rows = F.local_rows; call.h = F.h; call.tile_rows = F.tile_rows; call.tiles_x = F.tiles_x;
    call.k_begin = F.k_begin; call.k_end = F.k_end;
    CallPlan C;
    if (begin_call(s, plan_inputs(s, call, (int)sizeof(StackT)), C)) return 1;     // refused: no allocation, free or memset has happened
    sq_plan& P = s->plan;
    const SceneView S = call_view(s, C);
    const bool ad = C.ad, sky = C.sky;
    const int depth = s->depth, n_lights = C.in.state.n_lights, n_call = C.n_call;
    const long long pixels = C.pixels;
    const size_t px_lds = C.px_lds;
    Sky KS{};
    if (sky) { std::memcpy(KS.up, s->sky.up, sizeof KS.up); std::memcpy(KS.down, s->sky.down, sizeof KS.down); }
    // The per-lane forms: one kernel, one lane per pixel.  The branches below choose the kernel and what follows S and F in its arguments.
    constexpr bool kCanAd = SRC == kSrcCamera;
    auto launch_per_lane = [&](auto kernel, const char* name, auto... args) -> int {
        if (px_lds > 64 * 1024) SQ_HIP(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)px_lds));
        P.launched = 1;
        if (stage_cams(s, F, cams, stream)) return 1;
        return timed_launch(s, [&] { hipLaunchKernelGGL(kernel, dim3((unsigned)C.px_blocks), dim3(kBlock), px_lds, stream, S, F, args...); }, name, stream);
    };
    if (C.path == kPathLaneCast) {                                     // caller-given lights: sq_cast_pixels beside sq_render_pixels
        const Lights L{ s->d_lights, n_lights, nullptr, 0, n_lights };
        return with_ad<kCanAd>(ad, [&](auto AD) { return launch_per_lane(sq_cast_pixels<StackT, SRC, AD()>, "sq_cast_pixels", L); });
    }
    if (C.path == kPathLaneDeep)                                       // a depth other than 3, or a sky: sq_render_pixels_deep beside sq_render_pixels
        return with_ad_sky<kCanAd>(ad, sky, KS, [&](auto AD, auto... K) {
            return launch_per_lane(sq_render_pixels_deep<StackT, SRC, AD(), decltype(K)...>, sizeof...(K) ? "sq_render_pixels_deep_sky" : "sq_render_pixels_deep", depth, K...);
        });
    if (C.path == kPathLanePlain)
        return with_ad<kCanAd>(ad, [&](auto AD) { return launch_per_lane(sq_render_pixels<StackT, SRC, AD()>, "sq_render_pixels"); });
    // ---- wavefront pipeline ----
    const bool cast_wave = C.path == kPathWaveCast, deep = C.path == kPathWaveDeep;
    const void* const trace_fn = trace_kernel<StackT>(C);
    if (prepare_trace<StackT, SRC>(C, trace_fn)) return 1;
    if (ensure_workspace(s, pixels, C.slots, stream)) return 1;
    if (C.need_sum2 && ensure_px_sum2(s, pixels)) return 1;
    s->work.px_sum2 = C.need_sum2 ? s->d_px_sum2 : nullptr;
    const Work& W = s->work;
    if (C.need_lights && ensure_light_table(s)) return 1;
    if (C.need_deep && ensure_deep(s, W.slot_capacity, C.deep_slot_bytes, depth)) return 1;
    // the slots the workspace got (the allocation may have halved them): tracks, batches and, per launch, grids and reservations
    const Schedule Sch = plan_schedule(C, W.slot_capacity);
    const bool overlap = Sch.overlap;
    const int batch = Sch.batch, n_real = Sch.n_real;
    Work Wt[2] = { W, W };
    if (overlap) {                                                     // the second track: the other half of the slots, cursors of its own
        Work& V = Wt[1];
        V.state += Sch.track_slots; V.org += Sch.track_slots; V.dir += Sch.track_slots; V.tri1 += Sch.track_slots;
        V.head[0] = W.n_active + 64 + 16; V.head[1] = W.n_active + 64 + 32;
    }
    const int aux_blocks = C.aux_blocks;
    // sq_accumulate, by second moments and by its loop form (acc_grouped: every thread at most one pixel)
    void (*const accumulate_kernel)(SceneView, Frame, Work, int, int) =
        C.mom2 ? (C.acc_grouped ? &sq_accumulate<true, true> : &sq_accumulate<false, true>) : (C.acc_grouped ? &sq_accumulate<true> : &sq_accumulate<false>);
    P.launched = 1;                                                    // planned; what follows fails only on HIP errors
    // nothing is enqueued before this point, and a refused call has not come this far: it leaves every buffer as it was
    if (stage_cams(s, F, cams, stream)) return 1;                       // multi-view: before every kernel that reads the table (e_setup below)
    if (cast_wave && !s->lights_staged) {                               // never set: the table receives the reference's light
        if (stage_lights(s, s->lights, stream)) return 1;
        s->lights_staged = true;
    }
    const RngView R = C.rng_table ? ensure_rng_table(s, F, stream, C.rng_grow) : RngView{ nullptr, 0 };   // allocated behind the workspace; its fill and the wait for it come before every sq_gen_bounce1 (e_setup below)
    // (a masked call's dead pixels keep what they hold: its primary kernels write the black of the live misses, store_live_miss)
    if (F.out_avg && !ad) SQ_HIP(hipMemsetAsync(F.out_avg, 0, (size_t)pixels * 3 * sizeof(float), stream));   // pixels whose primary ray misses: black
    if (F.out_rgb && !ad) SQ_HIP(hipMemsetAsync(F.out_rgb, 0, (size_t)pixels * 3, stream));
    SQ_HIP(hipMemsetAsync(W.n_active, 0, 128 * sizeof(int32_t), stream));
    // primary rays: once per pixel.  With a resident scene they are traced out of LDS as well ...
    if (P.primary_form == SQ_PRIMARY_RESIDENT) {
        if (with_ad_sky<kCanAd>(ad, sky, KS, [&](auto AD, auto... K) -> int {
                const auto kernel = sq_primary_resident<StackT, SRC, AD(), decltype(K)...>;
                SQ_HIP(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)C.primary_lds));
                hipLaunchKernelGGL(kernel, dim3((unsigned)C.primary_grid), dim3(kResidentBlock), C.primary_lds, stream, S, F, W, C.stack_cap, K...);
                return 0;
            })) return 1;
    } else if (P.primary_form == SQ_PRIMARY_PER_LANE) {
        if (with_ad_sky<kCanAd>(ad, sky, KS, [&](auto AD, auto... K) -> int {
                const auto kernel = sq_primary<StackT, SRC, AD(), decltype(K)...>;
                if (px_lds > 64 * 1024) SQ_HIP(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)px_lds));
                hipLaunchKernelGGL(kernel, dim3((unsigned)C.primary_grid), dim3(kBlock), px_lds, stream, S, F, W, K...);
                return 0;
            })) return 1;
    }
    SQ_HIP(hipGetLastError());
    // per-sample kernels that run one thread per active pixel, for a batch of kc samples (pp_grid, sq_plan.h)
    auto grid_of = [&](int kc) { const Grid2 g = pp_grid(C, Sch, kc); return dim3(g.x, g.y); };
    if (P.primary_form == SQ_PRIMARY_POOLED) {                          // ... or through the pooled trace kernel
        Work Wp = W; Wp.n_active = W.n_active + 48;                     // the launch's queue is the shard's pixels, not the active ones
        SQ_HIP(hipMemsetAsync(W.head[0], 0, 32 * sizeof(int32_t), stream));
        with_ad<kCanAd>(ad, [&](auto AD) { hipLaunchKernelGGL((sq_primary_gen<SRC, AD()>), dim3(aux_blocks), dim3(kBlock), 0, stream, F, W, pixels); return 0; });
        SQ_HIP(hipGetLastError());
        if (launch_trace_kernel(s, S, C, trace_fn, Wp, pixels, 1, 0, stream, false)) return 1;
        with_ad_sky<kCanAd>(ad, sky, KS, [&](auto AD, auto... K) {
            hipLaunchKernelGGL((sq_primary_store<AD(), decltype(K)...>), dim3(aux_blocks), dim3(kBlock), 0, stream, F, W, pixels, K...);
            return 0;
        });
        SQ_HIP(hipGetLastError());
    }
    if (cast_wave) {
        // Light batch i holds the lights [i * batch, i * batch + kc): shadow rays into the slots, one level of the trace kernel, fold.
        // Everything on the caller's stream ("overlap" is for sample batches).
        for (int i = 0; i * batch < n_lights; ++i) {
            const int l0 = i * batch, kc = std::min(batch, n_lights - l0);
            const Lights L{ s->d_lights, n_lights, s->cast_carry, l0, l0 + kc };
            SQ_HIP(hipMemsetAsync(W.head[0], 0, 32 * sizeof(int32_t), stream));     // both dequeue cursors
            hipLaunchKernelGGL(sq_cast_gen<SRC>, grid_of(kc), dim3(kBlock), 0, stream, S, F, W, L);
            SQ_HIP(hipGetLastError());
            if (launch_trace_kernel(s, S, C, trace_fn, W, pixels, kc, 0, stream, false)) return 1;
            hipLaunchKernelGGL(sq_cast_fold<SRC>, dim3(aux_blocks), dim3(kBlock), 0, stream, S, F, W, L, l0 + kc == n_lights ? 1 : 0);
            SQ_HIP(hipGetLastError());
        }
        return 0;
    }
    if (deep) {
        // Sample batch i holds the samples [k0, k0 + kc): ray 1 into the slots, then level by level a trace launch and the bounce behind
        // it, then the ordered fold.  Everything on the caller's stream ("overlap" is for the three-level pipeline).
        const long long cap = (long long)W.slot_capacity;
        const DeepLayout DL = deep_layout(depth, sky, cap);
        float2* const oxy = (float2*)((char*)s->d_deep + DL.oxy);
        int32_t* const trail = (int32_t*)((char*)s->d_deep + DL.trail);
        const DeepSky DS{ KS, DL.has_tmiss ? (float*)((char*)s->d_deep + DL.tmiss) : nullptr };
        for (int i = 0; i * batch < n_call; ++i) {
            const int k0 = F.k_begin + i * batch, kc = std::min(batch, n_call - i * batch);
            if (depth >= 2) {
                SQ_HIP(hipMemsetAsync(W.head[0], 0, 32 * sizeof(int32_t), stream));     // both dequeue cursors
                hipLaunchKernelGGL(sq_deep_gen<SRC>, grid_of(kc), dim3(kBlock), 0, stream, S, F, W, k0, kc, R);
                SQ_HIP(hipGetLastError());
            }
            for (int b = 1; b < depth; ++b) {
                const Deep D{ depth, b, trail, oxy, cap };
                if (b >= 3) SQ_HIP(hipMemsetAsync(W.head[0], 0, 32 * sizeof(int32_t), stream));   // a cursor's second use
                if (launch_trace_kernel(s, S, C, trace_fn, W, pixels, kc, (b - 1) & 1, stream, false)) return 1;
                with_sky(sky, DS, [&](auto... K) { hipLaunchKernelGGL((sq_deep_bounce<SRC, decltype(K)...>), grid_of(kc), dim3(kBlock), 0, stream, S, F, W, k0, kc, D, K...); return 0; });
                SQ_HIP(hipGetLastError());
            }
            const Deep D{ depth, 0, trail, oxy, cap };
            with_sky(sky, DS, [&](auto... K) { hipLaunchKernelGGL(sq_deep_fold<decltype(K)...>, dim3(aux_blocks), dim3(kBlock), 0, stream, S, F, W, kc, (i + 1) * batch >= n_call ? 1 : 0, D, K...); return 0; });
            SQ_HIP(hipGetLastError());
        }
        return 0;
    }
    // batch i holds the samples [k0_of(i), k0_of(i) + kc_of(i)) of [k_begin, k_end); the call's last batch ends the fold (sq_accumulate)
    auto k0_of = [&](int i) { return F.k_begin + i * batch; };
    auto kc_of = [&](int i) { return std::max(0, std::min(batch, n_call - i * batch)); };
    // The steps of batch i, each on the stream `on` and over the batch's track Wt[i & 1]; the schedules below say only which stream a
    // step goes on and which events order it.
    auto launched = []() -> int { SQ_HIP(hipGetLastError()); return 0; };
    // Level-1 culling (sq_pack_level1.h, build_level1): where the plan says so
    Level1Cull L1 = s->level1;
    L1.on = C.level1_cull;
    auto gen = [&](int i, hipStream_t on) -> int {
        SQ_HIP(hipMemsetAsync(Wt[i & 1].head[0], 0, 32 * sizeof(int32_t), on));     // both dequeue cursors
        hipLaunchKernelGGL(sq_gen_bounce1<SRC>, grid_of(kc_of(i)), dim3(kBlock), 0, on, S, F, Wt[i & 1], k0_of(i), kc_of(i), R, L1);
        return launched();
    };
    auto trace = [&](int i, int level, hipStream_t on, bool with_mirror) -> int { return launch_trace_kernel(s, S, C, trace_fn, Wt[i & 1], pixels, kc_of(i), level, on, with_mirror); };
    auto shade = [&](int i, hipStream_t on) -> int {
        hipLaunchKernelGGL(sq_shade1<SRC>, grid_of(kc_of(i)), dim3(kBlock), 0, on, S, F, Wt[i & 1], kc_of(i));
        return launched();
    };
    auto accumulate = [&](int i, hipStream_t on, bool last) -> int {     // in batch order: the per-pixel sum is ordered (src/Lib.hs:88)
        hipLaunchKernelGGL(accumulate_kernel, dim3(aux_blocks), dim3(kBlock), 0, on, S, F, Wt[i & 1], kc_of(i), last ? 1 : 0);
        return launched();
    };
    // Once per frame, on the caller's stream: the depth-0 mirror ray of every active pixel (reused by every sample that mirrors),
    // generated into the slots from `base` on and, once traced, stored per pixel.
    auto mirror_gen = [&](long long base) -> int {
        hipLaunchKernelGGL(sq_mirror1_gen<SRC>, dim3(aux_blocks), dim3(kBlock), 0, stream, S, F, W, base);
        return launched();
    };
    auto mirror_store = [&](long long base) -> int {
        hipLaunchKernelGGL(sq_mirror1_store, dim3(aux_blocks), dim3(kBlock), 0, stream, W, base);
        return launched();
    };
    // Where the mirror rays ride (Schedule::mirror_rides): in front of batch 0, level 0 (slots behind the sample slots of both tracks,
    // dequeued first) instead of having a launch, and a ramp-down, of their own.
    const long long front = (long long)W.slot_capacity;
    if (Sch.kind == kSchedSerial) {
        // Plain schedule: everything on the caller's stream, batch after batch.
        for (int i = 0; i < n_real; ++i) {
            if (gen(i, stream)) return 1;
            if (i == 0 && mirror_gen(front)) return 1;
            if (trace(i, 0, stream, i == 0)) return 1;
            if (i == 0 && mirror_store(front)) return 1;
            if (shade(i, stream) || trace(i, 1, stream, false) || accumulate(i, stream, i == n_real - 1)) return 1;
        }
        return 0;
    }
    // The overlapped schedules a caller asks for give the mirror rays a launch of their own, before the tracks split.
    if (!Sch.mirror_rides) {
        SQ_HIP(hipMemsetAsync(W.head[0], 0, 32 * sizeof(int32_t), stream));
        if (mirror_gen(0) || launch_trace_kernel(s, S, C, trace_fn, W, pixels, 1, 0, stream, false) || mirror_store(0)) return 1;
    }
    if (!s->aux) {
        // The second stream carries the per-sample kernels (overlap 1) or the odd batches (overlap 2).  Lowest priority: when a
        // trace launch and a per-sample kernel become ready together, the trace workgroups (one per CU, all of its LDS) must be
        // placed first and the per-sample blocks fill the wave slots beside them; the other way round the trace workgroups wait
        // for whole CUs to drain (rocprofv3 timeline, profiles/r03c_timeline_clocks_coresidency.txt).
        int least = 0, greatest = 0;
        SQ_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
        if (s->opt.aux_low_priority) SQ_HIP(hipStreamCreateWithPriority(&s->aux, hipStreamNonBlocking, least));    // `least` = numerically largest = lowest priority
        else SQ_HIP(hipStreamCreateWithFlags(&s->aux, hipStreamNonBlocking));
    }
    const hipStream_t X = s->aux;
    size_t next_event = 0;
    auto new_event = [&](hipEvent_t* e) -> int {
        if (next_event == s->events.size()) { hipEvent_t n; SQ_HIP(hipEventCreateWithFlags(&n, hipEventDisableTiming)); s->events.push_back(n); }
        *e = s->events[next_event++];
        return 0;
    };
    if (Sch.kind == kSchedPipelines) {
        // Two pipelines: even batches run start to end on the caller's stream, odd batches on the second stream.  A trace
        // launch needs a whole CU's LDS per workgroup, so the two tracks' launches do not share CUs: the later one's
        // workgroups move in as the earlier one's finish, which fills the ramp-down of every launch (a ray takes
        // 150-300 us from fetch to hit, and a launch ends when its slowest rays do) and overlaps the per-sample kernels
        // of one track with the trace launches of the other.  Only the accumulation is ordered across tracks (src/Lib.hs:88) -- and,
        // where the mirror rays ride with batch 0, the second track's first shading behind their store: sq_shade1 reads the per-pixel
        // mirror hit, sq_gen_bounce1 and the trace launches do not.  A track's later batches never dequeue the front slots again.
        std::vector<hipEvent_t> eAcc((size_t)n_real);
        for (int i = 0; i < n_real; ++i) if (new_event(&eAcc[(size_t)i])) return 1;
        hipEvent_t e_setup2, e_done2, e_mirror = nullptr;
        if (new_event(&e_setup2) || new_event(&e_done2) || (Sch.mirror_rides && new_event(&e_mirror))) return 1;
        SQ_HIP(hipEventRecord(e_setup2, stream));
        SQ_HIP(hipStreamWaitEvent(X, e_setup2, 0));
        for (int i = 0; i < n_real; ++i) {
            const hipStream_t on = (i & 1) ? X : stream;
            const bool ride = Sch.mirror_rides && i == 0;                // batch 0 is on the caller's stream, as the mirror kernels are
            if (gen(i, on)) return 1;
            if (ride && mirror_gen(front)) return 1;
            if (trace(i, 0, on, ride)) return 1;
            if (ride) {
                if (mirror_store(front)) return 1;
                SQ_HIP(hipEventRecord(e_mirror, stream));
            }
            if (Sch.mirror_rides && i == 1) SQ_HIP(hipStreamWaitEvent(X, e_mirror, 0));
            if (shade(i, on) || trace(i, 1, on, false)) return 1;
            if (i > 0) SQ_HIP(hipStreamWaitEvent(on, eAcc[(size_t)i - 1], 0));
            if (accumulate(i, on, i == n_real - 1)) return 1;
            SQ_HIP(hipEventRecord(eAcc[(size_t)i], on));
        }
        SQ_HIP(hipEventRecord(e_done2, X));
        SQ_HIP(hipStreamWaitEvent(stream, e_done2, 0));
        return 0;
    }
    // Overlap 1: the trace launches on the caller's stream, the per-sample kernels on X.  The four events of a batch: G = its rays are
    // generated, T1 / T2 = a trace level is done, S1 = ray 2 is in the slots
    std::vector<hipEvent_t> eG((size_t)n_real), eT1((size_t)n_real), eS1((size_t)n_real), eT2((size_t)n_real);
    for (int i = 0; i < n_real; ++i) if (new_event(&eG[(size_t)i]) || new_event(&eT1[(size_t)i]) || new_event(&eS1[(size_t)i]) || new_event(&eT2[(size_t)i])) return 1;
    hipEvent_t e_setup, e_done;
    if (new_event(&e_setup) || new_event(&e_done)) return 1;
    SQ_HIP(hipEventRecord(e_setup, stream));
    SQ_HIP(hipStreamWaitEvent(X, e_setup, 0));
    auto gen_x = [&](int i) -> int {
        if (gen(i, X)) return 1;
        SQ_HIP(hipEventRecord(eG[(size_t)i], X));
        return 0;
    };
    auto trace_s = [&](int i, int level) -> int {
        SQ_HIP(hipStreamWaitEvent(stream, level == 0 ? eG[(size_t)i] : eS1[(size_t)i], 0));
        if (trace(i, level, stream, false)) return 1;
        SQ_HIP(hipEventRecord(level == 0 ? eT1[(size_t)i] : eT2[(size_t)i], stream));
        return 0;
    };
    auto shade_x = [&](int i) -> int {
        SQ_HIP(hipStreamWaitEvent(X, eT1[(size_t)i], 0));
        if (shade(i, X)) return 1;
        SQ_HIP(hipEventRecord(eS1[(size_t)i], X));
        return 0;
    };
    auto finish_x = [&](int i) -> int {
        SQ_HIP(hipStreamWaitEvent(X, eT2[(size_t)i], 0));
        if (accumulate(i, X, i == n_real - 1)) return 1;
        return i + 2 < n_real ? gen_x(i + 2) : 0;              // the track is free again
    };
    if (gen_x(0)) return 1;
    if (n_real > 1 && gen_x(1)) return 1;
    for (int a = 0; a < n_real; a += 2) {
        const int b = a + 1 < n_real ? a + 1 : -1;
        if (trace_s(a, 0)) return 1;
        if (b >= 0 && trace_s(b, 0)) return 1;
        if (shade_x(a)) return 1;
        if (b >= 0 && shade_x(b)) return 1;
        if (trace_s(a, 1)) return 1;
        if (b >= 0 && trace_s(b, 1)) return 1;
        if (finish_x(a)) return 1;
        if (b >= 0 && finish_x(b)) return 1;
    }
    SQ_HIP(hipEventRecord(e_done, X));
    SQ_HIP(hipStreamWaitEvent(stream, e_done, 0));
    return 0;
}

}  // namespace

namespace {
// (the largest frames a call takes, kMaxCallPixels / kMaxWavefrontPixels, and refuse_frame_size: sq_plan.h; ranges_overlap, NamedRange
// and refuse_overlaps: sq_call_checks.h)
// The camera and shard fields of the frame of a shard of `rows` local rows.
void set_camera(Frame& F, const sq_camera* cam, int32_t w, int32_t h, sq_shard sh, int32_t rows) {
    std::memcpy(F.cam_pos, cam->pos, sizeof F.cam_pos);
    std::memcpy(F.cam_rot, cam->rot, sizeof F.cam_rot);
    F.w = w; F.h = h; F.row_block = sh.row_block; F.shard = sh.shard; F.n_shards = sh.n_shards; F.local_rows = rows;
}
// Every render entry point: the samples [k_begin, k_end) of the `samples`-sample frame of n_views cameras (view-major buffers).  d_sum =
// nullptr (sq_render_rows_device) keeps the fold in the workspace; the caller has checked everything that is specific to its own entry
// point.  One camera takes the single-view kernels; more take their multi-view instantiations and the scene's camera table.
int render_rows(sq_device_scene* s, const sq_camera* cam, int32_t n_views, int32_t samples, int32_t w, int32_t h, int32_t cast, sq_shard sh,
                int32_t k_begin, int32_t k_end, float* d_sum, float* d_avg, uint8_t* d_rgb, void* hip_stream,
                const uint8_t* d_mask = nullptr, float* d_sum2 = nullptr, int32_t* d_count = nullptr) {
    if (!s || !cam) return sq_set_error("null argument");
    if (samples < 1 || w < 1 || h < 1) return sq_set_error("samples, width and height must be positive (got %d, %d, %d)", samples, w, h);
    const int32_t rows = sq_shard_rows(w, sh);
    if (rows < 0) return sq_set_error("bad shard {row_block=%d, shard=%d, n_shards=%d}", sh.row_block, sh.shard, sh.n_shards);
    if (rows == 0) return 0;                    // an empty shard (more shards than row blocks) has nothing to render
    if (!d_avg && !d_rgb && !d_sum) return sq_set_error("no output buffer");
    if (refuse_frame_size(n_views, rows, h, s->opt.variant != 1 && (!cast || s->opt.cast_wavefront))) return 1;   // before any 32-bit product of rows and h, and before the device is touched
    if (d_mask || d_sum2 || d_count) {   // a masked call: no two of its buffers may overlap (a live pixel's stores would be another pixel's mask, count or fold)
        const size_t px = (size_t)rows * (size_t)h;
        const NamedRange b[6] = { { "d_mask", d_mask, px }, { "d_sum", d_sum, px * 12 }, { "d_sum2", d_sum2, px * 12 }, { "d_count", d_count, px * 4 },
                                  { "d_avg", d_avg, px * 12 }, { "d_rgb", d_rgb, px * 3 } };
        if (refuse_overlaps(b, 6)) return 1;
    }
    SQ_HIP(hipSetDevice(s->device));
    Frame F{};
    set_camera(F, cam, w, h, sh, rows);
    F.samples = samples; F.cast = cast ? 1 : 0;
    {   // primary-ray tiles: as tall as the adjacency of local rows allows (8 x 8 on a whole image, 2 x 32 with blocks of 2 rows)
        const int rb = sh.n_shards <= 1 ? 8 : sh.row_block;
        F.tile_rows = rb >= 8 && rb % 8 == 0 ? 8 : rb >= 4 && rb % 4 == 0 ? 4 : rb >= 2 && rb % 2 == 0 ? 2 : 1;
        if (s->opt.primary_tiles == 0) F.tile_rows = 1;
        const int tw = 64 / F.tile_rows;
        F.tiles_x = (h + tw - 1) / tw;
    }
    F.out_avg = d_avg; F.out_rgb = d_rgb;
    F.k_begin = k_begin; F.k_end = k_end; F.sum = d_sum;
    F.diag = s->opt.coresidency ? std::max(1, s->n_cu - 8) : 0;   // "beside" = while all but a handful of the CUs hold a live trace workgroup
    F.n_views = n_views; F.view_pixels = rows * h; F.cams = nullptr;
    F.mask = d_mask; F.sum2 = d_sum2; F.count = d_count;
    hipStream_t stream = (hipStream_t)hip_stream;
    if (n_views == 1) return s->small_index ? launch_frame<uint16_t, kSrcCamera>(s, F, stream, nullptr) : launch_frame<uint32_t, kSrcCamera>(s, F, stream, nullptr);
    if (ensure_cam_table(s, n_views)) return 1;
    F.cams = s->d_cams;
    return s->small_index ? launch_frame<uint16_t, kSrcViews>(s, F, stream, cam) : launch_frame<uint32_t, kSrcViews>(s, F, stream, cam);
}
}  // namespace

extern "C" int sq_render_rows_device(sq_device_scene* s, const sq_camera* cam, int32_t samples, int32_t w, int32_t h,
                                     int32_t cast, sq_shard sh, float* d_avg, uint8_t* d_rgb, void* hip_stream) {
    return render_rows(s, cam, 1, samples, w, h, cast, sh, 0, samples, nullptr, d_avg, d_rgb, hip_stream);
}

extern "C" int sq_render_rows_device_range(sq_device_scene* s, const sq_camera* cam, int32_t samples, int32_t w, int32_t h,
                                           int32_t cast, sq_shard sh, int32_t k_begin, int32_t k_end,
                                           float* d_sum, float* d_avg, uint8_t* d_rgb, void* hip_stream) {
    return sq_render_rows_device_masked(s, cam, samples, w, h, cast, sh, k_begin, k_end, nullptr, d_sum, nullptr, nullptr, d_avg, d_rgb, hip_stream);
}

// The range call is this call without a mask, second moments and counts.
extern "C" int sq_render_rows_device_masked(sq_device_scene* s, const sq_camera* cam, int32_t samples, int32_t w, int32_t h,
                                            int32_t cast, sq_shard sh, int32_t k_begin, int32_t k_end,
                                            const uint8_t* d_mask, float* d_sum, float* d_sum2, int32_t* d_count,
                                            float* d_avg, uint8_t* d_rgb, void* hip_stream) {
    if (k_begin < 0 || k_end <= k_begin || k_end > samples)
        return sq_set_error("bad sample range [%d, %d) of a %d-sample frame (need 0 <= k_begin < k_end <= samples)", k_begin, k_end, samples);
    if (!d_sum) return sq_set_error("d_sum is required: it carries the per-pixel fold from one range call to the next");
    if ((void*)d_sum == (void*)d_avg) return sq_set_error("d_sum and d_avg must be different buffers");
    return render_rows(s, cam, 1, samples, w, h, cast, sh, k_begin, k_end, d_sum, d_avg, d_rgb, hip_stream, d_mask, d_sum2, d_count);
}

extern "C" int sq_adaptive_update_device(sq_device_scene* s, int64_t n_pixels, const float* d_sum, const float* d_sum2,
                                         const int32_t* d_count, float tol, float eps,
                                         uint8_t* d_mask, int32_t* d_live, void* hip_stream) {
    if (n_pixels < 0) return sq_set_error("n_pixels must not be negative (got %lld)", (long long)n_pixels);
    if (!(tol >= 0.0f) || !(eps >= 0.0f)) return sq_set_error("tol and eps must be numbers >= 0 (got %g, %g)", (double)tol, (double)eps);
    if (!s || !d_sum || !d_sum2 || !d_count || !d_mask || !d_live) return sq_set_error("null argument");
    // one thread per pixel in one launch of whole workgroups, and a launch has at most 2^32 - 1 threads; the kernel itself is 64-bit throughout
    if (n_pixels > 0xffffffffLL / kBlock * kBlock) return sq_set_error("too many pixels for one launch (%lld; at most 2^32 - 256)", (long long)n_pixels);
    const long long blocks = ((long long)n_pixels + kBlock - 1) / kBlock;
    SQ_HIP(hipSetDevice(s->device));
    hipStream_t stream = (hipStream_t)hip_stream;
    SQ_HIP(hipMemsetAsync(d_live, 0, sizeof(int32_t), stream));
    if (blocks == 0) return 0;
    hipLaunchKernelGGL(sq_adaptive_update, dim3((unsigned)blocks), dim3(kBlock), 0, stream, (long long)n_pixels, d_sum, d_sum2, d_count, tol, eps, d_mask, d_live);
    SQ_HIP(hipGetLastError());
    return 0;
}

extern "C" int sq_render_views_device(sq_device_scene* s, const sq_camera* cams, int32_t n_views, int32_t samples, int32_t w, int32_t h,
                                      int32_t cast, sq_shard sh, int32_t k_begin, int32_t k_end,
                                      float* d_sum, float* d_avg, uint8_t* d_rgb, void* hip_stream) {
    if (!s) return sq_set_error("null argument");
    if (!cams) return sq_set_error("cams is NULL");
    if (n_views < 1) return sq_set_error("n_views must be at least 1 (got %d)", n_views);
    if (k_begin < 0 || k_end <= k_begin || k_end > samples)
        return sq_set_error("bad sample range [%d, %d) of a %d-sample frame (need 0 <= k_begin < k_end <= samples)", k_begin, k_end, samples);
    if (!d_sum && (k_begin != 0 || k_end != samples))
        return sq_set_error("d_sum is required for a part [%d, %d) of a %d-sample frame: it carries the per-pixel fold", k_begin, k_end, samples);
    if (d_sum && (void*)d_sum == (void*)d_avg) return sq_set_error("d_sum and d_avg must be different buffers");
    const int32_t rows = sq_shard_rows(w, sh);
    if (refuse_frame_size(n_views, rows, h, false)) return 1;          // pixel indices (px_pixel) are 32-bit; render_rows adds the wavefront form's limit
    return render_rows(s, cams, n_views, samples, w, h, cast, sh, k_begin, k_end, d_sum, d_avg, d_rgb, hip_stream);
}

namespace {
// The query's rays [c0, c0 + m).
RayQuery query_part(const RayQuery& Q, long long c0, long long m) {
    RayQuery C = Q;
    C.org += 3 * c0; C.dir += 3 * c0; C.tri += c0;
    if (C.dist) C.dist += c0;
    if (C.point) C.point += 3 * c0;
    C.n = m;
    return C;
}
// sq_intersect_rays_device once its arguments are checked (Q.n > 0).  Plans like a frame (plan_call: s->plan, the same LDS refusals), then
// variant 1 runs the per-lane kernel and the default form runs chunks of stage -> one level of the trace kernel -> store.
template <typename StackT>
int intersect_rays(sq_device_scene* s, const RayQuery& Q, hipStream_t stream) {
    Call call;
    call.query = true; call.n_rays = Q.n;
    CallPlan C;
    if (begin_call(s, plan_inputs(s, call, (int)sizeof(StackT)), C)) return 1;
    sq_plan& P = s->plan;
    const SceneView S = call_view(s, C);
    if (C.path == kPathQueryLanes) {
        const size_t px_lds = C.px_lds;
        if (px_lds > 64 * 1024) SQ_HIP(hipFuncSetAttribute((const void*)sq_intersect_lanes<StackT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)px_lds));
        P.launched = 1;
        for (long long c0 = 0; c0 < Q.n; c0 += kLaneChunk) {
            const RayQuery Qc = query_part(Q, c0, std::min(kLaneChunk, Q.n - c0));
            if (timed_launch(s, [&] { hipLaunchKernelGGL(sq_intersect_lanes<StackT>, dim3((unsigned)((Qc.n + kBlock - 1) / kBlock)), dim3(kBlock), px_lds, stream, S, Qc); },
                             "sq_intersect_lanes", stream)) return 1;
        }
        return 0;
    }
    const void* const trace_fn = trace_kernel<StackT>(C);
    if (prepare_trace<StackT, kSrcCamera>(C, trace_fn)) return 1;
    if (ensure_workspace(s, C.pixels, C.slots, stream)) return 1;
    const Work& W = s->work;
    const long long chunk = plan_schedule(C, W.slot_capacity).query_chunk;
    Work Wq = W; Wq.n_active = W.n_active + 48;                         // the launch's queue length, written by sq_rays_stage
    P.launched = 1;                                                    // planned; what follows fails only on HIP errors
    for (long long c0 = 0; c0 < Q.n; c0 += chunk) {
        const RayQuery Qc = query_part(Q, c0, std::min(chunk, Q.n - c0));
        const dim3 grid((unsigned)std::min<long long>((Qc.n + kBlock - 1) / kBlock, (long long)s->n_cu * 8));
        SQ_HIP(hipMemsetAsync(W.head[0], 0, 32 * sizeof(int32_t), stream));     // both dequeue cursors
        hipLaunchKernelGGL(sq_rays_stage, grid, dim3(kBlock), 0, stream, Qc, W);
        SQ_HIP(hipGetLastError());
        if (launch_trace_kernel(s, S, C, trace_fn, Wq, Qc.n, 1, 0, stream, false)) return 1;
        hipLaunchKernelGGL(sq_rays_store, grid, dim3(kBlock), 0, stream, Qc, W);
        SQ_HIP(hipGetLastError());
    }
    return 0;
}
}  // namespace

extern "C" int sq_intersect_rays_device(sq_device_scene* s, const float* d_org, const float* d_dir, int64_t n,
                                        int32_t* d_tri, float* d_dist, float* d_point, void* hip_stream) {
    if (!s) return sq_set_error("null argument");
    if (n < 0) return sq_set_error("n must be >= 0 (got %lld)", (long long)n);
    if (n == 0) return 0;
    if (!d_org || !d_dir || !d_tri) return sq_set_error("d_org, d_dir and d_tri are required");
    if (n > (INT64_MAX / 12)) return sq_set_error("%lld rays are too many", (long long)n);
    const size_t n3 = (size_t)n * 12, n1 = (size_t)n * 4;
    const NamedRange r[5] = { { "d_org", d_org, n3 }, { "d_dir", d_dir, n3 }, { "d_tri", d_tri, n1 }, { "d_dist", d_dist, n1 }, { "d_point", d_point, n3 } };
    if (refuse_overlaps(r, 5)) return 1;
    SQ_HIP(hipSetDevice(s->device));
    const RayQuery Q{ d_org, d_dir, d_tri, d_dist, d_point, (long long)n };
    hipStream_t stream = (hipStream_t)hip_stream;
    return s->small_index ? intersect_rays<uint16_t>(s, Q, stream) : intersect_rays<uint32_t>(s, Q, stream);
}

extern "C" int sq_camera_rays_device(sq_device_scene* s, const sq_camera* cam, int32_t w, int32_t h, sq_shard sh,
                                     float* d_org, float* d_dir, void* hip_stream) {
    if (!s || !cam || !d_org || !d_dir) return sq_set_error("null argument");
    if (w < 1 || h < 1) return sq_set_error("width and height must be positive (got %d, %d)", w, h);
    const int32_t rows = sq_shard_rows(w, sh);
    if (rows < 0) return sq_set_error("bad shard {row_block=%d, shard=%d, n_shards=%d}", sh.row_block, sh.shard, sh.n_shards);
    if (rows == 0) return 0;                    // an empty shard has no pixels
    const long long total = (long long)rows * h;
    if (ranges_overlap(d_org, (size_t)total * 12, d_dir, (size_t)total * 12)) return sq_set_error("d_org and d_dir overlap");
    SQ_HIP(hipSetDevice(s->device));
    Frame F{};
    set_camera(F, cam, w, h, sh, rows);
    const dim3 grid((unsigned)std::min<long long>((total + kBlock - 1) / kBlock, (long long)s->n_cu * 8));
    hipLaunchKernelGGL(sq_camera_rays, grid, dim3(kBlock), 0, (hipStream_t)hip_stream, F, d_org, d_dir, total);
    SQ_HIP(hipGetLastError());
    return 0;
}

// ----------------------------------------------------------------------------------------------
// Radiance queries (sq_raytrace_rays_device, sq_raycast_rays_device): raytrace / raycast of caller-given rays, src/Lib.hs:127-151
// ----------------------------------------------------------------------------------------------
namespace {
// A query's arrays: n rays, [n][3] floats for origin, direction, sum (raycast: the radiance), avg and [n][3] bytes for rgb; seed [n].
struct RadianceQuery {
    const float* org; const float* dir; const long long* seed;
    float* sum; float* avg; uint8_t* rgb;
    long long n;
};
// The query's rays [c0, c0 + m): all six arrays advance together (elements, not bytes).
RadianceQuery radiance_part(const RadianceQuery& Q, long long c0, long long m) {
    RadianceQuery C = Q;
    C.org += 3 * c0; C.dir += 3 * c0; C.sum += 3 * c0;
    if (C.seed) C.seed += c0;
    if (C.avg) C.avg += 3 * c0;
    if (C.rgb) C.rgb += 3 * c0;
    C.n = m;
    return C;
}
// A checked query (Q.n > 0): chunk by chunk a ray-source frame through launch_frame -- its plan, refusals, forms and schedules.  Every
// chunk has the same plan, and the first is the largest, so a refusal comes from the first chunk, before anything is enqueued.
template <typename StackT>
int radiance_rays(sq_device_scene* s, const RadianceQuery& Q, int32_t k_begin, int32_t k_end, bool cast, hipStream_t stream) {
    const long long chunk = radiance_chunk_rays(Q.n, s->opt.slots, s->opt.variant != 1 && (!cast || s->opt.cast_wavefront));
    for (long long c0 = 0; c0 < Q.n; c0 += chunk) {
        const RadianceQuery C = radiance_part(Q, c0, std::min(chunk, Q.n - c0));
        RayFrame F{};
        F.samples = k_end; F.w = 1; F.h = (int32_t)C.n; F.cast = cast ? 1 : 0;
        F.row_block = 1; F.shard = 0; F.n_shards = 1; F.local_rows = 1;
        F.tile_rows = 1; F.tiles_x = (int32_t)((C.n + 63) / 64);          // primary_padded: the chunk padded to whole waves
        F.out_avg = C.avg; F.out_rgb = C.rgb;
        F.k_begin = k_begin; F.k_end = k_end; F.sum = C.sum;
        F.diag = s->opt.coresidency ? std::max(1, s->n_cu - 8) : 0;
        F.n_views = 1; F.view_pixels = (int32_t)C.n; F.cams = nullptr;
        F.ray_org = C.org; F.ray_dir = C.dir; F.ray_seed = C.seed;
        if (launch_frame<StackT, kSrcRays>(s, F, stream, nullptr)) return 1;
    }
    return 0;
}
}  // namespace

extern "C" int sq_raytrace_rays_device(sq_device_scene* s, const float* d_org, const float* d_dir, const int64_t* d_seed, int64_t n,
                                       int32_t k_begin, int32_t k_end,
                                       float* d_sum, float* d_avg, uint8_t* d_rgb, void* hip_stream) {
    if (!s) return sq_set_error("null argument");
    if (n < 0) return sq_set_error("n must be >= 0 (got %lld)", (long long)n);
    if (k_begin < 0 || k_end <= k_begin) return sq_set_error("bad sample range [%d, %d) (need 0 <= k_begin < k_end)", k_begin, k_end);
    if (n == 0) return 0;
    if (!d_org || !d_dir || !d_seed || !d_sum) return sq_set_error("d_org, d_dir, d_seed and d_sum are required");
    if (n > (INT64_MAX / 12)) return sq_set_error("%lld rays are too many", (long long)n);
    const size_t n3 = (size_t)n * 12;
    const NamedRange r[6] = { { "d_org", d_org, n3 }, { "d_dir", d_dir, n3 }, { "d_seed", d_seed, (size_t)n * 8 },
                              { "d_sum", d_sum, n3 }, { "d_avg", d_avg, n3 }, { "d_rgb", d_rgb, (size_t)n * 3 } };
    if (refuse_overlaps(r, 6)) return 1;
    SQ_HIP(hipSetDevice(s->device));
    static_assert(sizeof(long long) == sizeof(int64_t), "seed bases are 64-bit");
    const RadianceQuery Q{ d_org, d_dir, (const long long*)d_seed, d_sum, d_avg, d_rgb, (long long)n };
    hipStream_t stream = (hipStream_t)hip_stream;
    return s->small_index ? radiance_rays<uint16_t>(s, Q, k_begin, k_end, false, stream) : radiance_rays<uint32_t>(s, Q, k_begin, k_end, false, stream);
}

extern "C" int sq_raycast_rays_device(sq_device_scene* s, const float* d_org, const float* d_dir, int64_t n,
                                      float* d_rad, void* hip_stream) {
    if (!s) return sq_set_error("null argument");
    if (n < 0) return sq_set_error("n must be >= 0 (got %lld)", (long long)n);
    if (n == 0) return 0;
    if (!d_org || !d_dir || !d_rad) return sq_set_error("d_org, d_dir and d_rad are required");
    if (n > (INT64_MAX / 12)) return sq_set_error("%lld rays are too many", (long long)n);
    const size_t n3 = (size_t)n * 12;
    const NamedRange r[3] = { { "d_org", d_org, n3 }, { "d_dir", d_dir, n3 }, { "d_rad", d_rad, n3 } };
    if (refuse_overlaps(r, 3)) return 1;
    SQ_HIP(hipSetDevice(s->device));
    const RadianceQuery Q{ d_org, d_dir, nullptr, d_rad, nullptr, nullptr, (long long)n };
    hipStream_t stream = (hipStream_t)hip_stream;
    return s->small_index ? radiance_rays<uint16_t>(s, Q, 0, 1, true, stream) : radiance_rays<uint32_t>(s, Q, 0, 1, true, stream);
}

extern "C" int sq_scene_set_lights(sq_device_scene* s, const sq_light* lights, int32_t n_lights, void* hip_stream) {
    if (!s) return sq_set_error("null argument");
    if (n_lights < 0) return sq_set_error("n_lights must be >= 0 (got %d)", n_lights);
    if (n_lights > kMaxLights) return sq_set_error("%d lights are too many (at most %d)", n_lights, kMaxLights);
    if (n_lights > 0 && !lights) return sq_set_error("lights is NULL with n_lights = %d", n_lights);
    if (n_lights == 0 && lights) return sq_set_error("n_lights is 0 with lights given (NULL and 0 restore the reference's light)");
    SQ_HIP(hipSetDevice(s->device));
    if (ensure_light_table(s)) return 1;
    std::vector<sq_light> v;
    if (n_lights > 0) v.assign(lights, lights + n_lights);
    else v.assign(1, sq_light{ { 0.0f, 3.0f, -1.0f }, { 2.0f, 2.0f, 2.0f } });   // src/Lib.hs:141-151
    if (stage_lights(s, v, (hipStream_t)hip_stream)) return 1;
    s->lights.swap(v);
    s->lights_set = n_lights > 0; s->lights_staged = true;
    return 0;
}
extern "C" int32_t sq_scene_get_lights(sq_device_scene* s, sq_light* out, int32_t cap) {
    if (!s) { sq_set_error("null argument"); return -1; }
    const int32_t n = (int32_t)s->lights.size();
    if (out && cap > 0) std::memcpy(out, s->lights.data(), (size_t)std::min(n, cap) * sizeof(sq_light));
    return n;
}

extern "C" int sq_scene_set_depth(sq_device_scene* s, int32_t depth) {
    if (!s) return sq_set_error("null argument");
    if (depth < 1 || depth > kMaxDepth) return sq_set_error("depth must be in 1..%d (got %d)", kMaxDepth, depth);
    s->depth = depth;
    return 0;
}
extern "C" int32_t sq_scene_get_depth(sq_device_scene* s) {
    if (!s) { sq_set_error("null argument"); return -1; }
    return s->depth;
}

extern "C" int sq_scene_set_sky(sq_device_scene* s, const sq_sky* sky) {
    if (!s) return sq_set_error("null argument");
    if (sky) s->sky = *sky;
    s->sky_set = sky != nullptr;
    return 0;
}
extern "C" int sq_scene_get_sky(sq_device_scene* s, sq_sky* out) {
    if (!s) { sq_set_error("null argument"); return -1; }
    if (s->sky_set && out) *out = s->sky;
    return s->sky_set ? 1 : 0;
}

extern "C" int64_t sq_scene_rng_table(sq_device_scene* s, int64_t first, int64_t count, uint32_t* out_words) {
    if (!s) { sq_set_error("null argument"); return -1; }
    const int64_t cover = s->rng.words ? s->rng.cover : 0;
    if (count == 0) return cover;
    if (!out_words || first < 0 || count < 0 || first > cover || count > cover - first) {
        sq_set_error("entries [%lld, %lld + %lld) are not in the scene's table of %lld seeds", (long long)first, (long long)first, (long long)count, (long long)cover);
        return -1;
    }
    if (hipSetDevice(s->device) != hipSuccess || hipEventSynchronize(s->rng.filled) != hipSuccess ||
        hipMemcpy(out_words, s->rng.words + 3 * first, (size_t)count * 12, hipMemcpyDeviceToHost) != hipSuccess) {
        sq_set_error("copying the table's entries failed: %s", hipGetErrorString(hipGetLastError()));
        return -1;
    }
    return cover;
}

extern "C" int sq_kernel_timing(sq_device_scene* s, double* avg_ms, int64_t* launches, const char** name) {
    if (!s) return sq_set_error("null argument");
    SQ_HIP(hipSetDevice(s->device));
    for (auto& p : s->pending) {
        SQ_HIP(hipEventSynchronize(p.second));
        float ms = 0;
        SQ_HIP(hipEventElapsedTime(&ms, p.first, p.second));
        s->total_ms += ms; s->launches++;
        (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second);
    }
    s->pending.clear();
    if (avg_ms) *avg_ms = s->launches ? s->total_ms / (double)s->launches : 0.0;
    if (launches) *launches = s->launches;
    if (name) *name = s->last_kernel;
    return 0;
}
extern "C" int sq_last_plan(sq_device_scene* s, sq_plan* out) {
    if (!s || !out) return sq_set_error("null argument");
    if (!s->has_plan) return sq_set_error("the scene has not planned a frame yet");
    *out = s->plan;
    return 0;
}
extern "C" void sq_kernel_timing_reset(sq_device_scene* s) {
    if (!s) return;
    for (auto& p : s->pending) { (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second); }
    s->pending.clear(); s->total_ms = 0; s->launches = 0;
}
extern "C" int sq_get_stats(sq_device_scene* s, uint64_t* out, int32_t n, int32_t reset) {
    if (!s || !out || n < 0 || n > kStatSlots) return sq_set_error("bad argument");
    for (int i = 0; i < n; ++i) out[i] = 0;
    if (!s->d_work) return 0;
    SQ_HIP(hipSetDevice(s->device));
    SQ_HIP(hipDeviceSynchronize());
    SQ_HIP(hipMemcpy(out, s->work.stats, (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (reset) SQ_HIP(hipMemset(s->work.stats, 0, kStatSlots * sizeof(uint64_t)));
    return 0;
}
extern "C" int sq_set_option(sq_device_scene* s, const char* key, int64_t value) {
    if (!s || !key) return sq_set_error("null argument");
    if (set_option(s->opt, key, value)) return 1;                       // names, ranges and messages: the option table (sq_plan_call.h)
    // "aux_low_priority" takes effect when the second stream is created (first overlapped frame)
    if (!std::strcmp(key, "aux_low_priority") && s->aux) { (void)hipStreamSynchronize(s->aux); (void)hipStreamDestroy(s->aux); s->aux = nullptr; }
    return 0;
}

// ---- one-shot entry points (the drop-in for src/Lib.hs:73-74) ----
namespace {
// One shard of a one-shot call on one device: upload, render into a compact device buffer, copy back.
struct OneshotPart {
    int device = 0; sq_shard shard{ 1, 0, 1 };
    std::vector<float> avg; std::vector<uint8_t> rgb;
    int rc = 0; std::string error;
};
// direct_avg / direct_rgb: the caller's own image (only when this part is the whole frame, rows in order): the finished frame is
// copied straight into it -- the only step left that can fail is that copy itself -- instead of through a staging vector.
int oneshot_part(const sq_scene* scene, const sq_camera* cam, int32_t samples, int32_t w, int32_t h, int32_t cast,
                 bool want_avg, bool want_rgb, OneshotPart& P, float* direct_avg = nullptr, uint8_t* direct_rgb = nullptr) {
    const int32_t rows = sq_shard_rows(w, P.shard);
    if (rows <= 0) return 0;
    // SQ_ONESHOT_TIMING=1: host wall time of each stage of the call on stderr (what a host that binds the one-shot call pays
    // around the frame itself)
    const bool timing = std::getenv("SQ_ONESHOT_TIMING") != nullptr;
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    const auto t0 = now();
    sq_device_scene* s = nullptr;
    if (sq_scene_upload(scene, P.device, &s)) return 1;
    s->opt.rng_table_mb = 0;                    // one scene per frame: filling a table costs more than the one frame saves
    const auto t1 = now();
    auto t2 = t1, t3 = t1, t4 = t1;
    const size_t npx = (size_t)rows * (size_t)h * 3;
    float* d_avg = nullptr; uint8_t* d_rgb = nullptr; hipStream_t stream = nullptr;
    auto body = [&]() -> int {
        SQ_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        if (want_avg) SQ_HIP(hipMalloc((void**)&d_avg, npx * sizeof(float)));
        if (want_rgb) SQ_HIP(hipMalloc((void**)&d_rgb, npx));
        t2 = now();
        if (sq_render_rows_device(s, cam, samples, w, h, cast, P.shard, d_avg, d_rgb, stream)) return 1;
        SQ_HIP(hipStreamSynchronize(stream));
        t3 = now();
        // staged through private buffers so nothing is written to the caller's memory on failure
        if (want_avg) { float* dst = direct_avg; if (!dst) { P.avg.resize(npx); dst = P.avg.data(); } SQ_HIP(hipMemcpy(dst, d_avg, npx * sizeof(float), hipMemcpyDeviceToHost)); }
        if (want_rgb) { uint8_t* dst = direct_rgb; if (!dst) { P.rgb.resize(npx); dst = P.rgb.data(); } SQ_HIP(hipMemcpy(dst, d_rgb, npx, hipMemcpyDeviceToHost)); }
        t4 = now();
        return 0;
    };
    const int rc = body();
    (void)hipFree(d_avg); (void)hipFree(d_rgb);
    if (stream) (void)hipStreamDestroy(stream);
    sq_scene_free(s);
    if (timing) std::fprintf(stderr, "sq one-shot (device %d): upload %.2f ms, stream+buffers %.2f, render+sync %.2f, copy back %.2f, free %.2f\n",
                             P.device, ms(t0, t1), ms(t1, t2), ms(t2, t3), ms(t3, t4), ms(t4, now()));
    return rc;
}

// Devices a one-shot call spreads its rows over.  Default: every visible device when the frame is worth it
// (>= 2^24 samples), else device 0.  SQ_DEVICES="0,1,3" names them explicitly; an index may repeat (several
// shards on one device, which is how the threading is tested on a one-GPU box).
int oneshot_devices(int64_t total_samples, int32_t w, std::vector<int>& out) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return sq_set_error("no HIP device available (this library has no CPU fallback)");
    out.clear();
    if (const char* env = std::getenv("SQ_DEVICES")) {
        const char* p = env;
        while (*p) {
            char* end = nullptr;
            const long v = std::strtol(p, &end, 10);
            if (end == p || v < 0 || v >= ndev) return sq_set_error("SQ_DEVICES='%s': expected a comma-separated list of device indices in 0..%d", env, ndev - 1);
            out.push_back((int)v);
            p = end;
            if (*p == ',') ++p;
            else if (*p) return sq_set_error("SQ_DEVICES='%s': expected a comma-separated list of device indices in 0..%d", env, ndev - 1);
        }
        if (out.empty()) return sq_set_error("SQ_DEVICES is empty");
        if (out.size() > 64) return sq_set_error("SQ_DEVICES names more than 64 shards");
        return 0;
    }
    const int blocks = (w + kOneshotRowBlock - 1) / kOneshotRowBlock;
    const int n = total_samples >= ((int64_t)1 << 24) ? std::min(ndev, std::max(blocks, 1)) : 1;
    for (int d = 0; d < n; ++d) out.push_back(d);
    return 0;
}

// The foreign call of src/Lib.hs:73-74.  The reference host is ONE process, so this is where a node's GPUs are
// put to work for it: rows are cut into interleaved blocks of 2 (the sq_shard scheme), one host thread per
// device renders its shard, and the shards are de-interleaved into the caller's image.  No exchange between
// devices: a pixel depends only on (x, y, samples, w).
int render_oneshot(const sq_scene* scene, const sq_camera* cam, int32_t samples, int32_t w, int32_t h, int32_t cast,
                   float* out_avg, uint8_t* out_rgb) {
    if (!scene || !cam || (!out_avg && !out_rgb)) return sq_set_error("null argument");
    if (samples < 1 || w < 1 || h < 1) return sq_set_error("samples, width and height must be positive (got %d, %d, %d)", samples, w, h);
    std::vector<int> devices;
    if (oneshot_devices((int64_t)w * h * samples, w, devices)) return 1;
    const int G = (int)devices.size();
    std::vector<OneshotPart> parts((size_t)G);
    for (int g = 0; g < G; ++g) { parts[(size_t)g].device = devices[(size_t)g]; parts[(size_t)g].shard = sq_shard{ G == 1 ? w : kOneshotRowBlock, g, G }; }
    for (const OneshotPart& P : parts)                             // a shard too large for one call: refused before a scene is uploaded or a buffer allocated
        if (refuse_frame_size(1, sq_shard_rows(w, P.shard), h, !cast))
            return sq_set_error("device %d (shard %d of %d): %s", P.device, P.shard.shard, G, std::string(sq_last_error()).c_str());
    auto run = [&](OneshotPart& P) {
        P.rc = oneshot_part(scene, cam, samples, w, h, cast, out_avg != nullptr, out_rgb != nullptr, P);
        if (P.rc) P.error = sq_last_error();                      // the message is thread-local: carry it out
    };
    if (G == 1) {                                                  // one device renders every row in order: no staging, no de-interleave
        if (oneshot_part(scene, cam, samples, w, h, cast, out_avg != nullptr, out_rgb != nullptr, parts[0], out_avg, out_rgb))
            return sq_set_error("device %d (shard 0 of 1): %s", parts[0].device, std::string(sq_last_error()).c_str());
        return 0;
    }
    {
        std::vector<std::thread> threads;
        for (int g = 1; g < G; ++g) threads.emplace_back(run, std::ref(parts[(size_t)g]));
        run(parts[0]);
        for (auto& t : threads) t.join();
    }
    for (const OneshotPart& P : parts)
        if (P.rc) return sq_set_error("device %d (shard %d of %d): %s", P.device, P.shard.shard, G, P.error.c_str());
    const size_t row_px = (size_t)h * 3;
    for (const OneshotPart& P : parts) {
        const int32_t rows = sq_shard_rows(w, P.shard);
        for (int32_t j = 0; j < rows; ++j) {
            const size_t dst = (size_t)sq_shard_global_row(j, P.shard) * row_px, src = (size_t)j * row_px;
            if (out_avg) std::memcpy(out_avg + dst, P.avg.data() + src, row_px * sizeof(float));
            if (out_rgb) std::memcpy(out_rgb + dst, P.rgb.data() + src, row_px);
        }
    }
    return 0;
}

}  // namespace

extern "C" int sq_render_rgb8(const sq_scene* scene, const sq_camera* cam, int32_t samples, int32_t w, int32_t h, int32_t cast, uint8_t* out) {
    return render_oneshot(scene, cam, samples, w, h, cast, nullptr, out);
}
extern "C" int sq_render_f32(const sq_scene* scene, const sq_camera* cam, int32_t samples, int32_t w, int32_t h, int32_t cast, float* out_avg) {
    return render_oneshot(scene, cam, samples, w, h, cast, out_avg, nullptr);
}

extern "C" int sq_debug_eval(int32_t device, int32_t op, const void* a, const void* b, int64_t n, void* out) {
    if (!a || !out || n < 0 || op < 0 || op > SQ_OP_CULL_SLAB) return sq_set_error("bad argument");
    if (op == SQ_OP_DIV && !b) return sq_set_error("SQ_OP_DIV needs b");
    if (n == 0) return 0;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return sq_set_error("no such HIP device %d", device);
    SQ_HIP(hipSetDevice(device));
    const size_t in_sz = (size_t)n * (op == SQ_OP_TFGEN3 ? 8 : op == SQ_OP_TONEMAP ? 12 : op == SQ_OP_CULL_SLAB ? 36 : 4);
    const size_t out_sz = (size_t)n * (op == SQ_OP_TFGEN3 ? 12 : op == SQ_OP_TONEMAP ? 3 : 4);
    void *da = nullptr, *db = nullptr, *dout = nullptr;
    auto body = [&]() -> int {
        SQ_HIP(hipMalloc(&da, in_sz)); SQ_HIP(hipMalloc(&dout, out_sz));
        SQ_HIP(hipMemcpy(da, a, in_sz, hipMemcpyHostToDevice));
        if (op == SQ_OP_DIV) { SQ_HIP(hipMalloc(&db, in_sz)); SQ_HIP(hipMemcpy(db, b, in_sz, hipMemcpyHostToDevice)); }
        hipLaunchKernelGGL(sq_debug_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, op, da, db, (long long)n, dout);
        SQ_HIP(hipGetLastError());
        SQ_HIP(hipDeviceSynchronize());
        SQ_HIP(hipMemcpy(out, dout, out_sz, hipMemcpyDeviceToHost));
        return 0;
    };
    const int rc = body();
    (void)hipFree(da); (void)hipFree(db); (void)hipFree(dout);
    return rc;
}

extern "C" int32_t sq_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}
extern "C" int32_t sq_abi_version(void) { return SQ_ABI_VERSION; }
#ifndef SQ_BUILD_ID
#define SQ_BUILD_ID "unknown"
#endif
extern "C" const char* sq_build_id(void) { return SQ_BUILD_ID; }
extern "C" const char* sq_last_error(void) { return sq_error_buffer(); }
