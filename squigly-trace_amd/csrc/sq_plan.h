// sq_plan.h — what a render or query call decides before it touches the device, free of any HIP include: the options, the planner's
// inputs, the plan of a call (plan_call), the schedule for the slots its workspace got (plan_schedule) and the workspace's layout.
// The planner itself is plain host C++ (sq_plan_call.h): it runs, is tested (tests/test_plan.py, through sq_plan_call) and is sanitized on
// a CPU.  sq_device.hip reads every size, grid and threshold from here; the trace kernels share trace_lds_layout with the host.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/squigly_hip.h"
#include "sq_layout.h"

#ifndef SQ_HD
#if defined(__HIPCC__)
#define SQ_HD __host__ __device__ __forceinline__
#else
#define SQ_HD inline
#endif
#endif

namespace sqd {
constexpr int kBlock = 256;        // per-pixel / per-sample kernels
constexpr int kTraceBlock = 512;   // persistent trace kernel, streaming form: 8 waves share one LDS copy of the top of the tree
constexpr int kResidentBlock = 1024; // persistent trace kernel, resident form: one workgroup per CU owns the whole scene in LDS
// Slots a wave reserves from the queue per atomic (multiple of 256 for the resident form).  Every reservation stalls
// the wave for the atomic's round trip and then for the flag loads of the scan, and a sparse chunk (8 % of the slots
// are live at the second bounce level) serves only part of the idle lanes: 64 -> 128 -> 256 -> 512 slots measured
// 4340 -> 5110 -> 5520 -> 5605 Msamples/s on the headline frame (768: 5520).  The per-wave list of live slots holds
// one byte per entry, an index within its 256-slot block (512 B of LDS per wave).
// The streaming form keeps 128: its rays are 5-10x longer, and on a frame of a few spp a wave that sits on 256 slots
// at the end of the queue makes the tail longer than the stalls it saves (-7 % at 1920x1080@16).
constexpr int kChunkResident = 512, kChunkStreaming = 128;
using LiveT = uint8_t;             // a live slot's index within its chunk
constexpr int kStatSlots = 32;            // sq_get_stats
// The largest frames a call takes.  Pixel indices are 32-bit wherever they are stored (Work::px_pixel, Frame::view_pixels)
// or divided (pixel_coords), so no call takes more than INT32_MAX pixels.  The wavefront form also indexes its active-pixel list and
// its ray queue with 32-bit values that reach 3 x pixels (px_sum[3 * a]), pixels + one grid stride (the `a` loops) and twice the slots
// (the trace kernel's cursor, with the mirror rays in front): they hold while pixels <= 2^29, which is also the cap of option "slots".
constexpr int64_t kMaxCallPixels = INT32_MAX, kMaxWavefrontPixels = (int64_t)1 << 29;
constexpr long long kLaneChunk = 1ll << 30;   // rays per launch of the per-lane query kernel (2^22 workgroups)
constexpr size_t kLdsBudget = 160 * 1024;     // the LDS of one CU

// LDS carve-up of the trace kernel (bytes, all 16-B aligned), shared by host and device.
struct TraceLds { uint32_t quads, refs, verts, trix, live, tab, stack, total; };
SQ_HD TraceLds trace_lds_layout(int n_lds, bool resident, int n_verts, int n_tris, int block, int stack_cap, int stack_elem, bool pool) {
    auto al = [](uint32_t b) { return (b + 15u) & ~15u; };
    TraceLds L; uint32_t off = 0;
    L.verts = off; off += resident ? al((uint32_t)n_verts * 16u) : 0u;     // first: a vertex's LDS address is its byte offset (ResidentTris)
    L.quads = off; off += al((uint32_t)n_lds * (resident ? 32u : 48u));   // resident: 2 quads per branch; streaming: 3
    L.refs = off;  off += resident ? al((uint32_t)n_lds * 8u) : 0u;
    L.trix = off;  off += resident ? al((uint32_t)(n_tris + kTriRunPad) * 8u) : 0u;  // + zero records: get_run may read past the last triangle
    L.live = off;  off += al((uint32_t)(block / 64) * (uint32_t)(resident ? kChunkResident : kChunkStreaming) * (uint32_t)sizeof(LiveT));
    L.tab = off;   off += pool ? al((uint32_t)block) : 0u;   // pooled form: the window-head table, one byte per lane
    L.stack = off; off += al((uint32_t)block * (uint32_t)stack_cap * (uint32_t)stack_elem);
    L.total = off;
    return L;
}
// Lanes of the tiled enumeration of a frame's primary rays, padding of the edge tiles included: what primary_padded (sq_device.hip) gives
// the kernels, which keep their own copy (routing them through this one reorders the instructions of the primary-ray kernels).
inline long long primary_padded_lanes(int local_rows, int tile_rows, int tiles_x) {
    return (long long)((local_rows + tile_rows - 1) / tile_rows) * tiles_x * 64;
}

// ---- options (sq_set_option; the table of names, ranges and messages is sq_plan_call.h's kOptionTable) ----
constexpr int64_t kRngTableDefaultMb = 24576;   // option "rng_table_mb": 24 GiB = 2^31 seeds (squigly_hip.h)
// Option "auto_overlap_slots": the sample slots (pixels x samples of the call) from which a call of the three-level pipeline is planned as
// two pipelines without being asked to (plan_schedule).  Measured, DESIGN.md 4.2: profiles/r14b_auto_overlap_threshold.txt.
constexpr int64_t kAutoOverlapSlots = 1ll << 26;
struct Options {
    int64_t timing = 0, variant = 2, slots = 512ll << 20, straggler_lanes = 8, resident = 1, profile = 0, lds_node_kb = 32,
            trace_blocks_per_cu = 0, overlap = 0, rng_table_mb = kRngTableDefaultMb, cast_wavefront = 0, deep = 0, pool = 1, guided = 1,
            primary_resident = 1, cull = 1, level1_cull = 1, primary_tiles = 1, primary_pooled = 0, coresidency = 0, aux_polite = 0,
            trace_prio = 0, aux_low_priority = 1, descend_extra = 2, descend_lanes = 16, pixel_major = -1, refill_min = 12, flush_min = 40,
            aux_blocks_per_cu = 0, auto_overlap = 1, auto_overlap_slots = kAutoOverlapSlots, batches_per_track = 1, mirror_ride = 0;
};
// Sets option `key` of O: 0, or sq_set_error with the option's own message (a value outside its range) or "unknown option".
int set_option(Options& O, const char* key, int64_t value);

// ---- the planner's inputs ----
// Where a kernel's primary rays come from: the frame's camera (makeRay, src/Lib.hs:107-114), the camera table of a multi-view frame,
// or the caller's arrays.
constexpr int kSrcCamera = 0, kSrcViews = 1, kSrcRays = 2;
struct SceneScalars {       // of the packed scene (sq_pack.h)
    int32_t n_branches = 0, n_verts = 0, n_tris = 0, height = 0;
    bool has_trix = false;                   // the resident encoding exists
    int32_t stack_word = 4;                  // bytes of a stack word: 2 with small_index
    int32_t packed_leaves = 0, n_emitters = -1, nonneg_materials = 0, finite_geometry = 0, shortcut_depth = 0, level1_on = 0;
};
struct DeviceScalars { int32_t n_cu = 256; };
struct SceneState { int32_t depth = 3; bool sky_set = false, lights_set = false; int32_t n_lights = 1; };
struct Call {
    int32_t src = kSrcCamera;
    bool cast = false, masked = false, mom2 = false;   // masked: a mask, second moments or counts are given; mom2: second moments are
    int32_t n_views = 1, local_rows = 1, h = 1, tile_rows = 1, tiles_x = 1, k_begin = 0, k_end = 1;
    bool query = false; int64_t n_rays = 0;  // an intersection query of n_rays rays: the frame fields above are unread
};
struct PlanInputs { Options opt; SceneScalars scene; DeviceScalars device; SceneState state; Call call; };

// ---- the plan of a call ----
// The path a call takes: the three per-lane kernels, the three wavefront forms, and the two forms of an intersection query.
enum Path { kPathLaneCast, kPathLaneDeep, kPathLanePlain, kPathWaveCast, kPathWaveDeep, kPathPipeline, kPathQueryLanes, kPathQueryWave };
struct CallPlan {
    sq_plan plan{};               // the public part (sq_last_plan); after a refusal: what was planned up to it, launched = 0
    bool planned = false;         // false: refused for its size, before anything was planned (`plan` is empty)
    PlanInputs in;                // what the call was planned from (plan_schedule and the launch arguments read the options)
    int path = kPathLanePlain;
    bool ad = false, mom2 = false, sky = false, deep = false;
    int32_t nonneg_materials = 0, n_emitters = -1; bool cull_off = false;   // the call's overrides of the scene view
    long long pixels = 0, px_blocks = 0; size_t px_lds = 0;
    int n_call = 0;               // samples (cast: lights) the call renders
    int64_t slots = 0;            // sample slots wanted of the workspace
    int trace_form = SQ_FORM_PER_PIXEL;
    bool resident = false, pool = false, profile = false, dense = false;
    int n_lds = 0, stack_cap = 0, trace_blocks = 0, trace_threads = 0; size_t tr_lds = 0;
    long long primary_grid = 0; size_t primary_lds = 0;      // the primary pass of a wavefront frame (resident or per-lane form)
    int aux_blocks = 0; bool acc_grouped = false;
    bool level1_cull = false;
    size_t deep_slot_bytes = 0;
    bool need_lights = false, need_sum2 = false, need_deep = false, rng_table = false, rng_grow = false;
};
// Plans the call: 0, or non-zero with sq_set_error (the refusal's text).  Pure integer arithmetic; touches no device.
int plan_call(const PlanInputs& in, CallPlan& out);
// Sets the refusal of a call of n_views x rows x h pixels that is too large for its form (wavefront: not the per-pixel kernel) and
// returns non-zero; 0 when the size is fine.  Everything in 64 bits.
int refuse_frame_size(int64_t n_views, int64_t rows, int64_t h, bool wavefront);
// Rays per chunk of a radiance query of n > 0 rays: every chunk is a frame of its own, so it stays within a frame's limits -- 2^29 "pixels" and
// one sample of every pixel in the workspace's `slots` (1 .. 2^29) in the wavefront form, a launch of 2^30 lanes in the per-lane form.
// Plain 64-bit host arithmetic: chunk c covers the rays [c * chunk, min(n, (c + 1) * chunk)), the last one may be short.
long long radiance_chunk_rays(long long n, long long slots, bool wavefront);

// ---- what depends on the slots the workspace actually got (the allocation may have halved them) ----
// The schedule's kind: everything on the caller's stream; the per-sample kernels on the second stream beside the trace launches; two
// pipelines, even batches on the caller's stream and odd ones on the second.
constexpr int kSchedSerial = 0, kSchedAux = 1, kSchedPipelines = 2;
struct Schedule {
    int kind = kSchedSerial;                      // what launch_frame enqueues; overlap = kind != kSchedSerial
    bool mirror_rides = true;                     // the per-pixel mirror rays: at the head of batch 0's first trace launch, or (false) in a launch of their own
    bool overlap = false; int tracks = 1; int64_t track_slots = 0;
    int batch = 0, n_batches = 0, n_real = 0;     // samples per batch; batches the split counts; batches that hold a sample
    long long query_chunk = 0;                    // an intersection query: rays per chunk
};
Schedule plan_schedule(const CallPlan& P, int64_t have_slots);
struct Grid2 { unsigned x, y; };
// Per-sample kernels that run one thread per active pixel, for a batch of kc samples.
Grid2 pp_grid(const CallPlan& P, const Schedule& S, int kc);
// One launch of the trace kernel over queue_rays x kc slots at bounce level `level`: its reservation size and queue order.
struct TraceLaunch { int chunk, guide_shift; bool pixel_major; };
TraceLaunch trace_launch(const CallPlan& P, int64_t queue_rays, int kc, int level);

// ---- the frame workspace: byte offsets of its arrays in one block (ensure_workspace), and of the deep block's ----
struct WorkLayout { size_t cnt, stats, pix, t0, tri0, sum, mt, mtri, state, org, dir, tri1, carry, total; };
// 0, or non-zero with sq_set_error when the offsets are not strictly ordered (a slip would be a GPU fault, not an error code).
int workspace_layout(int64_t pixels, int64_t slots, WorkLayout& out);
// The bytes of Deep a slot takes under depth D: a triangle per bounce level, and from D = 4 on the x and y of the ray's origin;
// under a sky also t of the ray that missed (DeepSky::tmiss), behind the trail.
inline size_t deep_slot_bytes(int depth, bool sky) { return depth < 2 ? 0 : (size_t)(depth - 1) * 4 + (depth >= 4 ? 8 : 0) + (sky ? 4 : 0); }
struct DeepLayout { size_t oxy, trail, tmiss; bool has_tmiss; };
DeepLayout deep_layout(int depth, bool sky, long long cap);
}  // namespace sqd
