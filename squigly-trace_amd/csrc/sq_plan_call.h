// sq_plan_call.h — the call planner (sq_plan.h) and its C-ABI window, and sq_rng_table_cover (include/squigly_host.h).  A part of the
// host translation unit (sq_host.cpp, which has the file map and the includes); not a header for anything else.
//
// Seeds [0, n_cover) that a scene's table of generator words holds for a w x h frame at `samples` (squigly_host.h): what the frame
// can use -- one past its largest seed, samples * (x + y * w) + samples - 1 at x = h - 1, y = w - 1 (src/Lib.hs:85-86) -- capped by
// the budget at 12 bytes per seed.  The product is taken in 128 bits: three factors below 2^31 reach 2^93.
extern "C" int64_t sq_rng_table_cover(int32_t w, int32_t h, int32_t samples, int64_t budget_bytes) {
    if (w < 1 || h < 1 || samples < 1 || budget_bytes < 12) return 0;
    const unsigned __int128 span = (unsigned __int128)samples * ((unsigned __int128)(w - 1) * (unsigned __int128)w + (unsigned __int128)h);
    const unsigned __int128 cap = (unsigned __int128)(budget_bytes / 12);
    return (int64_t)(span < cap ? span : cap);
}

// ----------------------------------------------------------------------------------------------
// Planning (sq_plan.h): what a render or query call decides before it touches the device.  Pure integer arithmetic on the scene's
// scalars, the options, the call's shape and the device's CU count; sq_device.hip allocates and enqueues by it.
// ----------------------------------------------------------------------------------------------
namespace sqd {
namespace {
// One row per option: how sq_set_option takes a value.  kAny: as it is; kRange: refused outside [lo, hi] with `refusal`; kBool: 0 or 1;
// kSign: -1 for a negative value, else 0 or 1; kIgnored: accepted, no effect.
enum OptionKind { kAny, kRange, kBool, kSign, kIgnored };
struct OptionRow { const char* name; int64_t Options::* member; OptionKind kind; int64_t lo, hi; const char* refusal; };
const OptionRow kOptionTable[] = {
    { "timing", &Options::timing, kAny, 0, 0, nullptr },
    { "variant", &Options::variant, kRange, 1, 2, "variant must be 1 (per-pixel kernel) or 2 (wavefront)" },
    { "slots", &Options::slots, kRange, 1, 512ll << 20, "slots must be in 1..2^29" },
    { "straggler_lanes", &Options::straggler_lanes, kRange, 0, 63, "straggler_lanes must be in 0..63" },
    { "resident", &Options::resident, kBool, 0, 1, nullptr },
    { "profile", &Options::profile, kBool, 0, 1, nullptr },
    { "lds_node_kb", &Options::lds_node_kb, kRange, 0, 128, "lds_node_kb must be in 0..128" },
    { "trace_blocks_per_cu", &Options::trace_blocks_per_cu, kRange, 0, 8, "trace_blocks_per_cu must be in 0..8" },
    { "overlap", &Options::overlap, kRange, 0, 2, "overlap must be 0, 1 or 2" },
    { "rng_table_mb", &Options::rng_table_mb, kRange, 0, 1ll << 20, "rng_table_mb must be in 0..2^20" },
    { "cast_wavefront", &Options::cast_wavefront, kBool, 0, 1, nullptr },
    { "deep", &Options::deep, kBool, 0, 1, nullptr },
    { "pool", &Options::pool, kBool, 0, 1, nullptr },
    { "guided", &Options::guided, kRange, 0, 3, "guided must be in 0..3" },
    { "primary_resident", &Options::primary_resident, kBool, 0, 1, nullptr },
    { "cull", &Options::cull, kBool, 0, 1, nullptr },
    { "level1_cull", &Options::level1_cull, kBool, 0, 1, nullptr },
    { "incremental", nullptr, kIgnored, 0, 0, nullptr },   // the incremental slab test was removed
    { "primary_tiles", &Options::primary_tiles, kBool, 0, 1, nullptr },
    { "primary_pooled", &Options::primary_pooled, kBool, 0, 1, nullptr },
    { "coresidency", &Options::coresidency, kBool, 0, 1, nullptr },
    { "aux_polite", &Options::aux_polite, kRange, 0, 8, "aux_polite must be in 0..8" },
    { "trace_prio", &Options::trace_prio, kRange, 0, 3, "trace_prio must be in 0..3" },
    { "aux_low_priority", &Options::aux_low_priority, kBool, 0, 1, nullptr },   // sq_set_option also drops the second stream
    { "descend_extra", &Options::descend_extra, kRange, 0, 16, "descend_extra must be in 0..16" },
    { "descend_lanes", &Options::descend_lanes, kRange, 1, 64, "descend_lanes must be in 1..64" },
    { "pixel_major", &Options::pixel_major, kSign, -1, 1, nullptr },
    { "refill_min", &Options::refill_min, kRange, 1, 64, "refill_min must be in 1..64" },
    { "flush_min", &Options::flush_min, kRange, 0, 64, "flush_min must be in 0..64" },
    { "aux_blocks_per_cu", &Options::aux_blocks_per_cu, kRange, 0, 16, "aux_blocks_per_cu must be in 0..16" },
    { "auto_overlap", &Options::auto_overlap, kBool, 0, 1, nullptr },           // environment default: SQ_AUTO_OVERLAP (sq_scene_upload)
    { "auto_overlap_slots", &Options::auto_overlap_slots, kRange, 1, 1ll << 62, "auto_overlap_slots must be in 1..2^62" },
    { "batches_per_track", &Options::batches_per_track, kRange, 1, 64, "batches_per_track must be in 1..64" },
    { "mirror_ride", &Options::mirror_ride, kBool, 0, 1, nullptr },
};
}  // namespace

int set_option(Options& O, const char* key, int64_t value) {
    for (const OptionRow& r : kOptionTable) {
        if (std::strcmp(key, r.name)) continue;
        if (r.kind == kRange && (value < r.lo || value > r.hi)) return sq_set_error("%s", r.refusal);
        if (r.kind != kIgnored) O.*r.member = r.kind == kBool ? (value ? 1 : 0) : r.kind == kSign ? (value < 0 ? -1 : value != 0) : value;
        return 0;
    }
    return sq_set_error("unknown option '%s'", key);
}

int refuse_frame_size(int64_t n_views, int64_t rows, int64_t h, bool wavefront) {
    if (rows <= 0 || h <= 0 || n_views <= 0) return 0;
    const int64_t view_rows = n_views * rows;                           // each factor is below 2^31: below 2^62
    const bool huge = view_rows > kMaxCallPixels || view_rows * h > kMaxCallPixels;
    const int64_t pixels = huge ? 0 : view_rows * h;
    if (n_views > 1) {
        if (huge) return sq_set_error("%lld views of %lld x %lld pixels exceed 2^31 - 1 pixels in one call", (long long)n_views, (long long)rows, (long long)h);
        if (wavefront && pixels > kMaxWavefrontPixels)
            return sq_set_error("%lld views of %lld x %lld pixels exceed 2^29 pixels in one call of the wavefront form (variant 1 takes 2^31 - 1)", (long long)n_views, (long long)rows, (long long)h);
        return 0;
    }
    if (huge) return sq_set_error("%lld x %lld pixels exceed 2^31 - 1 pixels in one call", (long long)rows, (long long)h);
    if (wavefront && pixels > kMaxWavefrontPixels)
        return sq_set_error("%lld x %lld pixels exceed 2^29 pixels in one call of the wavefront form (variant 1 and cast frames take 2^31 - 1)", (long long)rows, (long long)h);
    return 0;
}

long long radiance_chunk_rays(long long n, long long slots, bool wavefront) {
    const long long cap = wavefront ? std::min<long long>(std::max<long long>(slots, 1), kMaxWavefrontPixels) : kLaneChunk;
    return std::min(n, cap);
}

namespace {
// Chooses the trace form -- resident, streaming six-wave or streaming plain -- its LDS layout and workgroups per CU, and fills the
// trace fields of the plan.  Refuses a tree whose stacks do not fit the streaming form's LDS.
int plan_trace(const PlanInputs& in, CallPlan& C) {
    const Options& o = in.opt; const SceneScalars& S = in.scene;
    const int n_cu = in.device.n_cu, stack_cap = C.stack_cap, stack_elem = S.stack_word;
    sq_plan& P = C.plan;
    // persistent trace kernel geometry.  Resident form: the whole scene (branches, leaves, unique vertices,
    // 16-bit indexed triangles) plus every lane's stack fits in the 160 KB of one CU -> one 1024-thread
    // workgroup per CU, no global traffic except ray fetch and hit store.  Streaming form otherwise.
    const size_t lds_budget = kLdsBudget;
    bool resident = false, dense = false;
    const bool pool = o.pool != 0;
    TraceLds L{};
    if (o.resident && S.has_trix) {
        L = trace_lds_layout(S.n_branches, true, S.n_verts, S.n_tris, kResidentBlock, stack_cap, stack_elem, pool);
        resident = L.total <= lds_budget && S.n_verts <= 4096;         // vertex byte offsets are 16-bit (ResidentTris)
    }
    int n_lds = S.n_branches, trace_blocks = 0, trace_threads = 0;
    if (resident) {
        trace_blocks = n_cu; trace_threads = kResidentBlock;
    } else {
        const size_t max_node_bytes = (size_t)o.lds_node_kb * 1024;     // top of the tree; the rest of LDS buys occupancy
        const int n_lds_want = (int)std::min<size_t>((size_t)S.n_branches, max_node_bytes / 48);
        const TraceLds L0 = trace_lds_layout(0, false, S.n_verts, S.n_tris, kTraceBlock, stack_cap, stack_elem, pool);   // stacks, live lists, window tables
        if (L0.total > lds_budget) return sq_set_error("BIH height %d needs %u B of LDS per workgroup (max %zu)", S.height, L0.total, lds_budget);
        // Three workgroups per CU (the six-wave build) when a third of the LDS holds a workgroup's stacks plus at least 4 KB of
        // the tree's top (or all of it); otherwise two, or one, with up to lds_node_kb of tree each.
        const size_t third = (lds_budget / 3) & ~(size_t)2047;            // 52 KB: the hardware allocates LDS in granules, and 3 x 53.3 KB rounded up does not fit
        const bool dense_fits = L0.total + std::min<size_t>((size_t)S.n_branches * 48, 4096) + 16 <= third;
        dense = pool && !o.profile && (o.trace_blocks_per_cu == 0 ? dense_fits : o.trace_blocks_per_cu == 3 && dense_fits);
        int per_cu;
        if (dense) {
            per_cu = 3;
            n_lds = (int)std::min<size_t>((size_t)n_lds_want, (third - L0.total - 16) / 48);
        } else {
            n_lds = n_lds_want;
            while (n_lds > 0 && trace_lds_layout(n_lds, false, S.n_verts, S.n_tris, kTraceBlock, stack_cap, stack_elem, pool).total > lds_budget) n_lds /= 2;
        }
        L = trace_lds_layout(n_lds, false, S.n_verts, S.n_tris, kTraceBlock, stack_cap, stack_elem, pool);
        if (!dense) {
            per_cu = (int)std::max<size_t>(1, std::min<size_t>(2, lds_budget / L.total));    // the plain build's 86 VGPRs allow four waves per SIMD = two workgroups
            if (o.trace_blocks_per_cu > 0) per_cu = (int)std::min<int64_t>(o.trace_blocks_per_cu, (int64_t)std::max<size_t>(1, lds_budget / L.total));
        }
        trace_blocks = n_cu * per_cu; trace_threads = kTraceBlock;
    }
    const size_t tr_lds = L.total;
    P.trace_form = resident ? SQ_FORM_RESIDENT : dense ? SQ_FORM_STREAMING_SIX_WAVE : SQ_FORM_STREAMING_PLAIN;
    P.blocks_per_cu = trace_blocks / n_cu; P.n_lds = n_lds; P.trace_lds_bytes = (int32_t)tr_lds;
    C.trace_form = P.trace_form; C.resident = resident; C.pool = pool; C.profile = o.profile != 0; C.dense = dense;
    C.n_lds = n_lds; C.trace_blocks = trace_blocks; C.trace_threads = trace_threads; C.tr_lds = tr_lds;
    return 0;
}
}  // namespace

int plan_call(const PlanInputs& in, CallPlan& C) {
    C = CallPlan{};
    C.in = in;
    const Options& o = in.opt; const SceneScalars& S = in.scene; const SceneState& st = in.state; const Call& F = in.call;
    const int n_cu = in.device.n_cu;
    if (!F.query && refuse_frame_size(F.n_views, F.local_rows, F.h, o.variant != 1 && (!F.cast || o.cast_wavefront))) return 1;
    // What a frame and an intersection query do first, alike: the options' view of the scene, the per-lane stacks' size, and the
    // fixed part of the plan.
    C.planned = true;
    C.cull_off = !o.cull;                                              // no ray is inside the culling limits: every leaf is tested
    C.nonneg_materials = S.nonneg_materials; C.n_emitters = S.n_emitters;
    const int stack_cap = std::max(S.height, 1);
    const size_t px_lds = (size_t)kBlock * stack_cap * (size_t)S.stack_word;
    C.stack_cap = stack_cap; C.px_lds = px_lds;
    sq_plan& P = C.plan;
    P.variant = (int32_t)o.variant; P.stack_word_bytes = S.stack_word; P.height = S.height; P.stack_cap = stack_cap;
    P.pixel_lds_bytes = (int32_t)px_lds; P.packed_leaves = S.packed_leaves; P.n_emitters = S.n_emitters;
    P.trace_form = SQ_FORM_PER_PIXEL; P.primary_form = SQ_PRIMARY_NONE;
    if (F.query) {
        // variant 1 runs the per-lane kernel; the default form runs chunks of stage -> one level of the trace kernel -> store
        if (o.variant == 1) {
            if (px_lds > kLdsBudget) return sq_set_error("BIH height %d needs %zu B of LDS stack per workgroup (max 163840)", S.height, px_lds);
            C.path = kPathQueryLanes; P.launched = 1;
            return 0;
        }
        if (plan_trace(in, C)) return 1;
        // Chunks of at most `slots` rays (and what the workspace holds; the option caps the slots at 2^29, so a chunk's queue positions and
        // the trace kernel's 32-bit cursor never overflow).  One slot per ray: 37 B, against 40 B of caller arrays per ray.
        C.path = kPathQueryWave; C.pixels = 1; C.slots = std::min<int64_t>(o.slots, F.n_rays); P.launched = 1;
        return 0;
    }
    // nonneg_materials bounds the radiance below an absorbing surface for the reference's depth.  A deeper path nests more products,
    // one of which may be inf where the bound still held: 0 * inf is NaN in the reference, so past the packer's shortcut_depth
    // (material_flags) the generic-depth kernels of this launch take no s == 0 shortcut.
    if (!F.cast && st.depth > 3 && st.depth > S.shortcut_depth) C.nonneg_materials = 0;
    // Under a sky neither the absorbing-surface shortcut nor the last ray's emitter pre-test is an identity as it stands (the last ray
    // adds the sky when it misses; 0 * sky is NaN for an infinite sky): this launch's generic-depth kernels take neither.
    const bool sky = !F.cast && st.sky_set;
    if (sky) { C.nonneg_materials = 0; C.n_emitters = -1; P.n_emitters = -1; }
    const long long pixels = (long long)F.n_views * F.local_rows * F.h;   // every view's pixels, view-major
    const long long px_blocks = (pixels + kBlock - 1) / kBlock;
    // a masked call (sq_render_rows_device_masked with a mask, second moments or counts) takes the AD instantiations of the kernels that
    // decide who is active, and clears no buffer; every other call takes the instantiations, and the memsets, it always took
    const bool ad = F.src == kSrcCamera && F.masked;
    const bool mom2 = ad && F.mom2;
    C.sky = sky; C.pixels = pixels; C.px_blocks = px_blocks; C.ad = ad; C.mom2 = mom2;
    if (px_blocks > 0x7fffffffLL) return sq_set_error("image too large for one launch");
    if (px_lds > kLdsBudget) return sq_set_error("BIH height %d needs %zu B of LDS stack per workgroup (max 163840)", S.height, px_lds);
    // a cast frame: the per-lane form, or (option "cast_wavefront" with variant 2) the wavefront form with the lights as its samples
    const bool cast_wave = F.cast && o.variant == 2 && o.cast_wavefront;
    const int n_lights = st.n_lights;
    // a path-traced frame or query under a depth other than 3 (or under option "deep"): the generic-depth kernels
    const int depth = st.depth;
    const bool deep = !F.cast && (depth != 3 || o.deep || sky);
    C.deep = deep;
    // The per-lane forms: one kernel, one lane per pixel.
    if (F.cast && !cast_wave && st.lights_set) { C.path = kPathLaneCast; P.launched = 1; return 0; }   // caller-given lights: sq_cast_pixels beside sq_render_pixels
    if (o.variant == 1 && deep) { C.path = kPathLaneDeep; P.launched = 1; return 0; }                   // a depth other than 3, or a sky: sq_render_pixels_deep
    if (o.variant == 1 || (F.cast && !cast_wave)) { C.path = kPathLanePlain; P.launched = 1; return 0; }
    // ---- wavefront pipeline ----
    // the samples this call renders (a whole frame: F.samples); in a cast frame the lights take the samples' place in the slots
    const int n_call = cast_wave ? n_lights : F.k_end - F.k_begin;
    // at least one sample of every pixel per batch, never more slots than the call has samples
    const int64_t slots = std::max<int64_t>(pixels, std::min<int64_t>(o.slots, (int64_t)pixels * n_call));
    C.n_call = n_call; C.slots = slots;
    if (plan_trace(in, C)) return 1;
    const int aux_blocks = n_cu * (int)(o.aux_blocks_per_cu ? o.aux_blocks_per_cu : 8);
    // sq_accumulate, by its loop form: the grouped loop when the shard has no more pixels than the launch has threads (every thread
    // at most one pixel)
    C.aux_blocks = aux_blocks; C.acc_grouped = pixels <= (long long)aux_blocks * kBlock;
    P.primary_form = (o.primary_pooled && C.pool) ? SQ_PRIMARY_POOLED : (C.resident && o.primary_resident) ? SQ_PRIMARY_RESIDENT : SQ_PRIMARY_PER_LANE;
    // the per-lane primary pass is one launch with a thread per tile lane, padding included (a narrow frame's edge tiles are mostly
    // padding: up to 64 lanes per pixel at h = 1), and a launch has at most 2^32 - 1 threads; the other two passes stride over a fixed grid
    const long long padded = primary_padded_lanes(F.local_rows, F.tile_rows, F.tiles_x);
    if (P.primary_form == SQ_PRIMARY_PER_LANE && (padded * F.n_views + kBlock - 1) / kBlock * kBlock > 0xffffffffLL)
        return sq_set_error("image too large for one launch of the primary rays (%lld tile lanes; at most 2^32 - 1)", padded * F.n_views);
    C.need_lights = cast_wave; C.need_sum2 = mom2; C.need_deep = deep;
    C.deep_slot_bytes = deep ? deep_slot_bytes(depth, sky) : 0;
    C.rng_table = !cast_wave; C.rng_grow = F.src != kSrcRays && !deep;
    // primary rays: once per pixel.  With a resident scene they are traced out of LDS as well
    if (P.primary_form == SQ_PRIMARY_RESIDENT) {
        const TraceLds Lp = trace_lds_layout(S.n_branches, true, S.n_verts, S.n_tris, kResidentBlock, stack_cap, S.stack_word, false);
        const long long need = (padded * F.n_views + kResidentBlock - 1) / kResidentBlock;
        C.primary_grid = std::min<long long>(n_cu, need); C.primary_lds = Lp.total;
    } else if (P.primary_form == SQ_PRIMARY_PER_LANE) {
        C.primary_grid = (padded * F.n_views + kBlock - 1) / kBlock; C.primary_lds = px_lds;
    }
    C.path = cast_wave ? kPathWaveCast : deep ? kPathWaveDeep : kPathPipeline;
    // Level-1 culling (build_level1): the three-level pipeline only, and only with the shortcuts its lemma builds on
    if (C.path == kPathPipeline) {
        C.level1_cull = S.level1_on && o.level1_cull && C.n_emitters >= 0 && C.nonneg_materials && S.finite_geometry;
        P.level1_cull = C.level1_cull;
    }
    P.launched = 1;
    return 0;
}

Schedule plan_schedule(const CallPlan& C, int64_t have_slots) {
    Schedule D;
    const Options& o = C.in.opt;
    if (C.path == kPathQueryWave) { D.query_chunk = std::min<long long>(o.slots, have_slots); return D; }
    if (C.path != kPathWaveCast && C.path != kPathWaveDeep && C.path != kPathPipeline) return D;
    const long long pixels = C.pixels; const int n_call = C.n_call;
    // Overlapped schedules: the sample batches alternate between two halves of the workspace ("tracks").  Asked for by option
    // "overlap": 1 keeps every trace launch on the caller's stream, in the order T1(a) T1(b) T2(a) T2(b), with the per-sample kernels
    // (RNG + bounce, shading, accumulation) on a second stream beside them, ordered by events; 2 runs each track as a pipeline of
    // its own, even batches on the caller's stream and odd ones on the second.  Both give the mirror rays a launch of their own.
    // Chosen without being asked (option "auto_overlap", on by default): two pipelines, once the call is large enough to gain --
    // pixels x samples reaches option "auto_overlap_slots".  Its mirror rays have a launch of their own too; option "mirror_ride" puts
    // them at the head of batch 0's first trace launch instead, as in the serial schedule (0.25-0.4 ms faster on the headline frame in
    // every paired run, which is short of the landing rule: DESIGN.md 6).  The two tracks' launches fill each other's ramp-downs and hide the
    // memory-bound sq_shade1 and sq_accumulate of one track under the other's trace launches; a small frame
    // has no tail worth filling and pays for the events and the second stream instead.  Co-running launches slow each other
    // down, so what "timing", the roofline and a kernel trace say per kernel holds for the serial schedule only: the profiling
    // tools pin it (auto_overlap = 0, or SQ_AUTO_OVERLAP=0 in the environment).
    const bool can_overlap = C.path == kPathPipeline && n_call >= 2 && have_slots >= 2 * pixels;
    const bool automatic = can_overlap && !o.overlap && o.auto_overlap && (int64_t)pixels * n_call >= o.auto_overlap_slots;
    const int kind = !can_overlap ? kSchedSerial : automatic ? kSchedPipelines : (int)o.overlap;
    const bool overlap = kind != kSchedSerial;
    const int tracks = overlap ? 2 : 1;
    const int64_t track_slots = have_slots / tracks;
    // samples per batch: as many as a track holds, split evenly (few large launches: a small trace launch
    // wastes its ramp-up and drain, and the second-bounce launches only carry a few percent of the slots)
    const int max_batch = (int)std::max<int64_t>(1, std::min<int64_t>(n_call, track_slots / pixels));
    const int min_batches = automatic ? (int)std::min<int64_t>(n_call, tracks * o.batches_per_track) : tracks;
    int n_batches = std::max(min_batches, (n_call + max_batch - 1) / max_batch);
    int batch = (n_call + n_batches - 1) / n_batches;
    // The automatic schedule keeps a batch to the generator table's runs of four samples (a batch that starts inside a run reads its
    // entries as twelve dword loads, not three dwordx4): rounded up where the track holds it, else down; only the call's last batch is
    // ragged.  A track that holds fewer than four samples of every pixel cannot.
    if (automatic && n_call >= 8 && max_batch >= 4) {
        batch = std::min((batch + 3) / 4 * 4, max_batch / 4 * 4);
        n_batches = std::max(tracks, (n_call + batch - 1) / batch);
    }
    int n_real = 0;
    while (n_real < n_batches && std::max(0, std::min(batch, n_call - n_real * batch)) > 0) ++n_real;
    D.kind = kind; D.mirror_rides = !overlap || (automatic && o.mirror_ride);
    D.overlap = overlap; D.tracks = tracks; D.track_slots = track_slots; D.batch = batch; D.n_batches = n_batches; D.n_real = n_real;
    return D;
}

Grid2 pp_grid(const CallPlan& C, const Schedule& D, int kc) {
    const Options& o = C.in.opt; const int n_cu = C.in.device.n_cu; const long long pixels = C.pixels;
    // Overlapped schedules, option "aux_polite" = n > 0: the per-sample kernels get n workgroups per CU in all (grid-stride
    // loops do the rest), few enough that a trace workgroup -- 16 waves, all of the CU's LDS, 4 x 104 VGPRs per SIMD -- can
    // always be placed beside them, whichever kernel reaches a CU first.
    if (D.overlap && o.aux_polite > 0) return Grid2{ (unsigned)(n_cu * (int)o.aux_polite), 1u };
    // x covers the pixels, y splits a pixel's samples when the frame has too few pixels to fill the chip (one rank's share of a
    // frame, small frames)
    const long long bx = std::max<long long>(1, std::min<long long>((pixels + kBlock - 1) / kBlock, 1 << 20));
    const long long want_threads = (long long)n_cu * 2048 * 2;
    const long long ks = std::max<long long>(1, std::min<long long>(std::min(kc, 64), (want_threads + pixels - 1) / std::max<long long>(pixels, 1)));
    return Grid2{ (unsigned)bx, (unsigned)ks };
}

TraceLaunch trace_launch(const CallPlan& C, int64_t queue_rays, int kc, int level) {
    const Options& o = C.in.opt;
    const bool resident = C.resident;
    const int trace_blocks = C.trace_blocks, trace_threads = C.trace_threads;
    // a launch with few slots (the per-pixel mirror rays) takes small reservations, or only a few waves get any
    const int max_chunk = resident ? kChunkResident : kChunkStreaming;
    const int64_t per_wave = queue_rays * (int64_t)kc / std::max(1, trace_blocks * (trace_threads / 64));
    const int chunk = (int)std::min<int64_t>(max_chunk, std::max<int64_t>(64, (per_wave / 8) / 64 * 64));
    // queue order: a pixel's samples in a row pays once the triangles no longer fit the L2s (rays that start at one point
    // share their first leaves: 1M-triangle scene +2.5 %), and costs 1-7 % below that (strided queue reads)
    const bool pixel_major = o.pixel_major < 0 ? (!resident && (size_t)C.in.scene.n_tris * sizeof(DevTri) > ((size_t)4 << 20)) : o.pixel_major != 0;
    int guide_shift = 2;                                            // log2(4 x waves of the launch), rounded up
    while ((1ll << guide_shift) < 4ll * trace_blocks * (trace_threads / 64)) ++guide_shift;
    if (!((o.guided >> level) & 1)) guide_shift = 62;              // bit 0: first bounce level (and the mirror / primary launches), bit 1: second
    return TraceLaunch{ chunk, guide_shift, pixel_major };
}

int workspace_layout(int64_t pixels, int64_t slots, WorkLayout& W) {
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += al(bytes); return o; };
    W.cnt = take(128 * sizeof(int32_t)); W.stats = take(kStatSlots * sizeof(unsigned long long));
    W.pix = take(pixels * 4); W.t0 = take(pixels * 4); W.tri0 = take(pixels * 4); W.sum = take(pixels * 12);
    W.mt = take(pixels * 4); W.mtri = take(pixels * 4);
    // + pixels: the mirror rays' spare region behind the sample slots (state and the two ray quads)
    W.state = take(slots + pixels); W.org = take((slots + pixels) * 16); W.dir = take((slots + pixels) * 16); W.tri1 = take(slots * 4);
    W.carry = take(pixels * 12);                                    // behind everything else: no other array moves for it
    W.total = off;
    // every array has its own, ordered place in the block: a slip here would be a GPU fault, not an error code
    if (!(W.cnt < W.stats && W.stats < W.pix && W.pix < W.t0 && W.t0 < W.tri0 && W.tri0 < W.sum && W.sum < W.mt && W.mt < W.mtri &&
          W.mtri < W.state && W.state < W.org && W.org < W.dir && W.dir < W.tri1 && W.tri1 < W.carry && W.carry < off))
        return sq_set_error("internal error: frame workspace layout");
    return 0;
}

DeepLayout deep_layout(int depth, bool sky, long long cap) {
    DeepLayout L{};
    L.oxy = 0;                                                      // float2 per slot, from depth 4 on
    L.trail = depth >= 4 ? (size_t)cap * 8 : 0;                     // int32 per bounce level and slot
    L.has_tmiss = sky && depth >= 2;
    L.tmiss = L.has_tmiss ? L.trail + (size_t)(depth - 1) * cap * 4 : 0;
    return L;
}
}  // namespace sqd

// ---- the C-ABI window on the planner (include/squigly_host.h) ----
extern "C" int sq_plan_call(const char* const* in_names, const int64_t* in_values, int32_t n_in, int64_t have_slots,
                            sq_plan* plan, const char* const* out_names, int64_t* out_values, int32_t n_out) {
    using namespace sqd;
    if (!plan || n_in < 0 || n_out < 0 || (n_in > 0 && (!in_names || !in_values)) || (n_out > 0 && (!out_names || !out_values))) { sq_set_error("null argument"); return 2; }
    *plan = sq_plan{};
    for (int32_t i = 0; i < n_out; ++i) out_values[i] = 0;
    PlanInputs in;
    SceneScalars& S = in.scene; SceneState& st = in.state; Call& F = in.call;
    int64_t small_index = 0, trix = 0, sky = 0, lights_set = 0, cast = 0, masked = 0, mom2 = 0, query = 0, total_rays = 0;
    const struct { const char* name; int32_t* v32; int64_t* v64; } fields[] = {
        { "n_branches", &S.n_branches, nullptr }, { "n_verts", &S.n_verts, nullptr }, { "n_tris", &S.n_tris, nullptr }, { "height", &S.height, nullptr },
        { "trix", nullptr, &trix }, { "small_index", nullptr, &small_index }, { "packed_leaves", &S.packed_leaves, nullptr },
        { "n_emitters", &S.n_emitters, nullptr }, { "nonneg_materials", &S.nonneg_materials, nullptr }, { "finite_geometry", &S.finite_geometry, nullptr },
        { "shortcut_depth", &S.shortcut_depth, nullptr }, { "level1_on", &S.level1_on, nullptr }, { "n_cu", &in.device.n_cu, nullptr },
        { "depth", &st.depth, nullptr }, { "sky", nullptr, &sky }, { "lights_set", nullptr, &lights_set }, { "n_lights", &st.n_lights, nullptr },
        { "source", &F.src, nullptr }, { "cast", nullptr, &cast }, { "masked", nullptr, &masked }, { "mom2", nullptr, &mom2 },
        { "n_views", &F.n_views, nullptr }, { "local_rows", &F.local_rows, nullptr }, { "h", &F.h, nullptr }, { "tile_rows", &F.tile_rows, nullptr },
        { "tiles_x", &F.tiles_x, nullptr }, { "k_begin", &F.k_begin, nullptr }, { "k_end", &F.k_end, nullptr },
        { "query", nullptr, &query }, { "n_rays", nullptr, &F.n_rays }, { "total_rays", nullptr, &total_rays } };
    for (int32_t i = 0; i < n_in; ++i) {
        if (!in_names[i]) { sq_set_error("null argument"); return 2; }
        bool found = false;
        for (const auto& f : fields)
            if (!std::strcmp(in_names[i], f.name)) {
                if (f.v32 && (in_values[i] < INT32_MIN || in_values[i] > INT32_MAX)) { sq_set_error("%s = %lld is not a 32-bit value", f.name, (long long)in_values[i]); return 2; }
                if (f.v32) *f.v32 = (int32_t)in_values[i]; else *f.v64 = in_values[i];
                found = true;
            }
        if (!found && set_option(in.opt, in_names[i], in_values[i])) return 2;      // an option by sq_set_option's name, with its refusals
    }
    S.has_trix = trix != 0; S.stack_word = small_index ? 2 : 4;
    st.sky_set = sky != 0; st.lights_set = lights_set != 0;
    F.cast = cast != 0; F.masked = masked != 0; F.mom2 = mom2 != 0; F.query = query != 0;
    if (S.n_branches < 0 || S.n_verts < 0 || S.n_tris < 0 || S.height < 0 || in.device.n_cu < 1 || st.depth < 1 || st.depth > kDeepestPath || st.n_lights < 0 ||
        F.src < kSrcCamera || F.src > kSrcRays || F.n_views < 1 || F.local_rows < 1 || F.h < 1 || F.tile_rows < 1 || F.tiles_x < 1 ||
        F.k_begin < 0 || F.k_end <= F.k_begin || (F.query && F.n_rays < 1) || have_slots < 0 || total_rays < 0) {
        sq_set_error("bad planner input");
        return 2;
    }
    CallPlan C;
    const int rc = plan_call(in, C);
    *plan = C.plan;
    if (rc) { plan->launched = 0; return 1; }
    const int64_t have = have_slots ? have_slots : C.slots;            // 0: the workspace gave the slots the plan wanted
    const Schedule D = plan_schedule(C, have);
    WorkLayout W{};
    if (C.slots > 0 && workspace_layout(C.pixels, have, W)) return 1;
    const int tail_kc = D.n_real > 0 ? std::min(D.batch, C.n_call - (D.n_real - 1) * D.batch) : 0;
    const Grid2 g = pp_grid(C, D, D.batch), gt = pp_grid(C, D, tail_kc);
    const int64_t queue = C.path == kPathQueryWave ? std::min<int64_t>(D.query_chunk, F.n_rays) : C.pixels;
    const int kc = C.path == kPathQueryWave ? 1 : D.batch;
    const TraceLaunch t0 = trace_launch(C, queue, kc, 0), t1 = trace_launch(C, queue, kc, 1), tt = trace_launch(C, queue, tail_kc, 0), lone = trace_launch(C, C.pixels, 1, 0);
    const DeepLayout dl = deep_layout(st.depth, C.sky, have);
    const struct { const char* name; int64_t value; } all[] = {
        { "path", C.path }, { "ad", C.ad }, { "mom2", C.mom2 }, { "sky", C.sky }, { "deep", C.deep }, { "nonneg_materials", C.nonneg_materials },
        { "n_emitters", C.n_emitters }, { "cull_off", C.cull_off }, { "pixels", C.pixels }, { "px_blocks", C.px_blocks }, { "px_lds", (int64_t)C.px_lds },
        { "n_call", C.n_call }, { "slots", C.slots }, { "trace_form", C.trace_form }, { "resident", C.resident }, { "pool", C.pool }, { "profile", C.profile },
        { "dense", C.dense }, { "n_lds", C.n_lds }, { "stack_cap", C.stack_cap }, { "trace_blocks", C.trace_blocks }, { "trace_threads", C.trace_threads },
        { "tr_lds", (int64_t)C.tr_lds }, { "primary_grid", C.primary_grid }, { "primary_lds", (int64_t)C.primary_lds }, { "aux_blocks", C.aux_blocks },
        { "acc_grouped", C.acc_grouped }, { "level1_cull", C.level1_cull }, { "deep_slot_bytes", (int64_t)C.deep_slot_bytes }, { "need_lights", C.need_lights },
        { "need_sum2", C.need_sum2 }, { "need_deep", C.need_deep }, { "rng_table", C.rng_table }, { "rng_grow", C.rng_grow },
        { "chunk_rays", total_rays > 0 ? radiance_chunk_rays(total_rays, in.opt.slots, in.opt.variant != 1 && (!F.cast || in.opt.cast_wavefront)) : 0 },
        { "have_slots", have }, { "schedule", D.kind }, { "mirror_rides", D.mirror_rides }, { "overlap", D.overlap }, { "tracks", D.tracks }, { "track_slots", D.track_slots }, { "batch", D.batch },
        { "n_batches", D.n_batches }, { "n_real", D.n_real }, { "query_chunk", D.query_chunk }, { "tail_kc", tail_kc },
        { "pp_grid_x", g.x }, { "pp_grid_y", g.y }, { "tail_pp_grid_x", gt.x }, { "tail_pp_grid_y", gt.y },
        { "chunk_0", t0.chunk }, { "chunk_1", t1.chunk }, { "guide_shift_0", t0.guide_shift }, { "guide_shift_1", t1.guide_shift },
        { "pixel_major", t0.pixel_major }, { "tail_chunk", tt.chunk }, { "lone_chunk", lone.chunk },
        { "ws_cnt", (int64_t)W.cnt }, { "ws_stats", (int64_t)W.stats }, { "ws_pix", (int64_t)W.pix }, { "ws_t0", (int64_t)W.t0 }, { "ws_tri0", (int64_t)W.tri0 },
        { "ws_sum", (int64_t)W.sum }, { "ws_mt", (int64_t)W.mt }, { "ws_mtri", (int64_t)W.mtri }, { "ws_state", (int64_t)W.state }, { "ws_org", (int64_t)W.org },
        { "ws_dir", (int64_t)W.dir }, { "ws_tri1", (int64_t)W.tri1 }, { "ws_carry", (int64_t)W.carry }, { "ws_total", (int64_t)W.total },
        { "deep_oxy", (int64_t)dl.oxy }, { "deep_trail", (int64_t)dl.trail }, { "deep_tmiss", dl.has_tmiss ? (int64_t)dl.tmiss : -1 } };
    for (int32_t i = 0; i < n_out; ++i) {
        bool found = false;
        for (const auto& s : all) if (out_names[i] && !std::strcmp(out_names[i], s.name)) { out_values[i] = s.value; found = true; }
        if (!found) { sq_set_error("no plan scalar '%s'", out_names[i] ? out_names[i] : "(null)"); return 2; }
    }
    return 0;
}
