// sq_frame.h — what a kernel of sq_device.hip is handed: the frame, the workspace, the by-value arguments of the optional features,
// and the small device helpers that more than one of the kernel headers (sq_kernels_lane.h, _wave.h, _trace.h) uses.
#pragma once
#include "sq_plan.h"
#include "sq_scene.h"

using sq::f3;
using sq::load3;
using namespace sqd;

struct Frame {
    float cam_pos[3]; float cam_rot[9];
    int32_t samples, w, h, cast;
    int32_t row_block, shard, n_shards, local_rows;
    int32_t tile_rows, tiles_x;   // primary rays are enumerated in tiles of tile_rows x (64 / tile_rows) pixels (primary_tile), tiles_x per tile row
    float* out_avg; uint8_t* out_rgb;
    // the samples [k_begin, k_end) of the frame this call renders (a whole frame: [0, samples)); `sum`: the caller's per-pixel fold
    // (sq_render_rows_device_range, 3 floats per local pixel), read where the fold starts when k_begin > 0 and written where it
    // ends; nullptr = the fold lives in the workspace only
    int32_t k_begin, k_end;
    float* sum;
    int32_t diag;             // option "coresidency": the per-sample kernels and the trace kernel count who runs beside whom (sq_get_stats 24..27)
    // multi-view frames (sq_render_views_device, the kernels' kSrcViews instantiations): n_views views of view_pixels = local_rows * h pixels,
    // view-major, so a pixel index runs over [0, n_views * view_pixels); cams = the scene's camera table, kCamWords floats per view
    // (pos, rot).  A single-view frame has n_views = 1 and reads cam_pos / cam_rot.
    int32_t n_views, view_pixels;
    const float* cams;
    // masked calls (sq_render_rows_device_masked, the kernels' AD instantiations; read by no other instantiation): `mask` = the
    // caller's per-pixel mask (nullptr = every pixel), `sum2` = its fold of r * r, laid out and carried like `sum` (nullptr = none),
    // `count` = its per-pixel sample counts (nullptr = none).  pixel_live() says which pixels such a call renders.
    const uint8_t* mask; float* sum2; int32_t* count;
};
// Radiance queries (sq_raytrace_rays_device / sq_raycast_rays_device, the kernels' kSrcRays instantiations): a frame plus the caller's
// rays and seed bases.  A chunk of m rays is a frame of one row and m columns (local_rows = 1, h = m, tile_rows = 1), so "pixel" i is
// ray i of the chunk: origin ray_org[3 i ..], direction ray_dir[3 i ..], and the generator of its sample k is mkTFGen (ray_seed[i] + k)
// (nullptr in a raycast query, which draws nothing).  A type of its own, and the argument of the query kernels only: three more
// pointers in Frame, which every kernel takes by value, moved the SGPR counts of five of the frames' kernels.
struct RayFrame : Frame {
    const float* ray_org; const float* ray_dir; const long long* ray_seed;
};
// Where a kernel's primary rays come from: the frame's camera (makeRay, src/Lib.hs:107-114), the camera table of a multi-view frame,
// or the caller's arrays (kSrcCamera, kSrcViews, kSrcRays: sq_plan.h).  Every kernel family is one __global__ template keyed by it ("One entry point per body"): FrameOf<SRC> is the frame it takes.
template <int SRC> using FrameOf = std::conditional_t<SRC == kSrcRays, RayFrame, Frame>;
constexpr int kCamWords = 12;     // a view's entry in the camera table: pos[3], rot[9]
struct ViewCam { f3 pos; float rot[9]; };
// The camera of view v.  UNIFORM: v is the same in every lane of the wave (a primary-ray tile), so the 48 bytes come through scalar loads.
template <bool UNIFORM>
__device__ __forceinline__ ViewCam view_cam(const Frame& F, int v) {
    ViewCam c;
    if constexpr (UNIFORM) {
        v = __builtin_amdgcn_readfirstlane(v);
        const __attribute__((address_space(4))) float* p = (const __attribute__((address_space(4))) float*)(F.cams + (long long)kCamWords * v);
        c.pos = sq::mk(p[0], p[1], p[2]);
#pragma unroll
        for (int i = 0; i < 9; ++i) c.rot[i] = p[3 + i];
    } else {
        const float4* p = reinterpret_cast<const float4*>(F.cams + (long long)kCamWords * v);   // 48-B entries: 16-B aligned
        const float4 a = p[0], b = p[1], d = p[2];
        c.pos = sq::mk(a.x, a.y, a.z);
        c.rot[0] = a.w; c.rot[1] = b.x; c.rot[2] = b.y; c.rot[3] = b.z; c.rot[4] = b.w; c.rot[5] = d.x; c.rot[6] = d.y; c.rot[7] = d.z; c.rot[8] = d.w;
    }
    return c;
}
__device__ __forceinline__ void pixel_coords(const Frame& F, int pix, int& y, int& x) {   // 32-bit: cheap div/mod
    const int j = pix / F.h;
    x = pix - j * F.h;
    y = sq::shard_global_row(j, F.row_block, F.shard, F.n_shards);
}
// The q-th primary ray of a shard, q in [0, primary_padded(F)): a wave takes a TILE of tile_rows x (64 / tile_rows) neighbouring pixels
// instead of 64 pixels of one row, so that the 64 rays of a one-ray-per-lane walk -- which runs the UNION of their paths -- stay together
// in both image directions (tile_rows adjacent local rows are adjacent image rows: it divides row_block, or the shard is the whole image).
// Returns the pixel's row-major local index (what px_pixel holds and everything downstream uses), or -1 for the padding of edge tiles.
__device__ __forceinline__ long long primary_tile(const Frame& F, long long q) {
    const int lane = (int)(q & 63), tw = 64 / F.tile_rows;
    const long long tile = q >> 6;
    const long long ty = tile / F.tiles_x; const int tx = (int)(tile - ty * F.tiles_x);
    const int jj = lane / tw, xx = lane - jj * tw;
    const long long j = ty * F.tile_rows + jj; const int x = tx * tw + xx;
    return (j < F.local_rows && x < F.h) ? j * F.h + x : -1;
}
__host__ __device__ __forceinline__ long long primary_padded(const Frame& F) {
    return (long long)((F.local_rows + F.tile_rows - 1) / F.tile_rows) * F.tiles_x * 64;   // the planner's twin: primary_padded_lanes (sq_plan.h)
}
__device__ __forceinline__ void pixel_coords(const Frame& F, long long pix, int& y, int& x) {
    const int j = (int)(pix / F.h);
    x = (int)(pix - (long long)j * F.h);
    y = sq::shard_global_row(j, F.row_block, F.shard, F.n_shards);
}
// Multi-view frames: the view of a pixel index, and (y, x) of the pixel within its view.  Every view has the same pixels and seeds.
__device__ __forceinline__ int view_coords(const Frame& F, int pix, int& y, int& x) {   // px_pixel: n_views * view_pixels <= INT32_MAX
    const int v = pix / F.view_pixels;
    pixel_coords(F, pix - v * F.view_pixels, y, x);
    return v;
}
// The q-th primary ray of a multi-view frame, q in [0, n_views * primary_padded(F)): every view's tiles are padded to whole waves, so a
// wave never spans two views and its camera is wave-uniform.  Returns the pixel index (-1 for padding); `view` = its view.
__device__ __forceinline__ long long primary_tile_views(const Frame& F, long long q, int& view) {
    const long long per = primary_padded(F);
    view = (int)(q / per);
    if (view >= F.n_views) return -1;                                   // past the last view (a launch's last workgroup)
    const long long local = primary_tile(F, q - (long long)view * per);
    return local >= 0 ? (long long)view * F.view_pixels + local : -1;
}

// Where a pixel's fold starts: +0 on a fresh frame, else what the caller's earlier range call left in F.sum (src/Lib.hs:88 is a left
// fold, so resuming it from its exact fp32 partial sum gives the bits of one uninterrupted fold).
__device__ __forceinline__ f3 fold_start(const Frame& F, long long pix) {
    if (F.k_begin == 0) return sq::mk(0, 0, 0);
    const float* p = F.sum + pix * 3;
    return sq::mk(p[0], p[1], p[2]);
}
// A pixel whose primary ray misses folds black samples: its sum is +0 whatever range is rendered.
__device__ __forceinline__ void store_miss_sum(const Frame& F, long long pix) {
    if (F.sum) { float* p = F.sum + pix * 3; p[0] = 0.0f; p[1] = 0.0f; p[2] = 0.0f; }
}
// Masked calls.  Is the pixel live, i.e. does this call render it?  Its mask byte is set, and its fold stays a prefix: a pixel that an
// earlier range left out (its count is not k_begin) does not resume with a gap.  Everything else in a masked call follows from
// this one answer: a dead pixel gets no ray, no slot and no store.
__device__ __forceinline__ bool pixel_live(const Frame& F, long long pix) {
    if (F.mask && F.mask[pix] == 0) return false;
    return F.k_begin == 0 || !F.count || F.count[pix] == F.k_begin;
}
// Where the fold of r * r starts (F.sum2 given): like fold_start.
__device__ __forceinline__ f3 fold_start2(const Frame& F, long long pix) {
    if (F.k_begin == 0) return sq::mk(0, 0, 0);
    const float* p = F.sum2 + pix * 3;
    return sq::mk(p[0], p[1], p[2]);
}
// A live pixel's sample count after the call.
__device__ __forceinline__ void store_count(const Frame& F, long long pix) {
    if (F.count) F.count[pix] = F.k_end;
}
// A live pixel whose primary ray misses: +0 in both folds, the count, and black -- a masked call clears no buffer up front (its
// dead pixels keep what they hold), so the primary kernels write the black of their own misses.
__device__ __forceinline__ void store_live_miss(const Frame& F, long long pix) {
    store_miss_sum(F, pix);
    if (F.sum2) { float* p = F.sum2 + pix * 3; p[0] = 0.0f; p[1] = 0.0f; p[2] = 0.0f; }
    store_count(F, pix);
    if (F.out_avg) { float* p = F.out_avg + pix * 3; p[0] = 0.0f; p[1] = 0.0f; p[2] = 0.0f; }
    if (F.out_rgb) { uint8_t* p = F.out_rgb + pix * 3; p[0] = 0; p[1] = 0; p[2] = 0; }
}

// ----------------------------------------------------------------------------------------------
// Caller-given sky (sq_scene_set_sky): the radiance of a ray that leaves the scene
// ----------------------------------------------------------------------------------------------
// The kernels' SKY instantiations take it by value; every other instantiation is handed an empty one and reads nothing of it.
struct Sky { float up[3], down[3]; };
// A kernel under a sky takes it as a trailing argument pack of one (Sky, or DeepSky in the generic-depth pipeline); without a sky the
// pack is empty, the kernel has no such argument, and its body is handed an empty value of the type.
template <typename T> __device__ __forceinline__ T sky_arg() { return T{}; }
template <typename T> __device__ __forceinline__ const T& sky_arg(const T& k) { return k; }
// t of a ray's direction as it was traced (not normalised beforehand): every operation a single fp32 operation in this order.
__device__ __forceinline__ float sky_t(f3 d) {
    const float n = sq::fsqrt((d.x * d.x + d.y * d.y) + d.z * d.z);
    const float u = d.z / n;
    return 0.5f * u + 0.5f;
}
__device__ __forceinline__ f3 sky_at(const Sky& K, float t) {
    return sq::mk(K.down[0] + t * (K.up[0] - K.down[0]), K.down[1] + t * (K.up[1] - K.down[1]), K.down[2] + t * (K.up[2] - K.down[2]));
}
// The end of a pixel's fold: the caller's sum, avg over the k_end samples folded so far (src/Lib.hs:88) and its tonemap.
__device__ __forceinline__ void store_fold(const Frame& F, long long pix, f3 sum) {
    if (F.sum) { float* o = F.sum + pix * 3; o[0] = sum.x; o[1] = sum.y; o[2] = sum.z; }
    const f3 avg = sq::scale(1 / (float)F.k_end, sum);
    if (F.out_avg) { float* o = F.out_avg + pix * 3; o[0] = avg.x; o[1] = avg.y; o[2] = avg.z; }
    if (F.out_rgb) tonemap(avg, F.out_rgb + pix * 3);
}
// A (live) pixel whose primary ray misses under a sky: sky(d_0) folded once per sample of [k_begin, k_end) from where the pixel's
// fold starts -- single additions, not one multiplication -- and everything a hit pixel's fold ends with.
template <bool AD>
__device__ __forceinline__ void store_miss_sky(const Frame& F, long long pix, const Sky& K, f3 d0) {
    const f3 c = sky_at(K, sky_t(d0));
    f3 sum = fold_start(F, pix);
    for (int k = F.k_begin; k < F.k_end; ++k) sum = sum + c;
    if constexpr (AD) {
        if (F.sum2) {
            f3 sum2 = fold_start2(F, pix);
            for (int k = F.k_begin; k < F.k_end; ++k) sum2 = sum2 + c * c;
            float* o = F.sum2 + pix * 3; o[0] = sum2.x; o[1] = sum2.y; o[2] = sum2.z;
        }
        store_count(F, pix);
    }
    store_fold(F, pix, sum);
}

struct Work {                 // device workspace of one frame (HBM)
    // per active pixel (a pixel whose primary ray hits), indexed by a in [0, *n_active)
    int32_t* n_active;        // device counter
    int32_t* px_pixel;        // local pixel index
    float*   px_t0;           // primary hit: t
    int32_t* px_tri0;         // primary hit: triangle
    float*   px_sum;          // running ordered sum of sample radiances, 3 floats
    float*   px_mt;           // hit of the pixel's MIRROR bounce ray (reflectRay has no random input, so every
    int32_t* px_mtri;         //   sample of the pixel that mirrors at depth 0 shoots this same ray): t, triangle (-1 = miss)
    // per sample slot sid = k_local * A + a : the ray queue is dense in sid, dead entries are flagged
    uint8_t* state;           // one byte per slot: kDone / kRay1 / kMirror / kRay2.  The trace kernel's refill scan, shade1 and
                              //   sq_accumulate look at this byte first and touch a slot's 32 other bytes only if they need them
    // 37 bytes per slot (round 2: 61; 45 while a finished sample's radiance went through HBM).  A slot's two quads are reused as
    // the sample moves on:
    //   org : ray origin.xyz while the ray waits in the queue; the trace kernel puts the ray's HIT into .xy (t bits, triangle)
    //         when it is done with it -- nothing reads an origin after that (ray 1 starts at the pixel's primary hit point, which
    //         sq_shade1 recomputes).  .w = n1 of the sample's generator until sq_shade1 has used it; a kMirror slot, which holds
    //         no ray of its own, keeps n2 in .z as well.
    //   dir : ray direction.xyz.  .w = n2 of the generator (first bounce level), then the triangle hit by ray 1 (second level).
    // A sample that ends at the first bounce level (92 % of them) leaves no radiance in HBM: its radiance is a function of the
    // pixel's primary surface and of the triangle ray 1 hit (level1_radiance), so sq_shade1 stores that triangle and sq_accumulate,
    // which holds the primary surface anyway, evaluates it -- 4 bytes written and read where the radiance took 12.  The triangle
    // keeps a dense array of its own: both kernels are bound by the bytes they move, and read out of the 16-byte origin records
    // (where the trace kernel left it) it would cost sq_accumulate a whole record per sample (the lesson of
    // profiles/r03f_slots_ab.txt, where 16-byte records carrying 12 bytes of radiance lost 0.4 ms).
    float4*  org;
    float4*  dir;
    int32_t* tri1;            // finished sample (kDone): the triangle its ray 1 hit, -1 = a miss.  Not read for the samples of an
                              //   absorbing pixel, which all finish at depth 0: sq_accumulate sees that from the pixel's surface
    int32_t* head[2];         // dequeue cursors of the persistent trace kernel, one per bounce level
    unsigned long long* stats;  // cumulative trace-kernel statistics (TraceArgs::stats)
    int64_t  slot_capacity;
    float*   px_sum2;         // masked calls that carry second moments: running ordered sum of r * r per active pixel, 3 floats (else nullptr)
};
// Slot states.  kRay1 / kRay2: the slot holds a bounce ray of depth 1 / 2 for the trace launch of that level;
// kMirror: the sample mirrors at depth 0 and shares the pixel's mirror ray (traced once per pixel); kDone: it ended at the first
// bounce level (or at depth 0, on an absorbing pixel) and `tri1` says on what.
constexpr uint8_t kDone = 0, kRay1 = 1, kMirror = 2, kRay2 = 3;

// Diagnostic (option "coresidency", off by default; results unchanged): does a wave of a per-sample kernel run BESIDE the
// resident trace workgroups?  The trace kernel keeps a gauge of its live workgroups in stats[24]; it runs one workgroup per
// CU, so a per-sample wave that starts (stats[26]) or ends (stats[27]) while at least `full` of them are live shares its CU
// with one.  stats[25] counts the per-sample waves that looked.
constexpr int kDiagGauge = 24, kDiagWaves = 25, kDiagStartBeside = 26, kDiagEndBeside = 27;
constexpr int kStatLevel1Culled = 28;       // sq_get_stats 28: first-bounce rays sq_gen_bounce1 did not queue (level-1 culling)
constexpr int kStatLevel1Stretch = 29;      // sq_get_stats 29: those that only condition (4), the stretch against the cover, kept off the queue
constexpr int kStatLevel1Mirror = 30;       // sq_get_stats 30: those that only condition (5), the mirrored ray 2's reach, kept off the queue

// Appends `want` lanes of this wave to a list with one atomic: wave ballot + prefix rank.
__device__ __forceinline__ int wave_append(int32_t* counter, bool want) {
    const unsigned long long m = sq_ballot(want);
    if (m == 0) return -1;
    const int lane = threadIdx.x & 63;
    const int leader = __ffsll((long long)m) - 1;
    int base = 0;
    if (lane == leader) base = atomicAdd(counter, __popcll(m));
    base = __shfl(base, leader);
    return want ? base + __popcll(m & ((1ull << lane) - 1ull)) : -1;
}

// A pixel joins the active list: its primary hit and where its fold starts.  AD: a masked call's live pixel, also its count and,
// when the call carries second moments, where that fold starts.
template <bool AD>
__device__ __forceinline__ void store_active(const Frame& F, const Work& W, int a, long long pix, float t, int tri) {
    W.px_pixel[a] = (int32_t)pix; W.px_t0[a] = t; W.px_tri0[a] = tri;
    const f3 s0 = fold_start(F, pix);
    W.px_sum[3 * a] = s0.x; W.px_sum[3 * a + 1] = s0.y; W.px_sum[3 * a + 2] = s0.z;
    if constexpr (AD) {
        if (F.sum2) { const f3 q0 = fold_start2(F, pix); W.px_sum2[3 * a] = q0.x; W.px_sum2[3 * a + 1] = q0.y; W.px_sum2[3 * a + 2] = q0.z; }
        store_count(F, pix);
    }
}
// ... or does not: its primary ray misses.
template <bool AD>
__device__ __forceinline__ void store_miss(const Frame& F, long long pix) {
    if constexpr (AD) store_live_miss(F, pix); else store_miss_sum(F, pix);
}

// The scene's table of generator words (sq_device_scene::rng): entry `seed` holds tfgen3(seed) as three words, 12 bytes, for the
// seeds [0, cover).  A lane reads it in runs of kRngRun consecutive seeds (its pixel's next samples): 48 contiguous bytes.
constexpr int kRngRun = 4;
constexpr size_t kRngPad = 256;               // bytes behind the last entry: a run that starts below `cover` is read whole
struct RngView { const uint32_t* words; long long cover; };   // words = nullptr: no table, every lane computes

// The radiance of a sample whose primary ray hits s0 and ends there: an absorbing pixel, or a first bounce that misses.
__device__ __forceinline__ f3 level0_radiance(const Surface& s0) { return s0.surf * sq::mk(0, 0, 0) + s0.emit; }
// ... and of one that finish_level1 ended on a hit: L1 = s1*0 + e1, L0 = s0*L1 + e0 (src/Lib.hs:135-137).  Shade1 is what
// that takes of the hit triangle's surface record (surface_of), so that the caller can request it ahead.
struct Shade1 { f3 surf, emit; };
__device__ __forceinline__ Shade1 shade1_of(const SceneView& S, int tri) {
    const float4* q = S.surfs + 3 * (size_t)tri;
    return Shade1{ sq::mk(q[1].x, q[1].y, q[1].z), sq::mk(q[2].x, q[2].y, q[2].z) };
}
__device__ __forceinline__ f3 level1_radiance(const Surface& s0, const Shade1& s1) {
    const f3 L1 = s1.surf * sq::mk(0, 0, 0) + s1.emit;
    return s0.surf * L1 + s0.emit;
}

// Caller-given path depth (sq_scene_set_depth): raytrace with `bounces > 2` made `bounces > D - 1`, src/Lib.hs:127-137
// ----------------------------------------------------------------------------------------------
// A path of depth D is the rays 0 .. D-1; bounce b makes ray b + 1 from the generator words n_b (x and u) and n_{b+1} (v), so the
// last bounce, b = D - 2, reads n_{D-1}: with D <= 8 every word comes from the generator's one Threefish block.
constexpr int kMaxDepth = kDeepestPath;
// Word i (0 .. 7) of a generator whose block is c: the low, then the high half of each of its four words (tfgen3 keeps 0 .. 2).
__device__ __forceinline__ uint32_t tf_word(const uint64_t c[4], int i) {
    const uint64_t w = i < 2 ? c[0] : i < 4 ? c[1] : i < 6 ? c[2] : c[3];
    return (i & 1) ? (uint32_t)(w >> 32) : (uint32_t)w;
}
// The radiance of a path from its triangles: tr[b] = the triangle ray b hit, b = 1 .. kMaxDepth - 1, -1 from the path's end on (a
// miss, or the depth); s0 = the surface ray 0 hit.  L(b) = surfColor_b * L(b+1) + emissive_b *^ emitColor_b from the innermost hit
// outwards, starting from `inner`: black where the depth ends the path, and where a ray misses without a sky; sky(d) of the ray that
// missed under one.  The product with it is formed at the innermost level, as the reference forms it.
__device__ __forceinline__ f3 path_radiance(const SceneView& S, const Surface& s0, const int (&tr)[kMaxDepth], f3 inner) {
    f3 L = inner;
#pragma unroll
    for (int b = kMaxDepth - 1; b >= 1; --b)
        if (tr[b] >= 0) { const Shade1 q = shade1_of(S, tr[b]); L = q.surf * L + q.emit; }
    return s0.surf * L + s0.emit;
}

// ----------------------------------------------------------------------------------------------
// Caller-given point lights (sq_scene_set_lights): raycast with the light a parameter, src/Lib.hs:141-151
// ----------------------------------------------------------------------------------------------
// The lit kernels' own argument (Frame, RayFrame, SceneView, Work and TraceArgs stay as the tuned kernels take them): the scene's light
// table, kLightWords floats per light (pos, power: an sq_light), and how many it holds; the wavefront form's per-active-pixel carry
// of T between light batches (3 floats, in the workspace) and the lights [l_begin, l_end) of this batch.
constexpr int kLightWords = 6;
constexpr int kMaxLights = 4096;              // sq_scene_set_lights refuses more
struct Lights { const float* table; int32_t n; float* carry; int32_t l_begin, l_end; };
struct Light { f3 pos, power; };
__device__ __forceinline__ Light light_of(const Lights& L, int l) {   // l is the same in every lane: scalar loads
    const float* p = L.table + kLightWords * l;
    return Light{ sq::mk(p[0], p[1], p[2]), sq::mk(p[3], p[4], p[5]) };
}
// c_i of squigly_hip.h: what light Li adds at the point p of a surface s0, given the hit `sh` of the shadow ray (Ray p (pos - p)).
__device__ __forceinline__ f3 light_term(const Light& Li, f3 p, const Surface& s0, Hit sh) {
    const float dl = sq::norm(p - Li.pos);
    if (sh.tri >= 0 && !(hit_dist(p, Li.pos - p, sh.t) > dl)) return sq::mk(0, 0, 0);   // maybe True (\pos -> dist pos > dl)
    return sq::mk(Li.power.x / dl, Li.power.y / dl, Li.power.z / dl) * s0.surf;
}
// T folded into a pixel's sums, once per sample of [k_begin, k_end); a raycast query (kSrcRays) stores T itself: no samples, no fold.
template <int SRC>
__device__ __forceinline__ void fold_cast_samples(const Frame& F, f3 T, f3& sum, f3& sum2, bool mom2) {
    if constexpr (SRC == kSrcRays) sum = T;
    else for (int k = F.k_begin; k < F.k_end; ++k) sum = sum + T;
    if (mom2) for (int k = F.k_begin; k < F.k_end; ++k) sum2 = sum2 + T * T;
}

// ----------------------------------------------------------------------------------------------
// Ray queries (sq_intersect_rays_device): intersectBIH of caller-given rays, src/BIH.hs:101-141
// ----------------------------------------------------------------------------------------------
// One chunk of a query: n rays, [n][3] floats each for origin and direction; tri is required, dist and point optional.
struct RayQuery {
    const float* org; const float* dir;
    int32_t* tri; float* dist; float* point;
    long long n;
};
// Maybe Intersection { intersectPoint = o + t *^ d, dist = norm (point - o), surface } (src/Geometry.hs:71-75,134,141), from the very
// expressions the traversal compares (hit_dist); Nothing is tri = -1, dist = +inf, point = (+0, +0, +0).
__device__ __forceinline__ void store_ray_hit(const RayQuery& Q, long long i, f3 o, f3 d, Hit h) {
    const bool hit = h.tri >= 0;
    Q.tri[i] = hit ? h.tri : -1;
    if (Q.dist) Q.dist[i] = hit ? hit_dist(o, d, h.t) : __builtin_inff();
    if (Q.point) {
        const f3 p = hit ? o + sq::scale(h.t, d) : sq::mk(0, 0, 0);
        float* q = Q.point + 3 * i; q[0] = p.x; q[1] = p.y; q[2] = p.z;
    }
}

// The deep kernels' own argument (Frame, SceneView, Work and TraceArgs stay as the tuned kernels take them).  Per slot, in a block of
// the scene's own (sq_device_scene::d_deep), 64-bit offsets throughout:
//   trail : D - 1 arrays of `cap` triangles, level-major; trail[(b-1) * cap + sid] = the triangle ray b hit, -1 = a miss or "nothing
//           below this level adds light" (an absorbing surface, no emitter within the last ray's reach), which reads as a miss below it.
//           Written level by level up to the path's end; sq_deep_fold reads it down to the first -1.
//   oxy   : x and y of the origin of the ray in the slot (D >= 4 only).  The trace kernel puts the hit over org.xy, and
//           intersectPoint = o + t *^ d needs the origin; z stays in org.z.  Ray 1 starts at the pixel's primary hit point, which
//           sq_deep_bounce recomputes as sq_shade1 does, and the last ray's hit point is never formed.
// The words n_1, n_2 ride in the w of the slot's two quads as in the three-level pipeline; n_b, n_{b+1} of a bounce b >= 2 are
// recomputed from the sample's seed: one Threefish block per slot that is still alive there (8 % of the slots at b = 2 in the
// shipped room) moves no byte, where keeping n_3 .. n_{D-1} would write 4 (D - 3) bytes for every slot of the batch.
struct Deep { int32_t depth, level; int32_t* trail; float2* oxy; long long cap; };
// Under a sky (the SKY instantiations' further argument; Deep keeps its layout): the sky, and per slot
//   tmiss : t of the ray that missed (sky_t of its direction as traced), written by sq_deep_bounce where it writes the trail's -1
//           and read by sq_deep_fold behind that -1.  4 bytes where the radiance would take 12: no radiance travels through HBM.
struct DeepSky { Sky sky; float* tmiss; };
