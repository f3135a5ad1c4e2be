// sq_device.hip — gfx950 kernels and the render half of the C-ABI (include/squigly_hip.h).
//
// What runs on the GPU (all hand-written for CDNA4, wave64; per-ray primitives in sq_scene.h):
//   camera-ray generation            src/Lib.hs:107-114                      sq_primary
//   RNG + bounce (scatter / mirror)  src/Lib.hs:133-134,155-198              sq_gen_bounce1, sq_shade1
//   BIH traversal + Moller-Trumbore  src/BIH.hs:101-141, Geometry.hs:117-177 sq_trace_rays (dominant kernel)
//   emissive shade, radiance fold    src/Lib.hs:135-137                      sq_shade1, sq_accumulate
//   ordered per-pixel accumulation   src/Lib.hs:85-88                        sq_accumulate
//   atan tonemap                     src/Lib.hs:93-104                       sq_accumulate
//   raycast under caller-given lights src/Lib.hs:141-151                     sq_cast_pixels; sq_cast_gen, sq_cast_fold (wavefront form)
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
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <chrono>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/squigly_hip.h"
#include "../../include/squigly_host.h"
#include "sq_error.h"
#include "sq_pack.h"
#include "sq_plan.h"
#include "sq_scene.h"

using sq::f3;
using namespace sqd;

#define SQ_HIP(expr)                                                                             \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess) return sq_set_error("%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

constexpr int kOneshotRowBlock = 2; // rows per block when a one-shot call shards a frame over devices (balance: squigly-trace_amd/dist.py)
// Instruction-arbitration priority of a trace wave (s_setprio) in its return / branch steps, and in its leaf scan and pair windows (and
// the store / refill that follows them).  Priority 1 in the windows, 0 in the steps: with the flat steps the headline frame takes
// 52.4-52.5 ms instead of 53.3-53.4 (levels 1, 2 and 3 alike; raising the STEPS instead costs 0.5 ms), one rank's share at 8 ranks
// 8.09 -> 7.98 ms, the streaming form +-0 (profiles/r03zz5_setprio_flat.txt, r03zz6_setprio_stream.txt).  Round 2 had measured
// -0.5 % for the same setting on the kernels of its time and left it off.
constexpr int kPrioSteps = 0, kPrioWindows = 1;
// Pooled trace kernel: triangles a lane tests per window.  Two in both forms: one owner lookup and one set of pulls serve two tests
// (resident form: 83.0 -> 80.5 ms on the headline frame, same run).
constexpr int kPoolTrisResident = 2, kPoolTrisStreaming = 2;

// ----------------------------------------------------------------------------------------------
// Frame description shared by the kernels
// ----------------------------------------------------------------------------------------------
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
    const int blk = j / F.row_block;
    y = (blk * F.n_shards + F.shard) * F.row_block + (j - blk * F.row_block);
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
    const int blk = j / F.row_block;
    y = (blk * F.n_shards + F.shard) * F.row_block + (j - blk * F.row_block);
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

__device__ __forceinline__ f3 load3(const float* p, long long i) { return sq::mk(p[3 * i], p[3 * i + 1], p[3 * i + 2]); }

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
__device__ __forceinline__ void store_fold(const Frame& F, long long pix, f3 sum);
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

// ----------------------------------------------------------------------------------------------
// Variant 1: one lane per pixel, everything in one kernel (cross-check variant; also raycast mode)
// ----------------------------------------------------------------------------------------------
// MV: a multi-view frame (pixels are enumerated linearly, so the lanes of a wave may belong to two views: per-lane camera reads)
// AD: a masked call (single-view): dead pixels leave before the first ray -- nothing wave-wide follows, every lane walks alone --
// and live ones also fold r * r and store their count.
// SRC = kSrcRays: lane i takes the caller's ray i and seed base; its cast branch is raycast itself, not a fold.
template <typename StackT, int SRC, bool AD, typename FrameT>
__device__ __forceinline__ void render_pixels_body(const SceneView& S, const FrameT& F) {
    constexpr bool MV = SRC == kSrcViews;
    extern __shared__ float4 lds_raw[];
    SQ_LDS StackT* stk = to_lds<StackT>(lds_raw) + threadIdx.x;
    const long long pix = (long long)blockIdx.x * kBlock + threadIdx.x;
    int y, x; f3 o0, d0;
    if constexpr (SRC == kSrcRays) {
        if (pix >= (long long)F.h) return;
        y = 0; x = 0;
        o0 = load3(F.ray_org, pix); d0 = load3(F.ray_dir, pix);
    } else if constexpr (MV) {
        if (pix >= (long long)F.n_views * F.view_pixels) return;
        const ViewCam c = view_cam<false>(F, view_coords(F, (int)pix, y, x));
        o0 = c.pos; d0 = primary_dir(c.rot, F.w, F.h, y, x);
    } else {
        if (pix >= (long long)F.local_rows * F.h) return;
        if constexpr (AD) { if (!pixel_live(F, pix)) return; }
        pixel_coords(F, pix, y, x);
        o0 = sq::mk(F.cam_pos[0], F.cam_pos[1], F.cam_pos[2]);
        d0 = primary_dir(F.cam_rot, F.w, F.h, y, x);
    }
    const GlobalNodes N{ S.branches, S.cull_child, S.cull_child != nullptr };
    const int n = F.samples;
    f3 sum = sq::mk(0, 0, 0);                                           // sum = foldl (+) 0
    f3 sum2 = sq::mk(0, 0, 0);                                          // AD with F.sum2: the same fold of r * r
    const Hit h0 = trace_one(S, N, o0, d0, stk, kBlock);
    if (h0.tri >= 0) {
        sum = fold_start(F, pix);
        if constexpr (AD) { if (F.sum2) sum2 = fold_start2(F, pix); }
        const Surface s0 = surface_of(S, h0.tri);
        const f3 p0 = o0 + sq::scale(h0.t, d0);
        if (F.cast) {                                                   // raycast, src/Lib.hs:141-151
            const f3 light = sq::mk(0, 3, -1);
            const float dl = sq::norm(p0 - light);
            const Hit sh = trace_one(S, N, p0, light - p0, stk, kBlock);
            f3 c = sq::mk(0, 0, 0);
            if (!(sh.tri >= 0 && !(hit_dist(p0, light - p0, sh.t) > dl))) c = sq::scale(2 / dl, s0.surf);
            if constexpr (SRC == kSrcRays) sum = c;                       // raycast scene ray: no samples, no fold
            else for (int k = F.k_begin; k < F.k_end; ++k) sum = sum + c;
            if constexpr (AD) { if (F.sum2) for (int k = F.k_begin; k < F.k_end; ++k) sum2 = sum2 + c * c; }
        } else {
            long long rix;
            if constexpr (SRC == kSrcRays) rix = F.ray_seed[pix];       // the caller's seed base
            else rix = (long long)n * ((long long)x + (long long)y * (long long)F.w);   // src/Lib.hs:85
#pragma unroll 1
            for (int k = F.k_begin; k < F.k_end; ++k) {                 // raytrace gen scene ray 0, src/Lib.hs:127-137
                uint32_t n0, n1, n2;
                sq::tfgen3(rix + k, n0, n1, n2);
                f3 L1 = sq::mk(0, 0, 0);
                const f3 d1 = bounce_dir(d0, s0, n0, n1);
                const Hit h1 = trace_one(S, N, p0, d1, stk, kBlock);
                if (h1.tri >= 0) {
                    const Surface s1 = surface_of(S, h1.tri);
                    const f3 p1 = p0 + sq::scale(h1.t, d1);
                    const f3 d2 = bounce_dir(d1, s1, n1, n2);
                    const Hit h2 = trace_one(S, N, p1, d2, stk, kBlock);
                    f3 L2 = sq::mk(0, 0, 0);
                    if (h2.tri >= 0) { const Surface s2 = surface_of(S, h2.tri); L2 = s2.surf * sq::mk(0, 0, 0) + s2.emit; }
                    L1 = s1.surf * L2 + s1.emit;
                }
                const f3 r = s0.surf * L1 + s0.emit;
                sum = sum + r;
                if constexpr (AD) sum2 = sum2 + r * r;
            }
        }
    }
    if constexpr (AD) {
        if (F.sum2) { float* o = F.sum2 + pix * 3; o[0] = sum2.x; o[1] = sum2.y; o[2] = sum2.z; }
        store_count(F, pix);
    }
    if (F.sum) { float* o = F.sum + pix * 3; o[0] = sum.x; o[1] = sum.y; o[2] = sum.z; }
    const f3 avg = sq::scale(1 / (float)F.k_end, sum);                  // src/Lib.hs:88
    if (F.out_avg) { float* o = F.out_avg + pix * 3; o[0] = avg.x; o[1] = avg.y; o[2] = avg.z; }
    if (F.out_rgb) tonemap(avg, F.out_rgb + pix * 3);
}
template <typename StackT, int SRC, bool AD>
__global__ void __launch_bounds__(kBlock) sq_render_pixels(const SceneView S, const FrameOf<SRC> F) { render_pixels_body<StackT, SRC, AD>(S, F); }

// ----------------------------------------------------------------------------------------------
// Variant 2 (default): wavefront pipeline
// ----------------------------------------------------------------------------------------------
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
__device__ __forceinline__ void diag_aux_wave(const Work& W, int diag, bool at_start) {
    if (!diag || (threadIdx.x & 63) != 0) return;
    const unsigned long long live = atomicAdd(&W.stats[kDiagGauge], 0ull);
    if (at_start) atomicAdd(&W.stats[kDiagWaves], 1ull);
    if (live >= (unsigned long long)diag) atomicAdd(&W.stats[at_start ? kDiagStartBeside : kDiagEndBeside], 1ull);
}

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

// Primary rays: trace once per pixel, compact the pixels that hit.
// AD (here and in the other primary passes): a masked call; a dead pixel's lane is treated like the padding of an edge tile.
// kSrcRays: no image to tile -- the caller's rays in index order, 64 consecutive rays per wave.
// SKY (here and in the other primary passes): a miss folds sky(d_0) instead of storing black.
template <typename StackT, int SRC, bool AD, bool SKY, typename FrameT>
__device__ __forceinline__ void primary_body(const SceneView& S, const FrameT& F, const Work& W, const Sky& K) {
    constexpr bool MV = SRC == kSrcViews;
    extern __shared__ float4 lds_raw[];
    SQ_LDS StackT* stk = to_lds<StackT>(lds_raw) + threadIdx.x;
    const long long q = (long long)blockIdx.x * kBlock + threadIdx.x;
    int view = 0;
    long long pix;
    if constexpr (SRC == kSrcRays) pix = q < (long long)F.h ? q : -1;
    else if constexpr (MV) pix = q < primary_padded(F) * F.n_views ? primary_tile_views(F, q, view) : -1;
    else pix = q < primary_padded(F) ? primary_tile(F, q) : -1;
    bool in = pix >= 0;
    if constexpr (AD) in = in && pixel_live(F, pix);
    Hit h0; h0.tri = -1; h0.t = 0;
    f3 d0 = sq::mk(0, 0, 0);
    if (in) {
        int y, x;
        const GlobalNodes N{ S.branches, S.cull_child, S.cull_child != nullptr };
        if constexpr (SRC == kSrcRays) {
            const f3 o0 = load3(F.ray_org, pix);
            d0 = load3(F.ray_dir, pix);
            h0 = trace_one(S, N, o0, d0, stk, kBlock);
        } else if constexpr (MV) {
            pixel_coords(F, pix - (long long)view * F.view_pixels, y, x);
            const ViewCam c = view_cam<true>(F, view);
            d0 = primary_dir(c.rot, F.w, F.h, y, x);
            h0 = trace_one(S, N, c.pos, d0, stk, kBlock);
        } else {
            pixel_coords(F, pix, y, x);
            d0 = primary_dir(F.cam_rot, F.w, F.h, y, x);
            h0 = trace_one(S, N, sq::mk(F.cam_pos[0], F.cam_pos[1], F.cam_pos[2]), d0, stk, kBlock);
        }
    }
    const int a = wave_append(W.n_active, in && h0.tri >= 0);
    if (a >= 0) store_active<AD>(F, W, a, pix, h0.t, h0.tri);
    else if (in) { if constexpr (SKY) store_miss_sky<AD>(F, pix, K, d0); else store_miss<AD>(F, pix); }
}
template <typename StackT, int SRC, bool AD, typename... SkyT>
__global__ void __launch_bounds__(kBlock) sq_primary(const SceneView S, const FrameOf<SRC> F, const Work W, const SkyT... K) {
    primary_body<StackT, SRC, AD, sizeof...(SkyT) != 0>(S, F, W, sky_arg<Sky>(K...));
}

struct Pixel0 { f3 p0, d0; Surface s0; int y, x; };
// Everything the kernels downstream of the primary pass know about active pixel a, and the one place where they learn it.
// kSrcViews: the pixel's view comes from its index, and its camera from the table (once per active pixel, not per sample).
// kSrcRays: the "pixel" is the caller's ray px_pixel[a]; y and x stay unset (its seed base comes from seed_base, not from coordinates).
template <int SRC, typename FrameT>
__device__ __forceinline__ Pixel0 load_pixel0(const SceneView& S, const FrameT& F, const Work& W, int a) {
    constexpr bool MV = SRC == kSrcViews;
    Pixel0 P;
    if constexpr (SRC == kSrcRays) {
        const long long i = W.px_pixel[a];
        P.y = 0; P.x = 0;
        P.d0 = load3(F.ray_dir, i);
        P.p0 = load3(F.ray_org, i) + sq::scale(W.px_t0[a], P.d0);           // intersectPoint, src/Geometry.hs:134
    } else if constexpr (MV) {
        const ViewCam c = view_cam<false>(F, view_coords(F, (int)W.px_pixel[a], P.y, P.x));
        P.d0 = primary_dir(c.rot, F.w, F.h, P.y, P.x);
        P.p0 = c.pos + sq::scale(W.px_t0[a], P.d0);
    } else {
        pixel_coords(F, (int)W.px_pixel[a], P.y, P.x);
        P.d0 = primary_dir(F.cam_rot, F.w, F.h, P.y, P.x);
        P.p0 = sq::mk(F.cam_pos[0], F.cam_pos[1], F.cam_pos[2]) + sq::scale(W.px_t0[a], P.d0);   // intersectPoint, src/Geometry.hs:134
    }
    P.s0 = surface_of(S, W.px_tri0[a]);
    return P;
}
// The seed base of active pixel a: the generator of its sample k is mkTFGen (seed_base + k).  A frame's rule is src/Lib.hs:85;
// a query's is the caller's array.
template <int SRC, typename FrameT>
__device__ __forceinline__ long long seed_base(const FrameT& F, const Work& W, int a, const Pixel0& P) {
    if constexpr (SRC == kSrcRays) return F.ray_seed[W.px_pixel[a]];
    else return (long long)F.samples * ((long long)P.x + (long long)P.y * (long long)F.w);   // src/Lib.hs:85
}
// surfColor == 0 (an emitter such as data/scene.sq:13-15) makes `surfColor * raytrace ...` exactly +0
// whenever the nested radiance is finite and >= +0, so the nested rays need not be traced.  Only used
// when every material component is >= +0 (checked at upload), where that premise holds.
__device__ __forceinline__ bool absorbs(const SceneView& S, const Surface& s) {
    return S.nonneg_materials && s.surf.x == 0.0f && s.surf.y == 0.0f && s.surf.z == 0.0f;
}
// A sample ends at the first bounce level: ray 1 missed (tri1 = -1, raytrace ... 1 = black), or hit triangle tri1 and nothing
// beyond that hit can add light (an absorbing surface, or no emitter within reach of ray 2).
__device__ __forceinline__ void finish_level1(const Work& W, long long sid, int tri1) {
    W.tri1[sid] = tri1;
    W.state[sid] = kDone;
}
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
__device__ __forceinline__ int2 slot_hit(const float4& org) { return make_int2(__float_as_int(org.x), __float_as_int(org.y)); }   // what the trace kernel left in org.xy

// The scene's table of generator words (sq_device_scene::rng): entry `seed` holds tfgen3(seed) as three words, 12 bytes, for the
// seeds [0, cover).  A lane reads it in runs of kRngRun consecutive seeds (its pixel's next samples): 48 contiguous bytes.
constexpr int kRngRun = 4;
constexpr size_t kRngPad = 256;               // bytes behind the last entry: a run that starts below `cover` is read whole
struct RngView { const uint32_t* words; long long cover; };   // words = nullptr: no table, every lane computes
struct RngRun { uint32_t w[3 * kRngRun]; };
// The run of the seeds [seed, seed + kRngRun): three 16-byte loads when the run is 16-byte aligned (seed % 4 == 0), words otherwise.
__device__ __forceinline__ RngRun rng_load_run(const uint32_t* words, long long seed) {
    RngRun r;
    const uint32_t* p = words + 3 * seed;
    if ((seed & 3) == 0) {
        const uint4* q = reinterpret_cast<const uint4*>(p);
        const uint4 a = q[0], b = q[1], c = q[2];
        r.w[0] = a.x; r.w[1] = a.y; r.w[2] = a.z; r.w[3] = a.w; r.w[4] = b.x; r.w[5] = b.y; r.w[6] = b.z; r.w[7] = b.w;
        r.w[8] = c.x; r.w[9] = c.y; r.w[10] = c.z; r.w[11] = c.w;
    } else {
#pragma unroll
        for (int i = 0; i < 3 * kRngRun; ++i) r.w[i] = p[i];
    }
    return r;
}
// Fills the runs [quad_begin, quad_end) of the table: one thread per run, tfgen3 of its four seeds, three 16-byte stores (a wave
// writes 3 KB in a row).  The last run may reach into the padding behind the table.
__global__ void __launch_bounds__(kBlock) sq_rng_fill(uint32_t* words, long long quad_begin, long long quad_end) {
    for (long long q = quad_begin + (long long)blockIdx.x * kBlock + threadIdx.x; q < quad_end; q += (long long)gridDim.x * kBlock) {
        uint32_t w[3 * kRngRun];
#pragma unroll
        for (int j = 0; j < kRngRun; ++j) sq::tfgen3(q * kRngRun + j, w[3 * j], w[3 * j + 1], w[3 * j + 2]);
        uint4* o = reinterpret_cast<uint4*>(words + 3 * kRngRun * q);
        o[0] = make_uint4(w[0], w[1], w[2], w[3]); o[1] = make_uint4(w[4], w[5], w[6], w[7]); o[2] = make_uint4(w[8], w[9], w[10], w[11]);
    }
}

// Level-1 culling (sq_host.cpp, level1_tables, has the lemma): does the half-plane { p0 + t d1 + s nd : t >= 0, s real } provably
// miss the box [lo - m, hi + m]?  Binary64 on the exact fp32 values; either separation must hold by more than 1e-9 of the scale.
__device__ __forceinline__ bool halfplane_misses_box(f3 p0, f3 d1, f3 nd, const double* lo, const double* hi, double m) {
    const double px[3] = { p0.x, p0.y, p0.z }, dx[3] = { d1.x, d1.y, d1.z }, nx[3] = { nd.x, nd.y, nd.z };
    double g[3], h[3], scale = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) { g[k] = 0.5 * (lo[k] + hi[k]) - px[k]; h[k] = 0.5 * (hi[k] - lo[k]) + m; scale += __builtin_fabs(g[k]) + h[k]; }
    const double tol = 1e-9 * scale;
    const double N[3] = { dx[1] * nx[2] - dx[2] * nx[1], dx[2] * nx[0] - dx[0] * nx[2], dx[0] * nx[1] - dx[1] * nx[0] };
    const double dist = __builtin_fabs(N[0] * g[0] + N[1] * g[1] + N[2] * g[2]);
    const double rad = __builtin_fabs(N[0]) * h[0] + __builtin_fabs(N[1]) * h[1] + __builtin_fabs(N[2]) * h[2];
    if (dist > rad + tol) return true;                                  // the whole box on one side of the plane
    const double f = (dx[0] * nx[0] + dx[1] * nx[1] + dx[2] * nx[2]) / (nx[0] * nx[0] + nx[1] * nx[1] + nx[2] * nx[2]);
    const double w[3] = { dx[0] - f * nx[0], dx[1] - f * nx[1], dx[2] - f * nx[2] };
    const double side = w[0] * g[0] + w[1] * g[1] + w[2] * g[2] + __builtin_fabs(w[0]) * h[0] + __builtin_fabs(w[1]) * h[1] + __builtin_fabs(w[2]) * h[2];
    return side < -tol;                                                 // the whole box behind ray 1, seen across nd
}
// May the scattered ray 1 = (p0, d1) of a sample whose generator goes on with n1, n2 be dropped, the sample finished as a
// first-bounce miss?  Conditions (1)-(3) of the lemma; p0_ok: |p0|^2 is inside the lemma's limit (per pixel).
__device__ __forceinline__ bool level1_culled(const SceneView& S, const Level1Cull& C, bool p0_ok, f3 p0, f3 d1, uint32_t n1, uint32_t n2) {
    const float eps = 0.0001f, inf = __builtin_inff();
    // ray 1 inside the limits of sq_cull_boxes (as trav_begin decides Trav::cull)
    const f3 df = sq::mk(1.0f / d1.x, 1.0f / d1.y, 1.0f / d1.z);
    const f3 nodf = sq::mk(-p0.x * df.x, -p0.y * df.y, -p0.z * df.z);
    const float dd = sq::dot(d1, d1);
    if (!(p0_ok && finite3(d1) && finite3(df) && finite3(nodf) && dd >= C.d2min && dd <= C.d2max)) return false;
    // (2) the box of everything that would mirror: the class of the smallest value >= unit_float(n1), if any
    const float un1 = sq::unit_float(n1);
    bool has = false; float b[6] = { 0, 0, 0, 0, 0, 0 };
#pragma unroll
    for (int c = kLevel1Classes - 1; c >= 0; --c) {
        if (c < C.n_classes && C.class_val[c] >= un1) {
            has = true;
#pragma unroll
            for (int k = 0; k < 6; ++k) b[k] = C.class_box[c][k];
        }
    }
    if (has && cull_slab(b, df, nodf)) return false;
    // the direction of ray 2 up to its sign
    const f3 nd = random_vector(n1, n2);
    const float nn = sq::dot(nd, nd);
    if (!(nn >= C.d2min && nn <= C.d2max)) return false;
    // (1) no emitter accepts ray 1; and the smallest determinant with which one could accept ray 2
    float amin = inf;
    for (int j = 0; j < S.n_emitters; ++j) {
        const float* tp = S.tris + 9 * (size_t)S.emitters[j];
        const f3 v0 = sq::mk(tp[0], tp[1], tp[2]), e1 = sq::mk(tp[3], tp[4], tp[5]), e2 = sq::mk(tp[6], tp[7], tp[8]);
        float t_unused;
        if (moller_trumbore(p0, d1, v0, e1, e2, t_unused)) return false;
        const float a = sq::dot(e1, sq::cross(nd, e2));                 // moller_trumbore's `a` for (any origin, nd); -nd gives -a
        if (!(a > -eps && a < eps)) amin = sq::hmin(amin, __builtin_fabsf(a));
    }
    if (amin == inf) return true;                                       // every emitter rejects +-nd by its determinant alone
    if (!(amin < inf)) return false;
    // (3)
    return halfplane_misses_box(p0, d1, nd, C.em_lo, C.em_hi, C.em_rho * ((double)eps / (double)amin) + C.em_add);
}

// Depth-0 bounce of every sample of the batch: RNG, bounceRay, ray 1 into slot sid (src/Lib.hs:133-134).
// One thread per active pixel (blockIdx.y splits the samples of a pixel when a frame has few pixels): everything that is
// the same for every sample of a pixel -- the pixel's coordinates, primary direction, hit point, surface, seed base -- is
// computed once, not 256 times; consecutive threads still write consecutive slots (sid = k * A + a).
// The generator words of a sample come from the scene's table R when all the pixel's seeds [rix, rix + samples) lie in it, and
// from tfgen3 otherwise (no table, a seed row past its cover, a query's negative or huge seed): the same words either way.
// Neighbouring lanes are neighbouring pixels, samples * 12 bytes apart in the table, so a lane takes its samples in runs of
// kRngRun (a blockIdx.y gets a contiguous range of runs) and requests the next run before it works on the current one.
template <int SRC, typename FrameT>
__device__ __forceinline__ void gen_bounce1_body(const SceneView& S, const FrameT& F, const Work& W, int k_base, int k_count, const RngView R, const Level1Cull& C) {
    const int A = *W.n_active;
    unsigned int n_culled = 0;
    diag_aux_wave(W, F.diag, true);
    const int n_runs = (k_count + kRngRun - 1) / kRngRun, runs_per_y = (n_runs + (int)gridDim.y - 1) / (int)gridDim.y;
    const int g_begin = min(n_runs, (int)blockIdx.y * runs_per_y), g_end = min(n_runs, g_begin + runs_per_y);
    for (int a = blockIdx.x * kBlock + threadIdx.x; a < A; a += gridDim.x * kBlock) {
        const Pixel0 P = load_pixel0<SRC>(S, F, W, a);
        const long long rix = seed_base<SRC>(F, W, a, P);
        if (absorbs(S, P.s0)) {                                         // no ray, and nothing else per sample: sq_accumulate knows the pixel absorbs
            for (int kl = g_begin * kRngRun; kl < min(k_count, g_end * kRngRun); ++kl) W.state[(long long)kl * A + a] = kDone;
            continue;
        }
        const long long first = rix + k_base;                           // the seed of kl = 0: mkTFGen (rix + k), src/Lib.hs:86
        const bool use = R.words != nullptr && rix >= 0 && rix <= R.cover - (long long)F.samples;
        const bool p0_ok = C.on && finite3(P.p0) && sq::dot(P.p0, P.p0) <= C.o2max;   // level-1 culling: the pixel's share of ray 1's limits
        RngRun next{};
        if (use && g_begin < g_end) next = rng_load_run(R.words, first + (long long)g_begin * kRngRun);
        for (int g = g_begin; g < g_end; ++g) {
            RngRun cur = next;
            if (use && g + 1 < g_end) next = rng_load_run(R.words, first + (long long)(g + 1) * kRngRun);
#pragma unroll 1                                                   // one copy of the sample's code: unrolled, four Threefish blocks interleave into 256 VGPRs
            for (int kl = g * kRngRun; kl < min(k_count, (g + 1) * kRngRun); ++kl) {
                const long long sid = (long long)kl * A + a;
                uint32_t n0, n1, n2;
                if (use) {                                              // the run's first entry, then the run moves up by one
                    n0 = cur.w[0]; n1 = cur.w[1]; n2 = cur.w[2];
#pragma unroll
                    for (int i = 0; i + 3 < 3 * kRngRun; ++i) cur.w[i] = cur.w[i + 3];
                } else {
                    // the seed steps by one per iteration; seen as such, the optimiser turns the Threefish block's seed-dependent
                    // sums into induction variables of this loop (256 VGPRs and scratch): the empty asm hides the recurrence
                    long long seed = first + kl;
                    asm volatile("" : "+v"(seed));
                    sq::tfgen3(seed, n0, n1, n2);
                }
                if (!scatters(P.s0, n0)) {                              // mirror: traced once per pixel (sq_mirror1_*); the slot only carries n1, n2
                    W.state[sid] = kMirror;
                    *reinterpret_cast<float2*>(reinterpret_cast<float*>(W.org + sid) + 2) = make_float2(__uint_as_float(n2), __uint_as_float(n1));   // .z = n2, .w = n1
                    continue;
                }
                const f3 d1 = scatter_dir(P.d0, P.s0, n0, n1);
                // Level-1 culling: nothing ray 1 can hit changes the sample's radiance, which is that of a first-bounce miss
                if (C.on && level1_culled(S, C, p0_ok, P.p0, d1, n1, n2)) { finish_level1(W, sid, -1); ++n_culled; continue; }
                W.state[sid] = kRay1;
                W.org[sid] = make_float4(P.p0.x, P.p0.y, P.p0.z, __uint_as_float(n1));
                W.dir[sid] = make_float4(d1.x, d1.y, d1.z, __uint_as_float(n2));
            }
        }
    }
    if (C.on) {                                                         // rays culled, one atomic per wave (the loop above has ended for all its lanes)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) n_culled += __shfl_xor(n_culled, o);
        if ((threadIdx.x & 63) == 0 && n_culled) atomicAdd(&W.stats[kStatLevel1Culled], (unsigned long long)n_culled);
    }
    diag_aux_wave(W, F.diag, false);
}
// Four waves per SIMD (118 VGPRs, no scratch): with the level-1 culling test inlined, six (80 VGPRs) spill 38 registers and five
// (96) spill 22; the headline frame measured 43.2 / 42.1 / 41.7 ms at six / five / four
constexpr int kGen1Waves = 4;
template <int SRC>
__global__ void __launch_bounds__(kBlock, kGen1Waves) sq_gen_bounce1(const SceneView S, const FrameOf<SRC> F, const Work W, int k_base, int k_count, const RngView R, const Level1Cull C) { gen_bounce1_body<SRC>(S, F, W, k_base, k_count, R, C); }

// The depth-0 mirror ray of every active pixel, once per frame (slot a = active pixel a).
// `base`: first of the *n_active slots the mirror rays use (0 when they have a launch of their own, the spare region
// behind the sample slots when they ride at the head of the first bounce launch).
template <int SRC, typename FrameT>
__device__ __forceinline__ void mirror1_gen_body(const SceneView& S, const FrameT& F, const Work& W, long long base) {
    const int A = *W.n_active;
    for (int a = blockIdx.x * kBlock + threadIdx.x; a < A; a += gridDim.x * kBlock) {
        const Pixel0 P = load_pixel0<SRC>(S, F, W, a);
        const long long sl = base + a;
        if (absorbs(S, P.s0)) { W.state[sl] = kDone; continue; }
        const f3 d1 = mirror_dir(P.d0, P.s0);
        W.state[sl] = kRay1;
        W.org[sl] = make_float4(P.p0.x, P.p0.y, P.p0.z, 0.0f);
        W.dir[sl] = make_float4(d1.x, d1.y, d1.z, 0.0f);
    }
}
template <int SRC>
__global__ void __launch_bounds__(kBlock) sq_mirror1_gen(const SceneView S, const FrameOf<SRC> F, const Work W, long long base) { mirror1_gen_body<SRC>(S, F, W, base); }
__global__ void __launch_bounds__(kBlock) sq_mirror1_store(const Work W, long long base) {
    const int A = *W.n_active;
    for (int a = blockIdx.x * kBlock + threadIdx.x; a < A; a += gridDim.x * kBlock) {
        const bool live = W.state[base + a] == kRay1;
        const int2 hit = slot_hit(W.org[base + a]);
        W.px_mt[a] = live ? __int_as_float(hit.x) : 0.0f;
        W.px_mtri[a] = live ? hit.y : -1;
    }
}

// Primary rays through the pooled trace kernel (option "primary_pooled"): one slot per pixel of this shard, one trace launch with
// k_count = 1, then the hits are compacted into the active-pixel list exactly as sq_primary does.  The one-ray-per-lane walk of
// sq_primary(_resident) lasts as long as its most expensive wave (64 neighbouring pixels on dense geometry: 0.5 ms on the headline
// scene however small the shard); the pooled leaf phase walks such a wave faster.  W.n_active[48] is the launch's queue length.
// AD: a dead pixel's slot is flagged kDone, so it is not in the launch's queue and sq_primary_store skips it.
// kSrcRays: the caller's rays as they are.
template <int SRC, bool AD>
__global__ void __launch_bounds__(kBlock) sq_primary_gen(const FrameOf<SRC> F, const Work W, long long total) {
    if (blockIdx.x == 0 && threadIdx.x == 0) W.n_active[48] = (int32_t)total;
    for (long long pix = (long long)blockIdx.x * kBlock + threadIdx.x; pix < total; pix += (long long)gridDim.x * kBlock) {
        if constexpr (AD) { if (!pixel_live(F, pix)) { W.state[pix] = kDone; continue; } }
        if constexpr (SRC == kSrcRays) {
            const f3 o = load3(F.ray_org, pix), d = load3(F.ray_dir, pix);
            W.state[pix] = kRay1;
            W.org[pix] = make_float4(o.x, o.y, o.z, 0.0f);
            W.dir[pix] = make_float4(d.x, d.y, d.z, 0.0f);
        } else if constexpr (SRC == kSrcViews) {
            int y, x;
            const ViewCam c = view_cam<false>(F, view_coords(F, (int)pix, y, x));
            const f3 d = primary_dir(c.rot, F.w, F.h, y, x);
            W.state[pix] = kRay1;
            W.org[pix] = make_float4(c.pos.x, c.pos.y, c.pos.z, 0.0f);
            W.dir[pix] = make_float4(d.x, d.y, d.z, 0.0f);
        } else {
            int y, x;
            pixel_coords(F, pix, y, x);
            const f3 d = primary_dir(F.cam_rot, F.w, F.h, y, x);
            W.state[pix] = kRay1;
            W.org[pix] = make_float4(F.cam_pos[0], F.cam_pos[1], F.cam_pos[2], 0.0f);
            W.dir[pix] = make_float4(d.x, d.y, d.z, 0.0f);
        }
    }
}
// Under a sky a miss folds sky(d_0): d_0 is the direction sq_primary_gen put into the slot, which the trace kernel leaves as it took it.
template <bool AD, typename... SkyT>
__global__ void __launch_bounds__(kBlock) sq_primary_store(const Frame F, const Work W, long long total, const SkyT... K) {
    for (long long base = (long long)blockIdx.x * kBlock; base < total; base += (long long)gridDim.x * kBlock) {   // whole waves stay together (ballot)
        const long long pix = base + threadIdx.x;
        bool in = pix < total;
        if constexpr (AD) in = in && W.state[pix] == kRay1;              // what sq_primary_gen<AD> decided (the trace kernel leaves the state byte alone)
        const int2 hit = in ? slot_hit(W.org[pix]) : make_int2(0, -1);
        const int a = wave_append(W.n_active, in && hit.y >= 0);
        if (a >= 0) store_active<AD>(F, W, a, pix, __int_as_float(hit.x), hit.y);
        else if (in) {
            if constexpr (sizeof...(SkyT) != 0) { const float4 d = W.dir[pix]; store_miss_sky<AD>(F, pix, K..., sq::mk(d.x, d.y, d.z)); }
            else store_miss<AD>(F, pix);
        }
    }
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
// Default form, before the trace launch: the chunk's rays into the first n workspace slots as first-level rays of a one-level
// queue (k_count = 1, as sq_primary_gen does for the primary rays); W.n_active[48] is the launch's queue length.
__global__ void __launch_bounds__(kBlock) sq_rays_stage(const RayQuery Q, const Work W) {
    if (blockIdx.x == 0 && threadIdx.x == 0) W.n_active[48] = (int32_t)Q.n;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < Q.n; i += (long long)gridDim.x * kBlock) {
        const f3 o = load3(Q.org, i), d = load3(Q.dir, i);
        W.state[i] = kRay1;
        W.org[i] = make_float4(o.x, o.y, o.z, 0.0f);
        W.dir[i] = make_float4(d.x, d.y, d.z, 0.0f);
    }
}
// ... and after it: the hit the trace kernel left in each slot, with the caller's ray, into tri / dist / point.
__global__ void __launch_bounds__(kBlock) sq_rays_store(const RayQuery Q, const Work W) {
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < Q.n; i += (long long)gridDim.x * kBlock) {
        const int2 hit = slot_hit(W.org[i]);
        Hit h; h.t = __int_as_float(hit.x); h.tri = hit.y;
        store_ray_hit(Q, i, load3(Q.org, i), load3(Q.dir, i), h);
    }
}
// Variant 1: one lane per ray, the whole query in one kernel (the per-lane walk of sq_primary; the cross-check of the default form,
// and the form that takes the taller trees of the per-pixel kernel).
template <typename StackT>
__global__ void __launch_bounds__(kBlock) sq_intersect_lanes(const SceneView S, const RayQuery Q) {
    extern __shared__ float4 lds_raw[];
    SQ_LDS StackT* stk = to_lds<StackT>(lds_raw) + threadIdx.x;
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= Q.n) return;
    const GlobalNodes N{ S.branches, S.cull_child, S.cull_child != nullptr };
    const f3 o = load3(Q.org, i), d = load3(Q.dir, i);
    store_ray_hit(Q, i, o, d, trace_one(S, N, o, d, stk, kBlock));
}
// sq_camera_rays_device: the primary ray of every pixel of a shard (makeRay, src/Lib.hs:107-114), by the renderer's own primary_dir,
// laid out like a frame's d_avg ([rows][h][3], local row-major pixel index).
__global__ void __launch_bounds__(kBlock) sq_camera_rays(const Frame F, float* org, float* dir, long long total) {
    for (long long pix = (long long)blockIdx.x * kBlock + threadIdx.x; pix < total; pix += (long long)gridDim.x * kBlock) {
        int y, x;
        pixel_coords(F, pix, y, x);
        const f3 d = primary_dir(F.cam_rot, F.w, F.h, y, x);
        float* o = org + 3 * pix; o[0] = F.cam_pos[0]; o[1] = F.cam_pos[1]; o[2] = F.cam_pos[2];
        float* q = dir + 3 * pix; q[0] = d.x; q[1] = d.y; q[2] = d.z;
    }
}

// Multi-view frames: copies a chunk of cameras into the scene's camera table.  The cameras travel as kernel arguments, which are
// captured when the launch is enqueued: the table is filled in stream order, and the caller's array is not read after the call.
constexpr int kCamChunk = 64;                 // cameras per staging launch: 64 x 48 B = 3 KB of arguments (the limit is 4 KB)
struct CamChunk { float v[kCamWords * kCamChunk]; };
__global__ void __launch_bounds__(kBlock) sq_stage_cams(float* table, int n, const CamChunk C) {
    for (int i = threadIdx.x; i < kCamWords * n; i += kBlock) table[i] = C.v[i];
}

// After ray 1: a miss finishes the sample; a hit either finishes it (absorbing surface) or puts ray 2 in the slot.
// One thread per active pixel, like sq_gen_bounce1: the primary surface, the hit point and the pixel's mirror ray and its hit
// are per-pixel values.  It waits on memory two thirds of its time, so a slot's state byte decides what else is read (nothing
// for a finished slot, the generator words for a mirrored one, ray and hit for a traced one), the state and generator words
// are requested two samples ahead and the rest one sample ahead.
// (The body takes its arguments by value, as the kernel does: by reference the multi-view kernel's SGPR spills went from 25 to 30.)
template <int SRC, typename FrameT>
__device__ __forceinline__ void shade1_body(const SceneView S, const FrameT F, const Work W, int k_count) {
    const int A = *W.n_active;
    diag_aux_wave(W, F.diag, true);
    struct First { uint8_t st; float4 org; };     // org: .xy = the hit the trace kernel left (traced slots), .w = n1
    struct Second { float4 dir; };                // .w = n2.  Ray 1 starts at the pixel's primary hit point P.p0 (sq_gen_bounce1 stored that very value): no origin is re-read
    for (int a = blockIdx.x * kBlock + threadIdx.x; a < A; a += gridDim.x * kBlock) {
        const Pixel0 P = load_pixel0<SRC>(S, F, W, a);
        if (absorbs(S, P.s0)) continue;                                 // every slot of the pixel is kDone since sq_gen_bounce1
        const f3 d1_mirror = mirror_dir(P.d0, P.s0);
        const int2 hit_mirror = make_int2(__float_as_int(W.px_mt[a]), W.px_mtri[a]);
        const int step = gridDim.y;
        auto first = [&](int kl) { First f; const long long sid = (long long)kl * A + a; f.st = W.state[sid]; f.org = W.org[sid]; return f; };
        auto second = [&](int kl, uint8_t st) {
            Second q{};
            if (st == kRay1) { const long long sid = (long long)kl * A + a; q.dir = W.dir[sid]; }
            return q;
        };
        int kl = blockIdx.y;
        First f1{}, f2{}; Second q1{};
        if (kl < k_count) { f1 = first(kl); q1 = second(kl, f1.st); }
        if (kl + step < k_count) f2 = first(kl + step);
        for (; kl < k_count; kl += step) {
            const First cur = f1; const Second q = q1;
            f1 = f2;
            if (kl + step < k_count) q1 = second(kl + step, f1.st);
            if (kl + 2 * step < k_count) f2 = first(kl + 2 * step);
            if (cur.st == kDone) continue;
            const long long sid = (long long)kl * A + a;
            const uint2 r = make_uint2(__float_as_uint(cur.org.w), __float_as_uint(cur.st == kMirror ? cur.org.z : q.dir.w));   // (n1, n2)
            f3 d1, p0;
            int2 hit;
            if (cur.st == kMirror) { d1 = d1_mirror; p0 = P.p0; hit = hit_mirror; }          // the pixel's mirror ray and its hit
            else { d1 = sq::mk(q.dir.x, q.dir.y, q.dir.z); p0 = P.p0; hit = slot_hit(cur.org); }
            const int tri1 = hit.y;
            if (tri1 < 0) { finish_level1(W, sid, -1); continue; }      // raytrace ... 1 = black
            const Surface s1 = surface_of(S, tri1);
            if (absorbs(S, s1)) { finish_level1(W, sid, tri1); continue; }
            const f3 p1 = p0 + sq::scale(__int_as_float(hit.x), d1);
            const f3 d2 = bounce_dir(d1, s1, r.x, r.y);                 // gen advanced by one: x = u = p(n1), v = p(n2)
            // Ray 2 is the last one: all it contributes is L2 = s2*0 + e2, the emission of whatever it hits
            // (src/Lib.hs:129,135-137).  Whatever the traversal returns is a triangle that mollerTrumbore accepted
            // for this very ray, so if the SAME function rejects every emissive triangle, the result is a
            // non-emissive hit or a miss, and L2 is exactly (+0,+0,+0) either way (materials are finite).
            // Only rays that could reach an emitter are traced.
            if (S.n_emitters >= 0) {
                bool may_reach = false;
                for (int j = 0; j < S.n_emitters && !may_reach; ++j) {
                    const int et = S.emitters[j];
                    const float* tp = S.tris + 9 * (size_t)et;
                    float t_unused;
                    may_reach = moller_trumbore(p1, d2, sq::mk(tp[0], tp[1], tp[2]), sq::mk(tp[3], tp[4], tp[5]), sq::mk(tp[6], tp[7], tp[8]), t_unused);
                }
                if (!may_reach) { finish_level1(W, sid, tri1); continue; }    // L2 = +0: L1 is what an absorbing s1 gives
            }
            W.state[sid] = kRay2;
            W.org[sid] = make_float4(p1.x, p1.y, p1.z, 0.0f);
            W.dir[sid] = make_float4(d2.x, d2.y, d2.z, __int_as_float(tri1));
        }
    }
    diag_aux_wave(W, F.diag, false);
}
template <int SRC>
__global__ void __launch_bounds__(kBlock) sq_shade1(const SceneView S, const FrameOf<SRC> F, const Work W, int k_count) { shade1_body<SRC>(S, F, W, k_count); }

// After ray 2: L2 = s2*0 + e2 (or black), L1 = s1*L2 + e1, L0 = s0*L1 + e0   (src/Lib.hs:135-137).
// Not a kernel of its own: the 8 % of the slots that still hold a second bounce ray are folded where their radiance is
// consumed (sq_accumulate), which saves a pass over every slot's state and the round trip of their radiance through HBM.
__device__ __forceinline__ f3 shade2_radiance(const SceneView& S, const Work& W, long long sid, const Surface& s0) {
    const int tri1 = reinterpret_cast<const int*>(W.dir + sid)[3], tri2 = reinterpret_cast<const int*>(W.org + sid)[1];   // dir.w, and the hit's triangle in org.y: 4 bytes each
    f3 L2 = sq::mk(0, 0, 0);
    if (tri2 >= 0) { const Surface s2 = surface_of(S, tri2); L2 = s2.surf * sq::mk(0, 0, 0) + s2.emit; }
    const Surface s1 = surface_of(S, tri1);
    const f3 L1 = s1.surf * L2 + s1.emit;
    return s0.surf * L1 + s0.emit;
}

// sum outcomes, in sample order (src/Lib.hs:88); on the call's last batch: the fold to F.sum (range calls), avg over the k_end
// samples folded so far, tonemap, store.
// GROUPED: see the comment in the loop; two kernels because the grouped loop's registers cost the plain one a third of its waves.
// MOM2: the call carries second moments (F.sum2, W.px_sum2): every radiance r also adds r * r, each product rounded before its add,
// to a second fold.  A template parameter, so that every other frame runs the instruction stream it ran without it.
template <bool GROUPED, bool MOM2 = false>
__global__ void __launch_bounds__(kBlock) sq_accumulate(const SceneView S, const Frame F, const Work W, int k_count, int last) {
    const int A = *W.n_active;
    for (int a = blockIdx.x * kBlock + threadIdx.x; a < A; a += gridDim.x * kBlock) {
        f3 sum = sq::mk(W.px_sum[3 * a], W.px_sum[3 * a + 1], W.px_sum[3 * a + 2]);
        f3 sum2 = sq::mk(0, 0, 0);
        if constexpr (MOM2) sum2 = sq::mk(W.px_sum2[3 * a], W.px_sum2[3 * a + 1], W.px_sum2[3 * a + 2]);
        const Surface s0 = surface_of(S, W.px_tri0[a]);
        // The sum is the reference's left fold over the samples (src/Lib.hs:88): one dependent add per sample.  With fewer active
        // pixels than threads (one rank's share of a frame at 8 ranks) a thread is a chain of `samples` memory round trips and the
        // launch lasts as long as that chain: there (GROUPED, chosen by the host from the shard's pixel count) the states and triangles of 16 samples are requested together, then
        // their surface records (a slot that still holds a second bounce ray has no triangle yet; what is read there is not used),
        // and the radiances are added in order -- 384 -> 280 us on such a share when the radiances themselves were read.  A whole
        // frame is bound by the bytes it moves and keeps a loop with one request per sample (the grouped loop took 0.98 ... 1.58 ms
        // against 0.83 ms there with groups of 2 ... 16: profiles/r03l_accumulate_groups.txt).
        const f3 rad0 = level0_radiance(s0);
        auto add = [&](f3 rad) { sum = sum + rad; if constexpr (MOM2) sum2 = sum2 + rad * rad; };
        // What a slot says about its finished sample: its state and, for kDone, the triangle of finish_level1.  `at` requests the
        // surface record for it: triangle 0's where none is needed (a miss, or kRay2, whose tri1 entry is stale), so that the
        // request does not depend on a branch.
        struct Fin { uint8_t st; int tri; };
        auto fin_of = [&](long long sid) { Fin f; f.st = W.state[sid]; f.tri = W.tri1[sid]; return f; };
        auto hit1 = [](const Fin& f) { return f.st == kDone && f.tri >= 0; };
        auto at = [&](const Fin& f) { return shade1_of(S, hit1(f) ? f.tri : 0); };
        if (absorbs(S, s0)) {                                           // every sample ended at depth 0 (sq_gen_bounce1): nothing to read
            for (int k = 0; k < k_count; ++k) add(rad0);
        } else if constexpr (GROUPED) {
            constexpr int kAccGroup = 16;
            for (int k0 = 0; k0 < k_count; k0 += kAccGroup) {
                Fin f[kAccGroup]; f3 r[kAccGroup];
#pragma unroll
                for (int j = 0; j < kAccGroup; ++j) f[j] = fin_of((long long)min(k0 + j, k_count - 1) * A + a);   // past the end: the last sample again, dropped below
#pragma unroll
                for (int j = 0; j < kAccGroup; ++j) r[j] = hit1(f[j]) ? level1_radiance(s0, at(f[j])) : rad0;
#pragma unroll
                for (int j = 0; j < kAccGroup; ++j) {
                    if (k0 + j >= k_count) break;
                    const long long sid = (long long)(k0 + j) * A + a;
                    add(f[j].st == kRay2 ? shade2_radiance(S, W, sid, s0) : r[j]);
                }
            }
        } else {
            Fin next{ kDone, -1 };                                      // the next slot is requested one sample ahead
            if (k_count > 0) next = fin_of(a);
            for (int k = 0; k < k_count; ++k) {
                const long long sid = (long long)k * A + a;
                const Fin cur = next;
                if (k + 1 < k_count) next = fin_of(sid + A);
                const Shade1 s1 = at(cur);
                add(cur.st == kRay2 ? shade2_radiance(S, W, sid, s0) : hit1(cur) ? level1_radiance(s0, s1) : rad0);
            }
        }
        if constexpr (MOM2) {
            if (!last) { W.px_sum2[3 * a] = sum2.x; W.px_sum2[3 * a + 1] = sum2.y; W.px_sum2[3 * a + 2] = sum2.z; }
            else { float* o = F.sum2 + (long long)W.px_pixel[a] * 3; o[0] = sum2.x; o[1] = sum2.y; o[2] = sum2.z; }
        }
        if (!last) { W.px_sum[3 * a] = sum.x; W.px_sum[3 * a + 1] = sum.y; W.px_sum[3 * a + 2] = sum.z; continue; }
        const long long pix = W.px_pixel[a];
        if (F.sum) { float* o = F.sum + pix * 3; o[0] = sum.x; o[1] = sum.y; o[2] = sum.z; }
        const f3 avg = sq::scale(1 / (float)F.k_end, sum);
        if (F.out_avg) { float* o = F.out_avg + pix * 3; o[0] = avg.x; o[1] = avg.y; o[2] = avg.z; }
        if (F.out_rgb) tonemap(avg, F.out_rgb + pix * 3);
    }
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
// The end of a pixel's fold: the caller's sum, avg over the k_end samples folded so far (src/Lib.hs:88) and its tonemap.
__device__ __forceinline__ void store_fold(const Frame& F, long long pix, f3 sum) {
    if (F.sum) { float* o = F.sum + pix * 3; o[0] = sum.x; o[1] = sum.y; o[2] = sum.z; }
    const f3 avg = sq::scale(1 / (float)F.k_end, sum);
    if (F.out_avg) { float* o = F.out_avg + pix * 3; o[0] = avg.x; o[1] = avg.y; o[2] = avg.z; }
    if (F.out_rgb) tonemap(avg, F.out_rgb + pix * 3);
}
// T folded into a pixel's sums, once per sample of [k_begin, k_end); a raycast query (kSrcRays) stores T itself: no samples, no fold.
template <int SRC>
__device__ __forceinline__ void fold_cast_samples(const Frame& F, f3 T, f3& sum, f3& sum2, bool mom2) {
    if constexpr (SRC == kSrcRays) sum = T;
    else for (int k = F.k_begin; k < F.k_end; ++k) sum = sum + T;
    if (mom2) for (int k = F.k_begin; k < F.k_end; ++k) sum2 = sum2 + T * T;
}

// Per-lane form (option "cast_wavefront" = 0, or "variant" = 1): sq_render_pixels' cast branch with a loop over the light table.
template <typename StackT, int SRC, bool AD, typename FrameT>
__device__ __forceinline__ void cast_pixels_body(const SceneView& S, const FrameT& F, const Lights& L) {
    extern __shared__ float4 lds_raw[];
    SQ_LDS StackT* stk = to_lds<StackT>(lds_raw) + threadIdx.x;
    const long long pix = (long long)blockIdx.x * kBlock + threadIdx.x;
    int y, x; f3 o0, d0;
    if constexpr (SRC == kSrcRays) {
        if (pix >= (long long)F.h) return;
        o0 = load3(F.ray_org, pix); d0 = load3(F.ray_dir, pix);
    } else if constexpr (SRC == kSrcViews) {
        if (pix >= (long long)F.n_views * F.view_pixels) return;
        const ViewCam c = view_cam<false>(F, view_coords(F, (int)pix, y, x));
        o0 = c.pos; d0 = primary_dir(c.rot, F.w, F.h, y, x);
    } else {
        if (pix >= (long long)F.local_rows * F.h) return;
        if constexpr (AD) { if (!pixel_live(F, pix)) return; }
        pixel_coords(F, pix, y, x);
        o0 = sq::mk(F.cam_pos[0], F.cam_pos[1], F.cam_pos[2]);
        d0 = primary_dir(F.cam_rot, F.w, F.h, y, x);
    }
    const GlobalNodes N{ S.branches, S.cull_child, S.cull_child != nullptr };
    f3 sum = sq::mk(0, 0, 0), sum2 = sq::mk(0, 0, 0);
    const Hit h0 = trace_one(S, N, o0, d0, stk, kBlock);
    if (h0.tri >= 0) {
        sum = fold_start(F, pix);
        if constexpr (AD) { if (F.sum2) sum2 = fold_start2(F, pix); }
        const Surface s0 = surface_of(S, h0.tri);
        const f3 p0 = o0 + sq::scale(h0.t, d0);
        f3 T = sq::mk(0, 0, 0);
#pragma unroll 1
        for (int l = 0; l < L.n; ++l) {
            const Light Li = light_of(L, l);
            const f3 c = light_term(Li, p0, s0, trace_one(S, N, p0, Li.pos - p0, stk, kBlock));
            T = l == 0 ? c : T + c;                                     // the fold starts at c_0, not at +0
        }
        fold_cast_samples<SRC>(F, T, sum, sum2, AD && F.sum2 != nullptr);
    }
    if constexpr (AD) {
        if (F.sum2) { float* o = F.sum2 + pix * 3; o[0] = sum2.x; o[1] = sum2.y; o[2] = sum2.z; }
        store_count(F, pix);
    }
    store_fold(F, pix, sum);
}
template <typename StackT, int SRC, bool AD>
__global__ void __launch_bounds__(kBlock) sq_cast_pixels(const SceneView S, const FrameOf<SRC> F, const Lights L) { cast_pixels_body<StackT, SRC, AD>(S, F, L); }

// Wavefront form (option "cast_wavefront" = 1): the lights play the role of a frame's samples.  After the frame's own primary pass,
// per batch of lights [l_begin, l_end): sq_cast_gen writes the shadow ray of (active pixel a, light l) into slot (l - l_begin) * A + a,
// one level of the trace kernel traces them, and sq_cast_fold folds the batch's terms in order into T.
// One thread per active pixel; blockIdx.y splits the batch's lights when the frame has few pixels.
template <int SRC, typename FrameT>
__device__ __forceinline__ void cast_gen_body(const SceneView& S, const FrameT& F, const Work& W, const Lights& L) {
    const int A = *W.n_active;
    for (int a = blockIdx.x * kBlock + threadIdx.x; a < A; a += gridDim.x * kBlock) {
        const Pixel0 P = load_pixel0<SRC>(S, F, W, a);
        for (int l = L.l_begin + (int)blockIdx.y; l < L.l_end; l += (int)gridDim.y) {
            const long long sid = (long long)(l - L.l_begin) * A + a;
            const f3 d = light_of(L, l).pos - P.p0;                      // not normalised: the reference's is not
            W.state[sid] = kRay1;
            W.org[sid] = make_float4(P.p0.x, P.p0.y, P.p0.z, 0.0f);
            W.dir[sid] = make_float4(d.x, d.y, d.z, 0.0f);
        }
    }
}
template <int SRC>
__global__ void __launch_bounds__(kBlock) sq_cast_gen(const SceneView S, const FrameOf<SRC> F, const Work W, const Lights L) { cast_gen_body<SRC>(S, F, W, L); }
// ... and after the trace launch: T = c_0, T = T + c_l in the caller's order, carried from batch to batch in L.carry; on the last
// batch (`last`) the sample fold and the pixel's stores, as sq_accumulate does them (a masked call's count is set since the
// primary pass, store_active; the misses are black since then too).
template <int SRC, typename FrameT>
__device__ __forceinline__ void cast_fold_body(const SceneView& S, const FrameT& F, const Work& W, const Lights& L, int last) {
    const int A = *W.n_active;
    for (int a = blockIdx.x * kBlock + threadIdx.x; a < A; a += gridDim.x * kBlock) {
        const Pixel0 P = load_pixel0<SRC>(S, F, W, a);
        f3 T = sq::mk(0, 0, 0);
        if (L.l_begin > 0) T = sq::mk(L.carry[3 * a], L.carry[3 * a + 1], L.carry[3 * a + 2]);
        for (int l = L.l_begin; l < L.l_end; ++l) {
            const int2 hit = slot_hit(W.org[(long long)(l - L.l_begin) * A + a]);
            Hit sh; sh.t = __int_as_float(hit.x); sh.tri = hit.y;
            const f3 c = light_term(light_of(L, l), P.p0, P.s0, sh);
            T = l == 0 ? c : T + c;
        }
        if (!last) { L.carry[3 * a] = T.x; L.carry[3 * a + 1] = T.y; L.carry[3 * a + 2] = T.z; continue; }
        const long long pix = W.px_pixel[a];
        const bool mom2 = F.sum2 != nullptr;
        f3 sum = sq::mk(W.px_sum[3 * a], W.px_sum[3 * a + 1], W.px_sum[3 * a + 2]), sum2 = sq::mk(0, 0, 0);
        if (mom2) sum2 = sq::mk(W.px_sum2[3 * a], W.px_sum2[3 * a + 1], W.px_sum2[3 * a + 2]);
        fold_cast_samples<SRC>(F, T, sum, sum2, mom2);
        if (mom2) { float* o = F.sum2 + pix * 3; o[0] = sum2.x; o[1] = sum2.y; o[2] = sum2.z; }
        store_fold(F, pix, sum);
    }
}
template <int SRC>
__global__ void __launch_bounds__(kBlock) sq_cast_fold(const SceneView S, const FrameOf<SRC> F, const Work W, const Lights L, int last) { cast_fold_body<SRC>(S, F, W, L, last); }

// Copies a chunk of lights into the scene's light table: by value, as sq_stage_cams stages cameras.
constexpr int kLightChunk = 128;              // lights per staging launch: 128 x 24 B = 3 KB of arguments
struct LightChunk { float v[kLightWords * kLightChunk]; };
__global__ void __launch_bounds__(kBlock) sq_stage_lights(float* table, int n, const LightChunk C) {
    for (int i = threadIdx.x; i < kLightWords * n; i += kBlock) table[i] = C.v[i];
}

// The dominant kernel.  Persistent: each wave reserves a chunk of the (dense) ray queue with one
// atomic, compacts the chunk's live entries with ballots into a small LDS list, and each lane pulls
// its next ray from that list as soon as the previous one is finished, so a wave's lanes stay busy
// although ray lengths differ by 10x and although part of the queue is dead.  The first n_lds
// branches (breadth-first = the top of the tree) are staged in LDS once per workgroup; every lane
// keeps its frame stack in LDS (lane-minor layout, one word per frame, at most height-1 frames).
struct TraceArgs {
    float4* org; const float4* dir;          // a finished ray's hit (t bits, triangle) goes into org[slot].xy
    const uint8_t* state; int32_t want;      // a slot is in this launch's queue iff state[slot] == want (kRay1 / kRay2)
    long long front_base; int32_t front;     // front != 0: the queue starts with *n_active extra entries, the slots
                                             //   front_base + [0, *n_active) (the per-pixel mirror rays ride at the head of the
                                             //   first bounce launch instead of having a launch, and a ramp-down, of their own)
    const int32_t* n_active; int32_t k_count; int32_t* head;
    int32_t n_lds; int32_t stack_cap; int32_t straggler_lanes;
    int32_t chunk;               // slots per reservation: a multiple of 64, at most kChunkResident / kChunkStreaming
    int32_t guide_shift;         // towards the end of the queue a reservation shrinks to (slots left >> guide_shift), so that the
                                 //   launch does not end with a few waves still working through a full reservation (first bounce level
                                 //   only by default: on the sparse second-level queue it costs more round trips than it saves, option "guided")
    int32_t refill_min;          // pooled form: idle lanes a wave collects before it fetches new rays for them
    int32_t flush_min;           // pooled form: a trailing part-filled window of the pair pool is run at once from this many pairs on
    int32_t descend_extra, descend_lanes;   // pooled form: further branch steps per iteration for lanes that keep descending, and how many such lanes it takes
    int32_t diag;                // option "coresidency": keep the gauge of live workgroups in stats[24]
    int32_t prio;                // option "trace_prio": s_setprio level of the trace kernel's waves when they start (0 = leave it; the pooled
                                 //   kernel then sets its own levels per phase, kPrioSteps / kPrioWindows, so it only lasts in pool = 0 launches), for the overlapped
                                 //   schedules: per-sample kernels that share a SIMD with a trace workgroup then only get the issue
                                 //   slots the trace waves leave free
    int32_t pixel_major;         // queue ORDER: 0 = slot order (sample-major: neighbouring pixels, one sample each), 1 = all samples
                                 //   of a pixel in a row, so that a wave's rays start from one surface point (slots stay where they are)
    unsigned long long* stats;   // [0] rays traced; PROFILE builds: [1] advance iterations (waves), [2] lanes unwinding,
                                 // [3] lanes descending, [4] leaf iterations (waves), [5] lanes testing a triangle,
                                 // [6] outer iterations (waves), [7] refill executions (waves), [8] lanes refilled
                                 // pooled form: [1] iterations (waves), [2] lanes unwinding, [3] lanes descending,
                                 // [4] pair windows (waves), [5] pairs tested, [6] hits folded, [7] refill executions, [8] lanes refilled
};
// (the LDS carve-up of the trace kernel, TraceLds and trace_lds_layout: sq_plan.h)

__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}
// Copies the resident form of the scene (sq_scene.h) into the workgroup's LDS and points N / G at it.  The caller syncs.
template <int BLOCK>
__device__ __forceinline__ void stage_resident_scene(const SceneView& S, int n_branches, char* lds, const TraceLds& L, ResidentNodes& N, ResidentTris& G) {
    SQ_LDS v4f* lquads = to_lds<v4f>(lds + L.quads);
    SQ_LDS v2i* lrefs = to_lds<v2i>(lds + L.refs);
    SQ_LDS v4f* lv = to_lds<v4f>(lds + L.verts);
    SQ_LDS v4us* lt = to_lds<v4us>(lds + L.trix);
    for (int i = threadIdx.x; i < n_branches; i += BLOCK) {
        const uint32_t* r = S.rbranch + 10 * (size_t)i;
        lquads[i] = v4f{ __uint_as_float(r[0]), __uint_as_float(r[1]), __uint_as_float(r[2]), __uint_as_float(r[3]) };
        lquads[n_branches + i] = v4f{ __uint_as_float(r[4]), __uint_as_float(r[5]), __uint_as_float(r[6]), __uint_as_float(r[7]) };
        lrefs[i] = v2i{ (int)r[8], (int)r[9] };
    }
    // Several loads in flight per thread before the first LDS store (the plain loops wait for every load before the next is issued):
    // a trace launch's staging is on the path of every launch, and a rank's share of a frame at 8 ranks has three launches in 8.5 ms.
    for (int base = threadIdx.x; base < S.n_verts; base += BLOCK * 4) {
        float4 v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) { const int i = base + k * BLOCK; if (i < S.n_verts) v[k] = S.verts4[i]; }
#pragma unroll
        for (int k = 0; k < 4; ++k) { const int i = base + k * BLOCK; if (i < S.n_verts) lv[i] = v4f{ v[k].x, v[k].y, v[k].z, v[k].w }; }
    }
    for (int base = threadIdx.x; base < S.n_tris; base += BLOCK * 8) {     // vertex indices become byte offsets into the vertex table
        ushort4 t[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) { const int i = base + k * BLOCK; if (i < S.n_tris) t[k] = S.trix[i]; }
#pragma unroll
        for (int k = 0; k < 8; ++k) { const int i = base + k * BLOCK; if (i < S.n_tris) lt[i] = v4us{ (unsigned short)(t[k].x * 16u), (unsigned short)(t[k].y * 16u), (unsigned short)(t[k].z * 16u), t[k].w }; }
    }
    if (threadIdx.x < ResidentTris::kRunPad) lt[S.n_tris + threadIdx.x] = v4us{ 0, 0, 0, 0 };
    N = ResidentNodes{ lquads, lquads + n_branches, lrefs, S.cull_child16 != nullptr, S.cull_child16 };
    G = ResidentTris{ lt };
    if ((uintptr_t)lv != 0) __builtin_trap();                              // the kernels that use this have no static LDS: dynamic LDS starts at address 0
}

// Primary rays with the scene in LDS (the resident form): same per-ray code as sq_primary, but a branch or triangle costs an
// LDS read instead of an L2 round trip.  A primary ray is a chain of ~200 dependent reads, so on small frames -- one rank's
// share of a frame at 8 ranks -- the launch is as long as that chain: 0.58 ms from L2, 0.1-0.2 ms from LDS.
template <typename StackT, int SRC, bool AD, bool SKY, typename FrameT>
__device__ __forceinline__ void primary_resident_body(const SceneView& S, const FrameT& F, const Work& W, int stack_cap, const Sky& K) {
    constexpr bool MV = SRC == kSrcViews;
    extern __shared__ float4 lds_raw[];
    char* lds = reinterpret_cast<char*>(lds_raw);
    const TraceLds L = trace_lds_layout(S.n_branches, true, S.n_verts, S.n_tris, kResidentBlock, stack_cap, (int)sizeof(StackT), false);
    SQ_LDS StackT* stk = to_lds<StackT>(lds + L.stack) + threadIdx.x;
    ResidentNodes N; ResidentTris G;
    stage_resident_scene<kResidentBlock>(S, S.n_branches, lds, L, N, G);
    __syncthreads();
    const long long total = MV ? primary_padded(F) * F.n_views : primary_padded(F);
    for (long long base = (long long)blockIdx.x * kResidentBlock; base < total; base += (long long)gridDim.x * kResidentBlock) {
        int view = 0;
        long long pix;                                                      // (total is a multiple of 64: whole waves)
        if constexpr (SRC == kSrcRays) pix = base + threadIdx.x < (long long)F.h ? base + threadIdx.x : -1;   // index order, as in sq_primary
        else if constexpr (MV) pix = primary_tile_views(F, base + threadIdx.x, view);
        else pix = primary_tile(F, base + threadIdx.x);
        bool in = pix >= 0;
        if constexpr (AD) in = in && pixel_live(F, pix);
        Hit h0; h0.tri = -1; h0.t = 0;
        f3 d0 = sq::mk(0, 0, 0);
        if (in) {
            int y, x;
            if constexpr (SRC == kSrcRays) {
                const f3 o0 = load3(F.ray_org, pix);
                d0 = load3(F.ray_dir, pix);
                h0 = trace_one(S, N, G, S.rroot, o0, d0, stk, kResidentBlock);
            } else if constexpr (MV) {
                pixel_coords(F, pix - (long long)view * F.view_pixels, y, x);
                const ViewCam c = view_cam<true>(F, view);
                d0 = primary_dir(c.rot, F.w, F.h, y, x);
                h0 = trace_one(S, N, G, S.rroot, c.pos, d0, stk, kResidentBlock);
            } else {
                pixel_coords(F, pix, y, x);
                d0 = primary_dir(F.cam_rot, F.w, F.h, y, x);
                h0 = trace_one(S, N, G, S.rroot, sq::mk(F.cam_pos[0], F.cam_pos[1], F.cam_pos[2]), d0, stk, kResidentBlock);
            }
        }
        const int a = wave_append(W.n_active, in && h0.tri >= 0);
        if (a >= 0) store_active<AD>(F, W, a, pix, h0.t, h0.tri);
        else if (in) { if constexpr (SKY) store_miss_sky<AD>(F, pix, K, d0); else store_miss<AD>(F, pix); }
    }
}
template <typename StackT, int SRC, bool AD, typename... SkyT>
__global__ void __launch_bounds__(kResidentBlock) sq_primary_resident(const SceneView S, const FrameOf<SRC> F, const Work W, int stack_cap, const SkyT... K) {
    primary_resident_body<StackT, SRC, AD, sizeof...(SkyT) != 0>(S, F, W, stack_cap, sky_arg<Sky>(K...));
}

template <typename StackT, bool RESIDENT, int BLOCK, bool PROFILE, bool POOL>
__device__ __forceinline__ void trace_rays_body(const SceneView& S, const TraceArgs& A) {
    extern __shared__ float4 lds_raw[];
    char* lds = reinterpret_cast<char*>(lds_raw);
    const TraceLds L = trace_lds_layout(A.n_lds, RESIDENT, S.n_verts, S.n_tris, BLOCK, A.stack_cap, (int)sizeof(StackT), POOL);
    constexpr int kChunk = RESIDENT ? kChunkResident : kChunkStreaming;
    SQ_LDS LiveT* live = to_lds<LiveT>(lds + L.live) + (threadIdx.x >> 6) * kChunk;   // this wave's list
    SQ_LDS StackT* stk = to_lds<StackT>(lds + L.stack) + threadIdx.x;
    SQ_LDS v4f* lquads = to_lds<v4f>(lds + L.quads);
    using NodeSrc = typename std::conditional<RESIDENT, ResidentNodes, HybridNodes>::type;
    using TriSrc = typename std::conditional<RESIDENT, ResidentTris, GlobalTris>::type;
    NodeSrc N; TriSrc G;
    uint32_t root_ref;
    if constexpr (RESIDENT) {                                         // stage the whole scene (coalesced loads)
        stage_resident_scene<BLOCK>(S, A.n_lds, lds, L, N, G);
        root_ref = S.rroot;
    } else {
        for (int i = threadIdx.x; i < 3 * A.n_lds; i += BLOCK) { const float4 q = S.branches[i]; lquads[i] = v4f{ q.x, q.y, q.z, q.w }; }
        N = HybridNodes{ lquads, S.branches_m, (uint32_t)A.n_lds, S.cull_child != nullptr };
        G = GlobalTris{ S.tris, S.leaves, S.packed_leaves != 0, (size_t)S.n_tris * sizeof(DevTri) > ((size_t)4 << 20) };
        root_ref = S.root_ref;
    }
    __syncthreads();
    if (A.diag && threadIdx.x == 0) atomicAdd(&A.stats[kDiagGauge], 1ull);
    if (A.prio == 1) __builtin_amdgcn_s_setprio(1); else if (A.prio == 2) __builtin_amdgcn_s_setprio(2); else if (A.prio == 3) __builtin_amdgcn_s_setprio(3);
    const long long n_front = A.front ? (long long)(*A.n_active) : 0;
    const long long n = (long long)(*A.n_active) * A.k_count + n_front;          // queue positions; slot_of() maps them to slots
    const unsigned n_pix = (unsigned)(*A.n_active), kq = (unsigned)A.k_count;
    auto slot_of = [&](long long q) -> long long {
        if (q < n_front) return A.front_base + q;
        if (!A.pixel_major) return q - n_front;
        const unsigned r = (unsigned)(q - n_front), a = r / kq, k = r - a * kq;   // slot = sample * pixels + pixel (Work)
        return (long long)k * n_pix + a;
    };
    const int lane = threadIdx.x & 63;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    long long chunk_base = 0;               // wave-uniform
    int my_chunk = A.chunk;                 // wave-uniform: size of this wave's next reservation
    int list_pos = 0, list_len = 0;         // wave-uniform
    bool exhausted = false;                 // wave-uniform
    long long my_ray = -1;
    unsigned long long n_traced = 0;        // wave-uniform
    unsigned long long pf_adv = 0, pf_leaf = 0, pf_outer = 0, pf_refill = 0;   // wave-uniform (PROFILE)
    unsigned int pl_unw = 0, pl_desc = 0, pl_tri = 0, pl_ref = 0;               // per lane (PROFILE)
    Trav T; T.mode = M_DONE; T.sp = 0; T.cur = 0; T.R.tri = -1; T.R.t = 0;
    T.o = T.d = T.df = sq::mk(0, 0, 0);
    int sub_end[3] = { 0, 0, 0 };           // wave-uniform: list positions where the chunk's 2nd, 3rd, 4th 256-slot block start
    auto refill = [&](unsigned long long m, bool idle) {             // m = ballot(idle), wave-uniform
        while (!exhausted && list_pos == list_len) {                    // reserve and compact the next chunk
            int base = 0;
            if (lane == 0) base = atomicAdd(A.head, my_chunk);
            base = __builtin_amdgcn_readfirstlane(base);
            if (base >= n) { exhausted = true; break; }
            const int this_chunk = my_chunk;
            {   // guided self-scheduling: the next reservation is 1/(4 x waves) of what is left, between 64 and A.chunk slots
                const long long left = n - ((long long)base + this_chunk);
                const long long want = A.guide_shift >= 62 ? (long long)A.chunk : ((left >> A.guide_shift) & ~63ll);
                my_chunk = (int)(want < 64 ? 64 : (want > A.chunk ? A.chunk : want));
            }
            chunk_base = base; list_pos = 0; list_len = 0;
            sub_end[0] = sub_end[1] = sub_end[2] = 0x7fffffff;          // blocks a short reservation does not reach
#pragma unroll
            for (int j = 0; j < kChunk / 64; ++j) {
                if (j * 64 >= this_chunk) break;
                const long long idx = chunk_base + j * 64 + lane;
                const bool alive = idx < n && A.state[slot_of(idx)] == (uint8_t)A.want;
                const unsigned long long am = sq_ballot(alive);
                if (alive) live[list_len + __popcll(am & lt_mask)] = (LiveT)((j & 3) * 64 + lane);   // index within its 256-slot block
                list_len += __popcll(am);
                if ((j & 3) == 3 && j / 4 < 3) sub_end[j / 4] = list_len;
            }
            n_traced += (unsigned long long)list_len;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
        if (exhausted) return;
        const int rank = __popcll(m & lt_mask);
        const int avail = list_len - list_pos;
        if (PROFILE) ++pf_refill;
        if (idle && rank < avail) {
            if (PROFILE) ++pl_ref;
            const int p = list_pos + rank;
            int block = 0;
            if (kChunk > 256) block += p >= sub_end[0];
            if (kChunk > 512) block += p >= sub_end[1];
            if (kChunk > 768) block += p >= sub_end[2];
            my_ray = slot_of(chunk_base + block * 256 + live[p]);
            const float4 o = A.org[my_ray], d = A.dir[my_ray];
            trav_begin(T, S, root_ref, sq::mk(o.x, o.y, o.z), sq::mk(d.x, d.y, d.z));
        }
        list_pos += min(__popcll(m), avail);
    };
    if constexpr (POOL) {
        // Pooled form.  One iteration offers every lane one return (pop a frame), one branch step, and then tests the
        // triangles of ALL leaves the wave's rays have open as a pool of (ray, triangle) pairs: the pairs are numbered
        // by a prefix sum over the lanes' leaf sizes and pair p = 64*window + lane is tested by lane `lane`, whatever
        // ray owns it (the owner's origin, direction and triangle offset come over the DPP/bpermute network).  So a
        // leaf of 14 triangles beside leaves of 3 no longer holds 64 lanes for 14 rounds: the wave runs
        // ceil(sum / 64) full-width rounds.  Accepted hits are folded into the owning lane's R in pair order, which is
        // leaf order, with the very comparison of the one-lane leaf loop (minimumBy's rule, src/BIH.hs:105-109) --
        // the arithmetic of mollerTrumbore does not depend on the lane that runs it.
        constexpr int KW = kPoolWindows;
        constexpr bool kFlat = RESIDENT && !PROFILE;   // the flat steps (sq_scene.h): the resident form only, DESIGN.md 4.8
        bool flat_ok = false;               // wave-uniform (kFlat): every ray of the wave is safe and the scene has culling boxes
        SQ_LDS uint8_t* tab = to_lds<uint8_t>(lds + L.tab) + (threadIdx.x >> 6) * (64 * KW);   // this wave's window-head tables
        for (int k = 0; k < KW; ++k) tab[k * 64 + lane] = 0;
        const int lane_tag = lane * 4 + 1;  // a lane's mark in the head table: non-zero, grows with the lane, and is its ds_bpermute address
        int lf_first = 0, lf_cnt = 0;       // M_LEAFQ: the untested rest of this lane's open leaf
        bool carry = false;                 // wave-uniform: the previous iteration left queued pairs untested
        unsigned int pl_hit = 0, pl_hslow = 0;
        TravProf prof{};
        // PROFILE: wave time per section of the loop (s_memtime ticks = shader cycles; the stamps themselves cost ~10 %)
        unsigned long long tsec[8] = { 0, 0, 0, 0, 0, 0, 0, 0 }, tlast = PROFILE ? __builtin_amdgcn_s_memtime() : 0;
        auto stamp = [&](int sec) { if (PROFILE) { const unsigned long long now = __builtin_amdgcn_s_memtime(); tsec[sec] += now - tlast; tlast = now; } };
        for (;;) {
            if (PROFILE) ++pf_adv;
            const bool idle = (T.mode == M_DONE);
            const unsigned long long m = sq_ballot(idle);       // before the store's exec region: the compare's mask IS the ballot
            if (idle && my_ray >= 0) { *reinterpret_cast<int2*>(A.org + my_ray) = make_int2(__float_as_int(T.R.t), T.R.tri); my_ray = -1; }
            if (m) {
                if (__popcll(m) >= A.refill_min || m == ~0ull) {
                    refill(m, idle);
                    // the flat steps are for waves whose rays are all safe (a ray's flag only changes here) in scenes with culling boxes
                    if constexpr (kFlat) flat_ok = N.cull_on && sq_ballot(T.mode != M_DONE && !T.safe) == 0;
                }
                if (exhausted && m == ~0ull) break;
            }
            stamp(0);
            __builtin_amdgcn_s_setprio(kPrioSteps);                         // return / branch steps (results unchanged)
            if (PROFILE) pl_unw += (T.mode == M_UNWIND);
            if constexpr (kFlat) {
                // the return step with three exec regions (the step, COMBINE, FAR) instead of six nested ones: DONE, the pop and the
                // kind of the popped frame are decided by selects, the FAR half is trav_unwind_far_flat
                if (T.mode == M_UNWIND) {
                    constexpr uint32_t flag = StackTraits<StackT>::flag;
                    const bool done = T.sp == 0;
                    T.sp -= done ? 0 : 1;
                    const uint32_t e = stk[T.sp * BLOCK];                       // (slot 0, unused, for a ray that is done)
                    const bool is_combine = !done && (e & flag) != 0, is_far = !done && (e & flag) == 0;
                    if (is_combine) trav_unwind_combine<TriSrc, StackT>(T, G, e);
                    if (is_far) trav_unwind_far_flat<NodeSrc, StackT>(T, N, stk, BLOCK, e);
                    T.mode = done ? M_DONE : T.mode;
                }
            } else
            if (T.mode == M_UNWIND) trav_unwind(T, N, G, stk, BLOCK, PROFILE ? &prof : nullptr);
            stamp(1);
            if (PROFILE) pl_desc += (T.mode == M_DESCEND);
            if constexpr (kFlat) {
                if (T.mode == M_DESCEND) { if (flat_ok) trav_descend_flat<NodeSrc, StackT>(T, N, stk, BLOCK); else trav_descend(T, N, stk, BLOCK); }
            } else
            if (T.mode == M_DESCEND) trav_descend(T, N, stk, BLOCK);
            // With the culling boxes a ray takes four branch steps per leaf it opens: lanes that are still descending take up
            // to `descend_extra` more steps in this iteration (while at least `descend_lanes` of them are), instead of paying a
            // whole iteration -- return step, leaf scan, windows -- per branch step.
            for (int x = 0; x < A.descend_extra; ++x) {
                if (__popcll(sq_ballot(T.mode == M_DESCEND)) < A.descend_lanes) break;
                if (PROFILE) pl_desc += (T.mode == M_DESCEND);
                if constexpr (kFlat) {
                    if (T.mode == M_DESCEND) { if (flat_ok) trav_descend_flat<NodeSrc, StackT>(T, N, stk, BLOCK); else trav_descend(T, N, stk, BLOCK); }
                } else
                if (T.mode == M_DESCEND) trav_descend(T, N, stk, BLOCK);
            }
            stamp(2);
            __builtin_amdgcn_s_setprio(kPrioWindows);                       // ... leaf scan and pair windows
            if constexpr (kFlat) {                                         // open the leaf (src/BIH.hs:105): Nothing so far -- as selects
                const bool open = T.mode == M_LEAF;                         // (a resident leaf reference decodes without a load)
                const int2 lf = G.leaf(T.cur);
                lf_first = open ? lf.x : lf_first; lf_cnt = open ? lf.y : lf_cnt; T.R.tri = open ? -1 : T.R.tri;
                T.mode = open ? (lf.y > 0 ? M_LEAFQ : M_UNWIND) : T.mode;
            } else
            if (T.mode == M_LEAF) {                                         // open the leaf (src/BIH.hs:105): Nothing so far
                const int2 lf = G.leaf(T.cur);
                lf_first = lf.x; lf_cnt = lf.y; T.R.tri = -1;
                T.mode = lf.y > 0 ? M_LEAFQ : M_UNWIND;
            }
            if constexpr ((RESIDENT ? kPoolTrisResident : kPoolTrisStreaming) >= 2) {
                // NT triangles per lane and window.  The pool is counted in UNITS of NT consecutive triangles of one leaf (the
                // last unit of a leaf may be part-filled), so that one owner lookup and one set of pulls serve NT triangle
                // tests: the pulls are the most expensive part of a window (ds_bpermute, 6 cycles per CU each), and the
                // lookup's integer VALU work comes next.
                constexpr int NT = RESIDENT ? kPoolTrisResident : kPoolTrisStreaming;
                const int c2 = (T.mode == M_LEAFQ) ? lf_cnt : 0;                // triangles left in this lane's open leaf
                if (sq_ballot(c2 > 0) == 0) continue;
                const int u = (c2 + NT - 1) / NT;                               // units
                const int incl = wave_scan_add(u);
                const int U = __builtin_amdgcn_readlane(incl, 63);
                const int start = incl - u;
                const int tb2 = lf_first - NT * start;                          // first triangle of unit q = NT q + tb2
                const int tri_end = lf_first + c2;                              // one past the leaf's last triangle
                int nwin = U >> 6;
                const int rem = U & 63;
                const bool others = sq_ballot(T.mode == M_UNWIND || T.mode == M_DESCEND) != 0;
                if (rem && (!others || carry || rem >= A.flush_min)) ++nwin;
                stamp(3);
                for (int w = 0; w < nwin; ++w) {
                    const int base = w << 6;
                    const int h = start - base;
                    if (u > 0 && h < 64 && incl > base) tab[h > 0 ? h : 0] = (uint8_t)lane_tag;
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                    int own = tab[lane];
                    tab[lane] = 0;
                    own = wave_scan_max(own);
                    const int q = base + lane;
                    const bool act = q < U;
                    int tri0 = NT * q + lane_pull(tb2, own);
                    const int end_o = lane_pull(tri_end, own);
                    const f3 po = sq::mk(lane_pull(T.o.x, own), lane_pull(T.o.y, own), lane_pull(T.o.z, own));
                    const f3 pd = sq::mk(lane_pull(T.d.x, own), lane_pull(T.d.y, own), lane_pull(T.d.z, own));
                    if (!act) tri0 = 0;                                         // lanes past the last unit test triangle 0 and drop the answer
                    stamp(4);
                    f3 v0[NT], e1[NT], e2[NT];
                    G.template get_run<NT>(tri0, v0, e1, e2);                   // a part-filled unit tests the records after it and drops the answers
                    float tt[NT]; bool hit[NT]; unsigned long long hmk[NT], hm = 0;
#pragma unroll
                    for (int k = 0; k < NT; ++k) {
                        const bool valid = act && (k == 0 || tri0 + k < end_o);
                        hit[k] = moller_trumbore_flat(po, pd, v0[k], e1[k], e2[k], tt[k]) & valid;
                    }
                    stamp(5);
#pragma unroll
                    for (int k = 0; k < NT; ++k) { hmk[k] = sq_ballot(hit[k]); hm |= hmk[k]; if (PROFILE) pl_hit += (int)hit[k]; }
                    while (hm) {                                                // accepted hits in leaf order: lane by lane, a lane's triangles in turn
                        const int l = __ffsll((long long)hm) - 1;
                        hm &= hm - 1;
                        const int so = __builtin_amdgcn_readlane(own, l);
                        const int stri = __builtin_amdgcn_readlane(tri0, l);
#pragma unroll
                        for (int k = 0; k < NT; ++k) if ((hmk[k] >> l) & 1ull) {
                            const float st = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(tt[k]), l));
                            if (lane_tag == so && (T.R.tri < 0 || dist_gt(T.o, T.d, T.R.t, st, T.safe))) { T.R.t = st; T.R.tri = stri + k; }
                        }
                    }
                    stamp(6);
                }
                const int done = min(U, nwin << 6);                             // units tested
                if (PROFILE) { pf_leaf += nwin; pf_outer += NT * done; }
                if constexpr (kFlat) {
                    const bool fin = u > 0 && incl <= done;                     // the Leaf equation is finished: R is its value
                    const int adv = (u > 0 && incl > done && start < done) ? NT * (done - start) : 0;   // whole units come first
                    T.mode = fin ? M_UNWIND : T.mode; lf_first += adv; lf_cnt -= adv;
                } else
                if (u > 0) {
                    if (incl <= done) T.mode = M_UNWIND;                        // the Leaf equation is finished: R is its value
                    else if (start < done) { lf_first += NT * (done - start); lf_cnt -= NT * (done - start); }   // whole units come first
                }
                carry = done < U;
                stamp(7);
                continue;
            }
            const int c = (T.mode == M_LEAFQ) ? lf_cnt : 0;
            if (sq_ballot(c > 0) == 0) continue;
            const int incl = wave_scan_add(c);                              // pairs of lanes 0..lane
            const int P = __builtin_amdgcn_readlane(incl, 63);              // pairs queued in the wave
            const int start = incl - c;                                     // this lane's first pair
            const int tb = lf_first - start;                                // triangle of pair p = p + tb
            int nwin = P >> 6;
            const int rem = P & 63;
            const bool others = sq_ballot(T.mode == M_UNWIND || T.mode == M_DESCEND) != 0;
            if (rem && (!others || carry || rem >= A.flush_min)) ++nwin;
            stamp(3);
            // KW windows per step: their LDS round trips (head table, owner pulls, index record, vertices) are issued
            // together and waited for once, and the independent arithmetic of KW triangle tests interleaves.
            for (int w0 = 0; w0 < nwin; w0 += KW) {
                int own[KW], tri[KW]; f3 po[KW], pd[KW]; float t[KW]; bool hit[KW];
                // who owns pair base + lane?  Every owner whose pairs reach into a window writes its lane number at the
                // window position of its first pair there; a max-scan spreads it over the owner's run.
#pragma unroll
                for (int k = 0; k < KW; ++k) {
                    const int base = (w0 + k) << 6;
                    const int h = start - base;
                    if (c > 0 && h < 64 && incl > base) tab[k * 64 + (h > 0 ? h : 0)] = (uint8_t)lane_tag;
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
                for (int k = 0; k < KW; ++k) { own[k] = tab[k * 64 + lane]; tab[k * 64 + lane] = 0; }
#pragma unroll
                for (int k = 0; k < KW; ++k) own[k] = wave_scan_max(own[k]);
#pragma unroll
                for (int k = 0; k < KW; ++k) {
                    const int src = own[k];                                 // ds_bpermute takes lane * 4 and ignores the two low bits
                    const int p = ((w0 + k) << 6) + lane;
                    tri[k] = p + lane_pull(tb, src);
                    po[k] = sq::mk(lane_pull(T.o.x, src), lane_pull(T.o.y, src), lane_pull(T.o.z, src));
                    pd[k] = sq::mk(lane_pull(T.d.x, src), lane_pull(T.d.y, src), lane_pull(T.d.z, src));
                    hit[k] = p < P;                                         // so far: the pair exists
                    if (!hit[k]) tri[k] = 0;                                // lanes past the last pair test triangle 0 and drop the answer
                }
                if (PROFILE) { t[0] = po[0].x + pd[0].x + __int_as_float(tri[0]); asm volatile("" :: "v"(t[0])); }   // the pulls have arrived
                stamp(4);
                f3 v0[KW], e1[KW], e2[KW];
#pragma unroll
                for (int k = 0; k < KW; ++k) if (k == 0 || w0 + k < nwin) G.get1(tri[k], v0[k], e1[k], e2[k]);
#pragma unroll
                for (int k = 0; k < KW; ++k) {
                    if (k == 0 || w0 + k < nwin) { float tk; const bool ok = moller_trumbore_flat(po[k], pd[k], v0[k], e1[k], e2[k], tk); t[k] = tk; hit[k] = hit[k] & ok; }
                    else { t[k] = 0.0f; hit[k] = false; }
                }
                stamp(5);
#pragma unroll
                for (int k = 0; k < KW; ++k) {
                    unsigned long long hm = sq_ballot(hit[k]);
                    if (PROFILE) pl_hit += hit[k];
                    while (hm) {                                            // accepted hits in pair order
                        const int l = __ffsll((long long)hm) - 1;
                        hm &= hm - 1;
                        const int so = __builtin_amdgcn_readlane(own[k], l);
                        const float st = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(t[k]), l));
                        const int stri = __builtin_amdgcn_readlane(tri[k], l);
                        if (PROFILE && lane_tag == so && T.R.tri >= 0 && !(!(T.R.t > st) && st < __builtin_inff() && T.safe)) ++pl_hslow;
                        if (lane_tag == so && (T.R.tri < 0 || dist_gt(T.o, T.d, T.R.t, st, T.safe))) { T.R.t = st; T.R.tri = stri; }
                    }
                }
                stamp(6);
            }
            const int done = min(P, nwin << 6);
            if (PROFILE) { pf_leaf += nwin; pf_outer += done; }
            if (c > 0) {
                if (incl <= done) T.mode = M_UNWIND;                        // the Leaf equation is finished: R is its value
                else if (start < done) { lf_first += done - start; lf_cnt = incl - done; }
            }
            carry = done < P;
            stamp(7);
        }
        if (lane == 0) atomicAdd(&A.stats[0], n_traced);
        if (A.diag && threadIdx.x == 0) atomicAdd(&A.stats[kDiagGauge], ~0ull);   // -1: the workgroup's first wave is leaving (the others follow within a ray's length)
        if (PROFILE) {
            if (lane == 0) { atomicAdd(&A.stats[1], pf_adv); atomicAdd(&A.stats[4], pf_leaf); atomicAdd(&A.stats[5], pf_outer); atomicAdd(&A.stats[7], pf_refill); }
            atomicAdd(&A.stats[2], (unsigned long long)pl_unw); atomicAdd(&A.stats[3], (unsigned long long)pl_desc);
            atomicAdd(&A.stats[6], (unsigned long long)pl_hit); atomicAdd(&A.stats[8], (unsigned long long)pl_ref);
            atomicAdd(&A.stats[9], (unsigned long long)prof.combine); atomicAdd(&A.stats[10], (unsigned long long)prof.recompute_lanes);
            atomicAdd(&A.stats[11], (unsigned long long)prof.recompute_waves); atomicAdd(&A.stats[12], (unsigned long long)prof.slowcmp_lanes);
            atomicAdd(&A.stats[13], (unsigned long long)prof.slowcmp_waves); atomicAdd(&A.stats[14], (unsigned long long)pl_hslow);
            if (lane == 0) for (int i = 0; i < 8; ++i) atomicAdd(&A.stats[16 + i], tsec[i]);
        }
        return;
    }
    for (;;) {
        if (PROFILE) ++pf_outer;
        const bool idle = (T.mode == M_DONE);
        if (idle && my_ray >= 0) { *reinterpret_cast<int2*>(A.org + my_ray) = make_int2(__float_as_int(T.R.t), T.R.tri); my_ray = -1; }
        const unsigned long long m = sq_ballot(idle);
        if (m) {
            refill(m, idle);
            if (exhausted && m == ~0ull) break;
        }
        // advance until (almost) every lane has a leaf to test or is finished
        for (;;) {
            const bool adv = (T.mode == M_DESCEND) || (T.mode == M_UNWIND);
            const unsigned long long am = sq_ballot(adv);
            if (am == 0) break;
            if (__popcll(am) <= A.straggler_lanes && sq_ballot(T.mode == M_LEAF) != 0) break;
            if (PROFILE) { ++pf_adv; pl_unw += (T.mode == M_UNWIND); }
            if (T.mode == M_UNWIND) trav_unwind(T, N, G, stk, BLOCK);
            if (PROFILE) pl_desc += (T.mode == M_DESCEND);
            if (T.mode == M_DESCEND) trav_descend(T, N, stk, BLOCK);
        }
        if (PROFILE) {
            const int cnt = (T.mode == M_LEAF) ? G.leaf(T.cur).y : 0;
            pl_tri += cnt; pf_leaf += wave_max(cnt);
        }
        if (T.mode == M_LEAF) trav_leaf(T, G);
    }
    if (lane == 0) atomicAdd(&A.stats[0], n_traced);
    if (A.diag && threadIdx.x == 0) atomicAdd(&A.stats[kDiagGauge], ~0ull);
    if (PROFILE) {
        if (lane == 0) { atomicAdd(&A.stats[1], pf_adv); atomicAdd(&A.stats[4], pf_leaf); atomicAdd(&A.stats[6], pf_outer); atomicAdd(&A.stats[7], pf_refill); }
        atomicAdd(&A.stats[2], (unsigned long long)pl_unw); atomicAdd(&A.stats[3], (unsigned long long)pl_desc);
        atomicAdd(&A.stats[5], (unsigned long long)pl_tri); atomicAdd(&A.stats[8], (unsigned long long)pl_ref);
    }
}

template <typename StackT, bool RESIDENT, int BLOCK, bool PROFILE, bool POOL>
__global__ void __launch_bounds__(BLOCK) sq_trace_rays(const SceneView S, const TraceArgs A) {
    trace_rays_body<StackT, RESIDENT, BLOCK, PROFILE, POOL>(S, A);
}
// The streaming pooled kernel once more, compiled for SIX waves per SIMD (at most 80 VGPRs; the plain build takes 86, i.e. four):
// three 512-thread workgroups per CU instead of two when their stacks and a share of the tree's top fit in a third of the LDS.
// The streaming form waits on memory two thirds of its time, and the extra waves are worth more than the handful of spilled
// registers and the smaller LDS node prefix: 25.9 -> 24.5 ms (82k triangles), 30.7 -> 29.4 ms (1M triangles) at 64 spp, same
// call (profiles/r03c_stream_incremental.txt, rows libc16 / libw6c16 with incremental = 0).
template <typename StackT>
__global__ void __launch_bounds__(kTraceBlock, 6) sq_trace_rays_dense(const SceneView S, const TraceArgs A) {
    trace_rays_body<StackT, false, kTraceBlock, false, true>(S, A);
}

// ---- diagnostics: primitives of the numeric spec evaluated on the device ----
__global__ void sq_debug_kernel(int op, const void* a, const void* b, long long n, void* out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* fa = (const float*)a; const float* fb = (const float*)b; float* fo = (float*)out;
    switch (op) {
        case SQ_OP_SQRT: fo[i] = sq::fsqrt(fa[i]); break;
        case SQ_OP_DIV: fo[i] = fa[i] / fb[i]; break;
        case SQ_OP_SIN: fo[i] = sq::fsin(fa[i]); break;
        case SQ_OP_COS: fo[i] = sq::fcos(fa[i]); break;
        case SQ_OP_ACOS: fo[i] = sq::facos(fa[i]); break;
        case SQ_OP_ATAN: fo[i] = sq::fatan(fa[i]); break;
        case SQ_OP_UNIT_FLOAT: fo[i] = sq::unit_float(((const uint32_t*)a)[i]); break;
        case SQ_OP_TFGEN3: {
            uint32_t n0, n1, n2; sq::tfgen3(((const long long*)a)[i], n0, n1, n2);
            uint32_t* o = (uint32_t*)out + 3 * i; o[0] = n0; o[1] = n1; o[2] = n2; break;
        }
        case SQ_OP_TONEMAP: tonemap(sq::mk(fa[3 * i], fa[3 * i + 1], fa[3 * i + 2]), (uint8_t*)out + 3 * i); break;
        case SQ_OP_RCP_SWEEP: {                                            // all 65536 floats whose upper 16 bits are a[i]
            const uint32_t hi = ((const uint32_t*)a)[i] << 16; uint32_t bad = 0;
            for (uint32_t lo = 0; lo < 65536u; ++lo) {
                const float x = __uint_as_float(hi | lo);
                bad += __float_as_uint(rcp_midrange(x)) != __float_as_uint(1.0f / x);
            }
            ((uint32_t*)out)[i] = bad; break;
        }
        case SQ_OP_CULL_SLAB: {                                            // the culling slab test as the trace kernels run it
            const uint32_t* w = (const uint32_t*)a + 9 * i; const float* r = fa + 9 * i + 3;
            const f3 o = sq::mk(r[0], r[1], r[2]), d = sq::mk(r[3], r[4], r[5]);
            const f3 df = sq::mk(1.0f / d.x, 1.0f / d.y, 1.0f / d.z), nodf = sq::mk(-o.x * df.x, -o.y * df.y, -o.z * df.z);
            ((uint32_t*)out)[i] = cull_slab_half(w[0], w[1], w[2], df, nodf) ? 1u : 0u; break;
        }
        default: break;
    }
}

// ----------------------------------------------------------------------------------------------
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

// Per-lane form (option "variant" = 1): sq_render_pixels' raytrace branch with a loop over the levels.  A lane keeps the triangles
// of its path (registers: the level is matched by selects, not by an index) and folds L from the innermost level outwards.
// SKY: a ray that misses ends its path on sky(d) of that ray; a pixel whose ray 0 misses folds sky(d_0) once per sample.
template <typename StackT, int SRC, bool AD, bool SKY, typename FrameT>
__device__ __forceinline__ void render_pixels_deep_body(const SceneView& S, const FrameT& F, const int depth, const Sky& K) {
    extern __shared__ float4 lds_raw[];
    SQ_LDS StackT* stk = to_lds<StackT>(lds_raw) + threadIdx.x;
    const long long pix = (long long)blockIdx.x * kBlock + threadIdx.x;
    int y = 0, x = 0; f3 o0, d0;
    if constexpr (SRC == kSrcRays) {
        if (pix >= (long long)F.h) return;
        o0 = load3(F.ray_org, pix); d0 = load3(F.ray_dir, pix);
    } else if constexpr (SRC == kSrcViews) {
        if (pix >= (long long)F.n_views * F.view_pixels) return;
        const ViewCam c = view_cam<false>(F, view_coords(F, (int)pix, y, x));
        o0 = c.pos; d0 = primary_dir(c.rot, F.w, F.h, y, x);
    } else {
        if (pix >= (long long)F.local_rows * F.h) return;
        if constexpr (AD) { if (!pixel_live(F, pix)) return; }
        pixel_coords(F, pix, y, x);
        o0 = sq::mk(F.cam_pos[0], F.cam_pos[1], F.cam_pos[2]);
        d0 = primary_dir(F.cam_rot, F.w, F.h, y, x);
    }
    const GlobalNodes N{ S.branches, S.cull_child, S.cull_child != nullptr };
    f3 sum = sq::mk(0, 0, 0), sum2 = sq::mk(0, 0, 0);
    const Hit h0 = trace_one(S, N, o0, d0, stk, kBlock);
    if (h0.tri >= 0) {
        sum = fold_start(F, pix);
        if constexpr (AD) { if (F.sum2) sum2 = fold_start2(F, pix); }
        const Surface s0 = surface_of(S, h0.tri);
        const f3 p0 = o0 + sq::scale(h0.t, d0);
        long long rix;
        if constexpr (SRC == kSrcRays) rix = F.ray_seed[pix];
        else rix = (long long)F.samples * ((long long)x + (long long)y * (long long)F.w);   // src/Lib.hs:85
#pragma unroll 1
        for (int k = F.k_begin; k < F.k_end; ++k) {
            long long seed = rix + k;
            asm volatile("" : "+v"(seed));                              // as in sq_gen_bounce1: the block is not an induction of this loop
            uint64_t c[4];
            sq::threefish256_key_only((uint64_t)seed, c);
            int tr[kMaxDepth];
#pragma unroll
            for (int i = 0; i < kMaxDepth; ++i) tr[i] = -1;
            f3 o = p0, d = d0; Surface sb = s0;
            f3 inner = sq::mk(0, 0, 0);
#pragma unroll 1
            for (int b = 1; b < depth; ++b) {                           // ray b = bounceRay gen_{b-1} ray_{b-1} inter_{b-1}
                const f3 nd = bounce_dir(d, sb, tf_word(c, b - 1), tf_word(c, b));
                const Hit h = trace_one(S, N, o, nd, stk, kBlock);
                if (h.tri < 0) { if constexpr (SKY) inner = sky_at(K, sky_t(nd)); break; }
#pragma unroll
                for (int i = 1; i < kMaxDepth; ++i) tr[i] = i == b ? h.tri : tr[i];
                sb = surface_of(S, h.tri);
                o = o + sq::scale(h.t, nd); d = nd;                     // intersectPoint, src/Geometry.hs:134
            }
            const f3 r = path_radiance(S, s0, tr, inner);
            sum = sum + r;
            if constexpr (AD) sum2 = sum2 + r * r;
        }
    } else if constexpr (SKY) {
        sum = fold_start(F, pix);
        if constexpr (AD) { if (F.sum2) sum2 = fold_start2(F, pix); }
        const f3 r = sky_at(K, sky_t(d0));
        for (int k = F.k_begin; k < F.k_end; ++k) {
            sum = sum + r;
            if constexpr (AD) sum2 = sum2 + r * r;
        }
    }
    if constexpr (AD) {
        if (F.sum2) { float* o = F.sum2 + pix * 3; o[0] = sum2.x; o[1] = sum2.y; o[2] = sum2.z; }
        store_count(F, pix);
    }
    store_fold(F, pix, sum);
}
template <typename StackT, int SRC, bool AD, typename... SkyT>
__global__ void __launch_bounds__(kBlock) sq_render_pixels_deep(const SceneView S, const FrameOf<SRC> F, const int depth, const SkyT... K) {
    render_pixels_deep_body<StackT, SRC, AD, sizeof...(SkyT) != 0>(S, F, depth, sky_arg<Sky>(K...));
}

// Wavefront form: the levels go through the planned trace kernel one after the other.  A slot's state byte alternates between the
// two values the trace kernel knows: ray b waits as kRay1 when b is odd and as kRay2 when b is even, so the launch of one level never
// takes the rays the bounce kernel has just written for the next.  After the frame's own primary pass, per batch of samples:
// sq_deep_gen (ray 1), then for b = 1 .. D-1 a trace launch and sq_deep_bounce (records the triangle ray b hit; finishes the slot or
// writes ray b + 1), then sq_deep_fold.
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

// Bounce 0 of every sample of the batch: sq_gen_bounce1 without the shared mirror ray (a sample that mirrors gets a ray of its own).
template <int SRC, typename FrameT>
__device__ __forceinline__ void deep_gen_body(const SceneView& S, const FrameT& F, const Work& W, int k_base, int k_count, const RngView R) {
    const int A = *W.n_active;
    for (int a = blockIdx.x * kBlock + threadIdx.x; a < A; a += gridDim.x * kBlock) {
        const Pixel0 P = load_pixel0<SRC>(S, F, W, a);
        const long long rix = seed_base<SRC>(F, W, a, P);
        const bool dead = absorbs(S, P.s0);                             // no ray: sq_deep_fold knows the pixel absorbs
        const f3 d1_mirror = mirror_dir(P.d0, P.s0);
        const long long first = rix + k_base;
        const bool use = R.words != nullptr && rix >= 0 && rix <= R.cover - (long long)F.samples;   // the table is read, never grown
#pragma unroll 1
        for (int kl = blockIdx.y; kl < k_count; kl += gridDim.y) {
            const long long sid = (long long)kl * A + a;
            if (dead) { W.state[sid] = kDone; continue; }
            uint32_t n0, n1, n2;
            if (use) { const uint32_t* p = R.words + 3 * (first + kl); n0 = p[0]; n1 = p[1]; n2 = p[2]; }
            else {
                long long seed = first + kl;
                asm volatile("" : "+v"(seed));
                sq::tfgen3(seed, n0, n1, n2);
            }
            const f3 d1 = scatters(P.s0, n0) ? scatter_dir(P.d0, P.s0, n0, n1) : d1_mirror;
            W.state[sid] = kRay1;
            W.org[sid] = make_float4(P.p0.x, P.p0.y, P.p0.z, __uint_as_float(n1));
            W.dir[sid] = make_float4(d1.x, d1.y, d1.z, __uint_as_float(n2));
        }
    }
}
template <int SRC>
__global__ void __launch_bounds__(kBlock) sq_deep_gen(const SceneView S, const FrameOf<SRC> F, const Work W, int k_base, int k_count, const RngView R) { deep_gen_body<SRC>(S, F, W, k_base, k_count, R); }

// After the trace launch of level b = D.level (1 .. depth - 1): the slot's hit goes into the trail; a miss, the last level, an absorbing
// surface or a last ray that can reach no emitter finishes the slot, anything else puts ray b + 1 into it.  One thread per active pixel.
template <int SRC, bool SKY, typename FrameT>
__device__ __forceinline__ void deep_bounce_body(const SceneView S, const FrameT F, const Work W, int k_base, int k_count, const Deep D, const DeepSky K) {
    const int A = *W.n_active;
    const int b = D.level;
    const uint8_t mine = (b & 1) ? kRay1 : kRay2, next = (b & 1) ? kRay2 : kRay1;
    int32_t* trail_b = D.trail + (long long)(b - 1) * D.cap;
    for (int a = blockIdx.x * kBlock + threadIdx.x; a < A; a += gridDim.x * kBlock) {
        const Pixel0 P = load_pixel0<SRC>(S, F, W, a);
        if (absorbs(S, P.s0)) continue;                                 // every slot of the pixel is kDone since sq_deep_gen
        const long long first = seed_base<SRC>(F, W, a, P) + k_base;
#pragma unroll 1
        for (int kl = blockIdx.y; kl < k_count; kl += gridDim.y) {
            const long long sid = (long long)kl * A + a;
            if (W.state[sid] != mine) continue;
            const float4 org = W.org[sid];
            const int2 hit = slot_hit(org);
            const int tri = hit.y >= 0 ? hit.y : -1;
            trail_b[sid] = tri;
            if constexpr (SKY) { if (tri < 0) { const float4 dm = W.dir[sid]; K.tmiss[sid] = sky_t(sq::mk(dm.x, dm.y, dm.z)); } }
            if (tri < 0 || b + 1 >= D.depth) { W.state[sid] = kDone; continue; }   // nothing below, by a miss or by the depth
            const Surface sb = surface_of(S, tri);
            if (absorbs(S, sb)) { trail_b[sid + D.cap] = -1; W.state[sid] = kDone; continue; }
            const float4 dir = W.dir[sid];
            const f3 d = sq::mk(dir.x, dir.y, dir.z);
            f3 o = P.p0;
            if (b > 1) { const float2 xy = D.oxy[sid]; o = sq::mk(xy.x, xy.y, org.z); }
            const f3 p = o + sq::scale(__int_as_float(hit.x), d);       // intersectPoint, src/Geometry.hs:134
            uint32_t nu = __float_as_uint(org.w), nv = __float_as_uint(dir.w);   // (n_1, n_2)
            if (b > 1) {
                long long seed = first + kl;
                asm volatile("" : "+v"(seed));
                uint64_t c[4];
                sq::threefish256_key_only((uint64_t)seed, c);
                nu = tf_word(c, b); nv = tf_word(c, b + 1);
            }
            const f3 nd = bounce_dir(d, sb, nu, nv);
            // Ray b + 1 is the last one when b + 2 == depth: all it adds is the emission of what it hits, so, as in sq_shade1, a ray
            // whose own triangle test rejects every emitter (finite materials: n_emitters >= 0) need not be traced.
            if (b + 2 == D.depth && S.n_emitters >= 0) {
                bool may_reach = false;
                for (int j = 0; j < S.n_emitters && !may_reach; ++j) {
                    const float* tp = S.tris + 9 * (size_t)S.emitters[j];
                    float t_unused;
                    may_reach = moller_trumbore(p, nd, sq::mk(tp[0], tp[1], tp[2]), sq::mk(tp[3], tp[4], tp[5]), sq::mk(tp[6], tp[7], tp[8]), t_unused);
                }
                if (!may_reach) { trail_b[sid + D.cap] = -1; W.state[sid] = kDone; continue; }
            }
            if (b + 2 < D.depth) D.oxy[sid] = make_float2(p.x, p.y);    // a later bounce forms this ray's hit point
            W.state[sid] = next;
            W.org[sid] = make_float4(p.x, p.y, p.z, 0.0f);
            W.dir[sid] = make_float4(nd.x, nd.y, nd.z, 0.0f);
        }
    }
}
template <int SRC, typename... SkyT>
__global__ void __launch_bounds__(kBlock) sq_deep_bounce(const SceneView S, const FrameOf<SRC> F, const Work W, int k_base, int k_count, const Deep D, const SkyT... K) {
    // (not through sky_arg: the body takes the DeepSky by value, and a copy of a copy gave the sky instantiations another register allocation)
    if constexpr (sizeof...(SkyT) != 0) deep_bounce_body<SRC, true>(S, F, W, k_base, k_count, D, K...);
    else deep_bounce_body<SRC, false>(S, F, W, k_base, k_count, D, DeepSky{});
}

// The batch's samples folded in order, one thread per active pixel: each sample's radiance is rebuilt from its trail, inside out
// (path_radiance), and added to the pixel's sums; on the call's last batch the pixel's stores, as sq_accumulate does them.
template <typename... SkyT>
__global__ void __launch_bounds__(kBlock) sq_deep_fold(const SceneView S, const Frame F, const Work W, int k_count, int last, const Deep D, const SkyT... K) {
    const int A = *W.n_active;
    const bool mom2 = W.px_sum2 != nullptr;
    for (int a = blockIdx.x * kBlock + threadIdx.x; a < A; a += gridDim.x * kBlock) {
        f3 sum = sq::mk(W.px_sum[3 * a], W.px_sum[3 * a + 1], W.px_sum[3 * a + 2]), sum2 = sq::mk(0, 0, 0);
        if (mom2) sum2 = sq::mk(W.px_sum2[3 * a], W.px_sum2[3 * a + 1], W.px_sum2[3 * a + 2]);
        const Surface s0 = surface_of(S, W.px_tri0[a]);
        const f3 rad0 = level0_radiance(s0);
        const bool flat = D.depth < 2 || absorbs(S, s0);                // every sample ends at level 0: nothing was traced, nothing to read
        for (int k = 0; k < k_count; ++k) {
            f3 rad = rad0;
            if (!flat) {
                const long long sid = (long long)k * A + a;
                int tr[kMaxDepth];
#pragma unroll
                for (int i = 0; i < kMaxDepth; ++i) tr[i] = -1;
                bool more = true;
#pragma unroll
                for (int b = 1; b < kMaxDepth; ++b) {
                    if (more && b < D.depth) { tr[b] = D.trail[(long long)(b - 1) * D.cap + sid]; more = tr[b] >= 0; }
                }
                if constexpr (sizeof...(SkyT) != 0) {
                    // under a sky a -1 is a miss and nothing else (launch_frame turns the shortcuts off): behind it, t of the ray that missed
                    const DeepSky& DS = sky_arg<DeepSky>(K...);
                    rad = path_radiance(S, s0, tr, more ? sq::mk(0, 0, 0) : sky_at(DS.sky, DS.tmiss[sid]));
                } else rad = path_radiance(S, s0, tr, sq::mk(0, 0, 0));
            }
            sum = sum + rad;
            if (mom2) sum2 = sum2 + rad * rad;
        }
        if (mom2) {
            if (!last) { W.px_sum2[3 * a] = sum2.x; W.px_sum2[3 * a + 1] = sum2.y; W.px_sum2[3 * a + 2] = sum2.z; }
            else { float* o = F.sum2 + (long long)W.px_pixel[a] * 3; o[0] = sum2.x; o[1] = sum2.y; o[2] = sum2.z; }
        }
        if (!last) { W.px_sum[3 * a] = sum.x; W.px_sum[3 * a + 1] = sum.y; W.px_sum[3 * a + 2] = sum.z; continue; }
        store_fold(F, W.px_pixel[a], sum);
    }
}

// ----------------------------------------------------------------------------------------------
// Host: scene upload (validation and packing: sq_host.cpp, sq_pack.h)
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
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) s->n_cu = prop.multiProcessorCount;
    // One arena for every array of the scene: one hipMalloc, one host-packed hipMemcpy and (sq_scene_free) one hipFree
    // instead of thirteen of each -- the one-shot calls upload and free a scene per frame, and at the CLI's default frame
    // (540 x 540 at 10 samples) those calls were a third of the call's time.  Every array starts on a 256-byte boundary.
    // The table: each SceneView member and its vector, in arena order; an empty optional array takes no room and stays nullptr.
    SceneView& v = s->view;
    auto arrays = [&](auto&& f) {
        f(v.branches, P.branches, false); f(v.leaves, P.leaves, false); f(v.tris, P.tris, false); f(v.tri_mat, P.tri_mat, false);
        f(v.surfs, P.surfs, false); f(v.mats, P.mats, false); f(v.verts4, P.verts4, false); f(v.trix, P.trix, false);
        f(v.rbranch, P.rbranch, false); f(v.emitters, P.emitters, false);
        f(v.cull_child, P.cull_child, true); f(v.cull_child16, P.cull_child16, true); f(v.branches_m, P.branches_m, true);
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
    v.rtail = nullptr; v.incremental_ok = 0;               // unread by every kernel (sq_scene.h)
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
extern "C" int32_t sq_shard_global_row(int32_t j, sq_shard sh) {
    const int32_t blk = j / sh.row_block;
    return (blk * sh.n_shards + sh.shard) * sh.row_block + (j - blk * sh.row_block);
}

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

// What the planner (sq_plan.h, sq_host.cpp) reads of a scene for `call`: its packed scalars, options, device and state.
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
    static bool static_lds_checked = false;                           // per instantiation; once per process is enough
    if (C.resident && !static_lds_checked) {
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
        static_lds_checked = true;
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
    // Level-1 culling (sq_host.cpp, level1_tables): where the plan says so
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
    if (!overlap) {
        // Plain schedule: everything on the caller's stream, batch after batch.  The mirror rays ride in front of batch 0, level 0
        // (slots behind the sample slots, dequeued first) instead of having a launch, and a ramp-down, of their own.
        const long long front = (long long)W.slot_capacity;
        for (int i = 0; i < n_real; ++i) {
            if (gen(i, stream)) return 1;
            if (i == 0 && mirror_gen(front)) return 1;
            if (trace(i, 0, stream, i == 0)) return 1;
            if (i == 0 && mirror_store(front)) return 1;
            if (shade(i, stream) || trace(i, 1, stream, false) || accumulate(i, stream, i == n_real - 1)) return 1;
        }
        return 0;
    }
    // The overlapped schedules give the mirror rays a launch of their own, before the tracks split.
    SQ_HIP(hipMemsetAsync(W.head[0], 0, 32 * sizeof(int32_t), stream));
    if (mirror_gen(0) || launch_trace_kernel(s, S, C, trace_fn, W, pixels, 1, 0, stream, false) || mirror_store(0)) return 1;
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
    if (s->opt.overlap == 2) {
        // Two pipelines: even batches run start to end on the caller's stream, odd batches on the second stream.  A trace
        // launch needs a whole CU's LDS per workgroup, so the two tracks' launches do not share CUs: the later one's
        // workgroups move in as the earlier one's finish, which fills the ramp-down of every launch (a ray takes
        // 150-300 us from fetch to hit, and a launch ends when its slowest rays do) and overlaps the per-sample kernels
        // of one track with the trace launches of the other.  Only the accumulation is ordered across tracks (src/Lib.hs:88).
        std::vector<hipEvent_t> eAcc((size_t)n_real);
        for (int i = 0; i < n_real; ++i) if (new_event(&eAcc[(size_t)i])) return 1;
        hipEvent_t e_setup2, e_done2;
        if (new_event(&e_setup2) || new_event(&e_done2)) return 1;
        SQ_HIP(hipEventRecord(e_setup2, stream));
        SQ_HIP(hipStreamWaitEvent(X, e_setup2, 0));
        for (int i = 0; i < n_real; ++i) {
            const hipStream_t on = (i & 1) ? X : stream;
            if (gen(i, on) || trace(i, 0, on, false) || shade(i, on) || trace(i, 1, on, false)) return 1;
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
// (the largest frames a call takes, kMaxCallPixels / kMaxWavefrontPixels, and refuse_frame_size: sq_plan.h)
bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}
// The check every entry point makes of its device buffers: r = the ranges of which no two may overlap (NULL = not given).
struct NamedRange { const char* name; const void* p; size_t bytes; };
int refuse_overlaps(const NamedRange* r, int count) {
    for (int i = 0; i < count; ++i)
        for (int j = i + 1; j < count; ++j)
            if (r[i].p && r[j].p && ranges_overlap(r[i].p, r[i].bytes, r[j].p, r[j].bytes))
                return sq_set_error("%s and %s overlap", r[i].name, r[j].name);
    return 0;
}
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

// The stopping rule of the adaptive sampler (squigly_hip.h): one thread per pixel; every operation is one fp32 operation, in the
// header's order (the build has -ffp-contract=off).  A wave counts its live pixels with a ballot and adds them with one atomic.
__global__ void __launch_bounds__(kBlock) sq_adaptive_update(long long n_pixels, const float* sum, const float* sum2, const int32_t* count,
                                                             float tol, float eps, uint8_t* mask, int32_t* live_out) {
    const long long p = (long long)blockIdx.x * kBlock + threadIdx.x;
    bool live = false;
    if (p < n_pixels && mask[p] != 0) {
        const int32_t c = count[p];
        const float n = (float)c;
        float L = 0.0f, R = 0.0f;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float sc = sum[3 * p + ch], qc = sum2[3 * p + ch];
            const float ss = sc * sc;
            const float lhs = n * qc - ss, rhs = ss + eps * (n * n);
            L = ch == 0 ? lhs : L + lhs;
            R = ch == 0 ? rhs : R + rhs;
        }
        const bool converged = c >= 2 && L <= ((n - 1.0f) * (tol * tol)) * R;   // a NaN compares false: the pixel stays live
        if (converged) mask[p] = 0;
        live = !converged;
    }
    const unsigned long long m = sq_ballot(live);                       // every lane of the wave gets here
    if ((threadIdx.x & 63) == 0 && m != 0) atomicAdd(live_out, __popcll(m));
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
    if (set_option(s->opt, key, value)) return 1;                       // names, ranges and messages: the option table (sq_host.cpp)
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
