// sq_kernels_lane.h — variant 1, one lane per pixel (or per ray), everything in one kernel, each ray walked by trace_one (sq_scene.h): the
// cross-check variant, also raycast mode.  sq_render_pixels, sq_cast_pixels, sq_render_pixels_deep, sq_intersect_lanes.
#pragma once
#include "sq_frame.h"

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

// Ray queries (sq_intersect_rays_device), variant 1: one lane per ray, the whole query in one kernel (the per-lane walk of sq_primary; the cross-check of the default form,
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
