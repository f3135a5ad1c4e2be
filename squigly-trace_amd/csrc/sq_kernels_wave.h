// sq_kernels_wave.h — variant 2 (default), the wavefront pipeline: its per-pixel and per-sample kernels (everything around the trace
// launches, which are sq_kernels_trace.h) and the small service kernels.
#pragma once
#include "sq_frame.h"

// Option "coresidency" (the counters are named beside Work, sq_frame.h)
__device__ __forceinline__ void diag_aux_wave(const Work& W, int diag, bool at_start) {
    if (!diag || (threadIdx.x & 63) != 0) return;
    const unsigned long long live = atomicAdd(&W.stats[kDiagGauge], 0ull);
    if (at_start) atomicAdd(&W.stats[kDiagWaves], 1ull);
    if (live >= (unsigned long long)diag) atomicAdd(&W.stats[at_start ? kDiagStartBeside : kDiagEndBeside], 1ull);
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
__device__ __forceinline__ int2 slot_hit(const float4& org) { return make_int2(__float_as_int(org.x), __float_as_int(org.y)); }   // what the trace kernel left in org.xy

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

// Level-1 culling (sq_pack_level1.h, build_level1, has the lemma): does the half-plane { p0 + t d1 + s nd : t >= 0, s real } provably
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
// Condition (4) of the lemma, for a sample (3) keeps: the stretch [ta, tb] of ray 1 from whose points the line along nd reaches the
// box [lo - m, hi + m] -- three slabs in t, |t N_k - G_k| <= r_k with N = d1 x nd, G = g x nd, r_k = sum_j |(nd x e_k)_j| h_j -- is empty
// on t >= 0, or misses ray 1's fp32 slab interval of every box of the cover V.  Binary64 on the exact fp32 values; each slab is widened
// by 1e-9 of the scale and each quotient by 1e-9 of itself, and a slab whose |N_k| < 1e-6 constrains nothing.
#ifndef SQ_LEVEL1_COVER
#define SQ_LEVEL1_COVER 1               // 0: an experimental build without the cover (the stretch alone)
#endif
#ifndef SQ_LEVEL1_MIRROR
#define SQ_LEVEL1_MIRROR 1              // experimental builds: 0 without condition (5), 2 with its panels' image boxes alone
#endif
// lim: only the boxes that hold a triangle with `reflective` < lim count (condition 5 asks for the ones that scatter under n1; +inf: all).
__device__ __forceinline__ bool stretch_misses_cover(f3 p0, f3 d1, f3 nd, const double* lo, const double* hi, double m, const uint4* cover, float lim) {
    const double px[3] = { p0.x, p0.y, p0.z }, dx[3] = { d1.x, d1.y, d1.z }, nx[3] = { nd.x, nd.y, nd.z };
    double g[3], h[3], scale = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) { g[k] = 0.5 * (lo[k] + hi[k]) - px[k]; h[k] = 0.5 * (hi[k] - lo[k]) + m; scale += __builtin_fabs(g[k]) + h[k]; }
    const double tol = 1e-9 * scale;
    const double N[3] = { dx[1] * nx[2] - dx[2] * nx[1], dx[2] * nx[0] - dx[0] * nx[2], dx[0] * nx[1] - dx[1] * nx[0] };
    const double G[3] = { g[1] * nx[2] - g[2] * nx[1], g[2] * nx[0] - g[0] * nx[2], g[0] * nx[1] - g[1] * nx[0] };
    const double r[3] = { __builtin_fabs(nx[2]) * h[1] + __builtin_fabs(nx[1]) * h[2], __builtin_fabs(nx[2]) * h[0] + __builtin_fabs(nx[0]) * h[2],
                          __builtin_fabs(nx[1]) * h[0] + __builtin_fabs(nx[0]) * h[1] };
    // one division for the three quotients: 1 / N_k = (the product of the other two) / (the product of all), an unused N_k counting as 1
    bool use[3]; double Nu[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { use[k] = __builtin_fabs(N[k]) >= 1e-6; Nu[k] = use[k] ? N[k] : 1.0; }
    const double inv = 1.0 / ((Nu[0] * Nu[1]) * Nu[2]);
    const double rc[3] = { inv * (Nu[1] * Nu[2]), inv * (Nu[0] * Nu[2]), inv * (Nu[0] * Nu[1]) };
    double ta = 0.0, tb = (double)__builtin_inff();
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double w = r[k] + tol;
        const double q1 = (G[k] - w) * rc[k], q2 = (G[k] + w) * rc[k];
        const double ql = __builtin_fmin(q1, q2), qh = __builtin_fmax(q1, q2);
        ta = use[k] ? __builtin_fmax(ta, ql - 1e-9 * __builtin_fabs(ql)) : ta;
        tb = use[k] ? __builtin_fmin(tb, qh + 1e-9 * __builtin_fabs(qh)) : tb;
    }
    if (ta > tb) return true;                                           // from no point of ray 1 does a line along nd reach the box
    if (!SQ_LEVEL1_COVER || cover == nullptr) return false;
    // the stretch as fp32 numbers, rounded outwards (0 <= ta <= tb here)
    const float ta32 = ta > 1e-30 ? (float)(ta * (1.0 - 0x1p-20)) : 0.0f, tb32 = (float)(tb * (1.0 + 0x1p-20));
    // 1 / d1 and -p0 / d1 as condition (2) formed them, computed again: kept alive across randomVector and the emitter loop they take
    // six registers and the kernel spills (the empty asm keeps the optimiser from seeing the same quotients)
    f3 dh = d1;
    asm volatile("" : "+v"(dh.x), "+v"(dh.y), "+v"(dh.z));
    const f3 df = sq::mk(1.0f / dh.x, 1.0f / dh.y, 1.0f / dh.z);
    const f3 nodf = sq::mk(-p0.x * df.x, -p0.y * df.y, -p0.z * df.z);
    const __attribute__((address_space(4))) float* V = (const __attribute__((address_space(4))) float*)cover;
    // all kLevel1Boxes boxes, without a branch (the packer fills unused entries with copies of the first): a wave leaves a loop with an
    // early exit only when its last lane does, and each turn of it waited for its own scalar loads
    bool may_end = false;                                               // Level1Cover: n | r[] | c[] | box[][6]
#pragma unroll
    for (int j = 0; j < kLevel1Boxes; ++j) {
        const float rj = V[4 + j], cj = V[4 + kLevel1Boxes + j];
        const __attribute__((address_space(4))) float* b = V + 4 + 2 * kLevel1Boxes + 6 * j;
        const float t1 = __builtin_fmaf(b[0], df.x, nodf.x), t2 = __builtin_fmaf(b[3], df.x, nodf.x);
        const float t3 = __builtin_fmaf(b[1], df.y, nodf.y), t4 = __builtin_fmaf(b[4], df.y, nodf.y);
        const float t5 = __builtin_fmaf(b[2], df.z, nodf.z), t6 = __builtin_fmaf(b[5], df.z, nodf.z);
        const float tmin = vmax3(vmin(t1, t2), vmin(t3, t4), vmin(t5, t6));
        const float tmax = vmin3(vmax(t1, t2), vmax(t3, t4), vmax(t5, t6));
        // X's parameter t lies in [tmin, tmax]; the computed t^ within r |t| + c of it
        const float tlo = (tmin - rj * __builtin_fabsf(tmin)) - cj, thi = (tmax + rj * __builtin_fabsf(tmax)) + cj;
        // ray 1 may end on a triangle of this box, at a point of the stretch (Level1Mirror::rmin lies 8 floats behind the cover's end)
        may_end |= vmax(tlo, ta32) <= vmin(thi, tb32) && (!SQ_LEVEL1_MIRROR || V[sizeof(Level1Cover) / 4 + 8 + j] < lim);
    }
    return !may_end;
}
// Ray 1's fp32 slab interval of the box b = lo.xyz, hi.xyz in constant memory, with the operations of cull_slab.
__device__ __forceinline__ void slab_interval(const __attribute__((address_space(4))) float* b, f3 df, f3 nodf, float& tmin, float& tmax) {
    const float t1 = __builtin_fmaf(b[0], df.x, nodf.x), t2 = __builtin_fmaf(b[3], df.x, nodf.x);
    const float t3 = __builtin_fmaf(b[1], df.y, nodf.y), t4 = __builtin_fmaf(b[4], df.y, nodf.y);
    const float t5 = __builtin_fmaf(b[2], df.z, nodf.z), t6 = __builtin_fmaf(b[5], df.z, nodf.z);
    tmin = vmax3(vmin(t1, t2), vmin(t3, t4), vmin(t5, t6));
    tmax = vmin3(vmax(t1, t2), vmax(t3, t4), vmax(t5, t6));
}
// Condition (5) of the lemma, its geometric half, for a sample whose ray 1 passes the box of its mirror class: no triangle that mirrors
// under n1 can send ray 2 to an emitter.  Ray 1 misses every rest box that holds such a triangle; its direction keeps every mirrored
// determinant above the floor; and for no panel of such triangles does ray 1, continued straight through the panel, reach the image of
// the emitters' box behind it.  M: the Level1Mirror record; df, nodf, dd: 1 / d1, -p0 / d1 and |d1|^2 as condition (2) formed them.
// Every comparison is written so that a NaN keeps the sample.
__device__ __forceinline__ bool mirror_cannot_reach(const __attribute__((address_space(4))) float* M, f3 d1, f3 df, f3 nodf, float dd, float un1) {
    const __attribute__((address_space(4))) int32_t* Mi = (const __attribute__((address_space(4))) int32_t*)M;
    const int n_panels = Mi[0], n_w = Mi[2];
    if (n_panels == 0) return false;
    bool keep = !(dd >= M[4] && dd <= M[5]);
    const __attribute__((address_space(4))) float* rest = M + 8 + kLevel1Boxes + 4 * kLevel1W;
#pragma unroll
    for (int j = 0; j < kLevel1Rest; ++j) {
        float tmin, tmax;
        slab_interval(rest + 8 * j, df, nodf, tmin, tmax);
        keep |= rest[8 * j + 6] >= un1 && !(tmax <= 0 || tmin >= tmax);  // (cull_slab's `tmax > 0 && tmin < tmax`, a NaN keeping the sample)
    }
    const float floor2 = M[3] * dd;
    for (int k = 0; k < n_w; ++k) {                                     // (wave-uniform: scene.obj has one)
        const __attribute__((address_space(4))) float* w = M + 8 + kLevel1Boxes + 4 * k;
        const float a = sq::dot(d1, sq::mk(w[0], w[1], w[2]));
        keep |= !(a * a >= floor2);
    }
    const __attribute__((address_space(4))) float* panels = rest + 8 * kLevel1Rest;
    // three panels at a time, without a branch among them (the packer fills unused entries with copies of the first); the groups in a
    // wave-uniform loop of its own, so that a scene with nine panels pays for nine
#pragma unroll 1
    for (int j0 = 0; j0 < n_panels; j0 += 3) {
        {
#pragma unroll
            for (int j = j0; j < j0 + 3; ++j) {
                const __attribute__((address_space(4))) float* b = panels + 16 * j;
                float pmin, pmax, imin, imax;
                slab_interval(b + 6, df, nodf, imin, imax);
#if SQ_LEVEL1_MIRROR == 2
                const bool cannot = imax < imin || imax <= -b[12];      // (the image box alone: tau >= t > -back)
#else
                slab_interval(b, df, nodf, pmin, pmax);
                // ray 1 cannot end on the panel, or its line passes the image box nowhere, or only before it can reach the panel
                const bool cannot = pmax < pmin || pmax <= -b[12] || imax < imin || imax < pmin;
#endif
                keep |= b[13] >= un1 && !cannot;
            }
        }
    }
    return !keep;
}
// May the scattered ray 1 = (p0, d1) of a sample whose generator goes on with n1, n2 be dropped, the sample finished as a
// first-bounce miss?  1: by conditions (1)-(3) of the lemma, 2: by (1), (2) and (4), 3: by (5) in the place of (2), 0: no; p0_ok:
// |p0|^2 is inside the lemma's limit (per pixel).
__device__ __forceinline__ int level1_culled(const SceneView& S, const Level1Cull& C, bool p0_ok, f3 p0, f3 d1, uint32_t n1, uint32_t n2) {
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
    bool mirror5 = false;                                               // (2) fails and (5) stands in for it
    if (has && cull_slab(b, df, nodf)) {
        if (!SQ_LEVEL1_MIRROR || !SQ_LEVEL1_COVER || S.rtail == nullptr) return 0;
        const __attribute__((address_space(4))) float* M = (const __attribute__((address_space(4))) float*)S.rtail + sizeof(Level1Cover) / 4;
        if (!mirror_cannot_reach(M, d1, df, nodf, dd, un1)) return 0;
        mirror5 = true;
    }
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
    if (amin == inf) return mirror5 ? 3 : 1;                            // every emitter rejects +-nd by its determinant alone
    if (!(amin < inf)) return 0;
    // (3), and (4) where it does not decide; under (5) they answer for the triangles that scatter under n1 alone
    const double m = C.em_rho * ((double)eps / (double)amin) + C.em_add;
    // (the box is the scene's: seen as such, its centre and half extents are formed once per kernel and kept in binary64 across the
    // sample loop, twelve registers of which some spill; the empty asm has them formed here)
    double elo[3], ehi[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { elo[k] = C.em_lo[k]; ehi[k] = C.em_hi[k]; asm volatile("" : "+s"(elo[k]), "+s"(ehi[k])); }
    if (halfplane_misses_box(p0, d1, nd, elo, ehi, m)) return mirror5 ? 3 : 1;
    if (!stretch_misses_cover(p0, d1, nd, elo, ehi, m, S.rtail, mirror5 ? sq::unit_float(n1) : inf)) return 0;
    return mirror5 ? 3 : 2;
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
    unsigned int n_culled = 0, n_culled4 = 0, n_culled5 = 0;            // by conditions (1)-(3), by (4) where (3) did not decide, by (5) alone
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
                if (C.on) {
                    const int why = level1_culled(S, C, p0_ok, P.p0, d1, n1, n2);
                    if (why) { finish_level1(W, sid, -1); n_culled += why == 1; n_culled4 += why == 2; n_culled5 += why == 3; continue; }
                }
                W.state[sid] = kRay1;
                W.org[sid] = make_float4(P.p0.x, P.p0.y, P.p0.z, __uint_as_float(n1));
                W.dir[sid] = make_float4(d1.x, d1.y, d1.z, __uint_as_float(n2));
            }
        }
    }
    if (C.on) {                                                         // rays culled, one atomic per wave (the loop above has ended for all its lanes)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { n_culled += __shfl_xor(n_culled, o); n_culled4 += __shfl_xor(n_culled4, o); n_culled5 += __shfl_xor(n_culled5, o); }
        if ((threadIdx.x & 63) == 0 && n_culled) atomicAdd(&W.stats[kStatLevel1Culled], (unsigned long long)n_culled);
        if ((threadIdx.x & 63) == 0 && n_culled4) atomicAdd(&W.stats[kStatLevel1Stretch], (unsigned long long)n_culled4);
        if ((threadIdx.x & 63) == 0 && n_culled5) atomicAdd(&W.stats[kStatLevel1Mirror], (unsigned long long)n_culled5);
    }
    diag_aux_wave(W, F.diag, false);
}
// Four waves per SIMD (126 VGPRs with condition (5), no scratch): with the level-1 culling test inlined, six (80 VGPRs) spill 38 registers and five
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

// ---- ray queries (sq_intersect_rays_device), default form, and sq_camera_rays_device ----
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

// ---- caller-given point lights (sq_scene_set_lights) ----
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

// ---- caller-given path depth (sq_scene_set_depth) ----
// Wavefront form: the levels go through the planned trace kernel one after the other.  A slot's state byte alternates between the
// two values the trace kernel knows: ray b waits as kRay1 when b is odd and as kRay2 when b is even, so the launch of one level never
// takes the rays the bounce kernel has just written for the next.  After the frame's own primary pass, per batch of samples:
// sq_deep_gen (ray 1), then for b = 1 .. D-1 a trace launch and sq_deep_bounce (records the triangle ray b hit; finishes the slot or
// writes ray b + 1), then sq_deep_fold.
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

// ---- service kernels ----
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
