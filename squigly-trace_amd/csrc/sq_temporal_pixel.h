// sq_temporal_pixel.h — the arithmetic of one pixel of a temporal accumulation (include/squigly_temporal.h), written once for the
// host and the device: sq_temporal_project compiles `project` with the host compiler, every lane of libsquigly_temporal.so's kernel
// compiles all of it with the device compiler, and tests/temporal_main.cpp (`project`) and tests/moving_main.cpp (`accumulate`, the
// static and the moving call's pixel alike) compile it with g++ under the sanitizers.  Only the temporal library lists this header.
//
// Every operation is one fp32 operation in the order of the header's contract (tests/temporal_restatement.py restates it in numpy);
// -ffp-contract=off and the correctly rounded divide keep the two equal.  Nothing is skipped for a zero weight: 0 * inf is NaN here too.
#pragma once
#include <stdint.h>

#include "sq_math.h"

namespace temporalpix {

// A 16-byte record of the history block.  Three planes of them: CV colour.rgb + variance, NL normal.xyz + length (an int32's bits),
// PT point.xyz + triangle (an int32's bits).
struct alignas(16) Rec { float x, y, z, w; };

SQ_HD float int_bits(int32_t i) { float f; __builtin_memcpy(&f, &i, sizeof f); return f; }
SQ_HD int32_t bits_int(float f) { int32_t i; __builtin_memcpy(&i, &f, sizeof i); return i; }

struct Params { float alpha_min; int32_t max_history; float sigma_p, cos_n; };

// The inverse of makeRay (src/Lib.hs:107-114) for the world point (px, py, pz) under the camera (pos, rot) of an image of ww rows
// and hh columns: fx is the column, fy the row.  False when the point does not project (behind the camera, or more than a pixel
// outside the image; a NaN compares false); fx and fy are then whatever the arithmetic left.
SQ_HD bool project(const float* pos, const float* rot, float ww, float hh, float px, float py, float pz, float& fx, float& fy) {
    const float ex = px - pos[0], ey = py - pos[1], ez = pz - pos[2];
    const float k0 = (ex * rot[0] + ey * rot[1]) + ez * rot[2];
    const float k1 = (ex * rot[3] + ey * rot[4]) + ez * rot[5];
    const float k2 = (ex * rot[6] + ey * rot[7]) + ez * rot[8];
    fx = 0.0f; fy = 0.0f;
    if (!(k0 > 0.0f)) return false;
    const float xo = k1 / k0, yo = k2 / k0;
    fx = xo * ww + ww / 2.0f;
    fy = hh / 2.0f - yo * hh;
    return fx >= -1.0f && fx < hh && fy >= -1.0f && fy < ww;
}

struct Pixel { float r, g, b, v; int32_t len; };

// What the moving call adds to a pixel: the way back through its object's move, and the clamp.
struct Clamp { int32_t radius; float k; };
struct Bounds { float lo[3], hi[3]; };

constexpr uint32_t kBlended = 1u, kClamped = 2u, kMoved = 4u;          // the bits of d_out_flags

// The point (px, py, pz) and the direction (nx, ny, nz) taken through the row-major 3 x 4 B = [L | t]: P' = L P + t, n' = L n.
SQ_HD void move_back(const float* B, float& px, float& py, float& pz, float& nx, float& ny, float& nz) {
    const float qx = ((B[0] * px + B[1] * py) + B[2] * pz) + B[3];
    const float qy = ((B[4] * px + B[5] * py) + B[6] * pz) + B[7];
    const float qz = ((B[8] * px + B[9] * py) + B[10] * pz) + B[11];
    const float mx = (B[0] * nx + B[1] * ny) + B[2] * nz;
    const float my = (B[4] * nx + B[5] * ny) + B[6] * nz;
    const float mz = (B[8] * nx + B[9] * ny) + B[10] * nz;
    px = qx; py = qy; pz = qz; nx = mx; ny = my; nz = mz;
}

// The clamp's bounds from the window's taps.  tap(j, i, c) says whether the tap (row offset j, column offset i) counts -- inside the
// image and a hit -- and then leaves its colour in c[3]: the kernel's two forms differ in where a tap is read from and in nothing
// else.  The centre of a hit pixel counts, so n >= 1 wherever the bounds are used.
template <class Tap>
SQ_HD Bounds window_bounds(const Clamp& K, Tap tap) {
    float n = 0.0f, s[3] = { 0.0f, 0.0f, 0.0f }, s2[3] = { 0.0f, 0.0f, 0.0f };
    for (int j = -K.radius; j <= K.radius; ++j)
        for (int i = -K.radius; i <= K.radius; ++i) {
            float c[3];
            if (!tap(j, i, c)) continue;
            n = n + 1.0f;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                s[ch] = s[ch] + c[ch];
                s2[ch] = s2[ch] + c[ch] * c[ch];
            }
        }
    Bounds b;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const float mu = s[ch] / n;
        float vr = s2[ch] / n - mu * mu;
        if (!(vr > 0.0f)) vr = 0.0f;
        const float sd = sq::fsqrt(vr);
        const float ks = K.k * sd;
        b.lo[ch] = mu - ks;
        b.hi[ch] = mu + ks;
    }
    return b;
}

// The pixel's result from its inputs and the previous block (cv, nl, pt: the three planes; nullptr = no history), for both calls.
// alpha < 0 never raises a (the caller passes -1 without d_alpha: a >= alpha_min >= 0 > -1).  The point and the normal are taken
// through B (12 floats, read only if `moved`; otherwise the pixel is static: P' = P and n' = n, bit for bit) and the history colour
// is held to the window's bounds (K; nullptr = no clamp, and `tap` is then never called).  flags receives the bits of d_out_flags.
// The window is read only where history is blended.  The old call's pixel is moved = false and K = nullptr.  (`moved` and B stay two
// arguments: handed `moved ? B : nullptr` the device compiler keeps the transform in scratch.)
template <class Tap>
SQ_HD Pixel accumulate(const Rec* cv, const Rec* nl, const Rec* pt, int32_t rows, int32_t cols, const float* pos, const float* rot,
                       const Params& P, float cr, float cg, float cb, float v, int32_t tri, float nx, float ny, float nz,
                       float px, float py, float pz, bool has_alpha, float alpha, bool moved, const float* B, const Clamp* K,
                       Tap tap, uint32_t& flags) {
    Pixel out = { cr, cg, cb, v, 1 };
    flags = 0u;
    if (!cv || tri < 0) return out;
    if (moved) {
        move_back(B, px, py, pz, nx, ny, nz);
        flags = kMoved;
    }
    float fx, fy;
    if (!project(pos, rot, (float)rows, (float)cols, px, py, pz, fx, fy)) return out;
    const float x0 = __builtin_floorf(fx), y0 = __builtin_floorf(fy);
    const float tx = fx - x0, ty = fy - y0;
    const long long ix = (long long)x0, iy = (long long)y0;
    float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sv = 0.0f;
    int32_t m = 0x7fffffff;
    // The twelve records of the four taps are loaded first, each from an address that does not depend on another load: a tap's three
    // loads one behind the other, each behind the test of the one before, left the kernel waiting for twelve round trips a pixel.  A
    // tap outside the image reads pixel 0 and is left out below.
    bool in[4];
    Rec pqs[4], nqs[4], cqs[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const long long qy = iy + (t >> 1), qx = ix + (t & 1);
        in[t] = qy >= 0 && qy < rows && qx >= 0 && qx < cols;
        const long long q = in[t] ? qy * cols + qx : 0;
        pqs[t] = pt[q];
        nqs[t] = nl[q];
        cqs[t] = cv[q];
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const Rec pq = pqs[2 * j + i], nq = nqs[2 * j + i], cq = cqs[2 * j + i];
            if (!in[2 * j + i] || bits_int(pq.w) < 0) continue;
            const float bw = (i ? tx : 1.0f - tx) * (j ? ty : 1.0f - ty);
            const float dn = (nx * nq.x + ny * nq.y) + nz * nq.z;
            if (!(dn >= P.cos_n)) continue;
            const float dx = pq.x - px, dy = pq.y - py, dz = pq.z - pz;
            const float pd = (nx * dx + ny * dy) + nz * dz;
            if (!(__builtin_fabsf(pd) <= P.sigma_p)) continue;
            sw = sw + bw;
            sr = sr + bw * cq.x;
            sg = sg + bw * cq.y;
            sb = sb + bw * cq.z;
            sv = sv + bw * cq.w;
            const int32_t lq = bits_int(nq.w);
            m = lq < m ? lq : m;
        }
    }
    if (!(sw > 0.0f)) return out;
    flags |= kBlended;
    float hc[3] = { sr / sw, sg / sw, sb / sw };
    const float hv = sv / sw;
    if (K) {
        const Bounds b = window_bounds(*K, tap);
        bool bit = false;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            if (hc[ch] < b.lo[ch]) { hc[ch] = b.lo[ch]; bit = true; }
            if (hc[ch] > b.hi[ch]) { hc[ch] = b.hi[ch]; bit = true; }
        }
        if (bit) flags |= kClamped;
    }
    const int32_t m1 = (int32_t)((uint32_t)m + 1u);
    float a = 1.0f / (float)m1;
    if (a < P.alpha_min) a = P.alpha_min;
    if (has_alpha && a < alpha) a = alpha;
    out.r = hc[0] + a * (cr - hc[0]);
    out.g = hc[1] + a * (cg - hc[1]);
    out.b = hc[2] + a * (cb - hc[2]);
    const float om = 1.0f - a;
    out.v = (om * om) * hv + (a * a) * v;
    out.len = m1 < P.max_history ? m1 : P.max_history;
    return out;
}

}  // namespace temporalpix
