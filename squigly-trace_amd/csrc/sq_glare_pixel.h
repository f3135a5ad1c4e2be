// sq_glare_pixel.h — the arithmetic of the glare stage (include/squigly_denoise.h: sq_denoise_glare_device), written once for the host
// and the device: every lane of libsquigly_denoise.so's glare kernels compiles it with the device compiler, and tests/glare_main.cpp
// compiles it with g++, plainly and under the sanitizers.  Only the denoise library lists this header.
//
// Every operation is one fp32 operation in the order of the header's contract (tests/glare_restatement.py restates it in numpy);
// -ffp-contract=off and the correctly rounded divide keep the two equal.  sq_math.h is read for SQ_HD and sq::f3.
#pragma once
#include <stdint.h>

#include "sq_math.h"

namespace glarepix {

constexpr int kMaxLevels = 8;

struct Glare { float gain[3]; float threshold, ceiling, spread, strength; };

// r_k of r_{k-1}: no level is ever empty.
SQ_HD int32_t half_up(int32_t n) { return (int32_t)(((int64_t)n + 1) / 2); }
SQ_HD int32_t clampi(int32_t v, int32_t lo, int32_t hi) { return v < lo ? lo : v > hi ? hi : v; }

// x_c = (e * c_c) * gain_c
SQ_HD sq::f3 exposed(float e, const Glare& G, sq::f3 c) { return sq::mk((e * c.x) * G.gain[0], (e * c.y) * G.gain[1], (e * c.z) * G.gain[2]); }

SQ_HD float bright_component(float s, float x, float ceiling) {
    float b = s * x;
    if (!(b >= 0.0f)) b = 0.0f;
    if (b > ceiling) b = ceiling;
    return b;
}
// The bright pass of an exposed pixel: every component of the result lies in [0, ceiling], whatever x holds.
SQ_HD sq::f3 bright(const Glare& G, sq::f3 x) {
    const float L = (0.25f * x.x + 0.5f * x.y) + 0.25f * x.z;
    const float m = L < G.ceiling ? L : G.ceiling;
    const float s = L > G.threshold ? (m - G.threshold) / L : 0.0f;
    return sq::mk(bright_component(s, x.x, G.ceiling), bright_component(s, x.y, G.ceiling), bright_component(s, x.z, G.ceiling));
}

// ---------------- the down step ----------------
// The four taps of output coordinate o over a fine extent n: 2o - 1 .. 2o + 2, each clamped to the fine image.
SQ_HD int32_t down_tap(int32_t o, int k, int32_t n) {
    const int64_t v = 2 * (int64_t)o - 1 + k;            // 2o + 2 can be 2^31 when n = 2^31 - 1
    return (int32_t)(v < 0 ? 0 : v > n - 1 ? n - 1 : v);
}
SQ_HD float tap4(float p0, float p1, float p2, float p3) { return (0.125f * p0 + 0.375f * p1) + (0.375f * p2 + 0.125f * p3); }
SQ_HD sq::f3 tap4(sq::f3 p0, sq::f3 p1, sq::f3 p2, sq::f3 p3) {
    return sq::mk(tap4(p0.x, p1.x, p2.x, p3.x), tap4(p0.y, p1.y, p2.y, p3.y), tap4(p0.z, p1.z, p2.z, p3.z));
}
// D(y, x) of a fine image of r x c that S(j, i) gives the pixels of: the horizontal four-tap of four fine rows, then the vertical one.
template <class Src>
SQ_HD sq::f3 down(const Src& S, int32_t r, int32_t c, int32_t y, int32_t x) {
    sq::f3 h[4];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < 4; ++k) {
        const int32_t j = down_tap(y, k, r);
        h[k] = tap4(S(j, down_tap(x, 0, c)), S(j, down_tap(x, 1, c)), S(j, down_tap(x, 2, c)), S(j, down_tap(x, 3, c)));
    }
    return tap4(h[0], h[1], h[2], h[3]);
}

// ---------------- the up step ----------------
// The two coarse coordinates and weights of fine coordinate v over a coarse extent N.
struct UpTap { int32_t i0, i1; float a, b; };
SQ_HD UpTap up_tap(int32_t v, int32_t N) {
    const int32_t i0 = (v - 1) >> 1;                    // arithmetic: -1 at v = 0
    UpTap t;
    t.i0 = clampi(i0, 0, N - 1);
    t.i1 = clampi(i0 + 1, 0, N - 1);
    t.a = (v & 1) ? 0.75f : 0.25f;
    t.b = 1.0f - t.a;
    return t;
}
SQ_HD float up4(const UpTap& Y, const UpTap& X, float p00, float p01, float p10, float p11) {
    return Y.a * (X.a * p00 + X.b * p01) + Y.b * (X.a * p10 + X.b * p11);
}
// U(y, x) of a coarse image of R x C that S(j, i) gives the pixels of.
template <class Src>
SQ_HD sq::f3 up(const Src& S, int32_t R, int32_t C, int32_t y, int32_t x) {
    const UpTap Y = up_tap(y, R), X = up_tap(x, C);
    const sq::f3 p00 = S(Y.i0, X.i0), p01 = S(Y.i0, X.i1), p10 = S(Y.i1, X.i0), p11 = S(Y.i1, X.i1);
    return sq::mk(up4(Y, X, p00.x, p01.x, p10.x, p11.x), up4(Y, X, p00.y, p01.y, p10.y, p11.y), up4(Y, X, p00.z, p01.z, p10.z, p11.z));
}

// A_k = B_k + spread * U(A_k+1);  out = x + strength * U(A_0): both are v + w * u.
SQ_HD sq::f3 add_scaled(sq::f3 v, float w, sq::f3 u) { return sq::mk(v.x + w * u.x, v.y + w * u.y, v.z + w * u.z); }

}  // namespace glarepix
