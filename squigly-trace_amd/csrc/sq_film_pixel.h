// sq_film_pixel.h — the arithmetic of the display stage (include/squigly_film.h), written once for the host and the device: every
// lane of libsquigly_film.so's kernels compiles it with the device compiler, and tests/film_main.cpp compiles it with g++, plainly and
// under the sanitizers.  Only the film library lists this header.
//
// Every operation is one fp32 operation in the order of the header's contract (tests/film_restatement.py restates it in numpy);
// -ffp-contract=off and the correctly rounded divide keep the two equal.  sq_math.h is read for sq::tonemap, fatan, to_word8 and kPi.
#pragma once
#include <stdint.h>

#include "sq_math.h"

namespace filmpix {

constexpr int kSlots = 2048;
enum { REFERENCE = 0, ATAN = 1, REINHARD = 2, FILMIC = 3, LINEAR = 4, kCurves = 5 };

SQ_HD uint32_t float_bits(float f) { uint32_t u; __builtin_memcpy(&u, &f, sizeof u); return u; }
SQ_HD float bits_float(uint32_t u) { float f; __builtin_memcpy(&f, &u, sizeof f); return f; }

// ---------------- the meter ----------------
SQ_HD float luminance(float r, float g, float b) { return (0.25f * r + 0.5f * g) + 0.25f * b; }
SQ_HD int slot(float L) {
    if (!(L > 0.0f)) return 0;
    if (L == __builtin_inff()) return kSlots - 1;
    return (int)(float_bits(L) >> 20);
}

struct Meter { float key; int32_t permille; float e_min, e_max, rate, fallback; };

SQ_HD bool usable(float p) { return p > 0.0f && p < __builtin_inff(); }          // finite and > 0 (a NaN compares false)
SQ_HD uint64_t rank_of(uint64_t M, int32_t permille) {
    const uint64_t r = (M * (uint64_t)permille + 999u) / 1000u;
    return r < 1 ? 1 : r;
}
// The exposure from the metered slot s (read only when M > 0) and the exposure of the frame before.
SQ_HD float exposure(uint64_t M, int s, const Meter& m, bool has_prev, float prev) {
    const bool carry = has_prev && usable(prev);
    if (M == 0) return carry ? prev : m.fallback;
    const float Lp = bits_float(((uint32_t)s << 20) | 0x80000u);
    float t = m.key / Lp;
    if (t < m.e_min) t = m.e_min;
    if (t > m.e_max) t = m.e_max;
    if (!carry) return t;
    const float step = t - prev;
    const float move = m.rate * step;
    return prev + move;
}
// ---------------- the development of a pixel ----------------
// The 8 x 8 Bayer matrix of the header, row y, column x.
SQ_HD float bayer_threshold(int y, int x) {
    static constexpr uint8_t B[64] = {  0, 32,  8, 40,  2, 34, 10, 42,
                                       48, 16, 56, 24, 50, 18, 58, 26,
                                       12, 44,  4, 36, 14, 46,  6, 38,
                                       60, 28, 52, 20, 62, 30, 54, 22,
                                        3, 35, 11, 43,  1, 33,  9, 41,
                                       51, 19, 59, 27, 49, 17, 57, 25,
                                       15, 47,  7, 39, 13, 45,  5, 37,
                                       63, 31, 55, 23, 61, 29, 53, 21 };
    return ((float)B[(y & 7) * 8 + (x & 7)] + 0.5f) * 0.015625f;
}

SQ_HD float table(const float* lut, int32_t n_lut, float d) {
    float v = d;
    if (!(v > 0.0f)) v = 0.0f;
    if (v > 1.0f) v = 1.0f;
    const float t = v * (float)(n_lut - 1);
    int i = (int)t;
    if (i > n_lut - 2) i = n_lut - 2;
    const float f = t - (float)i;
    const float lo = lut[i], hi = lut[i + 1];
    const float rise = hi - lo;
    return lo + f * rise;
}

SQ_HD uint8_t quantise(float d, float th) {
    const float q = d * 255.0f + th;
    if (!(q > 0.0f)) return 0;
    if (q >= 255.0f) return 255;
    return (uint8_t)(int)q;
}

SQ_HD float filmic(float v) {
    const float a = 2.51f * v + 0.03f;
    const float num = v * a;
    const float b = 2.43f * v + 0.59f;
    const float den = v * b + 0.14f;
    return num / den;
}

// (intensity / mx) of sq::tonemap, operation for operation.
SQ_HD float atan_scale(sq::f3 x) {
    const float mx = sq::hmax(sq::hmax(x.x, x.y), x.z), mn = sq::hmin(sq::hmin(x.x, x.y), x.z);
    const float lightness = 0.5f * (mx + mn);
    const float intensity = sq::fatan(lightness) / (sq::kPi / 2);
    return intensity / mx;
}

struct Develop { float white; const float* lut; int32_t n_lut; };

// One pixel: colour c at (row y, column x) under the exposure e.  CURVE, LUT and DITHER are the same for every pixel of a call, so
// they are template arguments: nothing of them is decided inside the pixel.  rgb: three bytes; disp: three floats.
template <int CURVE, bool LUT, bool DITHER>
SQ_HD void develop(const Develop& D, float e, sq::f3 c, int y, int x, uint8_t* rgb, float* disp) {
    const sq::f3 v = sq::mk(e * c.x, e * c.y, e * c.z);
    if (CURVE == REFERENCE) {
        sq::tonemap(v, rgb);
        const sq::f3 d = sq::scale(atan_scale(v), v);
        disp[0] = d.x; disp[1] = d.y; disp[2] = d.z;
        return;
    }
    sq::f3 d = v;
    if (CURVE == ATAN) d = sq::scale(atan_scale(v), v);
    if (CURVE == REINHARD) {
        const float L = luminance(v.x, v.y, v.z);
        const float w2 = D.white * D.white;
        const float t = 1.0f + L / w2;
        const float Ld = (L * t) / (1.0f + L);
        const float s = Ld / L;
        d = sq::scale(s, v);
    }
    if (CURVE == FILMIC) d = sq::mk(filmic(v.x), filmic(v.y), filmic(v.z));
    if (LUT) d = sq::mk(table(D.lut, D.n_lut, d.x), table(D.lut, D.n_lut, d.y), table(D.lut, D.n_lut, d.z));
    const float th = DITHER ? bayer_threshold(y, x) : 0.5f;
    rgb[0] = quantise(d.x, th); rgb[1] = quantise(d.y, th); rgb[2] = quantise(d.z, th);
    disp[0] = d.x; disp[1] = d.y; disp[2] = d.z;
}

}  // namespace filmpix
