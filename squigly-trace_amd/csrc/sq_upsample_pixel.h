// sq_upsample_pixel.h — the arithmetic of sparse frames (include/squigly_denoise.h: sq_denoise_sparse_mask_device and
// sq_denoise_upsample_device), written once for the host and the device: every lane of libsquigly_denoise.so's two sparse kernels
// compiles it with the device compiler, and tests/upsample_main.cpp compiles it with g++, plainly and under the sanitizers.  Only the
// denoise library lists this header.
//
// Every operation is one fp32 operation in the order of the header's contract (tests/upsample_restatement.py restates it in numpy);
// -ffp-contract=off and the correctly rounded divide keep the two equal.  sq_math.h is read for SQ_HD alone.
#pragma once
#include <stdint.h>

#include "sq_math.h"

namespace upspix {

constexpr int kMaxStride = 16;

struct Lattice { int32_t rows, cols, s, oy, ox; };           // 1 <= s <= 16, 0 <= oy, ox < s
struct Stops { float sigma_p, cos_n; };
struct Guides { const int32_t* tri; const float* normal; const float* point; };
struct Image { const float* color; const float* var; };      // var: NULL without a variance image
struct Sums { float sw, r, g, b, v; };

SQ_HD bool on_lattice(const Lattice& L, int32_t y, int32_t x) { return (y - L.oy) % L.s == 0 && (x - L.ox) % L.s == 0; }

// floor((v - o) / s) * s + o: the lattice coordinate at or before v; v - o >= -(s - 1), so the result may be negative.
SQ_HD int32_t cell(int32_t v, int32_t o, int32_t s) {
    const int32_t d = v - o;
    const int32_t q = d >= 0 ? d / s : -((s - 1 - d) / s);
    return q * s + o;
}

// sw, sc and sv of the pixel (y, x), which is not on the lattice.  COLOR = false: sw alone, from the guides alone (I is not read).
template <bool COLOR, bool VAR>
SQ_HD Sums gather(const Lattice& L, const Stops& K, const Guides& G, const Image& I, int32_t y, int32_t x) {
    const int64_t p = (int64_t)y * L.cols + x;
    const int32_t yl = cell(y, L.oy, L.s), xl = cell(x, L.ox, L.s);
    const float ty = (float)(y - yl) / (float)L.s, tx = (float)(x - xl) / (float)L.s;
    const bool hit = G.tri[p] >= 0;
    float npx = 0.0f, npy = 0.0f, npz = 0.0f, ppx = 0.0f, ppy = 0.0f, ppz = 0.0f;
    if (hit) {
        npx = G.normal[3 * p]; npy = G.normal[3 * p + 1]; npz = G.normal[3 * p + 2];
        ppx = G.point[3 * p]; ppy = G.point[3 * p + 1]; ppz = G.point[3 * p + 2];
    }
    Sums S = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int j = 0; j < 2; ++j) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int i = 0; i < 2; ++i) {
            const int64_t qy = (int64_t)yl + j * L.s, qx = (int64_t)xl + i * L.s;
            if (qy < 0 || qy >= L.rows || qx < 0 || qx >= L.cols) continue;
            const int64_t q = qy * L.cols + qx;
            const bool q_hit = G.tri[q] >= 0;
            if (hit) {
                if (!q_hit) continue;
                const float dn = (npx * G.normal[3 * q] + npy * G.normal[3 * q + 1]) + npz * G.normal[3 * q + 2];
                if (!(dn >= K.cos_n)) continue;
                const float dx = G.point[3 * q] - ppx, dy = G.point[3 * q + 1] - ppy, dz = G.point[3 * q + 2] - ppz;
                const float pd = (npx * dx + npy * dy) + npz * dz;
                if (!(__builtin_fabsf(pd) <= K.sigma_p)) continue;
            } else if (q_hit) {
                continue;
            }
            const float bw = (i ? tx : 1.0f - tx) * (j ? ty : 1.0f - ty);
            S.sw = S.sw + bw;
            if (COLOR) {
                S.r = S.r + bw * I.color[3 * q];
                S.g = S.g + bw * I.color[3 * q + 1];
                S.b = S.b + bw * I.color[3 * q + 2];
                if (VAR) S.v = S.v + bw * I.var[q];
            }
        }
    }
    return S;
}

// mask[p] of sq_denoise_sparse_mask_device.
SQ_HD uint8_t live(const Lattice& L, const Stops& K, const Guides& G, int32_t y, int32_t x) {
    if (on_lattice(L, y, x)) return 1;
    const Image none = { nullptr, nullptr };
    return gather<false, false>(L, K, G, none, y, x).sw > 0.0f ? 0 : 1;
}

// One pixel of sq_denoise_upsample_device: out (three floats) and, with VAR, *out_v.  A pixel that is copied through is moved, not
// computed with, so it keeps its bits (a NaN's payload too); colour and variance are loaded at p only when p is copied through.
template <bool VAR>
SQ_HD void upsample(const Lattice& L, const Stops& K, const Guides& G, const Image& I, const uint8_t* mask, int32_t y, int32_t x,
                    float* out, float* out_v) {
    const int64_t p = (int64_t)y * L.cols + x;
    if (mask[p] == 0 && !on_lattice(L, y, x)) {
        const Sums S = gather<true, VAR>(L, K, G, I, y, x);
        if (S.sw > 0.0f) {
            out[0] = S.r / S.sw; out[1] = S.g / S.sw; out[2] = S.b / S.sw;
            if (VAR) *out_v = S.v / S.sw;
            return;
        }
    }
    out[0] = I.color[3 * p]; out[1] = I.color[3 * p + 1]; out[2] = I.color[3 * p + 2];
    if (VAR) *out_v = I.var[p];
}

}  // namespace upspix
