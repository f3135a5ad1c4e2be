/* squigly_film.h — C-ABI of libsquigly_film.so: the display stage of the device pipeline.  It meters a frame's
 * luminance, settles an exposure and develops the fp32 frame the other libraries leave on the device into an 8-bit image, all on
 * the device: render -> adaptive -> lens / shutter -> denoise -> temporal -> film.
 *
 * The library knows nothing of scenes: it maps device images to device images.
 *
 * Conventions (squigly_temporal.h's)
 *  - plain C; every function that returns int returns 0 on success, non-zero on failure, and sq_film_last_error() then holds a
 *    message (thread-local).  Nothing is written on failure, and a refused call enqueues nothing.
 *  - a call only enqueues work on hip_stream, which may be any stream of `device`, non-blocking ones with work pending included.
 *    The library allocates nothing on the device and keeps no state: there is no HOST WAIT anywhere.  The host structs are read
 *    before the call returns.
 *  - images are rows x cols, row-major, 3 values per pixel; rows * cols <= 2^31 - 1.
 *  - values are not checked: NaN, infinite and negative inputs are inputs like any other.
 *  - the arithmetic is pinned operation by operation (below; tests/film_restatement.py restates it in numpy, and the text of
 *    csrc/sq_film_pixel.h is one for the host and the device).
 *
 * Out of scope: the C++ command line; shards and more than one GPU; film on the main library's own out_rgb (sq_render_rows_device
 * and its kin keep the reference's tonemap).  Glare and white balance come before this stage: squigly_denoise.h's
 * sq_denoise_glare_device makes the exposed frame that develop then takes at exposure 1.
 *
 * The contract.  Every operation is one fp32 operation, in exactly this order.
 *
 * Luminance and its slot.  L = (0.25f * r + 0.5f * g) + 0.25f * b (the denoiser's weights).  slot(L) = 0 if !(L > 0) (zero,
 * negative, NaN); 2047 if L == +inf; otherwise float_as_uint(L) >> 20: eight slots per stop, 0 .. 2039; the positive subnormals
 * share slots 0 .. 7 (slot 0 with the values that are not positive).
 *
 * Exposure (sq_film_expose_device).  M = sum of hist[1 .. 2046] as uint64.
 *   M == 0:  e = *d_prev if d_prev is given and *d_prev is finite and > 0, else fallback.
 *   else:    rank = max(1, (M * permille + 999) / 1000);  s = the smallest slot >= 1 whose running sum over 1 .. s reaches rank
 *            Lp = uint_as_float((s << 20) | 0x80000);  t = key / Lp
 *            t = e_min if t < e_min;  t = e_max if t > e_max
 *            e = t if d_prev is NULL or *d_prev is not (finite and > 0);  else p = *d_prev, e = p + rate * (t - p)
 *
 * Development (sq_film_develop_device), per pixel (row y, column x) with colour c:
 *   e = d_exposure ? *d_exposure : params->exposure;  x = e * c per component
 *   curve 0 REFERENCE: rgb = rgbFloatToPixelRGB(x) (src/Lib.hs:93-104) with its wrap and NaN quirks, what the renderer itself
 *                      writes when e == 1; d_display, if given, holds (intensity / mx) * x.  No table, no dither.
 *   curve 1 ATAN:      mx = max(max(x.r, x.g), x.b), mn = min(...) (Haskell's Ord: x <= y ? y : x);  lightness = 0.5f * (mx + mn)
 *                      intensity = atan(lightness) / (pi / 2) (the project's binary64 arctangent, rounded once)
 *                      d = (intensity / mx) * x
 *   curve 2 REINHARD:  L of x;  w2 = white * white;  t = 1 + L / w2;  Ld = (L * t) / (1 + L);  s = Ld / L;  d = s * x
 *   curve 3 FILMIC:    per component v:  d = (v * (2.51f * v + 0.03f)) / (v * (2.43f * v + 0.59f) + 0.14f)     (Narkowicz's fit)
 *   curve 4 LINEAR:    d = x
 *   table, if d_lut is given, per component:  v = d;  v = 0 if !(v > 0);  v = 1 if v > 1
 *                      t = v * (float)(n_lut - 1);  i = (int)t;  i = n_lut - 2 if larger;  f = t - (float)i
 *                      d = lut[i] + f * (lut[i + 1] - lut[i])
 *   quantise (curves 1 .. 4):  th = dither ? ((float)B[y & 7][x & 7] + 0.5f) * 0.015625f : 0.5f, B the 8 x 8 Bayer matrix below
 *                      q = d * 255.0f + th;  byte = 0 if !(q > 0), 255 if q >= 255, else (uint8_t)(int)q
 *   d_display receives d (after the table).
 *
 * The Bayer matrix B, row y, column x:
 *       0 32  8 40  2 34 10 42
 *      48 16 56 24 50 18 58 26
 *      12 44  4 36 14 46  6 38
 *      60 28 52 20 62 30 54 22
 *       3 35 11 43  1 33  9 41
 *      51 19 59 27 49 17 57 25
 *      15 47  7 39 13 45  5 37
 *      63 31 55 23 61 29 53 21
 */
#ifndef SQUIGLY_FILM_H
#define SQUIGLY_FILM_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SQ_FILM_SLOTS 2048            /* uint32 counts of a histogram */

enum { SQ_FILM_REFERENCE = 0, SQ_FILM_ATAN = 1, SQ_FILM_REINHARD = 2, SQ_FILM_FILMIC = 3, SQ_FILM_LINEAR = 4 };

typedef struct {
    float   key;           /* the luminance the metered percentile is brought to */
    int32_t permille;      /* 1..1000: the percentile of the positive, finite luminances that is metered */
    float   e_min, e_max;  /* 0 < e_min <= e_max, finite: the clamp of the target exposure */
    float   rate;          /* 0..1: how far an exposure moves from *d_prev to its target in one call */
    float   fallback;      /* > 0: the exposure of a frame without a positive, finite luminance and without a previous one */
} sq_film_meter;

typedef struct {
    float   exposure;      /* read when d_exposure is NULL */
    int32_t curve;         /* SQ_FILM_REFERENCE .. SQ_FILM_LINEAR */
    float   white;         /* curve 2: > 0, not NaN; +inf = plain Reinhard.  Not read by the other curves */
    int32_t n_lut;         /* 2..65536 entries of d_lut; not read when d_lut is NULL */
    int32_t dither;        /* 0 or 1 */
} sq_film_params;

const char* sq_film_last_error(void);
/* Hash of the library's source, headers and flags (build.py: film_source_id). */
const char* sq_film_build_id(void);

/* The luminance histogram of a frame: d_hist receives SQ_FILM_SLOTS uint32 counts, whose sum is rows * cols.  The call zeroes d_hist
 * on the stream and then counts; the counts are integer adds, so the result is exact and does not depend on the launch's shape.
 * Refused: d_color or d_hist NULL; rows or cols < 1 or rows * cols > 2^31 - 1; d_hist not 4-byte aligned; d_color and d_hist
 * overlapping. */
int sq_film_histogram_device(int32_t device, int32_t rows, int32_t cols, const float* d_color, uint32_t* d_hist, void* hip_stream);

/* Auto-exposure on the device: one float out, from a histogram, the meter and, optionally, the exposure of the frame before.
 * d_prev may be d_exposure (the state of a sequence, updated in place).
 * Refused: d_hist, meter or d_exposure NULL; d_hist not 4-byte aligned; permille outside 1..1000; e_min or e_max not finite, e_min
 * <= 0 or e_min > e_max; rate outside 0..1 or NaN; fallback not > 0; any overlap other than d_prev == d_exposure. */
int sq_film_expose_device(int32_t device, const uint32_t* d_hist, const sq_film_meter* meter, const float* d_prev /* optional */,
                          float* d_exposure, void* hip_stream);

/* Develops a frame: d_rgb receives rows * cols * 3 bytes and d_display, when given, rows * cols * 3 floats.
 * d_exposure: optional, one float on the device (sq_film_expose_device's); d_lut: optional, params->n_lut floats.
 * Where d_color is 16-byte aligned and d_rgb 4-byte aligned a lane develops four consecutive pixels (16-byte loads, dword stores);
 * otherwise a lane develops one pixel.  The two forms give the same bits.
 * Refused: d_color, params or d_rgb NULL; a bad size; curve outside 0..4; with curve 2 a white that is NaN or not > 0; with d_lut
 * an n_lut outside 2..65536; dither other than 0 or 1; d_lut or dither with curve 0; any overlap among d_color, d_exposure, d_lut,
 * d_rgb and d_display. */
int sq_film_develop_device(int32_t device, int32_t rows, int32_t cols, const float* d_color, const float* d_exposure /* optional */,
                           const sq_film_params* params, const float* d_lut /* optional */, uint8_t* d_rgb,
                           float* d_display /* optional */, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif
