/* squigly_denoise.h — C-ABI of libsquigly_denoise.so: a variance- and geometry-guided edge-avoiding filter for the frames
 * libsquigly_hip.so leaves on the device.
 *
 * The filter knows nothing of scenes, trees or generators: it maps device images to device images.  Its inputs are what the
 * other library's calls leave behind: d_sum, d_sum2, d_count of sq_render_rows_device_masked (the variance), d_tri and d_point
 * of sq_intersect_rays_device over sq_camera_rays_device (the guides).
 *
 * Conventions (squigly_hip.h's)
 *  - plain C; every function that returns int returns 0 on success, non-zero on failure, and sq_denoise_last_error() then
 *    holds a message (thread-local).  Nothing is written on failure, and a refused call enqueues nothing.
 *  - a call only enqueues work on hip_stream, which may be any stream of `device`, non-blocking ones with work pending
 *    included.  The library allocates nothing on the device and keeps no state: there is no HOST WAIT anywhere.
 *  - images are rows x cols, row-major, laid out like d_avg (the project's "w rows x h columns"): a colour, normal or point
 *    image has 3 floats per pixel, a variance or triangle image one value.
 *  - values are not checked: NaN, infinite and negative inputs are inputs like any other.
 *  - the arithmetic is pinned operation by operation (below; tests/denoise_restatement.py restates it in numpy), so every
 *    kernel form gives the same bits.
 */
#ifndef SQUIGLY_DENOISE_H
#define SQUIGLY_DENOISE_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    int32_t passes;            /* 1..8; pass i uses step 2^i */
    float   sigma_l, eps_l;    /* luminance stop, in standard deviations; floor */
    float   sigma_p;           /* plane-distance stop, world units */
    int32_t normal_squarings;  /* 0..8: normal weight = max(0, n_p.n_q)^(2^k) */
    int32_t form;              /* 0 = choose per pass; 1.. = force one kernel form (tests, timing) */
} sq_denoise_params;

/* Kernel forms of a pass (params.form).  Every form gives the same bits. */
#define SQ_DENOISE_FORM_AUTO   0   /* per pass: what sq_denoise_pass_form says */
#define SQ_DENOISE_FORM_DIRECT 1   /* every tap is read from the workspace records (L1 / L2) */
#define SQ_DENOISE_FORM_TILED  2   /* a 16 x 16 tile plus its halo of 2 * step pixels is staged in LDS; steps 1, 2 and 4 only:
                                      a larger step takes the direct form even when this one is forced */
#define SQ_DENOISE_N_FORMS     2

const char* sq_denoise_last_error(void);
/* Hash of the library's source, headers and flags (build.py: denoise_source_id). */
const char* sq_denoise_build_id(void);
/* The form form = 0 runs pass `pass` (step 2^pass) in; -1 when pass is not in 0..7. */
int32_t sq_denoise_pass_form(int32_t pass);

/* Bytes of workspace sq_denoise_device needs for a rows x cols image: four 16-byte records per pixel (normal + validity, point,
 * and two of colour + variance that the passes go to and fro between).  0 when rows or cols < 1 or rows * cols > 2^31 - 1.
 * Monotone in both arguments. */
size_t sq_denoise_workspace_bytes(int32_t rows, int32_t cols);

/* The variance of the pixel mean's luminance from a masked call's statistics, for n_pixels >= 0 pixels.  Every operation is
 * one fp32 operation, in this order:
 *     n = (float)count;   per channel c:  m_c = s_c / n;  d_c = q_c / n - m_c * m_c;  var_c = d_c > 0 ? d_c / (n - 1) : +0
 *     v = (0.0625 * var_0 + 0.25 * var_1) + 0.0625 * var_2
 * a pixel with count < 2 gets v = l * l with l = (0.25 * m_0 + 0.5 * m_1) + 0.25 * m_2, a pixel with count < 1 gets +0.
 * d_var must not overlap an input.  Refused: a NULL pointer, n_pixels < 0, an overlap. */
int sq_denoise_variance_device(int32_t device, int64_t n_pixels, const float* d_sum, const float* d_sum2,
                               const int32_t* d_count, float* d_var, void* hip_stream);

/* The filter.  Pass i = 0 .. passes-1 uses s = 2^i and maps (C_i, V_i) to (C_i+1, V_i+1); C_0 = d_color, V_0 = d_var, the last
 * pair goes to d_out and d_out_var.  valid(p) = d_tri[p] >= 0; n_p, P_p = d_normal[p], d_point[p];
 * l(c) = (0.25 * c.r + 0.5 * c.g) + 0.25 * c.b;  K = {0.375, 0.25, 0.0625};  G = {0.5, 0.25}.  Every operation is one fp32
 * operation, in exactly this order:
 *   a pixel that is not valid is copied through, colour and variance, bit for bit, in every pass.  For a valid p = (y, x):
 *   with variance:  gs = gw = +0;  for dy = -1, 0, 1 (outer), dx = -1, 0, 1, q = (y+dy, x+dx) inside the image and valid:
 *                       g = G[|dy|] * G[|dx|];  gs = gs + g * V_i[q];  gw = gw + g
 *                   gv = gs / gw;  sd = sigma_l * sqrt(gv) + eps_l
 *   sw = +0, sc = (+0, +0, +0), sv = +0;  taps dy = -2..2 (outer), dx = -2..2 (inner), q = (y + dy*s, x + dx*s); a tap outside the
 *   image or not valid is left out, otherwise
 *       kw = K[|dy|] * K[|dx|]
 *       dn = (n_p.x*n_q.x + n_p.y*n_q.y) + n_p.z*n_q.z;  t = dn > 0 ? dn : +0;  t = t * t, normal_squarings times
 *       e = P_q - P_p;  pd = (n_p.x*e.x + n_p.y*e.y) + n_p.z*e.z;  a = pd / sigma_p;  wz = 1 / (1 + a * a)
 *       with variance:  b = (l(C_i[q]) - l(C_i[p])) / sd;  wl = 1 / (1 + b * b);  w = ((kw * t) * wz) * wl
 *       without d_var:  w = (kw * t) * wz
 *       sw = sw + w;  sc_c = sc_c + w * C_i[q]_c;  sv = sv + (w * w) * V_i[q]
 *   if sw > 0:  C_i+1[p]_c = sc_c / sw,  V_i+1[p] = sv / (sw * sw);  otherwise (a NaN compares false) the pixel is copied through.
 * A tap whose weight is zero is still added (0 * inf is the NaN the expression says).
 *
 * d_var and d_out_var are optional (NULL), d_out_var only with d_var.  d_out == d_color and d_out_var == d_var are allowed.
 * d_work: work_bytes >= sq_denoise_workspace_bytes(rows, cols) bytes on the device, 16-byte aligned; its contents on entry do
 * not matter and are undefined afterwards.
 * Refused before anything is enqueued: a NULL required pointer; rows or cols < 1 or rows * cols > 2^31 - 1; passes,
 * normal_squarings or form out of range; a sigma that is NaN or <= 0, eps_l NaN or < 0; d_out_var without d_var; work_bytes too
 * small or d_work misaligned; any other overlap among the buffers or with the workspace. */
int sq_denoise_device(int32_t device, int32_t rows, int32_t cols,
                      const float* d_color, const float* d_var /* optional */,
                      const int32_t* d_tri, const float* d_normal, const float* d_point,
                      const sq_denoise_params* params,
                      float* d_out, float* d_out_var /* optional, only with d_var */,
                      void* d_work, size_t work_bytes, void* hip_stream);

/* Measurement aid (tools/gpu_denoise.py): one stage of the call above on its own, so that it can be timed between two events.
 * stage -1 is the pack pre-pass (inputs -> workspace records), stage i in 0..passes-1 is pass i, which reads the workspace as
 * the stages before it left it.  Running the stages -1, 0, .., passes-1 in order is sq_denoise_device. */
int sq_denoise_stage_device(int32_t device, int32_t rows, int32_t cols,
                            const float* d_color, const float* d_var, const int32_t* d_tri, const float* d_normal,
                            const float* d_point, const sq_denoise_params* params, float* d_out, float* d_out_var,
                            void* d_work, size_t work_bytes, void* hip_stream, int32_t stage);

/* ---- Sparse frames: trace a lattice of pixels and the holes, fill the rest from the guides ----
 *
 * The seed of a sample does not depend on the call, so a pixel that sq_render_rows_device_masked traces under the mask below holds
 * bit for bit what the dense frame holds there; only the pixels filled in are new arithmetic.  Every operation is one fp32 operation,
 * in exactly this order; integers are int32.
 *
 * The lattice of stride s (1..16) and offset (oy, ox), 0 <= oy, ox < s, is the set of pixels (y, x) with (y - oy) % s == 0 and
 * (x - ox) % s == 0.  For a pixel p = (y, x) that is not on the lattice, sw(p), sc(p) and sv(p) are
 *     yl = floor((y - oy) / s) * s + oy;  xl likewise          (floor division: yl may be < 0)
 *     ty = (float)(y - yl) / (float)s;    tx = (float)(x - xl) / (float)s
 *     sw = +0;  sc = (+0, +0, +0);  sv = +0
 *     taps j = 0, 1 (outer), i = 0, 1 (inner):  q = (yl + j*s, xl + i*s); a tap outside the image is left out.
 *       if tri[p] >= 0 the tap is accepted only if all of these hold (a NaN compares false):
 *           tri[q] >= 0
 *           dn = (n_p.x*n_q.x + n_p.y*n_q.y) + n_p.z*n_q.z   and  dn >= cos_n
 *           d = P_q - P_p;  pd = (n_p.x*d.x + n_p.y*d.y) + n_p.z*d.z   and  fabsf(pd) <= sigma_p
 *       if tri[p] < 0 the tap is accepted only if tri[q] < 0: sky is filled in from sky.
 *       for an accepted tap:
 *           bw = (i ? tx : 1 - tx) * (j ? ty : 1 - ty)
 *           sw = sw + bw;  sc_c = sc_c + bw * C[q]_c;  sv = sv + bw * V[q]
 * A tap whose weight is zero is still added (0 * inf is the NaN the expression says).
 *
 * Both calls: no workspace, no allocation, no state, no host wait, any stream.  Refused before anything is enqueued: a NULL required
 * pointer; rows or cols < 1 or rows * cols > 2^31 - 1; stride outside 1..16; oy or ox outside [0, stride); sigma_p NaN or < 0; cos_n
 * NaN; d_out_var without d_var; any overlap among the buffers.
 * Out of scope: lens, shutter, adaptive and cast frames as the sparse renderer, shards and several devices, and a history weight
 * that favours traced over filled-in pixels (the Python driver, temporal.py, renders whole path-traced frames on one device). */
typedef struct {
    float sigma_p;             /* plane-distance stop, world units; >= 0 */
    float cos_n;               /* least n_p . n_q of an accepted tap */
} sq_denoise_sparse_params;

/* Which pixels have to be traced.  d_mask[p] (uint8, rows * cols) = 1 if p is on the lattice, or if sw(p) > 0 is false -- a hole: a
 * pixel no traced neighbour may speak for; 0 otherwise.  It reads the guides alone, so the mask exists before anything is rendered,
 * and one masked render call serves the lattice and the holes together. */
int sq_denoise_sparse_mask_device(int32_t device, int32_t rows, int32_t cols, int32_t stride, int32_t oy, int32_t ox,
                                  const int32_t* d_tri, const float* d_normal, const float* d_point,
                                  const sq_denoise_sparse_params* params, uint8_t* d_mask, void* hip_stream);

/* Fills in the pixels that were not traced.  A pixel that is on the lattice or has d_mask[p] != 0 is copied through, colour and
 * variance, bit for bit.  Any other pixel gets out_c = sc_c / sw and out_v = sv / sw if sw(p) > 0, and is copied through as well if
 * not -- under the mask above there is no such pixel; this makes the call total for any mask.  Colour and variance are loaded only
 * at pixels that are copied through and at lattice pixels (the taps): under the mask above, only where the masked call rendered.
 * d_var and d_out_var are optional (NULL), d_out_var only with d_var.  d_out and d_out_var overlap no input. */
int sq_denoise_upsample_device(int32_t device, int32_t rows, int32_t cols, int32_t stride, int32_t oy, int32_t ox,
                               const float* d_color, const float* d_var /* optional */,
                               const int32_t* d_tri, const float* d_normal, const float* d_point, const uint8_t* d_mask,
                               const sq_denoise_sparse_params* params,
                               float* d_out, float* d_out_var /* optional, only with d_var */, void* hip_stream);

/* ---- Glare and white balance: a bloom pyramid ahead of the film stage ----
 *
 * The frame is exposed and white-balanced, what of it is brighter than `threshold` is carried down a pyramid of `levels` levels and
 * up again, and the sum is added to the exposed frame: the float frame squigly_film.h's develop call then takes at exposure 1.
 * The conventions are this header's: nothing is enqueued on a refusal; no allocation, no state, no host wait, any stream; images are
 * rows x cols x 3 floats with rows * cols <= 2^31 - 1; values are not checked.  Every operation is one fp32 operation, in exactly the
 * order written; integers are int32 and byte offsets 64-bit.
 *
 * Level sizes: r_-1 = rows, c_-1 = cols; r_k = (r_k-1 + 1) / 2 and c_k likewise, so no level is ever empty.
 *
 * Exposed pixel:  e = d_exposure ? *d_exposure : params->exposure;  x_c = (e * c_c) * gain_c
 *
 * Bright pass, per full-resolution pixel:
 *     L = (0.25 * x.r + 0.5 * x.g) + 0.25 * x.b
 *     m = L < ceiling ? L : ceiling
 *     s = L > threshold ? (m - threshold) / L : +0
 *     b_c = s * x_c;   b_c = +0 if !(b_c >= 0);   b_c = ceiling if b_c > ceiling
 * NaN, negative and infinite values therefore stay in their own pixel: every b lies in [0, ceiling].
 *
 * Down step D: a fine image p of r x c gives (r + 1) / 2 x (c + 1) / 2.  All coordinates are clamped to the fine image, so every tap
 * always takes part.  With a = 0.125 and b = 0.375:
 *     fine row j, output column x:  h(j, x) = (a * p(j, 2x-1) + b * p(j, 2x)) + (b * p(j, 2x+1) + a * p(j, 2x+2))
 *     output row y:                 D(y, x) = (a * h(2y-1, x) + b * h(2y, x)) + (b * h(2y+1, x) + a * h(2y+2, x)),   per component
 *     B_0 = D(b),  B_k = D(B_k-1)
 *
 * Up step U: a coarse image p of R x C gives a fine size r x c.
 *     y0 = (y - 1) >> 1 (arithmetic shift: -1 at y = 0),  y1 = y0 + 1,  both clamped to [0, R - 1]
 *     ay = (y & 1) ? 0.75 : 0.25,  by = 1 - ay;   columns likewise
 *     U(y, x) = ay * (ax * p(y0, x0) + bx * p(y0, x1)) + by * (ax * p(y1, x0) + bx * p(y1, x1))
 *
 * Glare:  A_levels-1 = B_levels-1;   A_k = B_k + spread * U(A_k+1) for k = levels-2 .. 0
 *     levels >= 1:  out_c = x_c + strength * U(A_0)_c at full resolution
 *     levels == 0:  out_c = x_c; nothing else runs, and d_work may be NULL.
 *
 * d_out == d_color, the exact same pointer, is allowed: the last kernel reads d_color at its own pixel only.
 * d_work: work_bytes >= sq_denoise_glare_work_bytes(rows, cols, levels) bytes on the device, 16-byte aligned; its contents on entry
 * do not matter and are undefined afterwards.
 * Refused before anything is enqueued: a NULL required pointer; rows or cols < 1 or rows * cols > 2^31 - 1; levels or form out of
 * range; threshold NaN, negative or infinite; ceiling not finite or not > threshold; spread or strength NaN, negative or infinite;
 * with levels >= 1, work_bytes too small, or d_work NULL or not 16-byte aligned; any overlap among d_color, d_exposure, d_out and
 * d_work other than d_out == d_color.
 * Out of scope: lens-flare streaks and diffraction spikes, per-level colour tints, shards and several devices. */
typedef struct {
    float   exposure;    /* read when d_exposure is NULL */
    float   gain[3];     /* white balance: per-channel factors */
    float   threshold;   /* >= 0, finite: exposed luminance above which a pixel glares */
    float   ceiling;     /* > threshold, finite: what a glaring value saturates at (fireflies, inf) */
    int32_t levels;      /* 0..8 pyramid levels; 0 = exposure and white balance only */
    float   spread;      /* >= 0, finite: weight of each coarser level in the one above it */
    float   strength;    /* >= 0, finite: weight of the glare in the result */
    int32_t form;        /* 0 = choose; 1 = direct; 2 = LDS-tiled (SQ_DENOISE_FORM_*; every form gives the same bits) */
} sq_denoise_glare_params;

/* Bytes of workspace the call below needs: 16 * sum over k < levels of r_k * c_k, a 16-byte record per level pixel.  0 for levels = 0,
 * for rows or cols < 1 or rows * cols > 2^31 - 1, and for levels outside 0..8.  Monotone in all three arguments. */
size_t sq_denoise_glare_work_bytes(int32_t rows, int32_t cols, int32_t levels);
int    sq_denoise_glare_device(int32_t device, int32_t rows, int32_t cols, const float* d_color,
                               const float* d_exposure /* optional, one device float: sq_film_expose_device's */,
                               const sq_denoise_glare_params* params, float* d_out,
                               void* d_work, size_t work_bytes, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif
