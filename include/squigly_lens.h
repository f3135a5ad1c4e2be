/* squigly_lens.h — C-ABI of libsquigly_lens.so: jittered, thin-lens primary rays for the frames of libsquigly_hip.so
 * (DESIGN.md 4.21).  A pixel integrates over its area (anti-aliasing) and the camera can have an aperture (depth of field).
 *
 * The library is a client of the public C-ABI of squigly_hip.h: it generates per-sample primary rays on the device, hands them to
 * sq_raytrace_rays_device with the frame's own seed bases, and folds the radiances back into pixels in a fixed order.  It adds
 * no kernel to libsquigly_hip.so and changes none of its sources.
 *
 * Conventions (squigly_hip.h's)
 *  - plain C; every function that returns int returns 0 on success, non-zero on failure, and sq_lens_last_error() then holds a
 *    message (thread-local).  A refused call enqueues nothing and leaves every buffer as it was.
 *  - a call only enqueues work on hip_stream, which may be any stream of the scene's device, non-blocking ones with work pending
 *    included.  The library allocates nothing on the device and keeps no state.  sq_lens_rays_device and
 *    sq_lens_fold_device never wait.  HOST WAIT: sq_lens_render_device inherits that of sq_raytrace_rays_device -- a wavefront
 *    query that outgrows the scene's workspace allocates, and may block the host while the old block is freed; a warm call only
 *    enqueues.
 *  - frames are w ROWS x h COLUMNS as everywhere in squigly_hip.h; a shard's pixels are P = sq_shard_rows(w, sh) * h, in local
 *    row-major order (pixel = local_row * h + x), laid out like d_avg.
 *  - INDEX WIDTHS.  Pixel and ray-slot indices are 32-bit in the kernels, byte offsets 64-bit: one call takes P <= 2^31 - 1 pixels
 *    and P * nb <= 2^31 - 1 ray slots, nb the sub-rays of one batch (for sq_lens_rays_device and sq_lens_fold_device:
 *    r_end - r_begin).  sq_lens_plan never plans a batch beyond that; a P beyond it is refused.  Seeds are 64-bit.
 *
 * THE CONTRACT.  Every operation is one fp32 operation in this order.
 * A frame has S samples per pixel and R sub-rays per pixel: R >= 1 and R divides S; n = S / R samples ride on each sub-ray.
 * R = S is a ray per sample; R = 16 at S = 256 is 16 stratified primary rays at 1/16 of the primary cost.
 * For pixel (y, x) of a w x h frame, with ww, hh as in makeRay (src/Lib.hs:107-114), and sub-ray r:
 *
 *   base   = S * (x + y * w) + r * n                       -- int64; the union over r is the frame's own seeds
 *   m0..m3 = the first four outputs of mkTFGen (NOT base)   -- bitwise complement, two's-complement 64 bits; the order sqo_tfgen_words gives
 *   xs     = fromIntegral x + jitter * random01 m0
 *   ys     = fromIntegral y + jitter * random01 m1
 *   xoffs  = (xs - ww / 2) / ww ;  yoffs = (hh / 2 - ys) / hh
 *   aperture == 0:  o = pos cam ;  dloc = V3 1 xoffs yoffs                     -- no lens arithmetic at all
 *   otherwise:      rad = aperture * sqrt (random01 m2) ;  th = 2 * pi * random01 m3      -- th as randomVector forms it
 *                   lx = rad * cos th ;  ly = rad * sin th                                 -- crd, the numeric spec's evaluation
 *                   o    = pos cam + (V3 0 lx ly `rotVert` rotation cam)
 *                   dloc = V3 1 (xoffs - lx / focus) (yoffs - ly / focus)
 *   d = dloc `rotVert` rotation cam
 *   s_r  = sq_raytrace_rays_device's d_sum for (o, d, seed = base), k in [0, n)     -- the scene's depth and sky apply
 *   sum  = s_0 ;  sum = sum + s_r  for r = 1 .. R-1 ;  sum2 likewise of s_r * s_r (optional output)
 *   avg  = (1 / (float) S) *^ sum ;  rgb = rgbFloatToPixelRGB avg
 *
 * (m0 .. m3 are the low and high halves of the first two words of the generator's Threefish block; random01 is randomR (0, 1),
 * src/Lib.hs:183-188; rotVert is src/Geometry.hs:104-107.)  The sub-rays of one pixel meet on the plane at forward distance focus.
 * With jitter = 0 and aperture = 0 every sub-ray is makeRay's ray, bit for bit; with R = 1 the frame is then bit for bit
 * sq_render_rows_device's; with R = S, sum2 is then a masked call's sum2 under a full mask.  jitter = 1 is a box filter over the
 * pixel.  tests/lens_restatement.py restates the formula in numpy.
 *
 * Out of scope: cast frames; multi-view lens frames; the C++ command line.  Masked and adaptive lens frames -- the same sub-rays for
 * the live pixels of a mask only -- are libsquigly_mlens.so's (include/squigly_mlens.h).
 */
#ifndef SQUIGLY_LENS_H
#define SQUIGLY_LENS_H
#include <stddef.h>
#include <stdint.h>

#include "squigly_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    float jitter;      /* 0 .. 1: the side of the square, in pixels, a sub-ray's image point is drawn from; 0 = the pixel's corner, makeRay's point */
    float aperture;    /* lens radius, world units, >= 0; 0 = a pinhole */
    float focus;       /* forward distance of the plane in focus, > 0; read only when aperture > 0 */
} sq_lens;

const char* sq_lens_last_error(void);
/* Hash of the library's source, headers and flags (build.py: lens_source_id). */
const char* sq_lens_build_id(void);

/* Bytes of workspace a batch of nb sub-rays of P pixels needs: per ray slot an 8-byte seed, 12 bytes of origin, 12 of direction and
 * 12 of sub-ray sum -- 44 bytes -- each of the four arrays rounded up to a multiple of 16.  0 when P < 1, nb < 1 or
 * P * nb > 2^31 - 1.  Monotone in both arguments. */
size_t sq_lens_work_bytes(int64_t P, int32_t nb);

/* The batch plan of sq_lens_render_device, GPU-free: the sub-ray range [r_begin, r_end) of a shard of P pixels is cut into
 * consecutive batches of nb_max sub-rays, the last one shorter, nb_max the largest nb with sq_lens_work_bytes(P, nb) <=
 * work_bytes and P * nb <= 2^31 - 1.  Writes the first min(count, cap) batches as pairs out_r[2 i], out_r[2 i + 1] = (r0, r1) to
 * the HOST array out_r (which may be NULL when cap <= 0) and returns the count; -1 (sq_lens_last_error) when P < 1 or
 * P > 2^31 - 1, r_begin < 0 or r_end <= r_begin, or work_bytes < sq_lens_work_bytes(P, 1). */
int32_t sq_lens_plan(int64_t P, int32_t r_begin, int32_t r_end, size_t work_bytes, int32_t* out_r, int32_t cap);

/* The sub-rays [r_begin, r_end) of every pixel of a shard: o, d and base of THE CONTRACT into d_org, d_dir (DEVICE
 * float[nb * P][3]) and d_seed (DEVICE int64[nb * P]), nb = r_end - r_begin, slot = (r - r_begin) * P + pixel, so that 64
 * consecutive rays are neighbouring pixels.  Needs no scene: `device` names the device the buffers live on.
 * Refused: NULL cam, lens or buffer; S < 1, R < 1 or S % R != 0; r_begin < 0, r_end <= r_begin or r_end > R; jitter outside
 * [0, 1] or not finite; aperture negative or not finite; aperture > 0 with focus not finite or <= 0; w or h < 1, a bad shard;
 * INDEX WIDTHS; any two of the three buffers overlapping.  An empty shard returns 0 and enqueues nothing. */
int sq_lens_rays_device(int32_t device, const sq_camera* cam, const sq_lens* lens, int32_t S, int32_t R,
                        int32_t r_begin, int32_t r_end, int32_t w, int32_t h, sq_shard sh,
                        float* d_org, float* d_dir, int64_t* d_seed, void* hip_stream);

/* The ordered fold of the sub-ray sums d_part (DEVICE float[nb][P][3], nb = r_end - r_begin, block i the sums s_(r_begin + i)) into
 * d_sum (DEVICE float[P][3], required) and d_sum2 (optional): with r_begin == 0 the fold starts from s_0 (and s_0 * s_0) and what
 * the two buffers hold is ignored; with r_begin > 0 it carries on from what they hold, as the _range calls of squigly_hip.h do, so
 * consecutive ranges give the bits of one call.  d_avg (float[P][3]) and d_rgb (uint8[P][3]) are optional and receive
 * (1 / (float) S) *^ sum of the sum folded so far and its tonemap.
 * Refused: NULL d_part or d_sum; P < 1; S < 1; r_begin < 0, r_end <= r_begin or r_end > S; INDEX WIDTHS; any two of the given
 * buffers overlapping. */
int sq_lens_fold_device(int32_t device, int64_t P, int32_t S, int32_t r_begin, int32_t r_end, const float* d_part,
                        float* d_sum, float* d_sum2, float* d_avg, uint8_t* d_rgb, void* hip_stream);

/* The frame: the sub-rays [r_begin, r_end) of the S-sample, R-sub-ray frame of a shard, folded into d_sum (required) and d_sum2
 * (optional) as sq_lens_fold_device does; d_avg and d_rgb (optional) are written by the last batch.  [0, R) is the whole frame.
 * The call enqueues exactly the batches of sq_lens_plan(P, r_begin, r_end, work_bytes): per batch the ray kernel,
 * sq_raytrace_rays_device(k in [0, S / R)) and the fold.  The result does not depend on the batching, and consecutive ranges give
 * the bits of one call.
 * d_work: work_bytes >= sq_lens_work_bytes(P, 1) bytes on the scene's device, 16-byte aligned; its contents on entry do not matter
 * and are undefined afterwards.  The device is the one d_work lives on.
 * Refused before anything is enqueued, every buffer left as it was: NULL scene, cam, lens, d_work or d_sum; everything
 * sq_lens_rays_device refuses; a workspace smaller than one sub-ray of the shard, or misaligned; any two of the given buffers, or a
 * buffer and the workspace, overlapping.  Whatever sq_raytrace_rays_device refuses (the LDS-height limits of the scene's form, ...)
 * is refused with its message passed through; that refusal comes from the first batch's query, after the batch's ray kernel --
 * which writes the workspace only -- was enqueued: every output buffer is as it was.  An empty shard returns 0. */
int sq_lens_render_device(sq_device_scene* s, const sq_camera* cam, const sq_lens* lens, int32_t S, int32_t R,
                          int32_t r_begin, int32_t r_end, int32_t w, int32_t h, sq_shard sh,
                          void* d_work, size_t work_bytes, float* d_sum, float* d_sum2, float* d_avg, uint8_t* d_rgb,
                          void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif
