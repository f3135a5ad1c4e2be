/* squigly_mlens.h — C-ABI of libsquigly_mlens.so: the lens frame of squigly_lens.h for the LIVE pixels of a mask only.
 * A dead pixel costs no ray.  It is what adaptive sampling (squigly_hip.h: sq_render_rows_device_masked, sq_adaptive_update_device)
 * needs to run on anti-aliased, depth-of-field frames.
 *
 * The library is a client of the public C-ABI of squigly_hip.h, as libsquigly_lens.so is: it lists the live pixels, generates the
 * sub-rays of the listed pixels, hands them to sq_raytrace_rays_device and folds the radiances back into the listed pixels.  It
 * adds no kernel to libsquigly_hip.so or libsquigly_lens.so and changes none of their exports; a sub-ray's arithmetic is the one
 * device function both lens libraries compile (csrc/sq_lens_ray.h).
 *
 * Conventions (squigly_lens.h's)
 *  - plain C; every function that returns int returns 0 on success, non-zero on failure, and sq_mlens_last_error() then holds a
 *    message (thread-local).  A refused call enqueues nothing and leaves every buffer as it was.
 *  - a call only enqueues work on hip_stream, which may be any stream of the device, non-blocking ones with work pending
 *    included.  The library allocates nothing on the device and keeps no state.  sq_mlens_live_device, sq_mlens_rays_device and
 *    sq_mlens_fold_device never wait.  HOST WAIT: sq_mlens_render_device inherits that of sq_raytrace_rays_device -- a wavefront
 *    query that outgrows the scene's workspace allocates, and may block the host while the old block is freed; a warm call only
 *    enqueues.
 *  - frames are w ROWS x h COLUMNS; a shard's pixels are P = sq_shard_rows(w, sh) * h, in local row-major order, laid out like
 *    d_avg of a masked call.
 *  - INDEX WIDTHS.  Pixel and ray-slot indices are 32-bit in the kernels, byte offsets 64-bit: P <= 2^31 - 1 pixels and
 *    L * nb <= 2^31 - 1 ray slots, L the pixels of the list and nb the sub-rays of one batch.
 *
 * PER-PIXEL STATE, in the layout of a masked call: d_sum and d_sum2 are float[P][3]; d_count is int32[P] and counts SUB-RAYS folded.
 * The terms of sum2 are sub-ray sums, and the n of a stopping rule must be the number of terms.  With S samples and R sub-rays per
 * pixel, n = S / R samples ride on each sub-ray as in squigly_lens.h; a pixel has received count * n samples.
 *
 * THE CONTRACT.  Every operation is one fp32 operation in this order.
 *   LIVE p = (d_mask == NULL || d_mask[p] != 0) && (r_begin == 0 || d_count == NULL || d_count[p] == r_begin)
 *            -- the gap guard of sq_render_rows_device_masked, in sub-rays: a pixel left out of a range cannot come back
 *   list   = the live pixels in ascending order, L of them
 *   for pixel p = list[j], sub-ray r in [r_begin, r_end):
 *     o, d, base = squigly_lens.h's for pixel p and sub-ray r (jitter, lens, seed base: unchanged)      -- ray slot (r - r_begin) * L + j
 *     s_r  = sq_raytrace_rays_device's d_sum for (o, d, seed = base), k in [0, n)     -- the scene's depth and sky apply
 *     sum  = s_0 when r_begin == 0, else what d_sum[p] holds ;  sum = sum + s_r in the order of r ;  sum2 likewise of s_r * s_r
 *     count = r_end
 *     avg  = (1 / (float) (r_end * n)) *^ sum ;  rgb = rgbFloatToPixelRGB avg
 *            -- the divisor is the pixel's own sample count, not S: pixels stop at different r.  At r_end == R it is 1 / (float) S.
 *   a pixel that is not listed is written in none of d_sum, d_sum2, d_count, d_avg, d_rgb.
 *
 * THE THREE PINS
 *  1. With the full list (NULL mask, r_begin = 0), sum and sum2 are sq_lens_render_device's bits for any lens; at r_end = R so are
 *     avg and rgb.
 *  2. With jitter = aperture = 0 and R = S, all five buffers are sq_render_rows_device_masked's bits for the same mask, counts and
 *     ranges; dead pixels are untouched.
 *  3. Consecutive ranges give the bits of one call, and the result does not depend on the batching.
 * tests/mlens_restatement.py restates the live rule, the list and the fold in numpy.
 *
 * Out of scope: cast frames; multi-view frames; both command lines.
 */
#ifndef SQUIGLY_MLENS_H
#define SQUIGLY_MLENS_H
#include <stddef.h>
#include <stdint.h>

#include "squigly_hip.h"
#include "squigly_lens.h"
#ifdef __cplusplus
extern "C" {
#endif

const char* sq_mlens_last_error(void);
/* Hash of the library's source, headers and flags (build.py: mlens_source_id). */
const char* sq_mlens_build_id(void);

/* The live list: d_index (DEVICE int32[P]) receives the LIVE pixels of THE CONTRACT in ascending order in its first L entries --
 * the entries behind them are not written -- and *d_n_live (DEVICE, one int32) receives L.  d_mask (uint8[P]) and d_count
 * (int32[P]) may each be NULL.  Deterministic: one launch in which every workgroup ranks its own 32768 pixels (wave ballots, the
 * wave offsets in LDS) behind its own count of the live pixels in front of them; no workgroup waits for another.  Needs no scene.
 * Refused: NULL d_index or d_n_live; P < 1 or P > 2^31 - 1; r_begin < 0; any two of the given buffers overlapping. */
int sq_mlens_live_device(int32_t device, int64_t P, int32_t r_begin, const uint8_t* d_mask, const int32_t* d_count,
                         int32_t* d_index, int32_t* d_n_live, void* hip_stream);

/* The sub-rays [r_begin, r_end) of the L listed pixels: o, d and base into d_org, d_dir (DEVICE float[nb * L][3]) and d_seed (DEVICE
 * int64[nb * L]), nb = r_end - r_begin, slot = (r - r_begin) * L + j for pixel d_index[j]: with an ascending list 64 consecutive
 * rays are neighbouring pixels.  An entry outside [0, P) gets o = d = +0 and seed 0: a wrong list is no out-of-range access.
 * Refused: everything sq_lens_rays_device refuses (with L for P in INDEX WIDTHS); NULL d_index; L < 0 or L > P; overlaps among
 * the four buffers.  An empty shard or L == 0 returns 0 and enqueues nothing. */
int sq_mlens_rays_device(int32_t device, const sq_camera* cam, const sq_lens* lens, int32_t S, int32_t R,
                         int32_t r_begin, int32_t r_end, int32_t w, int32_t h, sq_shard sh, const int32_t* d_index, int64_t L,
                         float* d_org, float* d_dir, int64_t* d_seed, void* hip_stream);

/* The ordered fold of THE CONTRACT for the listed pixels over d_part (DEVICE float[nb][L][3], block i the sums s_(r_begin + i) of the
 * listed pixels in list order).  d_sum is required; d_sum2, d_count, d_avg and d_rgb are optional.  With r_begin == 0 the fold starts
 * from s_0 and what d_sum and d_sum2 hold is ignored; with r_begin > 0 it carries on from what they hold (a d_sum2 that was not
 * carried so far carries on from what it holds all the same).  An entry outside [0, P) is skipped.
 * PRECONDITION: the list is strictly ascending, which is what sq_mlens_live_device writes.  A duplicate entry is a caller error: two
 * lanes would fold into one pixel.
 * Refused: NULL d_index, d_part or d_sum; P < 1 or P > 2^31 - 1; S < 1, R < 1 or S % R != 0; r_begin < 0, r_end <= r_begin or
 * r_end > R; L < 0 or L > P; INDEX WIDTHS; any two of the given buffers overlapping.  L == 0 returns 0 and enqueues nothing. */
int sq_mlens_fold_device(int32_t device, int64_t P, int32_t S, int32_t R, int32_t r_begin, int32_t r_end, const int32_t* d_index,
                         int64_t L, const float* d_part, float* d_sum, float* d_sum2, int32_t* d_count, float* d_avg, uint8_t* d_rgb,
                         void* hip_stream);

/* The frame: the sub-rays [r_begin, r_end) of the S-sample, R-sub-ray frame for the L listed pixels of a shard.  The call enqueues
 * exactly the batches of sq_lens_plan(L, r_begin, r_end, work_bytes) (squigly_lens.h): per batch the ray kernel,
 * sq_raytrace_rays_device(k in [0, S / R)) and the fold; d_count, d_avg and d_rgb are written by the last batch.  The workspace is
 * sq_lens_work_bytes(L, nb): 44 bytes a slot over L * nb slots.
 * L comes from the HOST: it is what sq_mlens_live_device left in *d_n_live, which an adaptive loop reads back after every step
 * anyway.  An L below the list's true length renders its first L pixels.
 * d_work: work_bytes >= sq_lens_work_bytes(L, 1) bytes on the scene's device, 16-byte aligned; contents undefined afterwards.
 * Refused before anything is enqueued, every buffer left as it was: everything sq_lens_render_device refuses, with P replaced by L
 * where sizes are meant; NULL d_index; L < 0 or L > P; any two of the given buffers, or a buffer and the workspace, overlapping.
 * Whatever sq_raytrace_rays_device refuses is refused with its message passed through, as in sq_lens_render_device: after the first
 * batch's ray kernel -- which writes the workspace only -- was enqueued.  An empty shard or L == 0 returns 0 and enqueues nothing. */
int sq_mlens_render_device(sq_device_scene* s, const sq_camera* cam, const sq_lens* lens, int32_t S, int32_t R,
                           int32_t r_begin, int32_t r_end, int32_t w, int32_t h, sq_shard sh, const int32_t* d_index, int64_t L,
                           void* d_work, size_t work_bytes, float* d_sum, float* d_sum2, int32_t* d_count, float* d_avg,
                           uint8_t* d_rgb, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif
