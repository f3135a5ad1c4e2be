/* squigly_shutter.h — C-ABI of libsquigly_shutter.so: motion blur, the lens frames of squigly_lens.h and squigly_mlens.h under a
 * camera that moves while the shutter is open.  The R sub-rays of a pixel are R consecutive instants of the
 * exposure: time is the third thing they are spread over, beside the pixel's area (jitter) and the lens (aperture, focus).
 *
 * The library is a client of the public C-ABI of squigly_hip.h, as the two lens libraries are: it generates the sub-rays, hands them
 * to sq_raytrace_rays_device and folds the radiances back.  It adds no kernel to the other libraries and changes none of their
 * exports; a sub-ray's lens arithmetic, the kernel bodies and the batch loop are the headers all three compile (csrc/sq_lens_ray.h,
 * csrc/sq_lens_frame.h), and the pose of an instant is csrc/sq_shutter_pose.h, compiled for the host (sq_shutter_pose) and for the
 * device (every lane computes its own pose) from one text.
 *
 * Conventions (squigly_lens.h's)
 *  - plain C; every function that returns int returns 0 on success, non-zero on failure, and sq_shutter_last_error() then holds a
 *    message (thread-local).  A refused call enqueues nothing and leaves every buffer as it was.
 *  - a call only enqueues work on hip_stream, which may be any stream of the device, non-blocking ones with work pending
 *    included.  The library allocates nothing on the device and keeps no state.  sq_shutter_pose touches no device;
 *    sq_shutter_rays_device never waits.  HOST WAIT: sq_shutter_render_device inherits that of sq_raytrace_rays_device, as
 *    sq_lens_render_device does.
 *  - frames, shards, the dense slot order and INDEX WIDTHS are squigly_lens.h's; the listed form's are squigly_mlens.h's (P <= 2^31 - 1
 *    pixels, and P * nb or L * nb <= 2^31 - 1 ray slots a batch).
 *  - the plan, the two folds and the live list are not repeated here: sq_lens_plan and sq_lens_work_bytes, sq_lens_fold_device and
 *    sq_mlens_fold_device, sq_mlens_live_device.
 *
 * THE CONTRACT.  Every operation is one fp32 operation in this order.
 * For pixel (y, x) and sub-ray r of an S-sample, R-sub-ray frame, base, m0..m3, xs, ys, xoffs, yoffs and the lens draws are
 * squigly_lens.h's, unchanged.  Then:
 *
 *   m4   = the fifth output of mkTFGen (NOT base)          -- the low half of the third word of the same Threefish block
 *   tt   = (fromIntegral r + time_jitter * random01 m4) / fromIntegral R
 *   pos  = pos0 + tt *^ (pos1 - pos0)                       -- per component: dc = pos1_c - pos0_c ; pos0_c + tt * dc
 *   ang  = ang0 + tt *^ (ang1 - ang0)                       -- likewise
 *   rot  = rotMatrixRads ang.x ang.y ang.z                  -- bit for bit what sq_rot_matrix_rads returns for these three floats:
 *                                                              crd sine and cosine, yx = ry * rx, rot = rz * yx, an entry the fold
 *                                                              r = a[i][k] * b[k][j] + r over k = 0, 1, 2 from r = +0
 *   o, d = squigly_lens.h's lines with (pos, rot) in place of (pos cam, rotation cam)
 *   s_r, sum, sum2, count, avg, rgb: squigly_lens.h's (dense) or squigly_mlens.h's (listed), unchanged
 *
 *  - DRAWS.  No draw is made when jitter == 0 && aperture == 0 && time_jitter == 0; m4 costs nothing beyond the block m0..m3 come from.
 *  - The exposure is cut into R equal parts and sub-ray r takes its instant from the r-th: its start with time_jitter = 0, anywhere
 *    in it with time_jitter = 1.  Sub-ray 0 of time_jitter = 0 is the open pose; the close pose itself is never reached.
 *  - UNCHECKED INPUTS.  Positions and angles are not checked, as sky and light values are not: NaN and infinity are inputs like any
 *    other, and go through the arithmetic above.
 *  - SIGNED ZEROS.  x + tt * (+0) turns a -0 component of an open pose into +0 (-0 + +0 = +0), also when the two poses are equal: a
 *    position component of -0 comes out as +0.  An angle of -0 gives the same sine and cosine products either way.
 *  - With equal poses the frame is sq_lens_render_device's (dense) or sq_mlens_render_device's (listed) under sq_shutter_pose(m, 0),
 *    bit for bit, for any time_jitter.  With time_jitter = 0, sub-ray r is sq_lens_rays_device's under sq_shutter_pose(m, r / R).
 *
 * tests/shutter_restatement.py restates the formula in numpy.
 * Out of scope: the C++ command line; cast frames; multi-view frames; moving geometry.
 */
#ifndef SQUIGLY_SHUTTER_H
#define SQUIGLY_SHUTTER_H
#include <stddef.h>
#include <stdint.h>

#include "squigly_hip.h"
#include "squigly_lens.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    float pos0[3], ang0[3];   /* position and rotMatrixRads' angles (alpha, beta, gamma: the two lines of a camera file) as the shutter opens */
    float pos1[3], ang1[3];   /* as it closes */
    float time_jitter;        /* 0 .. 1: how much of its own 1/R of the exposure a sub-ray's instant is drawn from; 0 = its start */
} sq_motion;

const char* sq_shutter_last_error(void);
/* Hash of the library's source, headers and flags (build.py: shutter_source_id). */
const char* sq_shutter_build_id(void);

/* The camera at the instant tt: pos and rot of THE CONTRACT for this tt into *out.  Host code, no device: the same text the kernels
 * compile (csrc/sq_shutter_pose.h).  tt is not checked (the frames use [0, 1)); neither is time_jitter, which the pose does not
 * depend on.  Refused: NULL motion or out. */
int sq_shutter_pose(const sq_motion* motion, float tt, sq_camera* out);

/* The sub-rays [r_begin, r_end) of THE CONTRACT: o, d and base into d_org, d_dir and d_seed.
 * d_index == NULL: every pixel of the shard, as sq_lens_rays_device lays them out (slot = (r - r_begin) * P + pixel); L is ignored.
 * Otherwise: the first L entries of the list, as sq_mlens_rays_device (slot = (r - r_begin) * L + j for pixel d_index[j]); an entry
 * outside [0, P) gets o = d = +0 and seed 0.  Needs no scene: `device` names the device the buffers live on.
 * Refused: NULL motion, lens or buffer; everything sq_lens_rays_device refuses about S, R, the range, the lens, w, h and the shard;
 * time_jitter outside [0, 1] or not finite; with a list, L < 0 or L > P; INDEX WIDTHS; overlaps among the buffers.  An empty
 * shard, or a list with L == 0, returns 0 and enqueues nothing. */
int sq_shutter_rays_device(int32_t device, const sq_motion* motion, const sq_lens* lens, int32_t S, int32_t R,
                           int32_t r_begin, int32_t r_end, int32_t w, int32_t h, sq_shard sh, const int32_t* d_index, int64_t L,
                           float* d_org, float* d_dir, int64_t* d_seed, void* hip_stream);

/* The frame: the sub-rays [r_begin, r_end) of the S-sample, R-sub-ray frame under the moving camera.
 * d_index == NULL: sq_lens_render_device's frame over the shard's P pixels -- avg = (1 / (float) S) *^ sum -- and d_count must be
 * NULL; L is ignored.  Otherwise: sq_mlens_render_device's frame over the first L entries of the list -- count = r_end, avg divided by
 * the pixel's own sample count r_end * (S / R), a pixel that is not listed written nowhere.
 * The call enqueues exactly the batches of sq_lens_plan(P or L, r_begin, r_end, work_bytes): per batch the ray kernel,
 * sq_raytrace_rays_device(k in [0, S / R)) and the fold; d_count, d_avg and d_rgb are written by the last batch.  The workspace is
 * sq_lens_work_bytes(P or L, nb), 16-byte aligned, on the scene's device.  The result does not depend on the batching, and consecutive
 * ranges give the bits of one call.
 * Refused before anything is enqueued, every buffer left as it was: NULL scene, motion, lens, d_work or d_sum; everything
 * sq_shutter_rays_device refuses about the frame and the list; d_count without a list; a workspace smaller than one sub-ray, or
 * misaligned; any two of the given buffers, or a buffer and the workspace, overlapping.  Whatever sq_raytrace_rays_device refuses is
 * refused with its message passed through, as in sq_lens_render_device: after the first batch's ray kernel -- which writes the
 * workspace only -- was enqueued. */
int sq_shutter_render_device(sq_device_scene* s, const sq_motion* motion, const sq_lens* lens, int32_t S, int32_t R,
                             int32_t r_begin, int32_t r_end, int32_t w, int32_t h, sq_shard sh, const int32_t* d_index, int64_t L,
                             void* d_work, size_t work_bytes, float* d_sum, float* d_sum2, int32_t* d_count, float* d_avg,
                             uint8_t* d_rgb, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif
