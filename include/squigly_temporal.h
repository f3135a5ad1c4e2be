/* squigly_temporal.h — C-ABI of libsquigly_temporal.so: temporal accumulation of the frames libsquigly_hip.so leaves on the device
 * under a camera that moves from frame to frame.  It is the temporal third of an SVGF-style pipeline whose
 * variance estimate and a-trous filter are libsquigly_denoise.so's.
 *
 * The library knows nothing of scenes, trees or generators: it maps device images to device images.  Its inputs are what the other
 * libraries' calls leave behind: the frame's mean colour, the variance of sq_denoise_variance_device, and d_tri, d_point and the
 * unit normal of the first hit (DeviceScene.guides).  The geometry is static, so the world-space points of two frames are compared
 * directly: there are no motion vectors.
 *
 * Conventions (squigly_denoise.h's)
 *  - plain C; every function that returns int returns 0 on success, non-zero on failure, and sq_temporal_last_error() then holds
 *    a message (thread-local).  Nothing is written on failure, and a refused call enqueues nothing.  (sq_temporal_project returns
 *    1 / 0 for "projects" / "does not", and < 0 when refused.)
 *  - a call only enqueues work on hip_stream, which may be any stream of `device`, non-blocking ones with work pending included.
 *    The library allocates nothing on the device and keeps no state: there is no HOST WAIT anywhere.
 *  - images are rows x cols, row-major, laid out like d_avg (the project's "w rows x h columns"): a colour, normal or point image
 *    has 3 floats per pixel, a variance, alpha, length or triangle image one value.
 *  - values are not checked: NaN, infinite and negative inputs are inputs like any other.
 *  - the arithmetic is pinned operation by operation (below; tests/temporal_restatement.py restates it in numpy).
 *
 * Whole frames on one device only: a shard's pixels reproject into rows it does not hold.
 *
 * Out of scope: shards and more than one GPU; lens, shutter and adaptive frames as the per-frame renderer; cast frames; moving
 * geometry; neighbourhood colour clamping; the C++ command line.
 *
 * The history block is opaque to callers: sq_temporal_history_bytes(rows, cols) bytes, 16-byte aligned, three planes of 16-byte
 * records, a record per pixel in each (colour.rgb + variance; normal.xyz + length; point.xyz + triangle), so that a bilinear tap
 * is three 16-byte loads and a wave's loads of one plane are contiguous.  Only sq_temporal_accumulate_device writes one, and a block
 * that it did not write is not a history (its lengths are taken as they are).  Callers go to and fro between two blocks.
 *
 * The contract.  Every operation is one fp32 operation, in exactly this order.  For the pixel p = (row y, column x): colour c,
 * variance v, triangle tri, normal n_p, point P_p; ww = (float)rows, hh = (float)cols.
 *   No history: out_c = c, out_v = v, len = 1, bit for bit -- when d_prev == NULL, tri < 0, the projection fails, or no tap is
 *   accepted (sw > 0 is false).
 *   Projection, the inverse of makeRay (src/Lib.hs:107-114) with its index quirk: the column offset is scaled by the row count and
 *   the row offset by the column count.
 *       e = P_p - prev.pos, per component;  k_i = (e.x * rot[3i] + e.y * rot[3i+1]) + e.z * rot[3i+2], i = 0, 1, 2
 *       fails unless k_0 > 0;  xo = k_1 / k_0;  yo = k_2 / k_0
 *       fx = xo * ww + ww / 2 (the column);  fy = hh / 2 - yo * hh (the row)
 *       fails unless fx >= -1 && fx < hh && fy >= -1 && fy < ww (a NaN compares false)
 *       x0 = floorf(fx), y0 = floorf(fy);  tx = fx - x0, ty = fy - y0
 *   Taps q = (y0 + j, x0 + i), j = 0, 1 (outer), i = 0, 1 (inner).  A tap outside the image or with tri_prev[q] < 0 is left out;
 *   otherwise
 *       bw = (i ? tx : 1 - tx) * (j ? ty : 1 - ty)
 *       dn = (n_p.x * n_q.x + n_p.y * n_q.y) + n_p.z * n_q.z;                    accepted only if dn >= cos_n
 *       d = P_q - P_p;  pd = (n_p.x * d.x + n_p.y * d.y) + n_p.z * d.z;           accepted only if fabsf(pd) <= sigma_p
 *       accepted:  sw = sw + bw;  sc = sc + bw * C_q;  sv = sv + bw * V_q;  m = min(m, len_q)
 *   the sums start from +0, and a tap of weight 0 is still added.
 *   Blend, if sw > 0:
 *       hc = sc / sw;  hv = sv / sw;  a = 1 / (float)(m + 1)
 *       a = alpha_min if a < alpha_min;  then a = d_alpha[p] if d_alpha is given and a < d_alpha[p]
 *       out_c = hc + a * (c - hc);  om = 1 - a;  out_v = (om * om) * hv + (a * a) * v;  len = min(m + 1, max_history)
 *   The next block holds out_c, out_v, len and the CURRENT guides (tri, n_p, P_p), whichever branch was taken.
 */
#ifndef SQUIGLY_TEMPORAL_H
#define SQUIGLY_TEMPORAL_H
#include <stddef.h>
#include <stdint.h>

#include "squigly_hip.h"      /* sq_camera; nothing of that library is called */
#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    float   alpha_min;     /* 0..1: the least weight of the new frame */
    int32_t max_history;   /* 1..65536: where a pixel's history length stops growing */
    float   sigma_p;       /* >= 0: the plane-distance stop of a tap, world units */
    float   cos_n;         /* the least n_p . n_q of a tap */
} sq_temporal_params;

const char* sq_temporal_last_error(void);
/* Hash of the library's source, headers and flags (build.py: temporal_source_id). */
const char* sq_temporal_build_id(void);

/* Bytes of a history block of a rows x cols image: three 16-byte records per pixel.  0 when rows or cols < 1 or rows * cols >
 * 2^31 - 1.  Monotone in both arguments. */
size_t sq_temporal_history_bytes(int32_t rows, int32_t cols);

/* The contract's projection, on the host and without a device, of the world point `point` into the w rows x h columns image of
 * the camera prev: *fx the column, *fy the row.  Returns 1 if the point projects, 0 if not (fx and fy are then not meaningful),
 * and < 0 when refused: a NULL pointer, w or h < 1. */
int sq_temporal_project(const sq_camera* prev, int32_t w, int32_t h, const float point[3], float* fx, float* fy);

/* One frame of the accumulation: reads the frame's plain images and the previous block, writes the next block and the plain
 * d_out (rows * cols * 3 floats), d_out_var (rows * cols floats) and, when given, d_out_len (rows * cols int32).
 * d_alpha: optional, rows * cols floats.  d_prev: optional; NULL = no history (the first frame), prev_cam is then not read.
 * d_out may be d_color and d_out_var may be d_var.
 * Refused before anything is enqueued: a NULL required pointer (d_color, d_var, d_tri, d_normal, d_point, params, d_next, d_out,
 * d_out_var; prev_cam when d_prev is given); rows or cols < 1 or rows * cols > 2^31 - 1; alpha_min outside [0, 1] or NaN;
 * max_history outside 1..65536; sigma_p NaN or < 0; cos_n NaN; a history block that is not 16-byte aligned; any overlap among the
 * buffers other than the two allowed -- d_prev with d_next included. */
int sq_temporal_accumulate_device(int32_t device, int32_t rows, int32_t cols,
                                  const float* d_color, const float* d_var,
                                  const int32_t* d_tri, const float* d_normal, const float* d_point,
                                  const float* d_alpha /* optional */,
                                  const sq_camera* prev_cam, const void* d_prev /* optional history block */,
                                  const sq_temporal_params* params,
                                  void* d_next /* history block */, float* d_out, float* d_out_var,
                                  int32_t* d_out_len /* optional */, void* hip_stream);

/* A history block as plain images, for tests and checkpoints: every output is optional (NULL), but at least one must be given.
 * Refused: d_hist NULL or misaligned, no output, a bad size, any overlap. */
int sq_temporal_unpack_device(int32_t device, int32_t rows, int32_t cols, const void* d_hist,
                              float* d_color, float* d_var, int32_t* d_len, int32_t* d_tri, float* d_normal, float* d_point,
                              void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif
