/* squigly_temporal.h — C-ABI of libsquigly_temporal.so: temporal accumulation of the frames libsquigly_hip.so leaves on the device
 * under a camera that moves from frame to frame.  It is the temporal third of an SVGF-style pipeline whose
 * variance estimate and a-trous filter are libsquigly_denoise.so's.
 *
 * The library knows nothing of scenes, trees or generators: it maps device images to device images.  Its inputs are what the other
 * libraries' calls leave behind: the frame's mean colour, the variance of sq_denoise_variance_device, and d_tri, d_point and the
 * unit normal of the first hit (DeviceScene.guides).  sq_temporal_accumulate_device takes the geometry as static: the world-space
 * points of two frames are compared directly.  sq_temporal_accumulate_moving_device (below) takes rigid objects that move between
 * two frames: a pixel's point and normal go back through its object's transform first, and a clamp to the neighbourhood's colours
 * answers the light that a moving object changes on surfaces that did not move.
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
 * Out of scope: shards and more than one GPU; lens, shutter and adaptive frames as the per-frame renderer; cast frames; deforming
 * meshes and per-vertex motion (objects are rigid); moving lights and a sky that changes; a history length that shortens where the
 * clamp bites; the C++ command line.
 *
 * The history block is opaque to callers: sq_temporal_history_bytes(rows, cols) bytes, 16-byte aligned, three planes of 16-byte
 * records, a record per pixel in each (colour.rgb + variance; normal.xyz + length; point.xyz + triangle), so that a bilinear tap
 * is three 16-byte loads and a wave's loads of one plane are contiguous.  Only the two accumulate calls write one, and a block
 * that neither wrote is not a history (its lengths are taken as they are).  Callers go to and fro between two blocks.
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
 *
 * The moving call's contract is the one above with these additions, each operation again one fp32 operation in this order.
 *   Objects (d_object with n_tris, d_back with n_objects; both or neither).  d_object[t] is the rigid object of triangle t of the
 *   CURRENT scene (an index < 0: static); d_back holds 12 floats an object, the row-major 3 x 4 B = [L | t] that takes a world point
 *   of the current frame to where the same surface point was in the previous frame.  For a pixel with tri >= 0, when d_prev is given:
 *       o = (tri < n_tris) ? d_object[tri] : -1
 *       if 0 <= o < n_objects:  P'_i = ((L_i0 * P.x + L_i1 * P.y) + L_i2 * P.z) + t_i;  n'_i = (L_i0 * n.x + L_i1 * n.y) + L_i2 * n.z
 *       otherwise P' = P_p and n' = n_p, bit for bit.
 *   n' is not renormalised.  P' and n' take the place of P_p and n_p in the projection, in dn, in d = P_q - P' and in pd.  The next
 *   block still holds the current guides.  An index outside its table is never read through: a wrong index is data, not a fault.
 *   Clamp (clamp = { radius, k }; NULL = off).  The window is the taps q = (y + j, x + i), j = -radius .. radius (outer),
 *   i = -radius .. radius (inner); only taps inside the image with tri[q] >= 0 count.  Per channel of the CURRENT d_color, the sums
 *   from +0 and n counted in fp32 (n = n + 1):
 *       s = s + C_q;  s2 = s2 + C_q * C_q
 *       mu = s / n;  vr = s2 / n - mu * mu;  vr = 0 unless vr > 0;  sd = sqrtf(vr);  ks = k * sd;  lo = mu - ks;  hi = mu + ks
 *   and after hc = sc / sw, before the blend, per channel:  if (hc < lo) hc = lo;  if (hc > hi) hc = hi  (a NaN compares false and
 *   leaves hc alone).  hv, a and len stay as they are.  The window is read only where history is blended.
 *   Flags (d_out_flags): bit 0 history was blended; bit 1 some channel was clamped; bit 2 the pixel went back through an object
 *   (d_prev given, tri >= 0, 0 <= o < n_objects -- whether or not it then found history).
 *   With d_object, d_back, clamp and d_out_flags all NULL the call writes the bytes of sq_temporal_accumulate_device, the next
 *   block included.
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

typedef struct {
    int32_t radius;   /* 1..3: the window is (2 radius + 1)^2 taps */
    float   k;        /* >= 0: the bounds are mu -/+ k standard deviations; +inf clamps nothing where sd > 0 */
} sq_temporal_clamp;

/* Kernel forms of the clamp's window (form).  Every form gives the same bits. */
#define SQ_TEMPORAL_FORM_AUTO   0   /* the library's choice */
#define SQ_TEMPORAL_FORM_DIRECT 1   /* every tap of the window is read from d_color and d_tri (L1 / L2) */
#define SQ_TEMPORAL_FORM_TILED  2   /* the tile and its halo of `radius` pixels are staged in LDS once */
#define SQ_TEMPORAL_N_FORMS     2

#define SQ_TEMPORAL_FLAG_BLENDED 1
#define SQ_TEMPORAL_FLAG_CLAMPED 2
#define SQ_TEMPORAL_FLAG_MOVED   4

/* sq_temporal_accumulate_device under geometry that moves (the contract's additions above): d_object (n_tris int32) and d_back
 * (n_objects * 12 floats) go together, clamp and d_out_flags (rows * cols bytes) are optional; form is read under a clamp only.
 * Refused before anything is enqueued: everything sq_temporal_accumulate_device refuses; n_tris or n_objects < 0; one of d_object
 * and d_back without the other; a table pointer with a count of 0; clamp.radius outside 1..3, clamp.k NaN or < 0; form outside
 * 0..2; any overlap that involves d_object, d_back or d_out_flags; and, under a clamp, d_out == d_color (neighbours are read;
 * d_out_var == d_var stays allowed). */
int sq_temporal_accumulate_moving_device(int32_t device, int32_t rows, int32_t cols,
                                         const float* d_color, const float* d_var,
                                         const int32_t* d_tri, const float* d_normal, const float* d_point,
                                         const float* d_alpha /* optional */,
                                         const sq_camera* prev_cam, const void* d_prev /* optional history block */,
                                         const sq_temporal_params* params,
                                         const int32_t* d_object /* optional */, int32_t n_tris,
                                         const float* d_back /* optional */, int32_t n_objects,
                                         const sq_temporal_clamp* clamp /* optional */, int32_t form,
                                         void* d_next /* history block */, float* d_out, float* d_out_var,
                                         int32_t* d_out_len /* optional */, uint8_t* d_out_flags /* optional */, void* hip_stream);

/* A history block as plain images, for tests and checkpoints: every output is optional (NULL), but at least one must be given.
 * Refused: d_hist NULL or misaligned, no output, a bad size, any overlap. */
int sq_temporal_unpack_device(int32_t device, int32_t rows, int32_t cols, const void* d_hist,
                              float* d_color, float* d_var, int32_t* d_len, int32_t* d_tri, float* d_normal, float* d_point,
                              void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif
