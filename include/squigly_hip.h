/* squigly_hip.h — C-ABI of libsquigly_hip.so: the MI355X drop-in for squigly-trace's
 * per-pixel sampling loop.
 *
 * The reference (rrruko/squigly-trace) has no FFI.  Its hot path sits behind
 *     render :: Scene a -> Camera -> Settings -> IO ()            (src/Lib.hs:68-75)
 * and the narrowest seam is src/Lib.hs:73-74,
 *     img = computeAs S (makeArray Par (w :. h) (renderPixel scene cam samples cast dims))
 * i.e. "fill a w-rows x h-columns buffer of Pixel RGB Word8".  sq_render_rgb8() below is
 * what a `foreign import ccall safe` at that line binds (INTEGRATION.md shows the stub).
 *
 * Conventions
 *  - plain C, no exceptions, no ownership transfer.  Every function returns 0 on success,
 *    non-zero on failure; sq_last_error() then holds a message (thread-local).
 *  - all input arrays are caller-owned, read-only, valid for the duration of the call.
 *  - nothing is written to an output buffer on failure.
 *  - there is NO CPU fallback: without a usable HIP device every render entry point fails.
 *  - a call that takes a hip_stream may be given any stream of the scene's device, non-blocking ones (hipStreamNonBlocking) with work
 *    pending on them included: everything the call launches, clears or copies is ordered behind that stream's earlier work and in
 *    front of its later work, and host arguments are read before the call returns (tests/test_gpu_streams.py holds every such call
 *    to that).  A WARM call only enqueues.  A call that needs more room than the scene has -- its first frame or query, a larger
 *    frame (workspace, table of generator words), more views (camera table), the first masked call with second moments -- allocates
 *    on the host, and where it outgrows a block it frees the old one, which waits for the device: such a call still orders all its
 *    work on hip_stream (the clearing of a new workspace included; no call touches the null stream unless that is the stream it was
 *    given), but it may block the host until earlier work, on any stream, is done.  The entry points that can wait say HOST WAIT.
 *  - citations are relative to the reference repository root.
 */
#ifndef SQUIGLY_HIP_H
#define SQUIGLY_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define SQ_ABI_VERSION 1

/* ---- data model (kept from the reference) ---- */
typedef struct { float lo[3], hi[3]; } sq_bounds;            /* Bounds, src/Geometry.hs:153 */

/* One BIH tree node, nodes stored in PRE-ORDER (a branch's left child is the next node).
 * Tree a b / BIHNode, src/BIH.hs:26,37-40.
 *   kind & 3 : 0,1,2 = Branch splitting on X,Y,Z ; 3 = Leaf
 *   branch   : lmax, rmin = BIHN payload ; link = index of the RIGHT child
 *   leaf     : link = index of its first triangle in `tris` (BIH.flatten order, src/BIH.hs:50-52);
 *              kind >> 2 = number of triangles (0 allowed: src/BIH.hs:70-75) */
typedef struct { int32_t kind; float lmax, rmin; int32_t link; } sq_node;

typedef struct { float v0[3], v1[3], v2[3]; int32_t mat; } sq_tri;          /* Triangle, src/Geometry.hs:49-54 (material by index) */
typedef struct { float reflective, surf[3], emissive, emit[3]; } sq_material; /* Material, src/Color.hs:78-83 */
typedef struct { float pos[3]; float rot[9]; } sq_camera;    /* Camera, src/Geometry.hs:41; rot row-major = rotMatrixRads a b g (:90-102) */

typedef struct {
    sq_bounds          root;      /* bounds of BIH, src/BIH.hs:42 */
    const sq_node*     nodes;     int32_t n_nodes;
    const sq_tri*      tris;      int32_t n_tris;    /* leaf order */
    const sq_material* mats;      int32_t n_mats;
    int32_t            height;    /* BIH.height, src/BIH.hs:46-48 (sizes the traversal stack); 0 = compute */
} sq_scene;
/* Every lane keeps `height` stack frames in LDS, 2 bytes each when the scene has < 0x8000 branches and < 0x8000 triangles,
 * else 4.  Largest heights, measured (tests/test_gpu_limits.py), with 2 / 4 byte frames:
 *   per-pixel kernel (variant 1, cast frames *)         320 / 160   (256 lanes x height x word <= 160 KB)
 *   wavefront pipeline, streaming trace form            158 / 79    (512 lanes; 159 / 79 with option "pool" = 0)
 *   streaming six-wave build (3 workgroups per CU)       46 / 23    (taller trees take the plain build)
 *   resident form                                       whatever leaves the scene itself room in 160 KB (data/scene.obj: 13;
 *                                                       14 with option "pool" = 0)
 * (*) with option "cast_wavefront" = 1 a cast frame has the wavefront pipeline's limits.
 * A taller tree is refused on the host before any launch: the render call returns non-zero and sq_last_error() says
 * "BIH height H needs N B of LDS ...". */

/* ---- one-shot drop-in for src/Lib.hs:73-74 ---- */
/* The reference host is one process, so the one-shot calls put a node's GPUs to work themselves: rows are cut
 * into interleaved blocks of 2 rows (the sq_shard scheme below), one host thread per device renders its shard, and
 * the shards are de-interleaved into `out`; no exchange between devices is needed (a pixel depends only on
 * x, y, samples, w).  Devices: all visible ones when the frame has >= 2^24 samples, else device 0; the
 * environment variable SQ_DEVICES="0,1,3" names them explicitly (an index may repeat).
 * out: w*h*3 bytes, row-major, w ROWS x h COLUMNS (massiv `w :. h`, src/Lib.hs:70-71,80), RGB8 =
 * rgbFloatToPixelRGB of each pixel (src/Lib.hs:93-104).  cast != 0 selects raycast (src/Lib.hs:141-151).
 * With one device the finished frame is copied straight into `out`; with several, each shard is staged and de-interleaved.  Either way
 * nothing is written to `out` unless every device's render succeeded.  SQ_ONESHOT_TIMING=1 prints the call's stages (scene
 * upload, buffers, render, copy back, free) on stderr.
 * Size: every device's shard is one sq_render_rows_device call and has that call's limits (below); a frame that is too large for the
 * devices it is spread over is refused before a scene is uploaded ("device D (shard I of G): R x H pixels exceed ..."). */
int sq_render_rgb8(const sq_scene* scene, const sq_camera* cam, int32_t samples, int32_t w, int32_t h,
                   int32_t cast, uint8_t* out);
/* out_avg: w*h*3 floats = the pre-tonemap `avg` of src/Lib.hs:88 (for tolerance checks). */
int sq_render_f32(const sq_scene* scene, const sq_camera* cam, int32_t samples, int32_t w, int32_t h,
                  int32_t cast, float* out_avg);

/* Frame workspaces (15 GB for a 1080p frame at 256 spp, at most 24 GB) are kept, one block per device, when a scene is
 * freed, so that repeated one-shot calls do not re-allocate them (a hipMalloc right after the hipFree of a block
 * that large can wait seconds for the driver to scrub it).  So is the largest table of generator words (option "rng_table_mb"),
 * filled as it is: its entries do not depend on the scene.  This hands them back to the driver. */
void sq_release_cached_memory(void);

/* ---- resident API: scene stays in HBM, output stays on the device (bench, multi-GPU) ---- */
typedef struct sq_device_scene sq_device_scene;
int  sq_scene_upload(const sq_scene* scene, int32_t device, sq_device_scene** out);
void sq_scene_free(sq_device_scene* s);

/* Row sharding (role of massiv's Par scheduler, src/Lib.hs:73): the w image rows are cut into
 * blocks of `row_block` rows and block b belongs to shard (b % n_shards).  A shard renders its rows
 * into a COMPACT buffer of sq_shard_rows() rows, local row j <-> global row sq_shard_global_row(). */
typedef struct { int32_t row_block, shard, n_shards; } sq_shard;
int32_t sq_shard_rows(int32_t w, sq_shard sh);
int32_t sq_shard_global_row(int32_t local_row, sq_shard sh);

/* d_avg (float, rows*h*3) and d_rgb (uint8, rows*h*3) are DEVICE pointers on the scene's device;
 * either may be NULL.  hip_stream is a hipStream_t (NULL = the null stream); the call only enqueues
 * work on it and returns (no synchronisation).
 * FRAME SIZE.  Pixel indices are 32-bit, so one call -- this one, the range, masked and views calls below -- takes at most
 * 2^31 - 1 pixels (rows * h, times n_views), e.g. 46340 x 46340; buffer offsets are 64-bit, so the buffers of such a call may pass
 * 4 GB.  That is the limit of the per-pixel kernel (option "variant" = 1, and cast frames unless option "cast_wavefront" is 1).  The wavefront form (the default)
 * indexes its active pixels and its ray queue with 32-bit numbers that reach three times the pixel count, and takes at most 2^29
 * pixels per call (536 870 912, e.g. 16384 x 32768), which is also the cap of option "slots".  A larger call is refused before the
 * device is touched, every buffer left as it was: "R x H pixels exceed 2^31 - 1 pixels in one call", or "... exceed 2^29 pixels in
 * one call of the wavefront form ...".  Larger images are rendered as several shards (sq_shard): the limit is per call.
 * HOST WAIT (the preamble's last convention): a wavefront call that outgrows the scene's workspace or its table of generator words
 * allocates, and may block the host while the old block is freed; a warm call only enqueues. */
int sq_render_rows_device(sq_device_scene* s, const sq_camera* cam, int32_t samples, int32_t w, int32_t h,
                          int32_t cast, sq_shard sh, float* d_avg, uint8_t* d_rgb, void* hip_stream);

/* Progressive rendering: the samples [k_begin, k_end) of the `samples`-sample frame.  Seeds come from `samples` exactly as in
 * a whole-frame render (src/Lib.hs:85), and a pixel's value is a left fold over its samples in order (src/Lib.hs:88), so a
 * frame rendered in consecutive ranges [0, k1) [k1, k2) ... [kn, samples) is bit for bit the frame of one call.
 *  d_sum : required; a DEVICE buffer of rows*h*3 floats laid out like d_avg.  On entry it holds the per-pixel fold over the
 *          samples [0, k_begin), as an earlier call left it (ignored when k_begin == 0); on return the fold over [0, k_end).
 *          A pixel whose primary ray misses gets +0 sums (the fold of black samples).
 *  d_avg / d_rgb : optional (either or both may be NULL); they receive (1 / (float)k_end) *^ sum and its tonemap.  With
 *          k_end == samples this is bit for bit what sq_render_rows_device writes for the same arguments.
 * Refused with an error code before anything is enqueued (every buffer left as it was): k_begin < 0, k_end <= k_begin,
 * k_end > samples, d_sum == NULL, d_sum == d_avg, and every refusal of sq_render_rows_device (bad shard, the LDS-height
 * limits, ...).  Like sq_render_rows_device the call only enqueues work on hip_stream; the calls of one frame must be
 * ordered by the caller (one stream).  sq_render_rows_device is the case [0, samples) without d_sum.  HOST WAIT: as for
 * sq_render_rows_device. */
int sq_render_rows_device_range(sq_device_scene* s, const sq_camera* cam, int32_t samples, int32_t w, int32_t h,
                                int32_t cast, sq_shard sh, int32_t k_begin, int32_t k_end,
                                float* d_sum, float* d_avg, uint8_t* d_rgb, void* hip_stream);

/* Adaptive sampling, the mechanism: sq_render_rows_device_range for the pixels of a mask only, with the statistics a stopping rule
 * needs.  All buffers are DEVICE buffers laid out like d_avg (rows = sq_shard_rows(w, sh); d_mask, d_count: rows*h entries; d_sum,
 * d_sum2, d_avg: rows*h*3 floats; d_rgb: rows*h*3 bytes).  A pixel p is LIVE in the call iff
 *      (d_mask == NULL || d_mask[p] != 0)  and  (k_begin == 0 || d_count == NULL || d_count[p] == k_begin).
 * The second clause keeps every fold a prefix of the pixel's samples: a pixel that an earlier range left out cannot resume with a
 * gap.  Without d_count the caller answers for that.
 *  live pixel : exactly what sq_render_rows_device_range does (d_sum required, in/out; d_avg / d_rgb optional, (1 / (float)k_end) *^
 *          sum and its tonemap; a primary miss gives +0 sums, avg 0, rgb 0), and in addition
 *          d_sum2  (optional, in/out like d_sum; ignored on entry when k_begin == 0): per channel the left fold q = q + r * r over
 *                  the pixel's sample radiances r in sample order, the product rounded to fp32 before the add; +0 for a miss;
 *          d_count (optional): set to k_end.
 *          The seed of sample k does not depend on the call (src/Lib.hs:85), so a pixel that stops after n samples holds bit for
 *          bit the reference's fold over the first n samples of the `samples`-sample frame.
 *  dead pixel : nothing is written, in any of the five output buffers (the call clears nothing up front), and it costs no ray, no
 *          random number and no slot.  All live pixels advance in lockstep over [k_begin, k_end).
 * With d_mask, d_sum2 and d_count all NULL the call is sq_render_rows_device_range: same bits, same launches.  A call in which no
 * pixel is live is valid, returns 0 and changes no buffer; the call cannot know that without waiting for the device, so it enqueues
 * its (empty) launches all the same and sq_last_plan reports launched = 1.
 * Refused before anything is enqueued (every buffer left as it was): everything sq_render_rows_device_range refuses, and any two
 * of the given buffers overlapping.  Works with every option sq_render_rows_device_range works with; multi-view frames have no
 * masked form.  HOST WAIT: as for sq_render_rows_device, and a wavefront call with d_sum2 that outgrows the scene's second-moment
 * buffer (the first one, a larger frame) allocates it and may block the host likewise. */
int sq_render_rows_device_masked(sq_device_scene* s, const sq_camera* cam, int32_t samples, int32_t w, int32_t h,
                                 int32_t cast, sq_shard sh, int32_t k_begin, int32_t k_end,
                                 const uint8_t* d_mask, float* d_sum, float* d_sum2, int32_t* d_count,
                                 float* d_avg, uint8_t* d_rgb, void* hip_stream);

/* Adaptive sampling, one producer of masks: a stopping rule on the two moments, as a kernel so that every caller gets the same
 * bits.  For every pixel with d_mask[p] != 0, with n = (float)d_count[p] and s_c, q_c the three channels of d_sum, d_sum2, every
 * operation a single fp32 operation in this order:
 *      lhs_c = n * q_c - s_c * s_c            rhs_c = s_c * s_c + eps * (n * n)
 *      L = (lhs_0 + lhs_1) + lhs_2            R = (rhs_0 + rhs_1) + rhs_2
 *      converged  iff  d_count[p] >= 2  and  L <= ((n - 1) * (tol * tol)) * R
 * i.e. the squared standard error of the pixel's mean colour, summed over the channels, is at most tol^2 * (|mean|^2 + 3 * eps).
 * A converged pixel gets d_mask[p] = 0; a NaN anywhere compares false, so such a pixel stays live; *d_live (one int32 on the
 * device) receives the number of pixels still live.  d_sum, d_sum2 and d_count are only read; nothing of the scene is read (s names
 * the device).
 * THE RULE IS A HEURISTIC.  It sees only the samples taken so far: a pixel whose samples were all equal -- on a scene lit by a
 * small emitter a sample is black or bright, so typically all black -- has L = 0 and counts as converged however many bright
 * samples were still to come.  The length of the first range is the caller's guard against that.  The mechanism above is exact
 * whatever mask it is given.
 * Refused: a NULL argument, n_pixels < 0, tol or eps negative or NaN, and n_pixels > 2^32 - 256 (one thread per pixel in one launch;
 * the kernel's own indices are 64-bit, so buffers past 2^31 elements are fine).  The call only enqueues work on hip_stream. */
int sq_adaptive_update_device(sq_device_scene* s, int64_t n_pixels, const float* d_sum, const float* d_sum2,
                              const int32_t* d_count, float tol, float eps,
                              uint8_t* d_mask, int32_t* d_live, void* hip_stream);

/* Many views of one scene in one call: a frame of n_views views is exactly n_views single-view frames.  View i is bit for bit what
 * sq_render_rows_device_range writes for cams[i] with the same other arguments (the seed of sample k of pixel (y, x) is
 * samples * (x + y * w) + k in every view, src/Lib.hs:85), in every kernel form, schedule and option.  All views share one primary
 * pass and one pair of trace launches per sample batch, so the fixed cost of a call (about 1.6 ms) is paid once, not n_views times.
 *  cams  : HOST array of n_views cameras; read during the call only (the caller may reuse it on return).
 *  d_sum, d_avg, d_rgb : DEVICE buffers, view-major [n_views][rows][h][3] with rows = sq_shard_rows(w, sh); block i is byte for byte
 *          what a single-view call writes for cams[i].  [k_begin, k_end) means what it means in sq_render_rows_device_range;
 *          d_sum may be NULL only when [k_begin, k_end) == [0, samples).  d_avg and d_rgb are optional.
 * Refused with an error code before anything is enqueued (every buffer left as it was): n_views < 1, cams == NULL,
 * n_views * rows * h > INT32_MAX (2^29 in the wavefront form: FRAME SIZE above), and every refusal of sq_render_rows_device_range (bad range, d_sum == d_avg, no output buffer,
 * bad shard, the LDS-height limits).  n_views == 1 takes exactly the single-view path.
 * Like the other entry points the call only enqueues work on hip_stream.  The calls on one scene share its workspace and camera
 * table, so they must be ordered on one stream.  HOST WAIT: as for sq_render_rows_device, and a call with more views than the
 * scene's camera table holds allocates a larger table and may block the host while the old one is freed. */
int sq_render_views_device(sq_device_scene* s, const sq_camera* cams, int32_t n_views, int32_t samples, int32_t w, int32_t h,
                           int32_t cast, sq_shard sh, int32_t k_begin, int32_t k_end,
                           float* d_sum, float* d_avg, uint8_t* d_rgb, void* hip_stream);

/* Ray queries on a resident scene: intersectBIH (src/BIH.hs:11,101-141), the `intersect` of Scene (src/Geometry.hs:62-65), of
 * each of n rays.  d_org, d_dir: DEVICE float[n][3] on the scene's device.  Results, per ray:
 *  d_tri   : required; the hit triangle's index in sq_scene.tris (leaf order = BIH.flatten, src/BIH.hs:50-52); -1 = Nothing.
 *  d_dist  : optional; dist = norm (intersectPoint - origin) (src/Geometry.hs:71-75,141).
 *  d_point : optional, float[n][3]; intersectPoint = o + t *^ d (src/Geometry.hs:134).
 * point and dist are the expressions the traversal itself compares, bit for bit the reference's.  A miss writes tri = -1,
 * dist = +inf and point = (+0, +0, +0).  Option "variant" picks the form: 2 (default) queues the rays in the workspace slots and
 * runs one level of the planned trace kernel (options pool, resident, trace_blocks_per_cu, cull, profile, timing and slots act as
 * for frames; a query runs in chunks of at most `slots` rays); 1 = one lane per ray, which takes the taller trees of the per-pixel
 * kernel.  Every form gives the same bits.
 * Refused with an error code before anything is enqueued (every buffer left as it was): s == NULL, n < 0, n > 0 with d_org, d_dir
 * or d_tri NULL, any two of the given ranges overlapping, and the LDS-height limits of a frame of the same form.  Any n that memory
 * holds is taken: ray indices and offsets are 64-bit, variant 1 runs launches of 2^30 rays and the default form chunks of at most
 * `slots` <= 2^29 rays.  n == 0 returns 0
 * and enqueues nothing.  The call only enqueues work on hip_stream; it shares the scene's workspace, so the queries and frames of
 * one scene must be ordered on one stream.  HOST WAIT (the preamble's last convention): a default-form query that outgrows the
 * scene's workspace allocates, and may block the host while the old block is freed. */
int sq_intersect_rays_device(sq_device_scene* s, const float* d_org, const float* d_dir, int64_t n,
                             int32_t* d_tri, float* d_dist, float* d_point, void* hip_stream);
/* The primary ray of every pixel of a shard (makeRay, src/Lib.hs:107-114), computed on the device exactly as the renderer traces it:
 * sq_intersect_rays_device of them gives the renderer's own primary hits.  d_org, d_dir: DEVICE float[rows][h][3], laid out like
 * d_avg, rows = sq_shard_rows(w, sh).  Refused: a NULL argument, w or h < 1, a bad shard, overlapping d_org and d_dir.  No size limit
 * but memory: pixel indices are 64-bit here, and a fixed grid strides over them. */
int sq_camera_rays_device(sq_device_scene* s, const sq_camera* cam, int32_t w, int32_t h, sq_shard sh,
                          float* d_org, float* d_dir, void* hip_stream);

/* Radiance queries on a resident scene: Lib.raytrace (src/Lib.hs:127-137) of caller-given rays with caller-given seed bases.  Per ray
 * i of n, d_sum receives the left fold, in sample order, of
 *      raytrace (mkTFGen (seed_i + k)) scene (Ray org_i dir_i) 0          for k in [k_begin, k_end)
 * started from +0 (k_begin == 0) or from what d_sum holds (k_begin > 0): src/Lib.hs:86-88 with the caller's ray and seed base.
 *  d_org, d_dir : DEVICE float[n][3] on the scene's device, as in sq_intersect_rays_device.
 *  d_seed : DEVICE int64[n], required.  The generator of sample k of ray i is mkTFGen (seed_i + k), the sum taken in two's-complement
 *          64 bits.  With seed_i = samples * (x + y * w) and the ray of sq_camera_rays_device this is sample k of pixel (y, x) of the
 *          `samples`-sample frame.
 *  d_sum  : DEVICE float[n][3], required, in/out exactly like d_sum of sq_render_rows_device_range.
 *  d_avg  : optional, float[n][3]; receives (1 / (float)k_end) *^ sum.
 *  d_rgb  : optional, uint8[n][3]; its tonemap rgbFloatToPixelRGB (src/Lib.hs:93-104).
 * A ray that hits nothing gets +0 sums, avg 0, rgb 0.  With k_begin = 0, k_end = 1 d_sum is 0 + raytrace gen scene ray 0: the plain
 * Lib.raytrace.  Consecutive ranges [0, k1) [k1, k2) ... on the same rays give bit for bit the sum of one call [0, kn).  Every ray is
 * independent of the batch it travels in: permuting the batch permutes the results, and a batch of one equals its entry.
 * Any n that memory holds is taken: the call runs in chunks of rays, each chunk a frame of its own of one row (so within FRAME SIZE:
 * at most `slots` <= 2^29 rays in the wavefront form, 2^30 in variant 1), sample batches inside a chunk as in a frame.  n == 0
 * returns 0 and enqueues nothing.
 * Forms: option "variant" 2 (default) runs the wavefront pipeline -- a primary pass over the caller's rays (64 consecutive rays per
 * wave), then exactly a frame's kernels, the mirror rays once per ray; 1 = one lane per ray in one kernel (the form for the taller
 * trees).  Every option that leaves a frame's bits alone leaves these alone (pool, resident, trace_blocks_per_cu, cull,
 * primary_resident, primary_pooled, overlap, slots, pixel_major, guided, profile, timing), and sq_last_plan reports the call like a
 * frame's (the plan of its last chunk; every chunk plans alike).
 * Refused with an error code before anything is enqueued (every buffer left as it was): s == NULL; n < 0; n > 0 with d_org, d_dir,
 * d_seed or d_sum NULL; k_begin < 0 or k_end <= k_begin; any two of the six ranges overlapping; and the LDS-height limits of a frame
 * of the same form, with the same message.  The call only enqueues work on hip_stream; it shares the scene's workspace, so the
 * queries and frames of one scene must be ordered on one stream.  HOST WAIT: a wavefront query that outgrows the scene's workspace
 * allocates, and may block the host while the old block is freed (queries never grow the table of generator words). */
int sq_raytrace_rays_device(sq_device_scene* s, const float* d_org, const float* d_dir, const int64_t* d_seed, int64_t n,
                            int32_t k_begin, int32_t k_end,
                            float* d_sum, float* d_avg, uint8_t* d_rgb, void* hip_stream);
/* Lib.raycast (src/Lib.hs:141-151) of each of n rays under the scene's lights (sq_scene_set_lights below; the reference's hard-coded
 * light at (0, 3, -1) unless set): d_rad (DEVICE float[n][3], required) receives T of sq_scene_set_lights -- with the reference's
 * light, raycast scene (Ray org_i dir_i) -- and (+0, +0, +0) for a miss; a light that is shadowed at the point adds (+0, +0, +0).
 * No random input and no fold.  One kernel, one lane per ray, in launches of at most 2^30 rays, as cast frames: in "variant" 1, and
 * in "variant" 2 unless option "cast_wavefront" is 1, which runs chunks of at most `slots` rays as a wavefront instead.  Refused like
 * sq_raytrace_rays_device, minus seeds and ranges: s == NULL, n < 0, n > 0 with d_org, d_dir or d_rad NULL, overlapping ranges,
 * and the LDS-height limit of the form that runs (the per-pixel kernel's; with "cast_wavefront" = 1 the wavefront form's, with its
 * message).  HOST WAIT: with "cast_wavefront" = 1, as for sq_raytrace_rays_device; the per-lane form never waits. */
int sq_raycast_rays_device(sq_device_scene* s, const float* d_org, const float* d_dir, int64_t n,
                           float* d_rad, void* hip_stream);

/* Caller-given point lights for the scene's cast computations: sq_render_rows_device, its _range and _masked forms and
 * sq_render_views_device, each with cast != 0, and sq_raycast_rays_device.  (The one-shot calls upload a scene of their own and keep
 * the reference's light.)  Under the lights L_0 ... L_{m-1} the radiance T of a ray is raycast (src/Lib.hs:141-151) with the light
 * made a parameter, every operation a single fp32 operation in this order; `inter` is the ray's intersectBIH, a miss gives
 * (+0, +0, +0) and evaluates no light:
 *      p     = intersectPoint inter
 *      dl_i  = norm (p - pos_i)                                       -- (x*x + y*y) + z*z, sqrt
 *      sh_i  = intersectBIH (Ray p (pos_i - p))                       -- the direction is not normalised
 *      lit_i = not (sh_i is a hit and not (dist sh_i > dl_i))         -- a NaN compares false
 *      c_i   = lit_i ? V3 (power_i.x / dl_i) (power_i.y / dl_i) (power_i.z / dl_i) * surfColor  :  (+0, +0, +0)
 *      T     = c_0;  T = T + c_i  for i = 1 .. m-1                    -- left fold in the caller's order, shadowed terms added too
 * and everything after T is as it was: a frame's fold sum = sum + T per sample of [k_begin, k_end), a masked call's
 * sum2 = sum2 + T * T, avg and the tonemap; a raycast query stores T.  With the single light { (0, 3, -1), (2, 2, 2) } T is bit for
 * bit the reference's value.  Coordinates and powers are not checked (NaN and infinite values are inputs like any other).
 *  lights : HOST array of n_lights lights, read during the call only; the scene keeps a copy for sq_scene_get_lights and enqueues
 *          the update of its device table on hip_stream, so the call is ordered like every other call on the scene (one stream): a
 *          frame enqueued before it keeps the lights it had.
 *  lights == NULL && n_lights == 0 restores the reference's light: a scene on which this function was never called, or which was
 *          reset, launches exactly the kernels it launched before this function existed.
 * Refused with a message, nothing changed: s == NULL, n_lights < 0, n_lights > 4096, n_lights > 0 with lights == NULL,
 * n_lights == 0 with lights != NULL. */
typedef struct { float pos[3]; float power[3]; } sq_light;   /* the reference's light: pos (0, 3, -1), power (2, 2, 2) */
int     sq_scene_set_lights(sq_device_scene* s, const sq_light* lights, int32_t n_lights, void* hip_stream);
/* The scene's lights (one, the reference's, unless set): returns the count and copies min(count, cap) of them to the HOST array
 * out (which may be NULL when cap <= 0); -1 (sq_last_error) for s == NULL. */
int32_t sq_scene_get_lights(sq_device_scene* s, sq_light* out, int32_t cap);

/* Caller-given path depth for the scene's path-traced computations: sq_render_rows_device, its _range and _masked forms and
 * sq_render_views_device, each with cast == 0, and sq_raytrace_rays_device.  (Cast frames and sq_raycast_rays_device ignore it; the
 * one-shot calls upload a scene of their own and keep depth 3.)  A scene has a depth D, 1 <= D <= 8, 3 until set.  Under depth D the
 * radiance of a sample is L(0) of the ray chain below: raytrace (src/Lib.hs:127-137) with `bounces > 2` made `bounces > D - 1`, every
 * operation a single fp32 operation in this order.  inter_b is the intersectBIH of ray b; n_0 ... n_7 are the first eight outputs of
 * the sample's generator mkTFGen seed, the low then high halves of the four words of its one Threefish block:
 *      L(b) = black (+0, +0, +0)                                   if b >= D
 *           = black                                                if inter_b is Nothing
 *           = surfColor_b * L(b+1) + emissive_b *^ emitColor_b     otherwise      -- the product with black IS formed at b = D - 1
 *      ray_{b+1} = bounceRay gen_b ray_b inter_b                    -- src/Lib.hs:155-181: x and u from n_b, v from n_{b+1};
 *                                                                     origin = intersectPoint inter_b
 * and everything after the sample's radiance is as it was: the ordered fold into sum, a masked call's sum2 = sum2 + r * r, counts,
 * avg and the tonemap.  D = 3 is the reference, bit for bit.  D = 1 is direct emission only and traces no bounce ray.  D <= 8 because
 * bounce b reads n_b and n_{b+1} and the last bounce is b = D - 2: no path leaves the generator's first block.  Non-finite and
 * negative materials are inputs like any other (inf * 0 is the NaN the expression says).
 * The depth is host state that the next call's planning reads: the set call enqueues nothing and needs no stream, and a frame enqueued
 * before it keeps the depth it had.  Option "variant" picks the form as for every frame: 2 (default) runs a wavefront around the
 * planned trace kernel, one trace launch per level (frame sizes, tree heights and refusal messages are the wavefront form's, sq_last_plan
 * reports trace_form and primary_form, "overlap" is ignored); 1 = one lane per pixel, one kernel.  At depth 3 both run exactly the
 * kernels and launches they ran before this function existed, unless option "deep" is 1.
 * HOST WAIT: the scene's first wavefront call under a depth other than 3 (or under "deep") allocates the per-slot path state, 4 (D - 1)
 * bytes per slot and 8 more from D = 4 on, and so does a later one that needs more (more slots, a larger depth); it may block the host
 * while the old block is freed.  A failed allocation is an error code before anything is enqueued.  Such calls read the table of
 * generator words the scene has and never grow it.
 * Refused with a message, nothing changed: s == NULL, depth < 1, depth > 8. */
int     sq_scene_set_depth(sq_device_scene* s, int32_t depth);
/* The scene's depth; -1 (sq_last_error) for s == NULL. */
int32_t sq_scene_get_depth(sq_device_scene* s);

/* Caller-given sky for the scene's path-traced computations: the radiance of a ray that leaves the scene.  It applies where the depth
 * applies: sq_render_rows_device, its _range and _masked forms and sq_render_views_device, each with cast == 0, and
 * sq_raytrace_rays_device, at every depth from 1 to 8, in "variant" 2 and 1, every trace form and every primary form.  (Cast frames and
 * sq_raycast_rays_device ignore it; the one-shot calls upload a scene of their own and have no sky.)  Under a sky the radiance of a
 * sample is L(0) of sq_scene_set_depth's chain with one line changed, every operation a single fp32 operation in this order; d_b is
 * the direction of ray b exactly as it was traced (for b = 0 primary_dir of the pixel, or the caller's direction), not normalised
 * beforehand:
 *      L(b) = black (+0, +0, +0)                                   if b >= D
 *           = sky(d_b)                                             if inter_b is Nothing          -- without a sky: black
 *           = surfColor_b * L(b+1) + emissive_b *^ emitColor_b     otherwise
 *      sky(d):  n = sqrt((d.x*d.x + d.y*d.y) + d.z*d.z);  u = d.z / n;  t = 0.5 * u + 0.5
 *               sky_c = down_c + t * (up_c - down_c)               for c = x, y, z
 * up is the radiance seen looking along +z, down along -z; up == down is a constant sky (up_c - down_c is +0, so sky = down for every
 * finite non-zero d).  Values are not checked, as with light powers: NaN, infinite and negative components, d = 0 (t is NaN) and
 * inf - inf are inputs like any other, and the expression's own NaN and inf are the result.  Everything after the sample's radiance is
 * as it was: the ordered fold into sum, a masked call's sum2 = sum2 + r * r, counts, avg and the tonemap.
 * A pixel or query ray whose ray 0 misses no longer gets the constant black: its fold adds sky(d_0) once for each k of
 * [k_begin, k_end), k_end - k_begin single additions from where the pixel's fold starts (not one multiplication), and it gets sum2,
 * count, avg and the tonemapped RGB like any other pixel.  A dead pixel of a masked call is still written nowhere.
 * The sky is host state that the next call's planning reads, like the depth: the set call enqueues nothing and takes no stream, and a
 * frame enqueued before it keeps the sky it had.  Under a sky a call runs the generic-depth kernels at every depth, D = 3 included,
 * whatever option "deep" says, without the absorbing-surface shortcut and the last ray's emitter pre-test (neither is an identity
 * under a sky), and sq_last_plan reports as for a deep call.  A wavefront call under a sky keeps 4 more bytes per slot of path state
 * than sq_scene_set_depth names (t of the ray that missed; D >= 2), allocated as described there (HOST WAIT).
 *  sky == NULL: no sky (the reference).  A scene that was never given a sky, or was reset with NULL, launches exactly the kernels and
 *          launches it launched before this function existed.  A sky of all +0 is a sky, not the unset state: it differs from black on
 *          a ray with d = 0.
 * Refused with a message, nothing changed: s == NULL. */
typedef struct { float up[3]; float down[3]; } sq_sky;     /* radiance seen looking along +z / along -z */
int     sq_scene_set_sky(sq_device_scene* s, const sq_sky* sky);
/* 1 = a sky is set (copied to out, which may be NULL), 0 = none (out untouched), -1 (sq_last_error) for s == NULL. */
int     sq_scene_get_sky(sq_device_scene* s, sq_sky* out);

/* Timing of the dominant kernel measured with hipEvents on the stream it was launched on:
 * average duration in ms over the launches since the last reset, and the launch count. */
int  sq_kernel_timing(sq_device_scene* s, double* avg_ms, int64_t* launches, const char** kernel_name);
void sq_kernel_timing_reset(sq_device_scene* s);
/* Cumulative statistics of the trace kernel, over the render and query calls since the last reset (synchronises the device), n <= 32:
 * out[0] = rays traced; out[1..23] = lane-occupancy counters, rare-path counts and per-section wave cycles of the
 * profile build, filled only with option "profile" = 1 (tools/gpu_pool.py prints them); out[28] = first-bounce rays that
 * level-1 culling (option "level1_cull") did not queue by its conditions (1)-(3); out[29] = those that only its condition (4) kept off
 * the queue (no point of the ray from which the second bounce could reach an emitter lies in the cover of the geometry); out[30] =
 * those that only its condition (5) kept off the queue (the ray may end on a mirror, but behind no mirror does it reach the image of
 * the emitters), so the rays dropped are out[28] + out[29] + out[30]. */
int  sq_get_stats(sq_device_scene* s, uint64_t* out, int32_t n, int32_t reset);
/* Tunables; every setting produces identical bits.  Keys:
 *   "variant"            1 = one-lane-per-pixel kernel, 2 = wavefront pipeline (default)
 *   "slots"              sample slots of the frame workspace (default 512 Mi at 37 B each = 20 GB of the
 *                        288 GB; a frame with fewer samples allocates only what it needs), 1 .. 2^29: slot numbers and the
 *                        trace kernel's queue cursor are 32-bit
 *   "resident"           1 = keep the whole scene in LDS when it fits (default), 0 = always stream
 *   "lds_node_kb"        streaming form: KB of LDS for the top of the tree (default 32; the six-wave build takes what its third of the LDS leaves)
 *   "pool"               1 = pooled trace kernel (default): a wave tests the triangles of all its open leaves as a pool of
 *                        (ray, triangle) pairs spread over its 64 lanes; 0 = every lane walks its own leaf
 *   "refill_min"         pooled kernel: idle lanes a wave collects before it fetches new rays (default 12)
 *   "flush_min"          pooled kernel: a trailing part-filled window of pairs runs at once from this many pairs on,
 *                        otherwise it waits one iteration for more (default 40)
 *   "pixel_major"        order in which a trace launch takes its queue: 0 = slot order (neighbouring pixels, one sample each),
 *                        1 = all samples of a pixel in a row (a wave's rays start at one surface point), -1 = choose (default:
 *                        1 when the triangles exceed the 4 MB L2s, else 0)
 *   "primary_resident"   1 = with a resident scene the primary rays are traced out of LDS too (default), 0 = from L2
 *   "primary_pooled"     1 = the primary rays go through the pooled trace kernel (one slot per pixel, one launch) instead of the
 *                        one-ray-per-lane pass: one rank's share of the headline frame at 8 ranks 8.20 -> 8.12 ms, the whole
 *                        frame 54.2 -> 54.4 ms; default 0
 *   "guided"             bit 0 (default 1): queue reservations of the first-bounce launches shrink towards the end of the queue, so that a
 *                        launch does not end with a few waves still working through a full reservation; bit 1: the same for the
 *                        second-bounce launches -- off by default since round 3: their queue is 8 % live, a shrunken reservation brings
 *                        a handful of rays for the same atomic and scan round trip, and every such launch took 0.34 ms longer with it
 *                        (one rank's share at 8 ranks: 1166 -> 825 us; whole frame: 4886 -> 4542 us); 0 = fixed size everywhere
 *   "straggler_lanes"    pool = 0: lanes still traversing when a wave turns to its leaves (default 8)
 *   "trace_blocks_per_cu" streaming form: 512-thread workgroups per CU.  0 (default) = three, with the kernel compiled for six waves per
 *                        SIMD (80 VGPRs), when a workgroup's stacks plus at least 4 KB of the tree's top fit in a third of the LDS, else
 *                        two with the plain build (86 VGPRs, up to lds_node_kb of tree); 1 / 2 = the plain build; 3 = the six-wave build if it fits
 *   "timing"             1 = bracket the dominant kernel with hipEvents for sq_kernel_timing (default 0)
 *   "profile"            1 = lane-occupancy counters in sq_get_stats (slower)
 *   "overlap"            0 = one stream (default; per-kernel durations stay clean for the roofline)
 *                        1 = two sample batches in flight: trace launches on the caller's stream, the per-sample
 *                            kernels beside them on an internal stream
 *                        2 = two pipelines: even and odd sample batches run start to end on two streams, so that one
 *                            track's launches fill the other's ramp-downs (1 and 2: -3 % on the whole headline frame, nothing on
 *                            half a frame or less, so both stay opt-in)
 *   "aux_blocks_per_cu"  workgroups per CU of the per-sample kernels (0 = default 8)
 *   "coresidency"        diagnostic, default 0: the trace kernel keeps a gauge of its live workgroups and every wave of the per-sample
 *                        kernels (RNG + bounce, shading) records whether it started / ended while (CUs - 8) or more of them were live,
 *                        i.e. beside a resident trace workgroup on its own CU; sq_get_stats slots 24..27 = gauge, per-sample waves,
 *                        started beside, ended beside (tools/gpu_overlap.py prints them per schedule)
 *   "descend_extra"      pooled trace kernel: further branch steps (default 2) a lane that keeps descending takes within one iteration,
 *   "descend_lanes"      each taken only while at least this many lanes (default 16) of the wave want one
 *   "cull"               1 (default): a ray inside the limits of sq_cull_boxes (squigly_host.h) that misses a leaf's culling box
 *                        skips the leaf's triangle tests -- the reference's mollerTrumbore would reject them all, so no bit
 *                        changes; 0: every leaf the reference visits is tested
 *   "level1_cull"        1 (default): a path-traced frame or query at depth 3 does not queue the scattered first-bounce ray of a
 *                        sample that provably ends with the radiance of a first-bounce miss (no emitter on the ray, no mirroring
 *                        surface on it, no emitter within reach of the second bounce: csrc/sq_pack_level1.h, build_level1) -- no bit
 *                        changes; 0: every such ray is traced.  sq_get_stats slots 28 to 30 count the rays dropped, sq_last_plan says
 *                        whether the frame used it
 *   "primary_tiles"      1 (default): the primary rays of a shard are enumerated in tiles (8 x 8 pixels on a whole image, 2 x 32 with
 *                        row blocks of 2) so that the 64 rays of a wave stay together in both image directions; 0: 64 pixels of a row
 *   "rng_table_mb"       budget in MiB of the scene's table of generator words (default 24576 = 24 GiB of the 288 GB, 0 = no table).  A
 *                        sample's three random words are tfgen3(seed), seed = samples * (x + y * w) + k: they depend on nothing but the
 *                        seed, so a resident scene keeps them, 12 bytes per seed, for the seeds [0, n_cover), n_cover =
 *                        sq_rng_table_cover(w, h, samples, budget) (squigly_host.h) of the largest frame it has rendered, and the
 *                        RNG + bounce kernel reads them instead of running Threefish-256 for every sample of every frame; a pixel
 *                        whose seeds are not all below n_cover computes them as before.  The table is allocated and filled by the
 *                        first wavefront frame that can use more seeds than it holds (the 1920 x 1080 frame at 256 spp: 943 M seeds =
 *                        11.3 GB; at 512 spp 22.6 GB; 3840 x 2160 at 1024 spp would take 181 GB and gets the first 24 GiB), always
 *                        behind the frame workspace, and a failed allocation only means no table.  Radiance queries read the table
 *                        the scene has and never grow it; the one-shot calls and the one-lane-per-pixel kernels build and read none
 *   "cast_wavefront"     0 (default): cast frames and raycast queries run one lane per ray in one kernel; 1 (with "variant" 2): they run
 *                        as a wavefront -- the frame's own primary pass, then per batch of lights (as many as the slots hold, at least
 *                        one) one shadow ray per (active pixel, light) through one level of the planned trace kernel and an ordered
 *                        fold; frame sizes, tree heights and refusal messages are then the wavefront form's, sq_last_plan reports the
 *                        planned trace_form and primary_form, and "overlap" is ignored
 *   "deep"               0 (default): a scene at depth 3 (sq_scene_set_depth) runs the three-level kernels, every other depth the
 *                        generic-depth ones; 1: depth 3 runs the generic-depth kernels too -- same bits, so that the generic pipeline
 *                        can be held to the reference and timed against the tuned one
 *   "incremental"        accepted, no effect: the variant it switched was removed (last built by commit 4abd717) */
int  sq_set_option(sq_device_scene* s, const char* key, int64_t value);

/* The scene's table of generator words (option "rng_table_mb"; tests and diagnostics): copies the entries [first, first + count) --
 * three uint32 per seed, tfgen3(seed) -- to the HOST array out_words and returns the number of seeds the table holds; count = 0
 * only asks for that number (0 = the scene has no table).  Returns -1 (sq_last_error) when the range is not inside the table.
 * Waits for the table's fill, not for the device. */
int64_t sq_scene_rng_table(sq_device_scene* s, int64_t first, int64_t count, uint32_t* out_words);

/* The launch plan of the scene's last render or query call (read only; diagnostics and tests): which kernel forms it
 * chose and the sizes they were chosen by.  Filled as the call plans the frame or query, so after a refused call (an error code
 * such as "BIH height ... needs ... LDS") it holds what was planned up to the refusal and launched = 0; a call is planned before it
 * touches the device, so a refused call has allocated, freed and cleared nothing (squigly_host.h: sq_plan_call plans without a GPU).  A query
 * (sq_intersect_rays_device) has primary_form SQ_PRIMARY_NONE.  Returns non-zero when the scene has not planned a call yet. */
enum { SQ_FORM_PER_PIXEL = 0, SQ_FORM_RESIDENT = 1, SQ_FORM_STREAMING_SIX_WAVE = 2, SQ_FORM_STREAMING_PLAIN = 3 };
enum { SQ_PRIMARY_NONE = 0, SQ_PRIMARY_PER_LANE = 1, SQ_PRIMARY_RESIDENT = 2, SQ_PRIMARY_POOLED = 3 };
typedef struct {
    int32_t launched;          /* 1 = the frame was enqueued, 0 = refused while planning */
    int32_t variant;           /* option "variant" (a cast frame runs the per-pixel kernel, trace_form 0, unless "cast_wavefront" is 1) */
    int32_t stack_word_bytes;  /* 2 (uint16_t frames: < 0x8000 branches and triangles) or 4 */
    int32_t height;            /* BIH height */
    int32_t stack_cap;         /* frames per lane */
    int32_t trace_form;        /* SQ_FORM_*; SQ_FORM_PER_PIXEL for variant 1 and for cast frames without "cast_wavefront" */
    int32_t blocks_per_cu;     /* trace workgroups per CU (0 with the per-pixel kernel) */
    int32_t n_lds;             /* streaming forms: branches of the tree's top kept in LDS; resident: all branches */
    int32_t trace_lds_bytes;   /* dynamic LDS of one trace workgroup (0 with the per-pixel kernel) */
    int32_t pixel_lds_bytes;   /* dynamic LDS of one 256-thread workgroup of the per-pixel kernel / per-lane primary rays */
    int32_t primary_form;      /* SQ_PRIMARY_*: how the primary rays of a wavefront frame were traced (NONE with the per-pixel kernel) */
    int32_t packed_leaves;     /* streaming forms: leaf references carry count << 24 | first (every leaf <= 31 triangles) */
    int32_t n_emitters;        /* length of the last-bounce emitter list, -1 = shortcut off (> 64 emitters, non-finite materials, or a call under a sky) */
    int32_t level1_cull;       /* 1 = the frame's first-bounce rays went through level-1 culling (option "level1_cull" and the scene's preconditions) */
} sq_plan;
int  sq_last_plan(sq_device_scene* s, sq_plan* out);

/* Diagnostics for the numeric spec (tests only): evaluate one primitive on the device for n inputs.
 *   SQ_OP_SQRT/SIN/COS/ACOS/ATAN : a = n floats -> out = n floats        (b unused)
 *   SQ_OP_DIV                    : a, b = n floats -> out = a/b
 *   SQ_OP_UNIT_FLOAT             : a = n uint32 -> out = n floats (randomR (0,1), src/Lib.hs:183-188)
 *   SQ_OP_TFGEN3                 : a = n int64 seeds -> out = 3n uint32 (first three outputs of mkTFGen seed)
 *   SQ_OP_TONEMAP                : a = 3n floats -> out = 3n bytes (src/Lib.hs:93-104)
 *   SQ_OP_RCP_SWEEP              : a = n uint32 (upper 16 bits of a float) -> out = n uint32: among the 65536 floats x with
 *                                  those upper bits, how many have the triangle test's short reciprocal != 1.0f / x
 *   SQ_OP_CULL_SLAB              : a = 9n words (a culling box as three packed binary16 pairs lo | hi << 16 for x, y, z; ray
 *                                  origin; ray direction) -> out = n uint32: 1 if the ray passes the kernels' culling slab test
 * a, b, out are HOST pointers. */
enum { SQ_OP_SQRT = 0, SQ_OP_DIV = 1, SQ_OP_SIN = 2, SQ_OP_COS = 3, SQ_OP_ACOS = 4, SQ_OP_ATAN = 5,
       SQ_OP_UNIT_FLOAT = 6, SQ_OP_TFGEN3 = 7, SQ_OP_TONEMAP = 8, SQ_OP_RCP_SWEEP = 9, SQ_OP_CULL_SLAB = 10 };
int sq_debug_eval(int32_t device, int32_t op, const void* a, const void* b, int64_t n, void* out);

int32_t     sq_device_count(void);
int32_t     sq_abi_version(void);
/* Identity of this build: the first 16 hex digits of a SHA-256 over the library's sources, the C headers and the compiler
 * flags (squigly-trace_amd/build.py: source_id).  Profile files under profiles/ are stamped with it, and bench.py refuses to
 * price a roofline with counters that were collected on a different build ("unknown" = built without build.py). */
const char* sq_build_id(void);
const char* sq_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
