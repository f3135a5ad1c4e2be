/* squigly_host.h — host side ABOVE the render boundary, as a C-ABI.
 *
 * In the reference these are Haskell functions (src/Obj.hs, src/BIH.hs, src/Geometry.hs) that a
 * Haskell host would keep calling unchanged.  No GHC exists in the build or GPU images, so the
 * same functions are provided in C++ (squigly-trace_amd/csrc/sq_host.cpp) with identical
 * arithmetic, and produce exactly the arrays that squigly_hip.h consumes.
 * Also here, with no counterpart in the reference: the culling boxes, a window on the scene packer, the host half of
 * sq_scene_upload(), so that what the kernels will read can be inspected on a machine without a GPU, and a window on the call
 * planner, the host half of every render and query call.
 * All citations are relative to the reference repository root.
 */
#ifndef SQUIGLY_HOST_H
#define SQUIGLY_HOST_H
#include "squigly_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* A loaded triangle soup in loader order (Obj.trisFromObj, src/Obj.hs:49-58). */
typedef struct sq_mesh sq_mesh;
int  sq_mesh_from_obj(const char* obj_path, const char* mtl_dir, sq_mesh** out);   /* mtl_dir plays "./data/" of src/Obj.hs:52 */
int  sq_mesh_from_text(const char* obj_text, size_t obj_len, const char* sq_text, size_t sq_len, sq_mesh** out);
int  sq_mesh_from_arrays(const sq_tri* tris, int32_t n_tris, const sq_material* mats, int32_t n_mats, sq_mesh** out);
int32_t sq_mesh_num_tris(const sq_mesh* m);
int32_t sq_mesh_num_materials(const sq_mesh* m);
const sq_tri*      sq_mesh_tris(const sq_mesh* m);
const sq_material* sq_mesh_materials(const sq_mesh* m);
void sq_mesh_free(sq_mesh* m);
/* What `--debug` prints while loading (src/Obj.hs:55-57): `print (head objs)` and `print mats`, in the text of Haskell's
 * derived Show instances (records, lists, `show :: Float -> String`).  The strings belong to the mesh; both are empty
 * for a mesh that did not come from .obj/.sq text, and *first_object is empty when the file has no object (the reference's
 * `head objs` throws there: the CLIs print "Prelude.head: empty list" and exit 1).  Names are escaped per GHC's showLitChar on
 * the UTF-8 decoded text (control characters by name, \DEL, \SO\&H, code points > 127 in decimal with \& before a digit). */
void sq_mesh_debug_show(const sq_mesh* m, const char** first_object, const char** materials);

/* Obj.loadCamera (src/Obj.hs:60-70): "px py pz\nalpha beta gamma" -> position + rotMatrixRads. */
int  sq_camera_from_file(const char* path, sq_camera* cam);
int  sq_camera_from_text(const char* text, size_t len, sq_camera* cam);
void sq_rot_matrix_rads(float alpha, float beta, float gamma, float out9[9]);     /* src/Geometry.hs:90-102 */

/* BIH.makeBIH (src/BIH.hs:62-99) + flatten (:50-52) into the pre-order arrays of squigly_hip.h.
 * The returned object owns the arrays; sq_bih_scene() fills an sq_scene that points into it. */
typedef struct sq_bih sq_bih;
int  sq_bih_build(const sq_mesh* mesh, sq_bih** out);
/* The same build on HIP device `device` (squigly-trace_amd/csrc/sq_bih_device.hip): level-synchronous,
 * element-parallel, and bit-identical to sq_bih_build -- same split planes (ordered fp32 sums), same stable
 * partitions, same boxes -- because tree shape and leaf order decide traversal tie-breaks.  Fails (non-zero,
 * sq_last_error) without a GPU or when a vertex coordinate is not finite; it never falls back to the host. */
int  sq_bih_build_device(const sq_mesh* mesh, int32_t device, sq_bih** out);
void sq_bih_scene(const sq_bih* b, sq_scene* out);
int32_t sq_bih_height(const sq_bih* b);        /* BIH.height       src/BIH.hs:46-48 */
int32_t sq_bih_num_leaves(const sq_bih* b);    /* BIH.numLeaves    src/BIH.hs:54-56 */
int32_t sq_bih_longest_leaf(const sq_bih* b);  /* BIH.longestLeaf  src/BIH.hs:58-60 */
void sq_bih_free(sq_bih* b);

/* Culling boxes (no counterpart in the reference; an exact reduction of its triangle tests).  boxes: 6 floats per node
 * of scene->nodes (lo.xyz, hi.xyz; a branch gets the union of its children).  A ray with ray_limits[1] <= |d|^2 <=
 * ray_limits[2], |o|^2 <= ray_limits[0] and finite o, d, 1/d, o/d that FAILS the fp32 slab test of a node's box is
 * rejected by the reference's mollerTrumbore (src/Geometry.hs:117-142) for every triangle of that node, so the node
 * returns Nothing (src/BIH.hs:105-109) without testing them.  The error analysis is in csrc/sq_cull_lemma.h; leaves it does
 * not cover get an infinite box, and ray_limits[0] < 0 says no ray may be culled.  The scene packer below calls this. */
int  sq_cull_boxes(const sq_scene* scene, float* boxes, float ray_limits[3]);
/* The binary16 encoding the resident kernels keep such a box in: the nearest value >= x (up != 0) or <= x, never subnormal. */
uint32_t sq_half_outward(float x, int32_t up);

/* The scene packer: everything sq_scene_upload() computes from a scene before it touches a device -- validation, the
 * breadth-first branch table, triangle / surface / material records, the 16-bit indexed and resident encodings, the culling
 * tables, the merged branch records, the emitter list and the flags that choose a kernel form.  sq_scene_upload() copies exactly
 * these arrays to the device.  Needs no GPU.  Arrays go by the name of the SceneView member they feed (csrc/sq_scene.h):
 * branches, leaves, tris, tri_mat, surfs, mats, verts4, trix, rbranch, emitters, cull_child, cull_child16, branches_m; `data`
 * points into the packed scene and lives as long as it.  Scalars: n_branches, n_leaves, height, root_ref, rroot, packed_leaves,
 * nonneg_materials, finite_geometry, n_emitters, n_verts, small_index, shortcut_depth (the largest path depth at which
 * nonneg_materials still holds; 0: none), and cull_o2max / cull_d2min / cull_d2max as the bits of the float.  The first-bounce
 * reduction (option "level1_cull"): array "level1" is the Level1Cull record sq_gen_bounce1 takes (csrc/sq_layout.h), scalars
 * level1_on (its preconditions hold) and level1_zero (s.surf * 0 + s.emit is bitwise +0 outside the emitter list); array
 * "level1_cover" is the Level1Cover record behind SceneView::rtail (one record where level1_on, else empty): at most 8 boxes that
 * hold the end point of every accepted first-bounce ray; array "level1_mirror" is the Level1Mirror record that follows it on the device
 * (one record wherever "level1_cover" has one): the mirror panels with their boxes and the images of the emitters' box, the rest boxes,
 * the smallest `reflective` per cover box and the determinant floor of condition (5); n_panels = 0 where that condition is off.  An
 * unknown name returns non-zero. */
typedef struct sq_packed sq_packed;
int   sq_scene_pack(const sq_scene* scene, sq_packed** out);
int   sq_packed_array(const sq_packed* p, const char* name, const void** data, size_t* bytes);
int   sq_packed_scalar(const sq_packed* p, const char* name, int64_t* value);
void  sq_packed_free(sq_packed* p);

/* The call planner: everything a render or query call decides before it touches the device -- kernel forms, LDS carve-up, slots,
 * batches, grids, reservation sizes, the workspace layout and every refusal -- from a few numbers.  Needs no GPU; the device code
 * plans by the same functions (csrc/sq_plan.h).  Inputs go by name and value:
 *   options    the names of sq_set_option, with its ranges and refusals (default: the option's default);
 *   scene      the names of sq_packed_scalar: n_branches, n_verts, height, small_index, packed_leaves, n_emitters, nonneg_materials,
 *              finite_geometry, shortcut_depth, level1_on; and n_tris (sq_scene.n_tris), trix (the packed array "trix" is not empty);
 *   device     n_cu, the compute units;
 *   state      depth (sq_scene_set_depth), sky (1: a sky is set), lights_set (1: sq_scene_set_lights gave lights), n_lights;
 *   the call   source (0 camera, 1 views, 2 caller-given rays), cast, masked (a mask, second moments or counts are given), mom2 (second
 *              moments are), n_views, local_rows, h, tile_rows, tiles_x (the tiling of the primary rays: 8 rows x 8 columns on a whole
 *              image, 1 x 64 with option primary_tiles 0 and for rays), k_begin, k_end; a chunk of a radiance query is a frame of one
 *              row, h = the chunk's rays, and total_rays = the query's rays asks for chunk_rays, the rays per chunk;
 *              query = 1 with n_rays: an intersection query.
 * have_slots: the sample slots the workspace holds (the allocation may have halved the plan's `slots`); 0 = what the plan wants.
 * Outputs: *plan as sq_last_plan would give it, and the named scalars of the plan and of its schedule for have_slots:
 *   path (0 per-lane cast with lights, 1 per-lane deep, 2 per-lane plain, 3 wavefront cast, 4 wavefront deep, 5 three-level pipeline,
 *   6 per-lane query, 7 wavefront query), ad, mom2, sky, deep, nonneg_materials, n_emitters, cull_off, pixels, px_blocks, px_lds, n_call,
 *   slots, trace_form, resident, pool, profile, dense, n_lds, stack_cap, trace_blocks, trace_threads, tr_lds, primary_grid, primary_lds,
 *   aux_blocks, acc_grouped, level1_cull, deep_slot_bytes, need_lights, need_sum2, need_deep, rng_table, rng_grow, chunk_rays;
 *   have_slots, overlap, tracks, track_slots, batch, n_batches, n_real, query_chunk, tail_kc (the samples of the last batch);
 *   pp_grid_x, pp_grid_y (per-sample kernels of a full batch), tail_pp_grid_x, tail_pp_grid_y; chunk_0, chunk_1, guide_shift_0,
 *   guide_shift_1, pixel_major (a full batch's trace launches at bounce level 0 and 1), tail_chunk, lone_chunk (a launch of one ray per pixel);
 *   ws_cnt ... ws_carry, ws_total (byte offsets of the workspace's arrays, in order: cnt, stats, pix, t0, tri0, sum, mt, mtri, state, org,
 *   dir, tri1, carry) and deep_oxy, deep_trail, deep_tmiss (of the deep block; -1: none).
 * Returns 0; 1 when the planner refuses the call (sq_last_error has the call's own refusal, *plan what was planned up to it with
 * launched = 0, the scalars are 0); 2 for an unknown name or a value no call could have. */
int sq_plan_call(const char* const* in_names, const int64_t* in_values, int32_t n_in, int64_t have_slots,
                 sq_plan* plan, const char* const* out_names, int64_t* out_values, int32_t n_out);

/* The table of generator words of a resident scene (squigly_hip.h, option "rng_table_mb"): how many seeds [0, n_cover) it holds
 * for a frame of w rows x h columns at `samples` samples under a budget of budget_bytes.  The frame's seeds are
 * samples * (x + y * w) + k (src/Lib.hs:85-86), so it can use samples * ((w - 1) * w + h) of them -- w * h * samples for a square
 * frame, more when the frame has more rows than columns, fewer when it has more columns than rows -- and the table holds
 * budget_bytes / 12 at most: n_cover is the smaller of the two, 0 for a budget below one entry or a non-positive argument.
 * Pure 64-bit host arithmetic (the product is formed in 128 bits); the device code decides by this very function. */
int64_t sq_rng_table_cover(int32_t w, int32_t h, int32_t samples, int64_t budget_bytes);

#ifdef __cplusplus
}
#endif
#endif
