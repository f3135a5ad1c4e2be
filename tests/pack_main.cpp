// pack_main.cpp — the scene packer as a stand-alone program, for a sanitizer build of the host code (tests/test_pack.py):
//   g++ -std=c++17 -ffp-contract=off -fsanitize=address,undefined squigly-trace_amd/csrc/sq_host.cpp tests/pack_main.cpp
//   ./a.out data/scene.obj data [raw scene file ...]
// Loads the scene, builds its BIH, packs it, reads every byte of every array and every scalar through the C-ABI window
// (include/squigly_host.h), plans a handful of calls on the packed scene through the planner's window (sq_plan_call) and frees
// everything; then builds, packs, reads and frees every raw scene file the same way.  A raw scene file is two int32 (triangles,
// materials), then the sq_tri records, then the sq_material records, loaded through sq_mesh_from_arrays.  One line of output per
// scene.  Exit status 0 and an empty stderr mean nothing was reported.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../include/squigly_host.h"
#include "../squigly-trace_amd/csrc/sq_error.h"

static int fail(const char* what) { std::fprintf(stderr, "%s: %s\n", what, sq_error_buffer()); return 1; }

static int mesh_from_raw_file(const char* path, sq_mesh** mesh) {
    std::FILE* f = std::fopen(path, "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", path); return 1; }
    int32_t n[2] = { 0, 0 };
    bool ok = std::fread(n, sizeof n, 1, f) == 1 && n[0] >= 0 && n[1] >= 0;
    std::vector<sq_tri> tris(ok ? (size_t)n[0] : 0); std::vector<sq_material> mats(ok ? (size_t)n[1] : 0);
    ok = ok && std::fread(tris.data(), sizeof(sq_tri), tris.size(), f) == tris.size() && std::fread(mats.data(), sizeof(sq_material), mats.size(), f) == mats.size();
    std::fclose(f);
    if (!ok) { std::fprintf(stderr, "%s: not a raw scene file\n", path); return 1; }
    return sq_mesh_from_arrays(tris.data(), n[0], mats.data(), n[1], mesh) ? fail("sq_mesh_from_arrays") : 0;
}

// build, pack, read everything, plan (the first scene only), free; takes the mesh over
static int run_scene(sq_mesh* mesh, bool plan_calls) {
    sq_bih* bih = nullptr; sq_packed* packed = nullptr;
    if (sq_bih_build(mesh, &bih)) return fail("sq_bih_build");
    sq_scene scene;
    sq_bih_scene(bih, &scene);
    if (sq_scene_pack(&scene, &packed)) return fail("sq_scene_pack");
    const char* arrays[] = { "branches", "leaves", "tris", "tri_mat", "surfs", "mats", "verts4", "trix", "rbranch", "emitters",
                             "cull_child", "cull_child16", "branches_m", "level1", "level1_cover", "level1_mirror" };
    const char* scalars[] = { "n_branches", "n_leaves", "height", "root_ref", "rroot", "packed_leaves", "nonneg_materials", "finite_geometry",
                              "n_emitters", "n_verts", "cull_o2max", "cull_d2min", "cull_d2max", "small_index", "shortcut_depth", "level1_zero", "level1_on" };
    size_t total = 0; uint64_t sum = 0; int n_arrays = 0;
    for (const char* name : arrays) {
        const void* data = nullptr; size_t bytes = 0;
        if (sq_packed_array(packed, name, &data, &bytes)) return fail(name);
        for (size_t i = 0; i < bytes; ++i) sum += ((const unsigned char*)data)[i];
        total += bytes; ++n_arrays;
    }
    for (const char* name : scalars) {
        int64_t v = 0;
        if (sq_packed_scalar(packed, name, &v)) return fail(name);
        sum += (uint64_t)v;
    }
    const void* data = nullptr; size_t bytes = 0;
    if (!sq_packed_array(packed, "no such array", &data, &bytes)) { std::fprintf(stderr, "an unknown name was accepted\n"); return 1; }
    // the planner on this scene: every path, a refusal, an unknown name, and every scalar it gives
    std::vector<const char*> base_names = { "n_tris", "trix", "n_cu" };
    std::vector<int64_t> base_values = { scene.n_tris, 0, 256 };
    if (sq_packed_array(packed, "trix", &data, &bytes)) return fail("trix");
    base_values[1] = bytes != 0;
    for (const char* name : { "n_branches", "n_verts", "height", "small_index", "packed_leaves", "n_emitters", "nonneg_materials", "finite_geometry",
                              "shortcut_depth", "level1_on" }) {
        int64_t v = 0;
        if (sq_packed_scalar(packed, name, &v)) return fail(name);
        base_names.push_back(name); base_values.push_back(v);
    }
    const char* outs[] = { "path", "ad", "mom2", "sky", "deep", "nonneg_materials", "n_emitters", "cull_off", "pixels", "px_blocks", "px_lds", "n_call", "slots",
                           "trace_form", "resident", "pool", "profile", "dense", "n_lds", "stack_cap", "trace_blocks", "trace_threads", "tr_lds", "primary_grid",
                           "primary_lds", "aux_blocks", "acc_grouped", "level1_cull", "deep_slot_bytes", "need_lights", "need_sum2", "need_deep", "rng_table",
                           "rng_grow", "chunk_rays", "have_slots", "overlap", "tracks", "track_slots", "batch", "n_batches", "n_real", "query_chunk", "tail_kc",
                           "pp_grid_x", "pp_grid_y", "tail_pp_grid_x", "tail_pp_grid_y", "chunk_0", "chunk_1", "guide_shift_0", "guide_shift_1", "pixel_major",
                           "tail_chunk", "lone_chunk", "ws_cnt", "ws_stats", "ws_pix", "ws_t0", "ws_tri0", "ws_sum", "ws_mt", "ws_mtri", "ws_state", "ws_org",
                           "ws_dir", "ws_tri1", "ws_carry", "ws_total", "deep_oxy", "deep_trail", "deep_tmiss" };
    const int n_outs = (int)(sizeof outs / sizeof outs[0]);
    struct PlannedCall { const char* what; int want_rc; int64_t have_slots; std::vector<const char*> names; std::vector<int64_t> values; };
    const PlannedCall calls[] = {
        { "frame", 0, 0, { "local_rows", "h", "tile_rows", "tiles_x", "k_end" }, { 540, 540, 8, 68, 10 } },
        { "frame, halved slots, overlap", 0, 291600, { "local_rows", "h", "tile_rows", "tiles_x", "k_end", "overlap", "slots" }, { 540, 540, 8, 68, 10, 2, 1166400 } },
        { "variant 1, depth 5, sky", 0, 0, { "local_rows", "h", "k_end", "variant", "depth", "sky" }, { 3, 70, 2, 1, 5, 1 } },
        { "deep wavefront, masked", 0, 0, { "local_rows", "h", "tile_rows", "tiles_x", "k_end", "depth", "sky", "masked", "mom2" }, { 8, 8, 8, 1, 3, 8, 1, 1, 1 } },
        { "cast wavefront", 0, 0, { "local_rows", "h", "cast", "cast_wavefront", "lights_set", "n_lights", "slots" }, { 8, 8, 1, 1, 1, 5, 64 } },
        { "cast with lights", 0, 0, { "local_rows", "h", "cast", "lights_set", "n_lights" }, { 8, 8, 1, 1, 3 } },
        { "two views, streaming", 0, 0, { "source", "n_views", "local_rows", "h", "k_end", "resident", "trace_blocks_per_cu", "lds_node_kb" }, { 1, 2, 8, 8, 2, 0, 2, 0 } },
        { "radiance chunk", 0, 0, { "source", "h", "tiles_x", "k_end", "total_rays", "slots", "primary_pooled" }, { 2, 64, 1, 2, 210, 64, 1 } },
        { "intersection query", 0, 0, { "query", "n_rays", "slots" }, { 1, 1000, 64 } },
        { "intersection query, variant 1", 0, 0, { "query", "n_rays", "variant" }, { 1, 1000, 1 } },
        { "too tall for the per-lane stacks", 1, 0, { "height", "variant" }, { 400, 1 } },
        { "too tall for the trace kernel", 1, 0, { "height" }, { 200 } },
        { "too many pixels", 1, 0, { "local_rows", "h" }, { 1 << 20, 1 << 20 } },
        { "too many tile lanes", 1, 0, { "local_rows", "tiles_x", "primary_resident" }, { 1 << 26, 1, 0 } },
        { "an option out of range", 2, 0, { "overlap" }, { 3 } },
        { "an unknown name", 2, 0, { "no such input" }, { 1 } },
    };
    int n_planned = 0;
    for (const PlannedCall& c : calls) {
        if (!plan_calls) break;
        std::vector<const char*> names = base_names; std::vector<int64_t> values = base_values;
        names.insert(names.end(), c.names.begin(), c.names.end()); values.insert(values.end(), c.values.begin(), c.values.end());
        sq_plan plan; std::vector<int64_t> got((size_t)n_outs, -7);
        const int rc = sq_plan_call(names.data(), values.data(), (int32_t)names.size(), c.have_slots, &plan, outs, got.data(), n_outs);
        if (rc != c.want_rc) { std::fprintf(stderr, "%s: sq_plan_call returned %d, expected %d (%s)\n", c.what, rc, c.want_rc, sq_error_buffer()); return 1; }
        if ((rc == 0) != (plan.launched == 1)) { std::fprintf(stderr, "%s: launched = %d with return code %d\n", c.what, plan.launched, rc); return 1; }
        for (int64_t v : got) sum += (uint64_t)v;
        sum += (uint64_t)plan.trace_form + (uint64_t)plan.trace_lds_bytes;
        n_planned += rc == 0;
    }
    sq_packed_free(packed); sq_bih_free(bih); sq_mesh_free(mesh);
    std::printf("packed %d arrays, %zu bytes, planned %d calls, byte sum %llu\n", n_arrays, total, n_planned, (unsigned long long)sum);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: %s scene.obj material-directory [raw scene file ...]\n", argv[0]); return 2; }
    sq_mesh* mesh = nullptr;
    if (sq_mesh_from_obj(argv[1], argv[2], &mesh)) return fail("sq_mesh_from_obj");
    if (int rc = run_scene(mesh, true)) return rc;
    for (int i = 3; i < argc; ++i) {
        mesh = nullptr;
        if (int rc = mesh_from_raw_file(argv[i], &mesh)) return rc;
        if (int rc = run_scene(mesh, false)) return rc;
    }
    return 0;
}
