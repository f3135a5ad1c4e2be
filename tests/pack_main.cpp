// pack_main.cpp — the scene packer as a stand-alone program, for a sanitizer build of the host code (tests/test_pack.py):
//   g++ -std=c++17 -ffp-contract=off -fsanitize=address,undefined squigly-trace_amd/csrc/sq_host.cpp tests/pack_main.cpp
//   ./a.out data/scene.obj data
// Loads the scene, builds its BIH, packs it, reads every byte of every array and every scalar through the C-ABI window
// (include/squigly_host.h) and frees everything.  Exit status 0 and an empty stderr mean nothing was reported.
#include <cstdint>
#include <cstdio>

#include "../include/squigly_host.h"
#include "../squigly-trace_amd/csrc/sq_error.h"

static int fail(const char* what) { std::fprintf(stderr, "%s: %s\n", what, sq_error_buffer()); return 1; }

int main(int argc, char** argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: %s scene.obj material-directory\n", argv[0]); return 2; }
    sq_mesh* mesh = nullptr; sq_bih* bih = nullptr; sq_packed* packed = nullptr;
    if (sq_mesh_from_obj(argv[1], argv[2], &mesh)) return fail("sq_mesh_from_obj");
    if (sq_bih_build(mesh, &bih)) return fail("sq_bih_build");
    sq_scene scene;
    sq_bih_scene(bih, &scene);
    if (sq_scene_pack(&scene, &packed)) return fail("sq_scene_pack");
    const char* arrays[] = { "branches", "leaves", "tris", "tri_mat", "surfs", "mats", "verts4", "trix", "rbranch", "emitters",
                             "cull_child", "cull_child16", "branches_m" };
    const char* scalars[] = { "n_branches", "n_leaves", "height", "root_ref", "rroot", "packed_leaves", "nonneg_materials", "finite_geometry",
                              "n_emitters", "n_verts", "cull_o2max", "cull_d2min", "cull_d2max", "small_index", "shortcut_depth" };
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
    sq_packed_free(packed); sq_bih_free(bih); sq_mesh_free(mesh);
    std::printf("packed %d arrays, %zu bytes, byte sum %llu\n", n_arrays, total, (unsigned long long)sum);
    return 0;
}
