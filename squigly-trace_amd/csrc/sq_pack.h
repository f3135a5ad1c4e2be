// sq_pack.h — the scene packer (sq_pack_scene.h): everything sq_scene_upload decides and lays out before it touches a device.
// Plain host C++, no HIP include, so it runs, is tested (tests/test_pack.py) and is sanitized on a CPU.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/squigly_hip.h"
#include "sq_layout.h"

constexpr int kDeepestPath = 8;                     // the largest depth sq_scene_set_depth takes

struct PackedScene {
    // one vector per device array, named after the SceneView member it feeds (sq_scene.h)
    std::vector<sqd::DevBranch> branches;           // breadth-first; left / right are the references the streaming forms read
    std::vector<sqd::DevLeaf> leaves;               // pre-order
    std::vector<sqd::DevTri> tris;                  // leaf order, then kTriRunPad zero records
    std::vector<int32_t> tri_mat;
    std::vector<sqd::DevSurf> surfs;
    std::vector<sqd::DevMat> mats;
    std::vector<float> verts4;                      // unique vertices, 4 floats each; empty unless 16-bit indices fit
    std::vector<uint16_t> trix;                     // 4 per triangle; empty unless the resident form can be encoded
    std::vector<uint32_t> rbranch;                  // 10 words per branch, with trix
    std::vector<int32_t> emitters;
    std::vector<float> cull_child;                  // 16 floats per branch; empty when nothing may be culled
    std::vector<uint32_t> cull_child16;             // 8 words per branch, with cull_child
    std::vector<uint32_t> branches_m;               // 20 words per branch
    int32_t nb = 0, nl = 0, height = 0;
    uint32_t root_ref = 0, rroot = 0;
    bool packed_leaves = false, nonneg_materials = false, finite_geometry = false;
    int32_t n_emitters = -1, n_verts = 0;
    int32_t shortcut_depth = 0;                     // the largest path depth (<= kDeepestPath) whose nested products nonneg_materials' bound covers
    float cull_limits[3] = { -1.0f, 0.25f, 1.5624f };   // SceneView::cull_o2max, cull_d2min, cull_d2max
    sqd::Level1Cull level1{};                       // the first-bounce reduction's tables; level1.on = its preconditions hold
    std::vector<sqd::Level1Cover> level1_cover;     // one record where level1.on (SceneView::rtail), else empty
    std::vector<sqd::Level1Mirror> level1_mirror;   // one record wherever level1_cover has one, behind it on the device
    bool level1_zero = false;                      // s.surf * 0 + s.emit is bitwise (+0, +0, +0) for every triangle outside `emitters`
    bool small_index = false;                       // < 0x8000 branches and triangles: 2-byte stack words
};

// The checks sq_scene_upload and sq_scene_pack make on their arguments before anything else: 0, or sq_set_error.
int sq_check_scene_args(const sq_scene* sc, const void* out);
// Validates the tree and fills `out`: 0, or sq_set_error.  `sc` has passed sq_check_scene_args.
int sq_pack_scene(const sq_scene& sc, PackedScene& out);
