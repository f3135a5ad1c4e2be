// sq_pack_scene.h — the scene packer (sq_pack.h) and its C-ABI window (include/squigly_host.h).  The level-1 records are built by
// sq_pack_level1.h, the culling boxes by sq_cull_lemma.h.  A part of the host translation unit (sq_host.cpp, which has the file map and
// the includes); not a header for anything else.
//
// ---- Scene packing (sq_pack.h): from the caller's pre-order sq_scene to the arrays the kernels read and the flags that decide
// which kernel form a scene gets.  sq_scene_upload copies the result to the device as it is. ----------------------------------
int sq_check_scene_args(const sq_scene* sc, const void* out) {
    if (!sc || !out) return sq_set_error("null argument");
    if (!sc->nodes || sc->n_nodes < 1) return sq_set_error("scene has no nodes");
    if (sc->n_tris < 0 || sc->n_mats < 0 || (sc->n_tris && !sc->tris) || (sc->n_mats && !sc->mats)) return sq_set_error("bad triangle/material arrays");
    for (int32_t i = 0; i < sc->n_tris; ++i)
        if (sc->tris[i].mat < 0 || sc->tris[i].mat >= sc->n_mats) return sq_set_error("triangle %d: material %d outside 0..%d", i, sc->tris[i].mat, sc->n_mats - 1);
    return 0;
}

namespace {
using namespace sqd;

// Walks the pre-order array once; checks that it is a well-formed tree, that every index is in
// range, and computes the height.  A malformed tree would otherwise fault on the GPU.
int validate_tree(const sq_scene& sc, int& height, std::vector<int32_t>& depth_of) {
    const int32_t n = sc.n_nodes;
    if (n < 1) return sq_set_error("scene has no nodes");
    depth_of.assign((size_t)n, 0);
    struct Fr { int32_t node, stage; };
    std::vector<Fr> st;
    st.push_back({ 0, 0 });
    int32_t next = 0;      // next unvisited pre-order index
    depth_of[0] = 1;
    height = 0;
    while (!st.empty()) {
        const int32_t node = st.back().node; const int stage = st.back().stage;
        const sq_node& nd = sc.nodes[node];
        const int kind = nd.kind & 3;
        if (stage == 0) {
            if (node != next) return sq_set_error("node %d is not in pre-order position (expected %d)", node, next);
            ++next;
            const int dep = depth_of[(size_t)node];
            if (dep > height) height = dep;
            if (kind == 3) {
                const int64_t cnt = nd.kind >> 2, first = nd.link;
                if (cnt < 0 || first < 0 || first + cnt > sc.n_tris) return sq_set_error("leaf %d has triangle range [%lld,+%lld) outside 0..%d", node, (long long)first, (long long)cnt, sc.n_tris);
                st.pop_back();
                continue;
            }
            if ((nd.kind >> 2) != 0) return sq_set_error("branch %d has stray bits in kind", node);
            if (node + 1 >= n) return sq_set_error("branch %d has no left child", node);
            st.back().stage = 1;
            depth_of[(size_t)node + 1] = dep + 1;
            st.push_back({ node + 1, 0 });
        } else if (stage == 1) {
            if (nd.link != next) return sq_set_error("branch %d: right child link %d, expected %d", node, nd.link, next);
            if (nd.link >= n) return sq_set_error("branch %d: right child %d out of range", node, nd.link);
            st.back().stage = 2;
            depth_of[(size_t)nd.link] = depth_of[(size_t)node] + 1;
            st.push_back({ nd.link, 0 });
        } else st.pop_back();
    }
    if (next != n) return sq_set_error("tree covers %d of %d nodes", next, n);
    return 0;
}

inline bool finite(float c) { return c - c == 0.0f; }
inline bool finite3(const float* v) { return finite(v[0]) && finite(v[1]) && finite(v[2]); }

struct Packer {
    const sq_scene& sc; PackedScene& P;
    std::vector<int32_t> depth;             // per pre-order node, the root at 1 (validate_tree)
    std::vector<uint32_t> ref;              // per pre-order node: branch number, or leaf number | kLeafBit
    std::vector<uint32_t> axis, grown;      // per branch: split axis; kGrownLeft | kGrownRight
    bool finite_materials = true;

    bool is_leaf(int32_t i) const { return (sc.nodes[i].kind & 3) == 3; }
    uint32_t with_leaf_range(uint32_t r) const {   // a leaf reference that carries (first, count) itself; branch references pass
        return (r & kLeafBit) ? kLeafBit | ((uint32_t)P.leaves[r & ~kLeafBit].count << 24) | (uint32_t)P.leaves[r & ~kLeafBit].first : r;
    }
    bool leaves_fit_a_reference() const {          // first in 24 bits, count in 5
        return sc.n_tris < (1 << 24) && std::all_of(P.leaves.begin(), P.leaves.end(), [](const DevLeaf& L) { return L.count <= 31; });
    }

    // Leaves keep pre-order numbering; branches are numbered breadth-first (stable within a level) so the top of the
    // tree is a prefix of the branch table.
    void renumber() {
        ref.resize((size_t)sc.n_nodes);
        std::vector<std::vector<int32_t>> by_depth((size_t)P.height + 1);
        for (int32_t i = 0; i < sc.n_nodes; ++i) {
            if (is_leaf(i)) ref[(size_t)i] = (uint32_t)P.nl++ | kLeafBit;
            else by_depth[(size_t)depth[(size_t)i]].push_back(i);
        }
        for (auto& level : by_depth) for (int32_t i : level) ref[(size_t)i] = (uint32_t)P.nb++;
    }
    // Each branch carries its traversal box: the root's, clipped along the path (src/BIH.hs:130-141).
    void branch_boxes() {
        P.branches.resize((size_t)P.nb); P.leaves.resize((size_t)P.nl); axis.resize((size_t)P.nb); grown.resize((size_t)P.nb);
        std::vector<sq_bounds> box((size_t)sc.n_nodes);
        box[0] = sc.root;
        for (int32_t i = 0; i < sc.n_nodes; ++i) {          // pre-order: parents come before children
            const sq_node& nd = sc.nodes[i]; const uint32_t me = ref[(size_t)i];
            if (is_leaf(i)) { P.leaves[me & ~kLeafBit] = { nd.link, nd.kind >> 2 }; continue; }
            const int ax = nd.kind & 3; const sq_bounds& b = box[(size_t)i]; DevBranch& d = P.branches[me];
            for (int c = 0; c < 3; ++c) { d.lo[c] = b.lo[c]; d.hi[c] = b.hi[c]; }
            d.lmax = d.lmax2 = nd.lmax; d.rmin = d.rmin2 = nd.rmin; d.left = ref[(size_t)i + 1]; d.right = ref[(size_t)nd.link];
            axis[me] = (uint32_t)ax; grown[me] = (nd.lmax > b.hi[ax] ? kGrownLeft : 0u) | (nd.rmin < b.lo[ax] ? kGrownRight : 0u);
            sq_bounds l = b, r = b;
            l.hi[ax] = nd.lmax; r.lo[ax] = nd.rmin;
            box[(size_t)i + 1] = l; box[(size_t)nd.link] = r;
        }
    }
    // One pass over the materials: the device copy, and what their values allow.  nonneg_materials keeps the s == 0 shortcuts
    // (absorbs()) on: every component >= +0 and <= 3e38, every emission product finite, and the bound max_s * max_e + max_e on a
    // nested radiance (in double; max_e the largest fp32 emission product, max_s the largest surface component) comfortably finite
    // in fp32 -- 0 * inf would be NaN in the reference (src/Lib.hs:135-136; DESIGN.md 3, "The surfColor == 0 shortcut and overflow").
    // That bound is one product deep, the reference's depth; shortcut_depth says how much deeper the same reasoning still holds.
    void material_flags() {
        static_assert(sizeof(sq_material) == sizeof(DevMat), "a material is copied as it is");
        P.mats.resize((size_t)sc.n_mats);
        bool nonneg = true; double max_e = 0.0, max_s = 0.0;
        for (int32_t i = 0; i < sc.n_mats; ++i) {
            const sq_material& m = sc.mats[i];
            float comp[8]; std::memcpy(comp, &m, sizeof comp); std::memcpy(&P.mats[(size_t)i], comp, sizeof comp);
            for (float c : comp) { nonneg = nonneg && !std::signbit(c) && c <= 3.0e38f; finite_materials = finite_materials && finite(c); }
            for (int k = 0; k < 3; ++k) {
                const float e = m.emissive * m.emit[k];
                nonneg = nonneg && finite(e);                                // the product itself may be inf
                max_e = std::max(max_e, (double)e); max_s = std::max(max_s, (double)m.surf[k]);
            }
        }
        P.nonneg_materials = nonneg && max_s * max_e + max_e <= 3.0e38;
        // That is the reference's depth, 3: one product below a path's level 0.  Under depth D a path nests D - 2 of them, and
        // max_e * (1 + max_s + ... + max_s^(D-2)) bounds them all.  shortcut_depth is the largest D the bound holds for (0: none); a
        // launch at a greater depth runs with the shortcuts off.  A sum that overflows or is NaN (0 * inf) fails the comparison.
        P.shortcut_depth = 0;
        double sum = 1.0, power = 1.0;
        for (int depth = 3; P.nonneg_materials && depth <= kDeepestPath; ++depth) {
            power *= max_s; sum += power;
            if (!(max_e * sum <= 3.0e38)) break;
            P.shortcut_depth = depth;
        }
    }
    // Triangles as (v0, e1, e2) and the per-triangle shading record (surface_of).
    void triangles_and_surfaces() {
        const size_t nt = (size_t)sc.n_tris;
        P.tris.resize(nt + kTriRunPad); P.tri_mat.resize(nt); P.surfs.resize(nt);   // zero triangles: get_run may read past the last one
        for (size_t i = 0; i < nt; ++i) {
            const sq_tri& t = sc.tris[i]; const sq_material& m = sc.mats[t.mat]; DevTri& d = P.tris[i];
            for (int c = 0; c < 3; ++c) { d.v0[c] = t.v0[c]; d.e1[c] = t.v1[c] - t.v0[c]; d.e2[c] = t.v2[c] - t.v0[c]; }
            P.tri_mat[i] = t.mat;
            const f3 nrm = sq::cross(sq::mk(d.e1[0], d.e1[1], d.e1[2]), sq::mk(d.e2[0], d.e2[1], d.e2[2]));
            const f3 em = sq::scale(m.emissive, sq::mk(m.emit[0], m.emit[1], m.emit[2]));
            P.surfs[i] = DevSurf{ { nrm.x, nrm.y, nrm.z }, m.reflective, { m.surf[0], m.surf[1], m.surf[2] }, 0, { em.x, em.y, em.z }, 0 };
        }
    }
    // Indexed form for LDS residency: unique vertices (bitwise) + 16-bit indices, when they fit.
    void vertex_index_form() {
        struct Key { uint32_t a, b, c; bool operator==(const Key& o) const { return a == o.a && b == o.b && c == o.c; } };
        struct KeyHash { size_t operator()(const Key& k) const { return ((size_t)k.a * 0x9E3779B1u) ^ ((size_t)k.b * 0x85EBCA77u) ^ ((size_t)k.c * 0xC2B2AE3Du); } };
        std::unordered_map<Key, uint32_t, KeyHash> ids;
        bool fits = sc.n_mats <= 65535;
        P.trix.resize((size_t)sc.n_tris * 4);
        for (int32_t i = 0; i < sc.n_tris && fits; ++i) {
            const float* vs[3] = { sc.tris[i].v0, sc.tris[i].v1, sc.tris[i].v2 };
            for (int k = 0; k < 3 && fits; ++k) {
                Key key; std::memcpy(&key, vs[k], sizeof key);
                auto it = ids.find(key);
                if (it == ids.end()) {
                    if (ids.size() >= 65535) { fits = false; break; }
                    it = ids.emplace(key, (uint32_t)ids.size()).first;
                    P.verts4.insert(P.verts4.end(), vs[k], vs[k] + 3); P.verts4.push_back(0.0f);
                }
                P.trix[(size_t)i * 4 + k] = (uint16_t)it->second;
            }
            P.trix[(size_t)i * 4 + 3] = (uint16_t)sc.tris[i].mat;
        }
        if (!fits) { P.verts4.clear(); P.trix.clear(); }
    }
    // Resident encoding of the branches (sq_scene.h): needs 16-bit indices, leaves that fit a reference and a 24-bit branch index.
    void resident_encoding() {
        if (P.trix.empty() || P.nb >= (1 << 24) || !leaves_fit_a_reference()) { P.trix.clear(); return; }
        P.rbranch.resize((size_t)P.nb * 10);
        for (int32_t i = 0; i < P.nb; ++i) {
            const DevBranch& d = P.branches[(size_t)i]; uint32_t* r = &P.rbranch[(size_t)i * 10];
            std::memcpy(r, &d, 32);                                          // lo, lmax | hi, rmin
            r[8] = with_leaf_range(d.left) | (axis[(size_t)i] << kAxisShift); r[9] = with_leaf_range(d.right) | (grown[(size_t)i] << kAxisShift);
        }
        P.rroot = with_leaf_range(ref[0]);
    }
    // Culling boxes (include/squigly_host.h: sq_cull_boxes) of a branch's two children, with the branch: as fp32 (GlobalNodes)
    // and as binary16 pairs rounded outwards (ResidentNodes, HybridNodes).
    int culling_tables() {
        std::vector<float> cbox((size_t)sc.n_nodes * 6);                     // per pre-order node
        if (sq_cull_boxes(&sc, cbox.data(), P.cull_limits)) return 1;
        if (!(P.cull_limits[0] >= 0.0f) || P.nb == 0) return 0;
        P.cull_child.resize((size_t)P.nb * 16); P.cull_child16.resize((size_t)P.nb * 8, 0u);
        for (int32_t i = 0; i < sc.n_nodes; ++i) {
            if (is_leaf(i)) continue;
            const float* child[2] = { &cbox[(size_t)(i + 1) * 6], &cbox[(size_t)sc.nodes[i].link * 6] };
            for (size_t side = 0; side < 2; ++side) {
                const float* bx = child[side]; const size_t at = (size_t)ref[(size_t)i] * 2 + side;
                float* o = &P.cull_child[at * 8];
                o[0] = bx[0]; o[1] = bx[1]; o[2] = bx[2]; o[3] = 0; o[4] = bx[3]; o[5] = bx[4]; o[6] = bx[5]; o[7] = 0;
                for (int c = 0; c < 3; ++c) P.cull_child16[at * 4 + (size_t)c] = sq_half_outward(bx[c], 0) | (sq_half_outward(bx[3 + c], 1) << 16);
            }
        }
        return 0;
    }
    // Streaming form: leaf references carry (first, count) themselves when they fit, which saves the dependent leaf-table
    // load of every leaf visit; the left word takes the split axis.
    int leaf_references() {
        P.packed_leaves = leaves_fit_a_reference();
        if (P.nb >= (1 << 29) || P.nl >= (1 << 29)) return sq_set_error("scene has %d branches and %d leaves; the device layout holds 2^29 of each", P.nb, P.nl);
        for (int32_t i = 0; i < P.nb; ++i) {
            DevBranch& d = P.branches[(size_t)i];
            if (P.packed_leaves) { d.left = with_leaf_range(d.left); d.right = with_leaf_range(d.right); }
            d.left |= axis[(size_t)i] << kAxisShift;
        }
        P.root_ref = P.packed_leaves ? with_leaf_range(ref[0]) : ref[0];
        return 0;
    }
    // Streaming form: branch record + its children's binary16 culling boxes as ONE packed 80-byte record (SceneView::branches_m,
    // HybridNodes); what it and a line-padded form measured: DESIGN.md 4.8, profiles/r03t_merged_branches_ab.txt.
    void merged_records() {
        P.branches_m.assign((size_t)P.nb * 20, 0u);        // (a scene without culling boxes keeps zeros there: they are never read)
        for (size_t b = 0; b < (size_t)P.nb; ++b) {
            std::memcpy(&P.branches_m[b * 20], &P.branches[b], 48);
            if (!P.cull_child16.empty()) std::memcpy(&P.branches_m[b * 20 + 12], &P.cull_child16[b * 8], 32);
        }
    }
    // Emissive triangles (for the last-bounce shortcut of sq_shade1): emission not exactly (+0, +0, +0).  Disabled (-1) when a
    // material value is not finite (then s*0 + e is not exactly +0 for non-emitters) or when the list is long enough to cost
    // more than it saves.
    void emitter_list() {
        static const float zero[3] = { 0.0f, 0.0f, 0.0f };
        for (int32_t i = 0; i < sc.n_tris; ++i) if (std::memcmp(P.surfs[(size_t)i].emit, zero, sizeof zero) != 0) P.emitters.push_back(i);
        P.n_emitters = (finite_materials && P.emitters.size() <= 64) ? (int32_t)P.emitters.size() : -1;
    }
    void geometry_flags() {                                 // v_min / v_max slabs need NaN-free planes
        bool fin = finite3(sc.root.lo) && finite3(sc.root.hi);
        for (const DevBranch& d : P.branches) fin = fin && finite3(d.lo) && finite3(d.hi) && finite(d.lmax) && finite(d.rmin);
        for (int32_t i = 0; i < sc.n_tris && fin; ++i) fin = finite3(sc.tris[i].v0) && finite3(sc.tris[i].v1) && finite3(sc.tris[i].v2);
        P.finite_geometry = fin;
        P.small_index = P.nb < 0x8000 && sc.n_tris < 0x8000;
        P.n_verts = (int32_t)(P.verts4.size() / 4);
    }
};

}  // namespace

int sq_pack_scene(const sq_scene& sc, PackedScene& out) {
    out = PackedScene{};
    Packer k{ sc, out };
    if (validate_tree(sc, out.height, k.depth)) return 1;
    if (sc.height && sc.height != out.height) return sq_set_error("scene.height = %d but the tree has height %d", sc.height, out.height);
    k.renumber(); k.branch_boxes(); k.material_flags(); k.triangles_and_surfaces(); k.vertex_index_form(); k.resident_encoding();
    if (k.culling_tables() || k.leaf_references()) return 1;
    k.merged_records(); k.emitter_list(); k.geometry_flags(); build_level1(sc, out, k.finite_materials);
    return 0;
}

// ---- the C-ABI window on the packer (include/squigly_host.h) ----
struct sq_packed : PackedScene {};
extern "C" int sq_scene_pack(const sq_scene* sc, sq_packed** out) {
    if (sq_check_scene_args(sc, out)) return 1;
    sq_packed* p = new sq_packed;
    if (sq_pack_scene(*sc, *p)) { delete p; return 1; }
    *out = p;
    return 0;
}
extern "C" void sq_packed_free(sq_packed* p) { delete p; }
extern "C" int sq_packed_array(const sq_packed* P, const char* name, const void** data, size_t* bytes) {
    if (!P || !name || !data || !bytes) return sq_set_error("null argument");
    bool found = false;
    auto is = [&](const char* n, const auto& v) { if (!found && !std::strcmp(name, n)) { found = true; *data = v.data(); *bytes = v.size() * sizeof(v[0]); } };
    is("branches", P->branches); is("leaves", P->leaves); is("tris", P->tris); is("tri_mat", P->tri_mat); is("surfs", P->surfs);
    is("mats", P->mats); is("verts4", P->verts4); is("trix", P->trix); is("rbranch", P->rbranch); is("emitters", P->emitters);
    is("cull_child", P->cull_child); is("cull_child16", P->cull_child16); is("branches_m", P->branches_m); is("level1_cover", P->level1_cover);
    is("level1_mirror", P->level1_mirror);
    if (!found && !std::strcmp(name, "level1")) { found = true; *data = &P->level1; *bytes = sizeof P->level1; }
    return found ? 0 : sq_set_error("no packed array '%s'", name);
}
extern "C" int sq_packed_scalar(const sq_packed* P, const char* name, int64_t* value) {
    if (!P || !name || !value) return sq_set_error("null argument");
    uint32_t lim[3]; std::memcpy(lim, P->cull_limits, sizeof lim);
    const struct { const char* name; int64_t value; } all[] = {
        { "n_branches", P->nb }, { "n_leaves", P->nl }, { "height", P->height }, { "root_ref", P->root_ref }, { "rroot", P->rroot },
        { "packed_leaves", P->packed_leaves }, { "nonneg_materials", P->nonneg_materials }, { "finite_geometry", P->finite_geometry },
        { "n_emitters", P->n_emitters }, { "n_verts", P->n_verts }, { "cull_o2max", lim[0] }, { "cull_d2min", lim[1] }, { "cull_d2max", lim[2] },
        { "small_index", P->small_index }, { "shortcut_depth", P->shortcut_depth }, { "level1_zero", P->level1_zero }, { "level1_on", P->level1.on } };
    for (const auto& s : all) if (!std::strcmp(name, s.name)) { *value = s.value; return 0; }
    return sq_set_error("no packed scalar '%s'", name);
}
