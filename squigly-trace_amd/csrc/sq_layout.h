// sq_layout.h — the records and bit positions of the device-resident scene, free of any HIP include: what the host packer
// (sq_pack_scene.h, sq_pack.h) writes and the kernels (sq_scene.h) read.  Citations are relative to the reference repository root.
#pragma once
#include <stdint.h>
namespace sqd {
constexpr uint32_t kLeafBit = 0x80000000u;   // child reference: leaf index | kLeafBit, or branch index

// HBM layout (read-only during a render).  Branches are numbered breadth-first so that the top
// of the tree is a prefix of the table (that prefix is what gets staged in LDS).
struct DevBranch {          // 48 B, three 16-byte quads
    float lo[3]; float lmax;    // traversal box of THIS branch: root bounds clipped along the path (src/BIH.hs:130-141)
    float hi[3]; float rmin;
    float lmax2, rmin2;         // the third quad alone serves a return into this branch (planes, axis, children):
    uint32_t left, right;       //   one 16-byte load instead of three.  Bits 30..29 of `left` hold the split axis.
};
struct DevLeaf { int32_t first, count; };
struct DevTri {             // 36 B: v0 | e1 = v1 - v0 | e2 = v2 - v0 (same rounding as src/Geometry.hs:130-131).
    float v0[3];            // Unpadded on purpose: the streaming kernel is bound by L2/MALL/HBM bytes on large
    float e1[3];            // scenes; the material index lives in its own array because only shading needs it.
    float e2[3];
};
struct DevMat { float reflective, sr, sg, sb, emissive, er, eg, eb; };   // 32 B
struct DevSurf {            // 48 B, three quads: everything shading needs from a hit triangle behind ONE index
    float n[3], reflective;     // normal = e1 x e2 (src/Geometry.hs:79-80) | Material.reflective
    float surf[3], pad0;        // surfColor
    float emit[3], pad1;        // emissive *^ emitColor (src/Lib.hs:136), the same fp32 products as on the device
};
static_assert(sizeof(DevBranch) == 48 && sizeof(DevLeaf) == 8 && sizeof(DevTri) == 36 && sizeof(DevMat) == 32 && sizeof(DevSurf) == 48,
              "the device records have the sizes their comments promise");

constexpr int kAxisShift = 29;                                 // a branch's reference words keep two flag bits each at 30..29:
constexpr uint32_t kAxisMask = 3u << kAxisShift;               //   the LEFT word the split axis,
// the RIGHT word of the resident form "the left / the right child's box GROWS", i.e. the plane that replaces one of this branch's
// own (lmax for hi[axis], rmin for lo[axis], src/BIH.hs:130-141) lies outside this branch's box.  That happens where
// lmax = max + 0.001 or rmin = min - 0.001 (src/BIH.hs:92-95) passes a plane of the root box that no ancestor has clipped yet
// (5 of scene.obj's 1278 children).  The packer still sets them (the removed incremental slab test read them);
// every reader masks them off.
constexpr uint32_t kGrownLeft = 1u, kGrownRight = 2u;
// The first-bounce reduction (sq_pack_level1.h, "Level-1 culling"; read by sq_gen_bounce1 alone, as a kernel argument of its own):
// a scattered ray 1 whose sample provably ends with the radiance of a first-bounce miss is never queued.
constexpr int kLevel1Classes = 4;
struct Level1Cull {
    int32_t on;                              // 0: nothing is culled (a precondition fails, or option "level1_cull" is 0)
    int32_t n_classes;                       // mirror classes in use, ascending by value
    float o2max, d2min, d2max;               // the culling lemma's limits on a ray (sq_cull_boxes), here for ray 1 and for +-randomVector
    float class_val[kLevel1Classes];         // class c: every triangle that mirrors when unit_float(n1) <= class_val[c] ...
    float class_box[kLevel1Classes][6];      // ... lies in this culling box (lo.xyz, hi.xyz; infinite where the lemma does not reach)
    double em_lo[3], em_hi[3];               // bounding box of the emissive triangles' vertices
    double em_rho, em_add;                   // its margin for a ray 2 whose smallest accepted |determinant| is a: em_rho * (eps / a) + em_add
};
// The cover of the geometry ray 1 can end on (sq_pack_level1.h, "Level-1 culling", condition 4): at most kLevel1Boxes boxes that together
// hold the exact point X in which an accepted ray 1 meets the plane of its triangle; the computed parameter t^ of the hit lies within
// r |t| + c of X's parameter t.  One record in device memory behind SceneView::rtail, read by sq_gen_bounce1 alone, wave-uniformly.
constexpr int kLevel1Boxes = 8;
struct Level1Cover {
    int32_t n; int32_t pad[3];               // distinct boxes, 1 .. kLevel1Boxes; the entries beyond them repeat the first
    float r[kLevel1Boxes], c[kLevel1Boxes];  // per box: |t^ - t| <= r |t| + c for every triangle in it (the rounding of the widened interval included)
    float box[kLevel1Boxes][6];              // lo.xyz, hi.xyz
};
static_assert(sizeof(Level1Cover) == 272, "the cover is seventeen 16-byte quads");
// Condition 5 (sq_pack_level1.h, "Level-1 culling", the mirror extension): for a sample whose ray 1 passes the box of its mirror class, what
// a MIRRORED ray 2 can reach.  A panel is a set of non-emissive triangles of one `reflective` value `val` close to one plane: `box` holds
// the exact point in which an accepted ray 1 meets the plane of one of them (a cover box), `image` the emitters' grown box reflected in
// the panel's plane, and a ray 1 that ends on the panel at a computed t^ > 0 has its exact parameter t > -back.  A rest box is a culling
// box of mirroring triangles outside every panel, the largest `reflective` among them rmax.  rmin[j]: the smallest `reflective` in box j
// of the cover.  w: at most kLevel1W vectors with | |a^| - |d1.w| | <= err |d1| for the determinant a^ of every (mirrored ray 2,
// emitter); thr2 >= (a0 + err)^2.  One record directly behind the cover (SceneView::rtail + 1 cover), read wave-uniformly.
constexpr int kLevel1Panels = 12, kLevel1Rest = 4, kLevel1W = 8;
struct Level1Mirror {
    int32_t n_panels, n_rest, n_w;           // n_panels = 0: the condition is off for the scene.  Entries beyond a count repeat the first
    float thr2;                              // the determinant floor: every (d1.w_k)^2 >= thr2 |d1|^2, or the sample is kept
    float d2lo, d2hi;                        // |d1|^2 inside these keeps the mirrored |d2|^2 inside Level1Cull's d2min, d2max
    float a0, m0;                            // the floor itself and the emitters' margin at it (what `image` was built with)
    float rmin[kLevel1Boxes];
    float w[kLevel1W][4];                    // xyz, unused
    float rest[kLevel1Rest][8];              // lo.xyz, hi.xyz, rmax, unused
    float panel[kLevel1Panels][16];          // box lo.xyz hi.xyz | image lo.xyz hi.xyz | back, val, unused x 2
};
static_assert(sizeof(Level1Mirror) == 1088, "the mirror record is sixty-eight 16-byte quads");
constexpr int kTriRunPad = 3;   // zero triangles after the last one, so that a run of loads may start at any triangle (GlobalTris::kRunPad)
}  // namespace sqd
