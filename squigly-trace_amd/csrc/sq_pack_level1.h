// sq_pack_level1.h — level-1 culling on the host: the lemma with its two extensions, and the builder of the three records it reads
// (Level1Cull, Level1Cover, Level1Mirror: sq_layout.h).  sq_pack_scene (sq_pack_scene.h) calls build_level1 as its last step.  A part of
// the host translation unit (sq_host.cpp, which has the file map and the includes); not a header for anything else.
//
// ---- Level-1 culling: the fourth exact reduction of the ray count (no counterpart in the reference) ----
// A depth-0 sample that scatters shoots ray 1 = (p0, d1).  sq_gen_bounce1 holds the generator's next words n1, n2, which decide
// everything random about the rest of the path: the surface ray 1 hits scatters iff reflective < unit_float(n1), and then ray 2
// leaves the computed hit point p1 = fl(p0 + fl(t^ d1)) along +-nd, nd = randomVector(n1, n2), the sign alone depending on the
// unknown normal.  The sample is finished at once, as a first-bounce miss, when
//   (1) mollerTrumbore(p0, d1, e) rejects every emitter e                      (the very function the traversal calls),
//   (2) ray 1 is inside the limits of sq_cull_boxes and fails the slab test of the box of its mirror class, and
//   (3) the half-plane H = { p0 + t d1 + s nd : t >= 0, s real } misses the emitters' box grown by the margin below.
// LEMMA.  Under the preconditions (nonneg_materials, finite materials and geometry, at most 64 emitters, level1_zero, every
// non-emissive triangle and every emitter with P <= 29, R1 <= 2^20) such a sample's radiance has the bits of level0_radiance(s0).
// Proof.  By (1) whatever the traversal returns for ray 1 is no emitter.  A miss gives level0_radiance(s0) by
//   definition.  Otherwise let T be the hit triangle, s1 its surface: s1.emit is (+0, +0, +0).  If ray 2 is not traced, or hits
//   no emitter, L1 = s1.surf * 0 + s1.emit, bitwise (+0, +0, +0) by level1_zero, and s0.surf * L1 + s0.emit is level0_radiance(s0).
//   So it is enough that no emitter accepts ray 2.
//   (2): class c holds every triangle with reflective >= v, v the smallest of the scene's values that is >= unit_float(n1)
//   (merged classes hold more), i.e. every triangle that would mirror.  Its box is the union of their culling boxes, so by the
//   culling lemma above (and its remark on unions) mollerTrumbore rejects them all for ray 1: T scatters, ray 2 = (p1, +-nd).
//   Where p1 can be: the lemma's exact solution X = p0 + t d1 of the accepted test lies within rho_T of T, so |X| <= vmax +
//   rho_T and |t| |d1| <= omax + vmax + rho_T =: reach.  The computed t^ = fl(fl(1/a^) Nt^) obeys
//   |t^ - t| <= |Nt^ - Nt|/|a^| + |t| |a - a^|/|a^| + 2.01u |t^| <= 8u S E1 E2/eps + r_T |t| + 2.01u |t^|,  r_T = 7u P_T/eps <= 1/8,
//   so Y = p0 + t^ d1, a point of ray 1 with t^ > 0, has |Y| <= vmax + g1, g1 = max_T rho_T + 1.01 (r_T reach + rho_T), and
//   |p1 - Y| <= u (|t^ d1| + |p1|) <= delta1 = 4u (2 (vmax + g1) + omax); |p1| <= R1 = vmax + g1 + delta1.
//   (3): let e accept (p1, +-nd) with computed determinant a^ (its magnitude is the same for both signs, and it depends on nd
//   and e alone, so the kernel evaluates it; |a^| < eps rejects outright).  The derivation above uses of `eps` only that it
//   bounds |a^| from below, so it holds with alpha = |a^| >= eps in its place: some point p1 + s (+-nd), s >= 0, lies within
//   (eps/alpha) rho'_e + 6u (E1 + E2) of e, rho'_e = 32 (u/eps) P_e (R1 + V0 + E1 + E2) (S <= R1 + V0; |nd|^2 is checked against
//   the lemma's limits by the kernel).  Then Y + s (+-nd), a point of H, lies within that plus delta1 of e, inside the emitters'
//   vertex box grown by em_rho (eps/amin) + em_add, amin the smallest accepted |a^|: H meets the grown box.  Contrapositive: (3)
//   means every emitter rejects ray 2.                                                                                       QED
// The kernel tests (3) in binary64 on the exact fp32 values: H lies in the plane through p0 with normal N = d1 x nd and on the
// side (x - p0).w >= 0 of it, w = d1 - (d1.nd / nd.nd) nd.  The computed N, w are within 1e-15 |d1| (|nd|) of the exact ones and
// every x of the box has |x - p0| <= scale = |g|_1 + |h|_1 (g = centre - p0, h = half extents), so "the box lies strictly on one
// side of the plane" or "strictly on the negative side of w", each by more than 1e-9 scale, proves H misses the box.
// tests/test_level1_cull.py restates all of this in numpy and searches for counter-examples against the oracle's mollerTrumbore.
//
// EXTENSION.  (3) may be replaced by
//   (4) for every box j of the cover (level1_cover below), the interval I_j of t in which ray 1 can end on a triangle of the box
//       misses the stretch [ta, tb] = { t >= 0 : some s has p0 + t d1 + s nd in B },  B = the emitters' box grown as in (3)
//       (an empty stretch satisfies this for every cover).
// Proof.  As above it is enough that no emitter accepts ray 2; suppose e does.  The traversal returned a triangle T that accepted
//   ray 1 -- no emitter by (1), scattering by (2) -- with computed parameter t^ > 0, and by the proof of (3) the line Y + s nd,
//   Y = p0 + t^ d1, meets B: t^ lies in the stretch.  The accepted test has the exact solution X = p0 + t d1 = v0 + u e1 + v e2 (the
//   kernels' rounded edges): X lies IN THE PLANE of the triangle T' = (v0, v0 + e1, v0 + e2) and within rho_T of T', so X - Z is a
//   vector of that plane for the nearest point Z of T', and its k-th component is at most rho_T s_k, s_k = sqrt(1 - n^_k^2) the
//   largest k-th component of a unit vector orthogonal to the unit normal n^.  X lies in the box of T' grown by rho_T s_k along axis
//   k, hence in the cover box j that holds it, hence t in the exact slab interval of that box for ray 1, which the computed fp32
//   interval [tmin_j, tmax_j] of the box grown by the slab test's own rounding contains (the culling lemma above).  And
//   |t^ - t| <= c_T + r_T |t| + 2.01u |t^|, c_T = 8u S E1 E2 / eps, S <= omax + V0, r_T <= 1/8.  t -> t + r|t| and t -> t - r|t| increase
//   with t, so t^ (1 - 2.01u) <= tmax_j + r_j |tmax_j| + c_j and, where t^ <= t (then 0 < t^ <= t), t^ >= tmin_j - (r_j + 2.01u) |tmin_j| -
//   c_j, r_j and c_j the largest of the box: t^ lies in I_j = [tmin_j - r'_j |tmin_j| - c'_j, tmax_j + r'_j |tmax_j| + c'_j], the table's
//   r' = r + 2e-6 and c' = c (1 + 1e-5) covering the 2.01u and the three fp32 operations of either end.  t^ in I_j and in the stretch
//   contradicts (4).                                                                                                          QED
// The stretch: a line with direction nd through x meets B = c +- h iff |n_k.(x - c)| <= sum_j |n_k,j| h_j for n_k = nd x e_k, k = 0, 1,
//   2 (B's projection along nd is a hexagon with these edge normals; the components of n_k are components of nd, exact).  For x = p0
//   + t d1 that is |t N_k - G_k| <= r_k, N = d1 x nd, G = (c - p0) x nd.  The kernel forms N, G, r in binary64 from the exact fp32
//   values (N_k: two exact products and one rounding; G_k, r_k within 1e-14 scale), widens every slab by 1e-9 scale and every
//   quotient by 1e-9 of itself (the quotients' own error is below 1e-15), lets a slab with |N_k| < 1e-6 constrain nothing, and rounds
//   ta down and tb up to fp32 by a factor 1 -+ 2^-20: the computed stretch contains the exact one.
// tests/test_level1_stretch.py restates (4) and searches for counter-examples against the oracle's traversal and mollerTrumbore.
//
// MIRROR EXTENSION.  Where ray 1 passes the box of its mirror class, (2) may be replaced by
//   (5) with the record of level1_mirror below and un1 = unit_float(n1):  d2lo <= |d1|^2 <= d2hi;  ray 1 fails the slab test of every
//       rest box with rmax >= un1;  (d1.W_k)^2 >= thr2 |d1|^2 for every W_k;  for every panel p with val_p >= un1, ray 1's fp32 slab
//       intervals [pmin, pmax] of the panel's box and [imin, imax] of its image box have pmax < pmin, or pmax <= -back_p, or
//       imax < imin, or imax < pmin;  and (3) or (4) holds with the cover reduced to its boxes j with rmin_j < un1.
// Proof.  Let the traversal return T for ray 1, no emitter by (1), with computed parameter t^ > 0 and hit point p1.  It is enough
//   that no emitter accepts ray 2.
//   T scatters (reflective_T < un1): ray 2 = (p1, +-nd), and T lies in a box j of the cover with rmin_j <= reflective_T < un1.  The
//   proofs of (3) and (4) use of (2) only that T scatters, and (4)'s uses the box that holds T alone: they apply as they stand.
//   T mirrors (reflective_T >= un1): ray 2 = (p1, d2), d2 = fl(d1 - 2 (dn.d1) dn), dn the computed unit normal of T.  T is in no rest
//   box: its rmax >= reflective_T >= un1, the box contains T's culling box, and ray 1 fails its slab test, so mollerTrumbore rejects
//   T (the culling lemma).  So T is in a panel p, val_p = reflective_T >= un1.  Suppose emitter e accepts (p1, d2), determinant a^.
//   1. By the derivation of (4) the exact solution X = p0 + t d1 of ray 1's accepted test lies in the panel's box (a union of cover
//      boxes, grown in-plane), t in the exact slab interval of that box, which [pmin, pmax] contains: pmin <= t <= pmax.
//      |t^ - t| <= c_p + r_p |t| + 2.01u |t^| and t^ > 0 give t > -c_p / (1 - r_p) >= -1.15 c_p >= -back_p.  X lies in T's own plane,
//      within rho_T of a point of T', which is within h_p of the panel's plane Pi_p (unit normal n^_p); the two normals differ by
//      at most delta_p, so dist(X, Pi_p) <= h_p + rho_p delta_p =: hX.  With Y = p0 + t^ d1: |p1 - Y| <= delta1 (the proof of (3)) and
//      |Y - X| = |t^ - t| |d1| <= 1.25 c_p + r_p reach_p + 2.01u 1.3 (reach_p + 1.25 c_p), reach_p = omax + the box's farthest corner
//      >= |t| |d1| = |X - p0|: |p1 - X| <= e1_p, their sum.
//   2. |dn - +-n^_p| <= delta_p: the exact unit normal of T' is within the measured distance of n^_p, the fp32 cross product within
//      3.5u E1 E2 of the exact one (relative 4u E1 E2 / |n| after normalising, triangles with |n| <= 1e-4 E1 E2 being left to the
//      rest boxes), its fp32 normalisation within 8u.  With R_p = I - 2 n^_p n^_p^T: the exact d1 - 2 (dn.d1) dn differs from R_p d1 by
//      2 |(eps.d1) n^ + (n^.d1) eps + (eps.d1) eps| <= 4.01 delta_p |d1| (delta_p <= 1e-3), and the five fp32 operations add less than
//      16u |d1|: |d2 - R_p d1| <= kappa_p |d1|, kappa_p = 4.01 delta_p + 16u <= 4.1e-3.  Hence |d2|^2 lies inside [d2min, d2max] when
//      1.01 d2min <= |d1|^2 <= 0.99 d2max, which (5) checks, and the lemma of (3) applies to (p1, d2).
//   3. a^ is the fp32 value of d2.(e2 x e1) up to its sign, within 7u E1 E2 |d2| of it; d2.(e2 x e1) is within kappa_p |d1| |e2 x e1| of
//      (R_p d1).(e2 x e1) = d1.W, W = R_p (e2 x e1), which the list holds up to its sign and a deviation dev; the kernel's fp32 dot
//      product of d1 and the rounded W_k is within 4.1u |d1| |W_k| of the exact one.  err is the largest sum of these (|d1| >= 1/2
//      turns 7u 1.26 E1 E2 into 17.7u E1 E2 |d1|), so (d1.W_k)^2 >= thr2 |d1|^2, thr2 >= (a0 + err)^2 with room for the three fp32
//      roundings of the comparison, gives |a^| >= a0.  By the proof of (3) with alpha = a0 some exact Ye = p1 + s d2, s >= 0, lies
//      within (eps / a0) rho'_e + 6u (E1 + E2) of e: inside B0 = the emitters' box grown by m0 = em_rho eps / a0 + em_add.
//   4. Reflect in Pi_p: Ye' = R_Pi(p1) + s R_p d2 lies in the reflected B0.  |R_Pi(p1) - X| <= |p1 - X| + 2 dist(X, Pi_p) <= e1_p +
//      2 hX and |R_p d2 - d1| = |d2 - R_p d1| <= kappa_p |d1|, with s |d2| = |Ye - p1| <= far_p + e1_p (far_p the largest distance between
//      a point of the panel's box and one of B0) and |d1| / |d2| <= 1.01: the point Q = p0 + (t + s) d1 of ray 1's line is within
//      g_p = e1_p + 2 hX + 1.01 (far_p + e1_p) kappa_p of Ye'.
//   5. So ray 1's exact line passes the image box -- the bounds of the reflected corners of B0, grown by g_p and by the slab test's
//      own rounding 8u (|l| + omax) -- at the parameter tau = t + s >= t, and [imin, imax] contains its exact interval of that box:
//      imin <= imax, imax >= tau >= t >= pmin, with pmin <= pmax and pmax >= t > -back_p.  None of the four alternatives of (5) holds
//      for p: contradiction.                                                                                                  QED
// Every comparison of (5) is written so that a NaN keeps the sample.  How triangles are grouped into panels and rest boxes does not
// enter the proof.  tests/test_level1_mirror.py restates (5) and searches for counter-examples against the oracle.
namespace {
using namespace sqd;

// What the proofs above take from the scene as a whole: its norms (sq_cull_lemma.h), where p1 can be (g1, delta1, |p1| <= R1), and the
// slab test's own rounding for a box whose planes lie within vmax_inf + g1 of the origin.
struct Level1Bounds { SceneNorms scene; double g1, delta1, R1, slab_slack; };

inline void cross3(const double a[3], const double b[3], double out[3]) {
    out[0] = a[1] * b[2] - a[2] * b[1]; out[1] = a[2] * b[0] - a[0] * b[2]; out[2] = a[0] * b[1] - a[1] * b[0];
}
inline double length3(const double a[3]) { return std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]); }
inline double lemma_r(const TriNorms& q) { return 7.0 * kLemmaU * q.P / kLemmaEps; }                 // r_T of the proofs

// One triangle as the proofs see it, in binary64: the kernels' rounded fp32 edges, the exact normal n = e1 x e2 of the kernels' triangle
// T' = (v0, v0 + e1, v0 + e2) and its length, the five points (the vertices and those of T'), the lemma's lengths with rho_T for ray
// origins within omax, r_T and c_T = 8u S E1 E2 / eps (S <= omax + V0), and `reflective`.  un is the unit normal up to sign (its largest
// component positive) and un_err the bound on the distance of the COMPUTED unit normal from +-un: the fp32 cross product is within
// 3.5u E1 E2 of n, its fp32 normalisation within 8u of the unit vector.  A sliver (|n| <= 1e-4 E1 E2) has un = 0 and un_err = 1.
struct TriGeom { TriNorms q; double rho, r, c, e1[3], e2[3], n[3], nn, un[3], un_err, pts[3][5]; float reflective; };   // pts[k][i]: coordinate k of point i
inline TriGeom tri_geom(const sq_tri& t, float reflective, double omax) {
    TriGeom g{}; g.reflective = reflective;
    g.q = tri_norms(t); g.rho = lemma_rho(g.q, omax); g.r = lemma_r(g.q); g.c = 8.0 * kLemmaU * (omax + g.q.V0) * g.q.E1 * g.q.E2 / kLemmaEps;
    for (int k = 0; k < 3; ++k) {
        g.e1[k] = (double)(t.v1[k] - t.v0[k]); g.e2[k] = (double)(t.v2[k] - t.v0[k]);
        g.pts[k][0] = t.v0[k]; g.pts[k][1] = t.v1[k]; g.pts[k][2] = t.v2[k]; g.pts[k][3] = (double)t.v0[k] + g.e1[k]; g.pts[k][4] = (double)t.v0[k] + g.e2[k];
    }
    cross3(g.e1, g.e2, g.n); g.nn = length3(g.n);
    const bool ok = g.nn > 1e-4 * g.q.E1 * g.q.E2;
    int big = 0;
    for (int k = 1; k < 3; ++k) if (std::fabs(g.n[k]) > std::fabs(g.n[big])) big = k;
    for (int k = 0; k < 3; ++k) g.un[k] = ok ? g.n[k] / g.nn * (g.n[big] < 0 ? -1.0 : 1.0) : 0.0;
    g.un_err = ok ? 4.0 * kLemmaU * g.q.E1 * g.q.E2 / g.nn + 8.0 * kLemmaU : 1.0;
    return g;
}

// The culling box of one triangle, in binary64: its vertex bounds grown by cull_margin(rho_T).  Rounded outward it is the box
// sq_cull_boxes gives a leaf of this triangle alone; f_down and f_up are monotone, so a union (join) may be rounded once, at the end.
struct CullBox { double lo[3], hi[3], rmax; };                        // rmax: the largest `reflective` in the box
inline CullBox cull_box(const sq_tri& t, float reflective, const SceneNorms& N) {
    const double m = cull_margin(lemma_rho(tri_norms(t), N.omax), N.vmax_inf, N.omax);
    CullBox b; b.rmax = (double)reflective;
    for (int k = 0; k < 3; ++k) {
        b.lo[k] = std::min({ (double)t.v0[k], (double)t.v1[k], (double)t.v2[k] }) - m; b.hi[k] = std::max({ (double)t.v0[k], (double)t.v1[k], (double)t.v2[k] }) + m;
    }
    return b;
}
template <class B> void grow_to_hold(B& a, const B& b) {
    for (int k = 0; k < 3; ++k) { a.lo[k] = std::min(a.lo[k], b.lo[k]); a.hi[k] = std::max(a.hi[k], b.hi[k]); }
}
CullBox join(const CullBox& a, const CullBox& b) {
    CullBox o = a; o.rmax = std::max(a.rmax, b.rmax);
    grow_to_hold(o, b);
    return o;
}
template <class B> double volume(const B& a) { return (a.hi[0] - a.lo[0]) * (a.hi[1] - a.lo[1]) * (a.hi[2] - a.lo[2]); }
// Merges the pair of boxes whose union (join(a, b), which keeps a's place) adds the least volume, until `keep` remain.  The first pair
// in scan order wins a tie.
template <class B> void merge_by_least_added_volume(std::vector<B>& boxes, size_t keep, B (*join)(const B&, const B&)) {
    while (boxes.size() > keep) {
        size_t bi = 0, bj = 1; double best = INFINITY;
        for (size_t i = 0; i < boxes.size(); ++i)
            for (size_t j = i + 1; j < boxes.size(); ++j) {
                const double grow = volume(join(boxes[i], boxes[j])) - volume(boxes[i]) - volume(boxes[j]);
                if (grow < best) { best = grow; bi = i; bj = j; }
            }
        boxes[bi] = join(boxes[bi], boxes[bj]);
        boxes.erase(boxes.begin() + (std::ptrdiff_t)bj);
    }
}

// Condition (4)'s cover (the lemma's extension above).  Per non-emissive triangle T: the box of the kernels' triangle (v0, v0 + e1,
// v0 + e2 with the rounded edges, and the vertices themselves) grown along axis k by rho_T s_k, s_k = sqrt(1 - n^_k^2) the largest
// k-th component of a unit vector in T's plane, and by the slab test's own rounding.  Any grouping into boxes is valid; this one finds
// the walls and panels of a room: triangles thin on an axis are grouped by (axis, coordinate cell) -- the kMaxGroups largest groups, to
// bound the work --, the others by the octant of their centre, and the pair of boxes whose union adds the least volume is merged until
// kLevel1Boxes remain.  A box's r and c are the largest of its triangles', with room for the kernel's fp32 evaluation of the widened
// interval: three operations, each within u of a value no larger than 1.13 |t| + c, and the 2.01u |t^|.
struct CoverBox { double lo[3], hi[3], r, c, rmin; int64_t count; int axis; int64_t cell; };
// the box of one triangle, as the paragraph above grows it, with its r_T, c_T and `reflective`
inline CoverBox cover_box(const TriGeom& g, double slab_slack) {
    CoverBox b{}; b.count = 1; b.axis = 3; b.cell = 0; b.rmin = (double)g.reflective; b.r = g.r; b.c = g.c;
    for (int k = 0; k < 3; ++k) {
        const double across = std::sqrt(g.n[(k + 1) % 3] * g.n[(k + 1) % 3] + g.n[(k + 2) % 3] * g.n[(k + 2) % 3]);
        // (n is within 3e-16 E1 E2 of the exact normal: above the sliver limit the quotient is good to 3e-10, below it s_k = 1)
        const double s = g.nn > 1e-6 * g.q.E1 * g.q.E2 ? std::min(1.0, across / g.nn + 1e-6) : 1.0;
        b.lo[k] = *std::min_element(g.pts[k], g.pts[k] + 5) - g.rho * s - slab_slack;
        b.hi[k] = *std::max_element(g.pts[k], g.pts[k] + 5) + g.rho * s + slab_slack;
    }
    return b;
}
CoverBox join(const CoverBox& a, const CoverBox& b) {
    CoverBox o = a; o.count += b.count; o.r = std::max(a.r, b.r); o.c = std::max(a.c, b.c); o.rmin = std::min(a.rmin, b.rmin);
    grow_to_hold(o, b);
    return o;
}
// Returns whether there is a cover at all; then V is its record and rmin the smallest `reflective` in each of its boxes (for
// condition (5); entries beyond n repeat the first, as the record's do).
bool level1_cover(const sq_scene& sc, const std::vector<DevSurf>& surfs, const std::vector<char>& emits, const Level1Bounds& B,
                  Level1Cover& V, float rmin[kLevel1Boxes]) {
    using Box = CoverBox;
    std::vector<Box> each;
    double slo[3] = { 1e300, 1e300, 1e300 }, shi[3] = { -1e300, -1e300, -1e300 };
    for (int32_t i = 0; i < sc.n_tris; ++i) {
        if (emits[(size_t)i]) continue;
        const Box b = cover_box(tri_geom(sc.tris[i], surfs[(size_t)i].reflective, B.scene.omax), B.slab_slack);
        for (int k = 0; k < 3; ++k) { slo[k] = std::min(slo[k], b.lo[k]); shi[k] = std::max(shi[k], b.hi[k]); }
        each.push_back(b);
    }
    // (the extent of the GROWN boxes of the non-emitters: not the scene's, which condition (5) groups by)
    const double cover_extent = each.empty() ? 0.0 : std::max({ shi[0] - slo[0], shi[1] - slo[1], shi[2] - slo[2] });
    for (Box& b : each) {
        const double ex[3] = { b.hi[0] - b.lo[0], b.hi[1] - b.lo[1], b.hi[2] - b.lo[2] }, longest = std::max({ ex[0], ex[1], ex[2] });
        for (int k = 2; k >= 0; --k) if (ex[k] <= 1e-4 * cover_extent && ex[k] < 0.05 * longest) b.axis = k;
        if (b.axis < 3) b.cell = (int64_t)std::floor(0.5 * (b.lo[b.axis] + b.hi[b.axis]) / std::max(1e-3 * cover_extent, 1e-300) + 0.5);
        else for (int k = 0; k < 3; ++k) b.cell |= (int64_t)(b.lo[k] + b.hi[k] >= slo[k] + shi[k]) << k;
    }
    std::stable_sort(each.begin(), each.end(), [](const Box& a, const Box& b) { return a.axis != b.axis ? a.axis < b.axis : a.cell < b.cell; });
    std::vector<Box> boxes, octants;
    for (size_t i = 0; i < each.size(); ++i) {
        std::vector<Box>& to = each[i].axis < 3 ? boxes : octants;
        if (i && each[i].axis == each[i - 1].axis && each[i].cell == each[i - 1].cell) to.back() = join(to.back(), each[i]);
        else to.push_back(each[i]);
    }
    constexpr size_t kMaxGroups = 56;
    if (boxes.size() > kMaxGroups) {                                  // the smaller groups join the octant of their centre
        std::stable_sort(boxes.begin(), boxes.end(), [](const Box& a, const Box& b) { return a.count > b.count; });
        for (size_t i = kMaxGroups; i < boxes.size(); ++i) octants.push_back(boxes[i]);
        boxes.resize(kMaxGroups);
    }
    boxes.insert(boxes.end(), octants.begin(), octants.end());
    merge_by_least_added_volume<CoverBox>(boxes, (size_t)kLevel1Boxes, join);
    if (boxes.empty()) return false;                                  // no record: condition (4) is the stretch alone
    V.n = (int32_t)boxes.size();
    for (size_t j = 0; j < (size_t)kLevel1Boxes; ++j) {               // entries beyond n repeat the first: the kernel reads them all
        const Box& b = boxes[j < boxes.size() ? j : 0];
        V.r[j] = f_up(b.r + 2e-6); V.c[j] = f_up(b.c * (1.0 + 1e-5) + 1e-30);
        for (int k = 0; k < 3; ++k) { V.box[j][k] = f_down(b.lo[k]); V.box[j][3 + k] = f_up(b.hi[k]); }
        rmin[j] = (float)b.rmin;                                      // (a `reflective` value, exact)
    }
    return true;
}

// Condition (5)'s record (the lemma's mirror extension above), written wherever the cover is; n_panels = 0 where the condition is off.
// Panels: non-emissive triangles with `reflective` > 0 (one with 0 mirrors only when unit_float(n1) is 0) are grouped by (value,
// unit normal up to sign in steps of 1e-3, offset along it in steps of 1e-3 of the scene's extent); a group of at least two triangles
// with at least a thousandth of the non-emissive area is a panel when its members lie within 1e-3 of the extent of their common plane
// and their computed unit normals within 1e-3 of its normal.  Everything else goes to the rest boxes, one per value, merged by least
// added volume down to kLevel1Rest.  Any grouping is valid; this one finds the walls of a room.
// Fills M (which arrives as the record that turns condition (5) off) and returns whether the condition is on.
bool level1_mirror(const sq_scene& sc, const std::vector<DevSurf>& surfs, const std::vector<int32_t>& emitters, const std::vector<char>& emits,
                   const Level1Bounds& B, const Level1Cull& L, Level1Mirror& M) {
    const double u = kLemmaU, eps = kLemmaEps, omax = B.scene.omax, vmax = B.scene.vmax, extent = B.scene.extent;
    if (emitters.empty() || !(extent > 0.0)) return false;
    auto geom = [&](int32_t i) { return tri_geom(sc.tris[i], surfs[(size_t)i].reflective, omax); };
    // a group's members, and their area and area-weighted normal, summed in triangle order
    struct Group { std::vector<int32_t> tris; double area, n[3]; };
    std::map<std::array<int64_t, 5>, Group> groups;
    std::vector<int32_t> rest;
    double area_all = 0.0;
    for (int32_t i = 0; i < sc.n_tris; ++i) {
        if (emits[(size_t)i]) continue;
        const TriGeom t = geom(i);
        area_all += t.nn;
        const float val = t.reflective;
        if (!(val > 0.0f) || t.un_err >= 1.0) { rest.push_back(i); continue; }
        uint32_t vb; std::memcpy(&vb, &val, 4);
        const double d = t.un[0] * t.pts[0][0] + t.un[1] * t.pts[1][0] + t.un[2] * t.pts[2][0];
        Group& g = groups[{ (int64_t)vb, (int64_t)std::floor(t.un[0] * 1e3 + 0.5), (int64_t)std::floor(t.un[1] * 1e3 + 0.5), (int64_t)std::floor(t.un[2] * 1e3 + 0.5),
                            (int64_t)std::floor(d / (1e-3 * extent) + 0.5) }];
        g.tris.push_back(i); g.area += t.nn;
        for (int k = 0; k < 3; ++k) g.n[k] += t.nn * t.un[k];
    }
    // a panel: its plane n.x = d and half thickness h, delta and rho as the proof names them, and the join of its members' cover boxes
    struct Panel { double n[3], d, h, delta, rho; float val; CoverBox box; };
    std::vector<Panel> panels;
    for (auto& [key, g] : groups) {
        Panel p{}; p.val = surfs[(size_t)g.tris[0]].reflective;
        double lo = 1e300, hi = -1e300;
        const double len = length3(g.n);
        bool ok = g.tris.size() >= 2 && g.area >= 1e-3 * area_all && len > 0.5 * g.area;
        if (ok) {
            for (int k = 0; k < 3; ++k) p.n[k] = g.n[k] / len;
            for (size_t m = 0; m < g.tris.size(); ++m) {
                const TriGeom t = geom(g.tris[m]);
                for (int i = 0; i < 5; ++i) { const double s = p.n[0] * t.pts[0][i] + p.n[1] * t.pts[1][i] + p.n[2] * t.pts[2][i]; lo = std::min(lo, s); hi = std::max(hi, s); }
                const double dv[3] = { t.un[0] - p.n[0], t.un[1] - p.n[1], t.un[2] - p.n[2] };
                p.delta = std::max(p.delta, length3(dv) + t.un_err + 1e-12);
                p.rho = std::max(p.rho, t.rho);
                p.box = m ? join(p.box, cover_box(t, B.slab_slack)) : cover_box(t, B.slab_slack);
            }
            p.d = 0.5 * (lo + hi); p.h = 0.5 * (hi - lo) + 1e-12 * (vmax + 1.0);
            ok = p.delta <= 1e-3 && p.h <= 1e-3 * extent;
        }
        if (ok) panels.push_back(p);
        else rest.insert(rest.end(), g.tris.begin(), g.tris.end());
    }
    if (panels.empty() || panels.size() > (size_t)kLevel1Panels) return false;
    // the determinant floor and the emitters' margin at it: the floor that makes the margin 2e-3 of the emitters' extent
    double em_ext = std::max({ L.em_hi[0] - L.em_lo[0], L.em_hi[1] - L.em_lo[1], L.em_hi[2] - L.em_lo[2] });
    if (!(em_ext > 0.0)) em_ext = extent;
    const double a0 = std::max(eps, L.em_rho * eps / (2e-3 * em_ext)), m0 = L.em_rho * (eps / a0) + L.em_add;
    // W and err; nE = e2 x e1 of an emitter, as the determinant has it
    struct EmitterNormal { double n[3], len, E1, E2; };
    std::vector<EmitterNormal> ems;
    for (int32_t e : emitters) {
        const TriGeom t = geom(e);
        EmitterNormal en{}; cross3(t.e2, t.e1, en.n); en.len = length3(en.n); en.E1 = t.q.E1; en.E2 = t.q.E2;
        ems.push_back(en);
    }
    struct Wk { double w[3], len; };
    std::vector<Wk> ws;
    double err = 0.0;
    for (const Panel& p : panels) {
        const double kappa = 4.01 * p.delta + 16.0 * u;
        for (const EmitterNormal& en : ems) {
            const double f = 2.0 * (p.n[0] * en.n[0] + p.n[1] * en.n[1] + p.n[2] * en.n[2]);
            const double W[3] = { en.n[0] - f * p.n[0], en.n[1] - f * p.n[1], en.n[2] - f * p.n[2] };
            double dev = INFINITY; size_t at = ws.size();
            for (size_t k = 0; k < ws.size(); ++k) {
                double dp = 0.0, dm = 0.0;
                for (int c = 0; c < 3; ++c) { dp += (W[c] - ws[k].w[c]) * (W[c] - ws[k].w[c]); dm += (W[c] + ws[k].w[c]) * (W[c] + ws[k].w[c]); }
                const double dk = std::sqrt(std::min(dp, dm));
                if (dk <= 1e-4 * ws[k].len && dk < dev) { dev = dk; at = k; }
            }
            if (at == ws.size()) {
                Wk w{};
                for (int c = 0; c < 3; ++c) { w.w[c] = (double)(float)W[c]; w.len += w.w[c] * w.w[c]; }   // as the kernel will read it
                w.len = std::sqrt(w.len);
                dev = 2.0 * u * (en.len + w.len);
                ws.push_back(w);
            }
            err = std::max(err, 4.1 * u * ws[at].len + dev + kappa * en.len * 1.0001 + 17.7 * u * en.E1 * en.E2 + 1e-30);
        }
    }
    if (ws.size() > (size_t)kLevel1W) return false;
    // the boxes
    const double B_lo[3] = { L.em_lo[0] - m0, L.em_lo[1] - m0, L.em_lo[2] - m0 }, B_hi[3] = { L.em_hi[0] + m0, L.em_hi[1] + m0, L.em_hi[2] + m0 };
    bool finite_all = std::isfinite(a0) && std::isfinite(m0) && std::isfinite(err);
    for (size_t j = 0; j < panels.size(); ++j) {
        const Panel& p = panels[j]; const CoverBox& b = p.box;
        double corner = 0.0, far2 = 0.0;
        for (int k = 0; k < 3; ++k) {
            const double c = std::max(std::fabs(b.lo[k]), std::fabs(b.hi[k])), f = std::max(std::fabs(b.hi[k] - B_lo[k]), std::fabs(B_hi[k] - b.lo[k]));
            corner += c * c; far2 += f * f;
        }
        const double reach = omax + std::sqrt(corner);
        const double e1 = B.delta1 + 1.25 * b.c + b.r * reach + 2.01 * u * 1.3 * (reach + 1.25 * b.c);
        const double hX = p.h + p.rho * p.delta, kappa = 4.01 * p.delta + 16.0 * u;
        const double g = (e1 + 2.0 * hX + 1.01 * (std::sqrt(far2) + e1) * kappa) * (1.0 + 1e-9) + 1e-9 * (vmax + 1.0);
        double ilo[3] = { 1e300, 1e300, 1e300 }, ihi[3] = { -1e300, -1e300, -1e300 }, big = 0.0;
        for (int corner_i = 0; corner_i < 8; ++corner_i) {
            double x[3];
            for (int k = 0; k < 3; ++k) x[k] = (corner_i >> k & 1) ? B_hi[k] : B_lo[k];
            const double s = 2.0 * (p.n[0] * x[0] + p.n[1] * x[1] + p.n[2] * x[2] - p.d);
            for (int k = 0; k < 3; ++k) { const double y = x[k] - s * p.n[k]; ilo[k] = std::min(ilo[k], y); ihi[k] = std::max(ihi[k], y); }
        }
        for (int k = 0; k < 3; ++k) { ilo[k] -= g; ihi[k] += g; big = std::max({ big, std::fabs(ilo[k]), std::fabs(ihi[k]) }); }
        const double slack = 8.0 * u * (big + omax) * 1.001 + 1e-20;
        float* o = M.panel[j];
        for (int k = 0; k < 3; ++k) {
            o[k] = f_down(b.lo[k]); o[3 + k] = f_up(b.hi[k]); o[6 + k] = f_down(ilo[k] - slack); o[9 + k] = f_up(ihi[k] + slack);
            finite_all = finite_all && std::isfinite(o[k]) && std::isfinite(o[3 + k]) && std::isfinite(o[6 + k]) && std::isfinite(o[9 + k]);
        }
        o[12] = f_up(1.15 * b.c * (1.0 + 1e-5) + 1e-30); o[13] = p.val;
        finite_all = finite_all && std::isfinite(o[12]) && big <= 1048576.0;
    }
    // rest boxes: culling boxes (as the mirror classes') of everything non-emissive outside the panels, per value
    std::vector<CullBox> rb;
    for (int32_t i : rest) {
        const CullBox b = cull_box(sc.tris[i], surfs[(size_t)i].reflective, B.scene);
        size_t at = 0;
        while (at < rb.size() && rb[at].rmax != b.rmax) ++at;
        if (at == rb.size()) rb.push_back(b); else rb[at] = join(rb[at], b);
    }
    merge_by_least_added_volume<CullBox>(rb, (size_t)kLevel1Rest, join);
    for (size_t j = 0; j < (size_t)kLevel1Rest && !rb.empty(); ++j) {
        const CullBox& b = rb[j < rb.size() ? j : 0];
        for (int k = 0; k < 3; ++k) { M.rest[j][k] = f_down(b.lo[k]); M.rest[j][3 + k] = f_up(b.hi[k]); }
        M.rest[j][6] = (float)b.rmax;
    }
    if (!finite_all) return false;
    for (size_t j = panels.size(); j < (size_t)kLevel1Panels; ++j) std::memcpy(M.panel[j], M.panel[0], sizeof M.panel[0]);
    for (size_t k = 0; k < (size_t)kLevel1W; ++k)
        for (int c = 0; c < 3; ++c) M.w[k][c] = (float)ws[k < ws.size() ? k : 0].w[c];
    M.n_panels = (int32_t)panels.size(); M.n_rest = (int32_t)rb.size(); M.n_w = (int32_t)ws.size();
    M.thr2 = f_up((a0 + err) * (a0 + err) * (1.0 + 1e-5));
    M.d2lo = f_up((double)L.d2min * 1.01); M.d2hi = f_down((double)L.d2max * 0.99);
    M.a0 = f_up(a0); M.m0 = f_up(m0);
    return true;
}

// The three records and level1_zero of P, from the scene, P.surfs, P.emitters, P.n_emitters, P.cull_limits and the three flags
// (nonneg_materials, finite_geometry, finite materials).  A precondition that fails leaves the records as far as they had come, `on` = 0.
void build_level1(const sq_scene& sc, PackedScene& P, bool finite_materials) {
    Level1Cull& L = P.level1; L = Level1Cull{};
    std::vector<char> emits((size_t)sc.n_tris, 0);
    for (int32_t e : P.emitters) emits[(size_t)e] = 1;
    P.level1_zero = true;
    for (int32_t i = 0; i < sc.n_tris; ++i) {
        if (emits[(size_t)i]) continue;
        const DevSurf& d = P.surfs[(size_t)i];
        float l1[3]; static const float zero[3] = { 0.0f, 0.0f, 0.0f };
        for (int k = 0; k < 3; ++k) l1[k] = d.surf[k] * 0.0f + d.emit[k];     // level1_radiance's L1, the same fp32 operations
        if (std::memcmp(l1, zero, sizeof zero) != 0) P.level1_zero = false;
    }
    if (P.n_emitters < 0 || !P.nonneg_materials || !P.finite_geometry || !finite_materials || !P.level1_zero || !(P.cull_limits[0] >= 0.0f)) return;
    const double u = kLemmaU, eps = kLemmaEps;
    Level1Bounds B{};
    const SceneNorms& N = B.scene = scene_norms(sc);                            // as sq_cull_boxes
    // where p1 can be
    for (int32_t i = 0; i < sc.n_tris; ++i) {
        if (emits[(size_t)i]) continue;
        const TriNorms q = tri_norms(sc.tris[i]);
        if (!(q.P <= kLemmaPmax)) return;
        const double rho = lemma_rho(q, N.omax);
        B.g1 = std::max(B.g1, rho + 1.01 * (lemma_r(q) * (N.omax + N.vmax + rho) + rho));
    }
    B.delta1 = 4.0 * u * (2.0 * (N.vmax + B.g1) + N.omax) * (1.0 + 1e-6); B.R1 = N.vmax + B.g1 + B.delta1;
    if (!(B.R1 <= 1048576.0)) return;
    // the emitters' box and its margin
    double six = 0.0;
    for (int c = 0; c < 3; ++c) { L.em_lo[c] = P.emitters.empty() ? 0.0 : 1e300; L.em_hi[c] = P.emitters.empty() ? 0.0 : -1e300; }
    for (int32_t e : P.emitters) {
        const sq_tri& t = sc.tris[e];
        const TriNorms q = tri_norms(t);
        if (!(q.P <= kLemmaPmax)) return;
        L.em_rho = std::max(L.em_rho, 32.0 * (u / eps) * q.P * (B.R1 + q.V0 + q.E1 + q.E2));
        six = std::max(six, 6.0 * u * (q.E1 + q.E2));
        for (const float* v : { t.v0, t.v1, t.v2 })
            for (int c = 0; c < 3; ++c) {
                L.em_lo[c] = std::min(L.em_lo[c], (double)v[c]);
                L.em_hi[c] = std::max(L.em_hi[c], (double)v[c]);
            }
    }
    L.em_add = six + B.delta1 + 1e-20;
    // mirror classes: the scene's distinct `reflective` values, the largest kLevel1Classes - 1 on their own and the rest merged
    // upward into the lowest class (its box then holds every triangle)
    std::vector<float> vals;
    for (int32_t i = 0; i < sc.n_tris; ++i) vals.push_back(P.surfs[(size_t)i].reflective);
    std::sort(vals.begin(), vals.end()); vals.erase(std::unique(vals.begin(), vals.end()), vals.end());
    const size_t nv = vals.size(), nc = std::min<size_t>(nv, (size_t)kLevel1Classes);
    L.n_classes = (int32_t)nc;
    CullBox class_box[kLevel1Classes]; bool beyond[kLevel1Classes] = {};        // beyond: a member with P > 29, the box infinite
    for (size_t c = 0; c < nc; ++c) {
        L.class_val[c] = vals[nv - nc + c];
        class_box[c] = CullBox{ { INFINITY, INFINITY, INFINITY }, { -INFINITY, -INFINITY, -INFINITY }, 0.0 };   // empty until a triangle joins
    }
    for (int32_t i = 0; i < sc.n_tris; ++i) {                                   // one box per triangle, joined to every class that holds it
        const CullBox b = cull_box(sc.tris[i], P.surfs[(size_t)i].reflective, N);
        const bool out_of_reach = !(tri_norms(sc.tris[i]).P <= kLemmaPmax);
        for (size_t c = 0; c < nc; ++c) {
            if (!(P.surfs[(size_t)i].reflective >= (c == 0 ? vals[0] : L.class_val[c]))) continue;
            beyond[c] = beyond[c] || out_of_reach;
            grow_to_hold(class_box[c], b);
        }
    }
    for (size_t c = 0; c < nc; ++c)
        for (int k = 0; k < 3; ++k) {
            L.class_box[c][k] = beyond[c] ? -INFINITY : f_down(class_box[c].lo[k]); L.class_box[c][3 + k] = beyond[c] ? INFINITY : f_up(class_box[c].hi[k]);
        }
    L.o2max = P.cull_limits[0]; L.d2min = P.cull_limits[1]; L.d2max = P.cull_limits[2];
    L.on = 1;
    B.slab_slack = 8.0 * u * (N.vmax_inf * (1.0 + 1e-6) + B.g1 + N.omax) + 1e-20;
    Level1Cover V{}; Level1Mirror M{};                                          // M: off, until level1_mirror has succeeded
    if (!level1_cover(sc, P.surfs, emits, B, V, M.rmin)) return;
    P.level1_cover.assign(1, V);
    for (int j = 0; j < kLevel1Rest; ++j) M.rest[j][6] = -1.0f;                 // (an unused rest box applies to no sample)
    P.level1_mirror.assign(1, M);
    if (level1_mirror(sc, P.surfs, P.emitters, emits, B, L, M)) P.level1_mirror.assign(1, M);
}

}  // namespace
