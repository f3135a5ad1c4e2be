// sq_cull_lemma.h — the culling lemma and what rests on it alone: sq_cull_boxes and sq_half_outward (include/squigly_host.h).
// A part of the host translation unit (sq_host.cpp, which has the file map and the includes); not a header for anything else.
//
// ---- Culling boxes: an exact reduction of the triangle tests (no counterpart in the reference) ----------------------
// A Leaf equation (src/BIH.hs:105-109) returns Nothing unless mollerTrumbore accepts one of its triangles.  The BIH only
// clips along split axes, so most leaves a ray visits are far from it: sq_cull_boxes() gives every node a box such that
//
//     a ray within the limits below whose fp32 mollerTrumbore (src/Geometry.hs:117-142, round-to-nearest, no FMA)
//     ACCEPTS some triangle of the node  ==>  the ray passes the fp32 slab test of the node's box,
//
// so a ray that fails the slab test can skip the node's triangles and the node still returns exactly what the reference
// returns (Nothing).  The box is the triangles' bounding box grown by a margin m that covers the rounding of the
// accepted test.  Derivation (u = 2^-24, eps = 0.0001f, s = o - v0, E1 = |e1|, E2 = |e2|, D >= |d|, S >= |s|, P = E1 E2 D;
// h = d x e2, a = e1.h, Nu = s.h, q = s x e1, Nv = d.q, Nt = e2.q; hats are the computed values):
//   |h^ - h|_2 <= 3.5u D E2 (two products and a difference per component), dot products are within 3.01u |x||y|, so
//   |a^ - a| <= 7u P,  |Nu^ - Nu| <= 8u S D E2,  |Nv^ - Nv| <= 8u S D E1,  |Nt^ - Nt| <= 8u S E1 E2.
//   Acceptance means |a^| >= eps, 0 <= u^ <= 1, 0 <= v^, u^ + v^ <= 1 (+u), t^ > eps.  With r = 7uP/eps <= 1/8 (P <= 29)
//   a and a^ have one sign and the exact solution (u, v, t) of  o + t d = v0 + u e1 + v e2  satisfies
//   |u - u^| <= 1.15 (r + 8u S D E2/eps) + 2.01u, the same for v with E1, and t > -1.15 * 8u S E1 E2 / eps.
//   So the point X = v0 + u e1 + v e2 lies on the ray's LINE at parameter t and within |u-u^| E1 + |v-v^| E2 of the
//   triangle; if t < 0 the origin is within |t| D of X.  Either way a point of the ray with t >= 0 lies within
//       rho = 28 (u/eps) P (S + E1 + E2) + 5u (E1 + E2)
//   of the triangle (the last term also covers e1 = fl(v1 - v0)).  The margin uses 32 and 6.
//   Slab test: with df = fl(1/d), nodf = fl(-o df) and plane value fma(l, df, nodf) (or fl(fl(l - o) df)) every plane
//   value is within 4u (|l| + |o|)/|d_k| of the exact one, so growing the box by a further 8u (|l| + |o|) makes every
//   computed interval contain the exact interval of the rho-box with room to spare: an exact hit of the rho-box passes
//   `tmax > 0 && tmin < tmax`.  Subnormal results add at most 2^-149 per operation, far below the floor added at the end.
// Limits under which this holds (rays outside them are simply not culled; leaves outside them get an infinite box):
//   every coordinate finite and <= 2^20 in magnitude (no overflow anywhere in the test), P <= 29 for every triangle of
//   the leaf, 0.25 <= |d|^2 <= 1.5624 (primary rays have |d| <= 1.2248, bounce rays |d| = 1 or the incoming length), |o|^2 <= o2max
//   = (2 max|vertex|)^2, and o, d, 1/d, o/d finite.
// Branch nodes: the box of a branch is the union (componentwise min / max) of its children's boxes, so each of its planes IS
//   a plane of some leaf box below it, slack included.  A ray that mollerTrumbore accepts for a triangle of leaf L hits L's
//   rho-box exactly; the union contains that box with L's slack or more on every side (a union plane sits further out by
//   some Delta >= 0, which adds Delta of slack against 4u Delta / |d_k| of additional plane-value error), so the computed
//   intervals of the union box contain the exact ones of L's rho-box and the ray passes the union's slab test as well.  Hence
//   "misses the box of a subtree" implies "misses the box of every leaf below", and the whole subtree returns Nothing.
// tests/test_cull.py searches for violations with adversarial grazing rays against exact (binary64 / rational) geometry: the
// leaf box and the box of every ancestor, in fp32 and in the binary16 encoding, plane values as single-rounding FMAs.
namespace {
inline float f_down(double x) { float f = (float)x; if ((double)f > x) f = std::nextafterf(f, -INFINITY); return f; }
inline float f_up(double x) { float f = (float)x; if ((double)f < x) f = std::nextafterf(f, INFINITY); return f; }
constexpr double kLemmaU = 5.9604644775390625e-8, kLemmaD = 1.25, kLemmaPmax = 29.0;
const double kLemmaEps = (double)0.0001f;
// The lengths the derivation above names, of one triangle: E1 = |e1|, E2 = |e2| (the kernels' rounded edges), V0 = |v0|, P = E1 E2 D.
struct TriNorms { double E1, E2, V0, P; };
inline TriNorms tri_norms(const sq_tri& t) {
    double E1 = 0, E2 = 0, V0 = 0;
    for (int c = 0; c < 3; ++c) {
        const float e1 = t.v1[c] - t.v0[c], e2 = t.v2[c] - t.v0[c];        // the kernels' edges (src/Geometry.hs:130-131)
        E1 += (double)e1 * e1; E2 += (double)e2 * e2; V0 += (double)t.v0[c] * t.v0[c];
    }
    E1 = std::sqrt(E1); E2 = std::sqrt(E2); V0 = std::sqrt(V0);
    return TriNorms{ E1, E2, V0, E1 * E2 * kLemmaD };
}
// rho (with the margin's 32 and 6) for rays whose origin lies within `reach` of the coordinate origin, so that S <= reach + V0
inline double lemma_rho(const TriNorms& q, double reach) {
    return 32.0 * (kLemmaU / kLemmaEps) * q.P * (reach + q.V0 + q.E1 + q.E2) + 6.0 * kLemmaU * (q.E1 + q.E2);
}
// The margin of a culling box: rho (or the largest of a leaf) and the slab test's own rounding, 8u (|l| + |o|) with |l| <= vmax_inf + rho
inline double cull_margin(double rho, double vmax_inf, double omax) { return rho + (8.0 * kLemmaU * (vmax_inf + rho + omax) + 1e-20); }
// What the lemma takes from the scene as a whole, over every vertex: the largest |coordinate| and |vertex|, omax = the bound on |o| the
// ray limits state (2 vmax, a hair more), and the bounds with their longest side (no triangles: inverted bounds, a negative extent).
// finite = false at the first coordinate that is not finite; the other values are then not to be used.
struct SceneNorms { bool finite; double vmax_inf, vmax, omax, lo[3], hi[3], extent; };
inline SceneNorms scene_norms(const sq_scene& sc) {
    SceneNorms N{ true, 0.0, 0.0, 0.0, { 1e300, 1e300, 1e300 }, { -1e300, -1e300, -1e300 }, 0.0 };
    double vmax2 = 0.0;
    for (int32_t i = 0; i < sc.n_tris; ++i)
        for (const float* v : { sc.tris[i].v0, sc.tris[i].v1, sc.tris[i].v2 }) {
            double q = 0.0;
            for (int c = 0; c < 3; ++c) {
                if (!(v[c] - v[c] == 0.0f)) { N.finite = false; return N; }
                N.vmax_inf = std::max(N.vmax_inf, std::fabs((double)v[c])); q += (double)v[c] * v[c];
                N.lo[c] = std::min(N.lo[c], (double)v[c]); N.hi[c] = std::max(N.hi[c], (double)v[c]);
            }
            vmax2 = std::max(vmax2, q);
        }
    N.vmax = std::sqrt(vmax2); N.omax = 2.0 * N.vmax * (1.0 + 1e-12);
    N.extent = std::max({ N.hi[0] - N.lo[0], N.hi[1] - N.lo[1], N.hi[2] - N.lo[2] });
    return N;
}
}
extern "C" int sq_cull_boxes(const sq_scene* sc, float* boxes, float ray_limits[3]) {
    if (!sc || !boxes || !ray_limits) return sq_set_error("null argument");
    const int32_t n = sc->n_nodes;
    const float inf = INFINITY;
    auto disable = [&]() { for (int32_t i = 0; i < n; ++i) { float* b = boxes + 6 * (size_t)i; b[0] = b[1] = b[2] = -inf; b[3] = b[4] = b[5] = inf; }
                           ray_limits[0] = -1.0f; ray_limits[1] = 0.25f; ray_limits[2] = 1.5624f; return 0; };
    const SceneNorms N = scene_norms(*sc);
    if (!N.finite || sc->n_tris == 0 || N.vmax_inf > 1048576.0) return disable();
    ray_limits[0] = f_down(N.omax * N.omax * (1.0 - 1e-6)); ray_limits[1] = 0.25f; ray_limits[2] = 1.5624f;
    for (int32_t i = n - 1; i >= 0; --i) {                          // children come after their parent in pre-order
        const sq_node& nd = sc->nodes[i];
        float* b = boxes + 6 * (size_t)i;
        if ((nd.kind & 3) != 3) {
            const float* l = boxes + 6 * (size_t)(i + 1); const float* r = boxes + 6 * (size_t)nd.link;
            for (int c = 0; c < 3; ++c) { b[c] = std::min(l[c], r[c]); b[3 + c] = std::max(l[3 + c], r[3 + c]); }
            continue;
        }
        const int32_t first = nd.link, cnt = nd.kind >> 2;
        double lo[3] = { 1e300, 1e300, 1e300 }, hi[3] = { -1e300, -1e300, -1e300 }, m = 0.0; bool ok = cnt > 0;
        for (int32_t k = first; k < first + cnt && ok; ++k) {
            const sq_tri& t = sc->tris[k];
            for (int c = 0; c < 3; ++c)
                for (const float* v : { t.v0, t.v1, t.v2 }) { lo[c] = std::min(lo[c], (double)v[c]); hi[c] = std::max(hi[c], (double)v[c]); }
            const TriNorms q = tri_norms(t);
            if (!(q.P <= kLemmaPmax)) { ok = false; break; }
            m = std::max(m, lemma_rho(q, N.omax));
        }
        if (!ok) { b[0] = b[1] = b[2] = -inf; b[3] = b[4] = b[5] = inf; continue; }
        m = cull_margin(m, N.vmax_inf, N.omax);                       // one margin, the leaf's largest, on the joint bounds
        for (int c = 0; c < 3; ++c) { b[c] = f_down(lo[c] - m); b[3 + c] = f_up(hi[c] + m); }
    }
    return 0;
}

// The binary16 value nearest to x on the side asked for (up: >= x, else <= x), never a subnormal: +-2^-14 or zero instead,
// so that the device's handling of binary16 denormals cannot matter.  NaN gives the infinity of that side.
extern "C" uint32_t sq_half_outward(float x, int32_t up_) {
    const bool up = up_ != 0;
    if (!(x == x)) return up ? 0x7C00u : 0xFC00u;
    const bool neg = std::signbit(x); const double ax = std::fabs((double)x);
    const bool mag_up = up != neg;                           // round the magnitude away from zero?
    uint32_t hb;
    if (ax == 0.0) hb = 0;
    else if (ax > 65504.0) hb = (mag_up || std::isinf(ax)) ? 0x7C00u : 0x7BFFu;
    else if (ax < 6.103515625e-05) hb = mag_up ? 0x0400u : 0u;
    else {
        int e; const double mant = std::frexp(ax, &e) * 2.0; e -= 1;     // ax = mant * 2^e, mant in [1, 2)
        const double m10 = mant * 1024.0 - 1024.0; const double fl = std::floor(m10);
        uint32_t q = (uint32_t)fl + ((mag_up && fl != m10) ? 1u : 0u);
        if (q == 1024u) { q = 0; ++e; }
        hb = e > 15 ? 0x7C00u : (((uint32_t)(e + 15) << 10) | q);
    }
    return neg ? (hb | 0x8000u) : hb;
}
