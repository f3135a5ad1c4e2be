// sq_host.cpp — host side above the render boundary: .obj/.sq/camera loaders and the BIH
// build + flatten, with the reference's arithmetic (include/squigly_host.h); and, below it, the
// culling boxes and the scene packer (sq_pack.h), the host half of sq_scene_upload.  No HIP anywhere.
//
// Array-based and O(n log n): the reference's list code (`!!` indexing, src/Obj.hs:83-85) is
// O(n^2) and cannot load the 1M-triangle configuration.  Tree shape, split planes and leaf
// order are bit-identical to src/BIH.hs because they decide traversal tie-breaks.
// Citations are relative to the reference repository root.
#include "../../include/squigly_host.h"
#include "sq_error.h"
#include "sq_host_types.h"
#include "sq_math.h"
#include "sq_pack.h"
#include "sq_plan.h"

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <unordered_map>
#include <vector>

using sq::f3;

// ----------------------------------------------------------------------------------------------
// Text scanning.  The reference grammar is Parsec (src/Obj.hs:96-171); this scanner accepts and
// rejects the same byte strings.  Malformed numbers, which the reference turns into lazy `read`
// failures, are reported as errors up front.
// ----------------------------------------------------------------------------------------------
namespace {

struct Scanner {
    const char* s; size_t n; size_t i = 0;
    Scanner(const char* p, size_t len) : s(p), n(len) {}
    int peek() const { return i < n ? (unsigned char)s[i] : -1; }
    static bool ws(int c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r' || c == '\f' || c == '\v'; }
    static bool digit(int c) { return c >= '0' && c <= '9'; }
    static bool alnum(int c) { return digit(c) || (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z'); }
    void skip_ws() { while (ws(peek())) ++i; }
    // Parsec `string`: returns 0 on match, 1 on failure with nothing consumed, 2 on failure after consuming
    int literal(const char* lit) {
        for (size_t k = 0; lit[k]; ++k) {
            if (peek() != (unsigned char)lit[k]) return k == 0 ? 1 : 2;
            ++i;
        }
        return 0;
    }
    // fractional (src/Obj.hs:115-121): -?digit*(.digit*)? then `read`, which needs digits on both sides of '.'
    bool number(float& out) {
        std::string tok;
        if (peek() == '-') { tok.push_back('-'); ++i; }
        size_t a = 0, b = 0; bool dot = false;
        while (digit(peek())) { tok.push_back((char)peek()); ++i; ++a; }
        if (peek() == '.') { tok.push_back('.'); ++i; dot = true; }
        while (digit(peek())) { tok.push_back((char)peek()); ++i; ++b; }
        if (a == 0 || (dot && b == 0)) { sq_set_error("no parse for number '%s' at byte %zu", tok.c_str(), i); return false; }
        out = std::strtof(tok.c_str(), nullptr);   // correctly rounded, like read/fromRational
        return true;
    }
    bool vec3(float v[3]) {                          // src/Obj.hs:166-171
        for (int k = 0; k < 3; ++k) { if (!number(v[k])) return false; skip_ws(); }
        return true;
    }
    bool word(std::string& out) {                    // src/Obj.hs:129-130
        out.clear();
        while (peek() >= 0 && !ws(peek())) { out.push_back((char)peek()); ++i; }
        if (out.empty()) { sq_set_error("expected a word at byte %zu", i); return false; }
        skip_ws();
        return true;
    }
};

struct ObjObject { std::string mtl; size_t face_begin, face_end, vert_end; };   // vert_end: vertices read up to and including this object
struct ObjFile {
    std::string mtllib;
    std::vector<f3> verts;                 // all objects' vertices, concatenated (src/Obj.hs:76)
    std::vector<int32_t> faces;            // 3 one-based indices per face
    std::vector<ObjObject> objects;
};

bool scan_obj(const char* text, size_t len, ObjFile& f) {
    Scanner sc(text, len);
    if (sc.literal("mtllib")) { sq_set_error("obj: expected 'mtllib' at byte %zu", sc.i); return false; }   // src/Obj.hs:126-127
    sc.skip_ws();
    if (!sc.word(f.mtllib)) return false;
    while (sc.peek() == 'o') {                                                                              // many parseObj, src/Obj.hs:97-103
        ++sc.i; sc.skip_ws();
        size_t name_len = 0;
        while (Scanner::alnum(sc.peek()) || sc.peek() == '.' || sc.peek() == '_') { ++sc.i; ++name_len; }  // src/Obj.hs:105-107
        if (!name_len) { sq_set_error("obj: empty object name at byte %zu", sc.i); return false; }
        sc.skip_ws();
        while (sc.peek() == 'v') {                                                                          // src/Obj.hs:109-110
            ++sc.i; sc.skip_ws();
            float v[3];
            if (!sc.vec3(v)) return false;
            f.verts.push_back(sq::mk(v[0], v[2], v[1]));                                                    // swapYZ, src/Obj.hs:112-113
        }
        if (sc.literal("usemtl")) { sq_set_error("obj: expected 'usemtl' at byte %zu", sc.i); return false; } // src/Obj.hs:123-124
        sc.skip_ws();
        ObjObject ob;
        ob.vert_end = f.verts.size();
        if (!sc.word(ob.mtl)) return false;
        if (sc.peek() == 's') {                                                                             // optional parseS, src/Obj.hs:132-133
            size_t mark = sc.i;
            if (sc.literal("s on")) {
                sc.i = mark;
                if (sc.literal("s off")) { sq_set_error("obj: bad 's' line at byte %zu", sc.i); return false; }
            }
            sc.skip_ws();
        }
        ob.face_begin = f.faces.size() / 3;
        while (sc.peek() == 'f') {                                                                          // src/Obj.hs:135-144
            ++sc.i; sc.skip_ws();
            for (int k = 0; k < 3; ++k) {
                if (!Scanner::digit(sc.peek())) { sq_set_error("obj: expected a face index at byte %zu", sc.i); return false; }
                long long v = 0;
                while (Scanner::digit(sc.peek())) { v = v * 10 + (sc.peek() - '0'); if (v > 2000000000LL) v = 2000000000LL; ++sc.i; }
                sc.skip_ws();
                f.faces.push_back((int32_t)v);
            }
        }
        ob.face_end = f.faces.size() / 3;
        f.objects.push_back(ob);
    }
    return true;
}

bool scan_sq(const char* text, size_t len, std::vector<std::string>& names, std::vector<sq_material>& mats) {  // src/Obj.hs:146-161
    Scanner sc(text, len);
    for (;;) {
        int r = sc.literal("newmtl ");
        if (r == 1) break;
        if (r == 2) { sq_set_error("sq: expected 'newmtl ' at byte %zu", sc.i); return false; }
        std::string name; sq_material m;
        if (!sc.word(name)) return false;
        sc.skip_ws();
        if (sc.literal("reflective ")) { sq_set_error("sq: expected 'reflective ' at byte %zu", sc.i); return false; }
        if (!sc.number(m.reflective)) return false;
        sc.skip_ws();
        if (!sc.vec3(m.surf)) return false;
        sc.skip_ws();
        if (sc.literal("emissive ")) { sq_set_error("sq: expected 'emissive ' at byte %zu", sc.i); return false; }
        if (!sc.number(m.emissive)) return false;
        sc.skip_ws();
        if (!sc.vec3(m.emit)) return false;
        sc.skip_ws();
        names.push_back(name); mats.push_back(m);
    }
    return true;
}

// ---- Haskell's derived Show text, for --debug (src/Obj.hs:55-57) ----
// show :: Float -> String (Numeric.showFloat): the shortest digits that identify the value; positional notation for
// 0.1 <= |x| < 10^7, otherwise d.ddde<n>; always a digit on both sides of the point.
std::string show_float(float x) {
    if (x != x) return "NaN";
    if (x - x != 0.0f) return x > 0 ? "Infinity" : "-Infinity";
    std::string out;
    uint32_t bits; std::memcpy(&bits, &x, 4);
    if (bits >> 31) { out = "-"; x = -x; }
    if (x == 0.0f) return out + "0.0";
    char buf[48]; std::string digits; int e10 = 0;
    for (int p = 1; p <= 9; ++p) {                      // shortest correctly rounded decimal that reads back as x
        std::snprintf(buf, sizeof buf, "%.*e", p - 1, (double)x);
        if (std::strtof(buf, nullptr) == x || p == 9) {
            digits.clear();
            const char* c = buf;
            for (; *c && *c != 'e'; ++c) if (*c >= '0' && *c <= '9') digits.push_back(*c);
            e10 = std::atoi(c + 1) + 1;                 // x = 0.d1d2... * 10^e10 (floatToDigits' convention)
            break;
        }
    }
    while (digits.size() > 1 && digits.back() == '0') digits.pop_back();
    if (e10 < 0 || e10 > 7) {                           // exponent form (formatRealFloat FFGeneric: e < 0 || e > 7)
        out += digits.substr(0, 1) + "." + (digits.size() > 1 ? digits.substr(1) : std::string("0")) + "e" + std::to_string(e10 - 1);
        return out;
    }
    std::string ip = digits.substr(0, std::min<size_t>((size_t)e10, digits.size()));
    ip.append((size_t)e10 - ip.size(), '0');
    if (ip.empty()) ip = "0";
    std::string fp = digits.size() > (size_t)e10 ? digits.substr((size_t)e10) : std::string("0");
    return out + ip + "." + fp;
}
std::string show_v3(const float v[3]) {                 // V3 {_x = .., _y = .., _z = ..}  (src/V3.hs:5)
    return "V3 {_x = " + show_float(v[0]) + ", _y = " + show_float(v[1]) + ", _z = " + show_float(v[2]) + "}";
}
// show :: String -> String, i.e. showList over GHC.Show.showLitChar.  The reference reads its files with readFile, which
// decodes them (UTF-8 in any modern locale) to code points before the parser sees them: a name is shown per CODE POINT.
//   > '\DEL'  -> \ddd (decimal), followed by \& if a digit comes next      '\DEL' -> \DEL      '\\' -> \\     '"' -> \"
//   >= ' '    -> itself              \a \b \f \n \r \t \v by letter            \SO -> \SO, followed by \& if an 'H' comes next
//   other control characters by their ASCII names (\NUL \SOH ... \US)
// A byte sequence that is not valid UTF-8 makes the reference's readFile throw; here each such byte is shown as the code
// point of the same number (Latin-1), which no test can pin.
std::string show_string(const std::string& t) {
    static const char* const kAscii[32] = { "NUL", "SOH", "STX", "ETX", "EOT", "ENQ", "ACK", "a", "b", "t", "n", "v", "f", "r", "SO", "SI",
                                            "DLE", "DC1", "DC2", "DC3", "DC4", "NAK", "SYN", "ETB", "CAN", "EM", "SUB", "ESC", "FS", "GS", "RS", "US" };
    std::vector<uint32_t> cps;
    for (size_t i = 0; i < t.size();) {                  // UTF-8 -> code points (shortest form, no surrogates, <= U+10FFFF)
        const unsigned char c = (unsigned char)t[i];
        int n = c < 0x80 ? 1 : (c >> 5) == 6 ? 2 : (c >> 4) == 14 ? 3 : (c >> 3) == 30 ? 4 : 0;
        uint32_t cp = n == 1 ? c : n == 2 ? (c & 0x1fu) : n == 3 ? (c & 0x0fu) : (c & 0x07u);
        bool ok = n > 0 && i + (size_t)n <= t.size();
        for (int k = 1; ok && k < n; ++k) { const unsigned char d = (unsigned char)t[i + (size_t)k]; ok = (d >> 6) == 2; cp = (cp << 6) | (d & 0x3fu); }
        static const uint32_t kMin[5] = { 0, 0, 0x80, 0x800, 0x10000 };
        if (ok && (cp < kMin[n] || cp > 0x10ffffu || (cp >= 0xd800u && cp <= 0xdfffu))) ok = false;
        if (!ok) { cps.push_back(c); ++i; } else { cps.push_back(cp); i += (size_t)n; }
    }
    std::string o = "\"";
    for (size_t i = 0; i < cps.size(); ++i) {
        const uint32_t c = cps[i];
        const uint32_t next = i + 1 < cps.size() ? cps[i + 1] : 0;
        if (c > 127) { o += "\\" + std::to_string(c); if (next >= '0' && next <= '9') o += "\\&"; }
        else if (c == 127) o += "\\DEL";
        else if (c == '"') o += "\\\"";
        else if (c == '\\') o += "\\\\";
        else if (c >= 32) o.push_back((char)c);
        else { o += std::string("\\") + kAscii[c]; if (c == 14 && next == 'H') o += "\\&"; }
    }
    return o + "\"";
}

bool read_file(const char* path, std::string& out) {
    FILE* fp = std::fopen(path, "rb");
    if (!fp) { sq_set_error("cannot open '%s'", path); return false; }
    char buf[1 << 16]; size_t got;
    out.clear();
    while ((got = std::fread(buf, 1, sizeof buf, fp)) > 0) out.append(buf, got);
    std::fclose(fp);
    return true;
}

}  // namespace

extern "C" int sq_mesh_from_text(const char* obj_text, size_t obj_len, const char* sq_text, size_t sq_len, sq_mesh** out) {
    if (!obj_text || !sq_text || !out) return sq_set_error("null argument");
    ObjFile f; std::vector<std::string> names; std::vector<sq_material> mats;
    if (!scan_obj(obj_text, obj_len, f)) return 1;
    if (!scan_sq(sq_text, sq_len, names, mats)) return 1;
    sq_mesh* m = new sq_mesh;
    m->mats = mats;
    if (!f.objects.empty()) {                           // print (head objs): Object {verts = [..], mtl = "..", faces = [..]}  (src/Obj.hs:88-94)
        const ObjObject& ob = f.objects[0];
        std::string t = "Object {verts = [";
        for (size_t i = 0; i < ob.vert_end; ++i) { const float v[3] = { f.verts[i].x, f.verts[i].y, f.verts[i].z }; t += (i ? "," : "") + show_v3(v); }
        t += "], mtl = " + show_string(ob.mtl) + ", faces = [";
        for (size_t fi = ob.face_begin; fi < ob.face_end; ++fi)
            t += std::string(fi > ob.face_begin ? "," : "") + "Face {_i1 = " + std::to_string(f.faces[3 * fi]) + ", _i2 = " + std::to_string(f.faces[3 * fi + 1]) +
                 ", _i3 = " + std::to_string(f.faces[3 * fi + 2]) + "}";
        m->show_first_object = t + "]}";
    }
    m->show_materials = "[";                            // print mats :: [(String, Material)]  (src/Color.hs:78-83)
    for (size_t i = 0; i < names.size(); ++i)
        m->show_materials += std::string(i ? "," : "") + "(" + show_string(names[i]) + ",Mat {reflective = " + show_float(mats[i].reflective) + ", surfColor = " +
                             show_v3(mats[i].surf) + ", emissive = " + show_float(mats[i].emissive) + ", emitColor = " + show_v3(mats[i].emit) + "})";
    m->show_materials += "]";
    // makeScene (src/Obj.hs:73-77): every (object, material) pair with equal names, objects outermost.
    for (const ObjObject& ob : f.objects)
        for (size_t mi = 0; mi < names.size(); ++mi) {
            if (ob.mtl != names[mi]) continue;
            for (size_t fi = ob.face_begin; fi < ob.face_end; ++fi) {                    // makeTris, src/Obj.hs:80-86
                sq_tri t;
                float* dst[3] = { t.v0, t.v1, t.v2 };
                for (int k = 0; k < 3; ++k) {
                    int32_t idx = f.faces[3 * fi + k];
                    if (idx < 1 || (size_t)idx > f.verts.size()) {
                        delete m;
                        return sq_set_error("obj: face index %d outside 1..%zu", idx, f.verts.size());
                    }
                    f3 v = f.verts[(size_t)idx - 1];
                    dst[k][0] = v.x; dst[k][1] = v.y; dst[k][2] = v.z;
                }
                t.mat = (int32_t)mi;
                m->tris.push_back(t);
            }
        }
    *out = m;
    return 0;
}

extern "C" int sq_mesh_from_obj(const char* obj_path, const char* mtl_dir, sq_mesh** out) {
    if (!obj_path || !mtl_dir || !out) return sq_set_error("null argument");
    std::string obj, sqt;
    if (!read_file(obj_path, obj)) return 1;
    ObjFile probe;
    {   // only the first line is needed to find the material file (src/Obj.hs:51-52)
        Scanner sc(obj.data(), obj.size());
        if (sc.literal("mtllib")) return sq_set_error("obj: expected 'mtllib' at byte %zu", sc.i);
        sc.skip_ws();
        if (!sc.word(probe.mtllib)) return 1;
    }
    std::string path = std::string(mtl_dir) + "/" + probe.mtllib;
    if (!read_file(path.c_str(), sqt)) return 1;
    return sq_mesh_from_text(obj.data(), obj.size(), sqt.data(), sqt.size(), out);
}

extern "C" int sq_mesh_from_arrays(const sq_tri* tris, int32_t n_tris, const sq_material* mats, int32_t n_mats, sq_mesh** out) {
    if ((!tris && n_tris) || (!mats && n_mats) || !out || n_tris < 0 || n_mats < 0) return sq_set_error("bad argument");
    for (int32_t i = 0; i < n_tris; ++i)
        if (tris[i].mat < 0 || tris[i].mat >= n_mats) return sq_set_error("triangle %d has material %d outside 0..%d", i, tris[i].mat, n_mats - 1);
    sq_mesh* m = new sq_mesh;
    m->tris.assign(tris, tris + n_tris);
    m->mats.assign(mats, mats + n_mats);
    *out = m;
    return 0;
}
extern "C" int32_t sq_mesh_num_tris(const sq_mesh* m) { return (int32_t)m->tris.size(); }
extern "C" int32_t sq_mesh_num_materials(const sq_mesh* m) { return (int32_t)m->mats.size(); }
extern "C" const sq_tri* sq_mesh_tris(const sq_mesh* m) { return m->tris.data(); }
extern "C" const sq_material* sq_mesh_materials(const sq_mesh* m) { return m->mats.data(); }
extern "C" void sq_mesh_free(sq_mesh* m) { delete m; }
extern "C" void sq_mesh_debug_show(const sq_mesh* m, const char** first_object, const char** materials) {
    if (first_object) *first_object = m ? m->show_first_object.c_str() : "";
    if (materials) *materials = m ? m->show_materials.c_str() : "";
}

// ----------------------------------------------------------------------------------------------
// Camera (src/Obj.hs:60-70, src/Geometry.hs:90-107)
// ----------------------------------------------------------------------------------------------
namespace {
// Data.Matrix product: every entry is a dot product folded from a zero accumulator, r <- a*b + r.
void mul3(const float a[9], const float b[9], float o[9]) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            float r = 0.0f;
            for (int k = 0; k < 3; ++k) r = a[3 * i + k] * b[3 * k + j] + r;
            o[3 * i + j] = r;
        }
}
}  // namespace

extern "C" void sq_rot_matrix_rads(float alp, float bet, float gam, float out9[9]) {
    float sa, ca, sb, cb, sg, cg;
    sq::fsincos(alp, sa, ca); sq::fsincos(bet, sb, cb); sq::fsincos(gam, sg, cg);
    const float rz[9] = { ca, -sa, 0, sa, ca, 0, 0, 0, 1 };
    const float ry[9] = { cb, 0, sb, 0, 1, 0, -sb, 0, cb };
    const float rx[9] = { 1, 0, 0, 0, cg, -sg, 0, sg, cg };
    float yx[9];
    mul3(ry, rx, yx);            // foldr1 (*): rz * (ry * rx)
    mul3(rz, yx, out9);
}
extern "C" int sq_camera_from_text(const char* text, size_t len, sq_camera* cam) {
    if (!text || !cam) return sq_set_error("null argument");
    Scanner sc(text, len);
    float p[3], e[3];
    if (!sc.vec3(p) || !sc.vec3(e)) return 1;
    std::memcpy(cam->pos, p, sizeof p);
    sq_rot_matrix_rads(e[0], e[1], e[2], cam->rot);
    return 0;
}
extern "C" int sq_camera_from_file(const char* path, sq_camera* cam) {
    std::string t;
    if (!path || !read_file(path, t)) return path ? 1 : sq_set_error("null argument");
    return sq_camera_from_text(t.data(), t.size(), cam);
}

// ----------------------------------------------------------------------------------------------
// BIH build (src/BIH.hs:62-99) straight into pre-order arrays.
// ----------------------------------------------------------------------------------------------
namespace {

struct Builder {
    const std::vector<sq_tri>& src;
    sq_bih& out;
    std::vector<int32_t> scratch;

    static const float* vert(const sq_tri& t, int k) { return k == 0 ? t.v0 : (k == 1 ? t.v1 : t.v2); }

    // boundingBox = getBounds . concatMap vertices (src/Geometry.hs:155-163,195-197): foldl1 min / max
    sq_bounds bounds_of(const int32_t* ids, size_t n) const {
        sq_bounds b; bool first = true;
        for (size_t i = 0; i < n; ++i)
            for (int k = 0; k < 3; ++k) {
                const float* v = vert(src[(size_t)ids[i]], k);
                if (first) { for (int c = 0; c < 3; ++c) b.lo[c] = b.hi[c] = v[c]; first = false; }
                else for (int c = 0; c < 3; ++c) { b.lo[c] = sq::hmin(b.lo[c], v[c]); b.hi[c] = sq::hmax(b.hi[c], v[c]); }
            }
        if (first) for (int c = 0; c < 3; ++c) b.lo[c] = b.hi[c] = 0.0f;
        return b;
    }
    // longestAxis (src/Geometry.hs:190-193): maximumBy keeps the later of equal maxima
    static int longest_axis(const sq_bounds& b) {
        int best = 0;
        for (int c = 1; c < 3; ++c) {
            float cur = b.hi[best] - b.lo[best], cand = b.hi[c] - b.lo[c];
            if (!sq::cmp_gt(cur, cand)) best = c;
        }
        return best;
    }
    // averagePoints (vertices tri), one component (src/Geometry.hs:181-182)
    float centroid(const sq_tri& t, int ax) const { return (((0.0f + t.v0[ax]) + t.v1[ax]) + t.v2[ax]) / 3.0f; }

    int32_t emit_leaf(const int32_t* ids, size_t n, int depth) {
        sq_node nd; nd.kind = 3 | ((int32_t)n << 2); nd.lmax = 0; nd.rmin = 0; nd.link = (int32_t)out.tris.size();
        for (size_t i = 0; i < n; ++i) out.tris.push_back(src[(size_t)ids[i]]);
        out.nodes.push_back(nd);
        out.leaves++;
        if ((int32_t)n > out.longest) out.longest = (int32_t)n;
        if (depth > out.height) out.height = depth;
        return (int32_t)out.nodes.size() - 1;
    }

    // bih bbox geom (src/BIH.hs:67-80); ids[0..n) is reordered in place (stable partition)
    void build(const sq_bounds& bbox, int32_t* ids, size_t n, int depth) {
        if (n < 15) { emit_leaf(ids, n, depth); return; }
        // split (src/BIH.hs:82-99)
        const int ax = longest_axis(bbox);
        std::vector<float> cen(n);
        float sum = 0.0f, count = 0.0f;
        for (size_t i = 0; i < n; ++i) { cen[i] = centroid(src[(size_t)ids[i]], ax); sum = sum + cen[i]; count = count + 1.0f; }
        const float plane = sum / count;
        scratch.resize(n);
        size_t nl = 0, nr = 0;
        for (size_t i = 0; i < n; ++i) { if (cen[i] < plane) ids[nl++] = ids[i]; else scratch[nr++] = ids[i]; }
        for (size_t i = 0; i < nr; ++i) ids[nl + i] = scratch[i];
        float lm = bbox.lo[ax], rm = bbox.hi[ax];                     // maximumDef / minimumDef defaults
        for (size_t i = 0; i < nl; ++i) for (int k = 0; k < 3; ++k) {
            float c = vert(src[(size_t)ids[i]], k)[ax];
            lm = (i == 0 && k == 0) ? c : sq::hmax(lm, c);
        }
        for (size_t i = 0; i < nr; ++i) for (int k = 0; k < 3; ++k) {
            float c = vert(src[(size_t)ids[nl + i]], k)[ax];
            rm = (i == 0 && k == 0) ? c : sq::hmin(rm, c);
        }
        sq_node nd; nd.kind = ax; nd.lmax = 0.001f + lm; nd.rmin = (-0.001f) + rm; nd.link = -1;
        const size_t me = out.nodes.size();
        out.nodes.push_back(nd);
        if (nl == 0) {                                                // src/BIH.hs:70-72
            emit_leaf(ids, 0, depth + 1);
            out.nodes[me].link = emit_leaf(ids, nr, depth + 1);
        } else if (nr == 0) {                                         // src/BIH.hs:73-75
            emit_leaf(ids, nl, depth + 1);
            out.nodes[me].link = emit_leaf(ids, 0, depth + 1);
        } else {                                                      // src/BIH.hs:76-78
            sq_bounds lb = bounds_of(ids, nl), rb = bounds_of(ids + nl, nr);
            build(lb, ids, nl, depth + 1);
            out.nodes[me].link = (int32_t)out.nodes.size();
            build(rb, ids + nl, nr, depth + 1);
        }
    }
};

}  // namespace

extern "C" int sq_bih_build(const sq_mesh* mesh, sq_bih** outp) {
    if (!mesh || !outp) return sq_set_error("null argument");
    sq_bih* b = new sq_bih;
    b->mats = mesh->mats;
    const size_t n = mesh->tris.size();
    std::vector<int32_t> ids(n);
    for (size_t i = 0; i < n; ++i) ids[i] = (int32_t)i;
    Builder bl{ mesh->tris, *b, {} };
    b->tris.reserve(n);
    b->root = bl.bounds_of(ids.data(), n);                            // makeBIH, src/BIH.hs:62-65
    bl.build(b->root, ids.data(), n, 1);
    *outp = b;
    return 0;
}
extern "C" void sq_bih_scene(const sq_bih* b, sq_scene* out) {
    out->root = b->root;
    out->nodes = b->nodes.data(); out->n_nodes = (int32_t)b->nodes.size();
    out->tris = b->tris.data();   out->n_tris = (int32_t)b->tris.size();
    out->mats = b->mats.data();   out->n_mats = (int32_t)b->mats.size();
    out->height = b->height;
}
extern "C" int32_t sq_bih_height(const sq_bih* b) { return b->height; }
extern "C" int32_t sq_bih_num_leaves(const sq_bih* b) { return b->leaves; }
extern "C" int32_t sq_bih_longest_leaf(const sq_bih* b) { return b->longest; }
extern "C" void sq_bih_free(sq_bih* b) { delete b; }

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
}
extern "C" int sq_cull_boxes(const sq_scene* sc, float* boxes, float ray_limits[3]) {
    if (!sc || !boxes || !ray_limits) return sq_set_error("null argument");
    const int32_t n = sc->n_nodes;
    const double u = kLemmaU, kPmax = kLemmaPmax;
    const float inf = INFINITY;
    auto disable = [&]() { for (int32_t i = 0; i < n; ++i) { float* b = boxes + 6 * (size_t)i; b[0] = b[1] = b[2] = -inf; b[3] = b[4] = b[5] = inf; }
                           ray_limits[0] = -1.0f; ray_limits[1] = 0.25f; ray_limits[2] = 1.5624f; return 0; };
    double vmax_inf = 0.0, vmax2 = 0.0;
    for (int32_t i = 0; i < sc->n_tris; ++i) {
        const float* vs[3] = { sc->tris[i].v0, sc->tris[i].v1, sc->tris[i].v2 };
        for (const float* v : vs) {
            double q = 0.0;
            for (int c = 0; c < 3; ++c) { if (!(v[c] - v[c] == 0.0f)) return disable(); vmax_inf = std::max(vmax_inf, std::fabs((double)v[c])); q += (double)v[c] * v[c]; }
            vmax2 = std::max(vmax2, q);
        }
    }
    if (sc->n_tris == 0 || vmax_inf > 1048576.0) return disable();
    const double omax = 2.0 * std::sqrt(vmax2) * (1.0 + 1e-12);
    ray_limits[0] = f_down(omax * omax * (1.0 - 1e-6)); ray_limits[1] = 0.25f; ray_limits[2] = 1.5624f;
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
            if (!(q.P <= kPmax)) { ok = false; break; }
            m = std::max(m, lemma_rho(q, omax));
        }
        if (!ok) { b[0] = b[1] = b[2] = -inf; b[3] = b[4] = b[5] = inf; continue; }
        m += 8.0 * u * (vmax_inf + m + omax) + 1e-20;
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
    void level1_tables() {
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
        double vmax_inf = 0.0, vmax2 = 0.0;
        for (int32_t i = 0; i < sc.n_tris; ++i)
            for (const float* v : { sc.tris[i].v0, sc.tris[i].v1, sc.tris[i].v2 }) {
                double q = 0.0;
                for (int c = 0; c < 3; ++c) { vmax_inf = std::max(vmax_inf, std::fabs((double)v[c])); q += (double)v[c] * v[c]; }
                vmax2 = std::max(vmax2, q);
            }
        const double vmax = std::sqrt(vmax2), omax = 2.0 * vmax * (1.0 + 1e-12);          // as sq_cull_boxes
        // where p1 can be
        double g1 = 0.0;
        for (int32_t i = 0; i < sc.n_tris; ++i) {
            if (emits[(size_t)i]) continue;
            const TriNorms q = tri_norms(sc.tris[i]);
            if (!(q.P <= kLemmaPmax)) return;
            const double rho = lemma_rho(q, omax), r = 7.0 * u * q.P / eps;
            g1 = std::max(g1, rho + 1.01 * (r * (omax + vmax + rho) + rho));
        }
        const double delta1 = 4.0 * u * (2.0 * (vmax + g1) + omax) * (1.0 + 1e-6), R1 = vmax + g1 + delta1;
        if (!(R1 <= 1048576.0)) return;
        // the emitters' box and its margin
        double six = 0.0;
        for (int c = 0; c < 3; ++c) { L.em_lo[c] = P.emitters.empty() ? 0.0 : 1e300; L.em_hi[c] = P.emitters.empty() ? 0.0 : -1e300; }
        for (int32_t e : P.emitters) {
            const sq_tri& t = sc.tris[e];
            const TriNorms q = tri_norms(t);
            if (!(q.P <= kLemmaPmax)) return;
            L.em_rho = std::max(L.em_rho, 32.0 * (u / eps) * q.P * (R1 + q.V0 + q.E1 + q.E2));
            six = std::max(six, 6.0 * u * (q.E1 + q.E2));
            for (const float* v : { t.v0, t.v1, t.v2 })
                for (int c = 0; c < 3; ++c) {
                    L.em_lo[c] = std::min(L.em_lo[c], (double)v[c]);
                    L.em_hi[c] = std::max(L.em_hi[c], (double)v[c]);
                }
        }
        L.em_add = six + delta1 + 1e-20;
        // mirror classes: the scene's distinct `reflective` values, the largest kLevel1Classes - 1 on their own and the rest merged
        // upward into the lowest class (its box then holds every triangle)
        std::vector<float> vals;
        for (int32_t i = 0; i < sc.n_tris; ++i) vals.push_back(P.surfs[(size_t)i].reflective);
        std::sort(vals.begin(), vals.end()); vals.erase(std::unique(vals.begin(), vals.end()), vals.end());
        const size_t nv = vals.size(), nc = std::min<size_t>(nv, (size_t)kLevel1Classes);
        L.n_classes = (int32_t)nc;
        for (size_t c = 0; c < nc; ++c) {
            L.class_val[c] = vals[nv - nc + c];
            const float from = (c == 0) ? vals[0] : L.class_val[c];
            float* b = L.class_box[c];
            b[0] = b[1] = b[2] = INFINITY; b[3] = b[4] = b[5] = -INFINITY;     // empty until a triangle joins
            for (int32_t i = 0; i < sc.n_tris; ++i) {
                if (!(P.surfs[(size_t)i].reflective >= from)) continue;
                const sq_tri& t = sc.tris[i];
                const TriNorms q = tri_norms(t);
                if (!(q.P <= kLemmaPmax)) { b[0] = b[1] = b[2] = -INFINITY; b[3] = b[4] = b[5] = INFINITY; break; }
                double m = lemma_rho(q, omax);
                m += 8.0 * u * (vmax_inf + m + omax) + 1e-20;                    // the slab test's own rounding, as sq_cull_boxes
                for (int k = 0; k < 3; ++k) {
                    const double lo = std::min({ (double)t.v0[k], (double)t.v1[k], (double)t.v2[k] }), hi = std::max({ (double)t.v0[k], (double)t.v1[k], (double)t.v2[k] });
                    b[k] = std::min(b[k], f_down(lo - m)); b[3 + k] = std::max(b[3 + k], f_up(hi + m));
                }
            }
        }
        L.o2max = P.cull_limits[0]; L.d2min = P.cull_limits[1]; L.d2max = P.cull_limits[2];
        L.on = 1;
        const double slab_slack = 8.0 * u * (vmax_inf * (1.0 + 1e-6) + g1 + omax) + 1e-20;
        level1_cover(emits, omax, slab_slack);
        level1_mirror(emits, omax, vmax, vmax_inf, delta1, slab_slack);
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
    CoverBox cover_box_of(int32_t i, double omax, double slab_slack) const {
        const double u = kLemmaU, eps = kLemmaEps;
        const sq_tri& t = sc.tris[i];
        const TriNorms q = tri_norms(t);
        const double rho = lemma_rho(q, omax);
        double e1[3], e2[3];
        for (int k = 0; k < 3; ++k) { e1[k] = (double)(t.v1[k] - t.v0[k]); e2[k] = (double)(t.v2[k] - t.v0[k]); }
        const double n[3] = { e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0] };
        const double nn = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
        CoverBox b{}; b.count = 1; b.axis = 3; b.cell = 0; b.rmin = (double)P.surfs[(size_t)i].reflective;
        b.r = 7.0 * u * q.P / eps; b.c = 8.0 * u * (omax + q.V0) * q.E1 * q.E2 / eps;
        for (int k = 0; k < 3; ++k) {
            const double across = std::sqrt(n[(k + 1) % 3] * n[(k + 1) % 3] + n[(k + 2) % 3] * n[(k + 2) % 3]);
            // (n is within 3e-16 E1 E2 of the exact normal: above the sliver limit the quotient is good to 3e-10, below it s_k = 1)
            const double s = nn > 1e-6 * q.E1 * q.E2 ? std::min(1.0, across / nn + 1e-6) : 1.0;
            const double pts[5] = { (double)t.v0[k], (double)t.v1[k], (double)t.v2[k], (double)t.v0[k] + e1[k], (double)t.v0[k] + e2[k] };
            b.lo[k] = *std::min_element(pts, pts + 5) - rho * s - slab_slack;
            b.hi[k] = *std::max_element(pts, pts + 5) + rho * s + slab_slack;
        }
        return b;
    }
    static CoverBox join(const CoverBox& a, const CoverBox& b) {
        CoverBox o = a; o.count += b.count; o.r = std::max(a.r, b.r); o.c = std::max(a.c, b.c); o.rmin = std::min(a.rmin, b.rmin);
        for (int k = 0; k < 3; ++k) { o.lo[k] = std::min(a.lo[k], b.lo[k]); o.hi[k] = std::max(a.hi[k], b.hi[k]); }
        return o;
    }
    static double volume(const CoverBox& a) { return (a.hi[0] - a.lo[0]) * (a.hi[1] - a.lo[1]) * (a.hi[2] - a.lo[2]); }
    float cover_rmin[kLevel1Boxes] = {};                    // the smallest `reflective` in each box of the cover, for level1_mirror
    void level1_cover(const std::vector<char>& emits, double omax, double slab_slack) {
        using Box = CoverBox;
        std::vector<Box> each;
        double slo[3] = { 1e300, 1e300, 1e300 }, shi[3] = { -1e300, -1e300, -1e300 };
        for (int32_t i = 0; i < sc.n_tris; ++i) {
            if (emits[(size_t)i]) continue;
            const Box b = cover_box_of(i, omax, slab_slack);
            for (int k = 0; k < 3; ++k) { slo[k] = std::min(slo[k], b.lo[k]); shi[k] = std::max(shi[k], b.hi[k]); }
            each.push_back(b);
        }
        const double extent = each.empty() ? 0.0 : std::max({ shi[0] - slo[0], shi[1] - slo[1], shi[2] - slo[2] });
        for (Box& b : each) {
            const double ex[3] = { b.hi[0] - b.lo[0], b.hi[1] - b.lo[1], b.hi[2] - b.lo[2] }, longest = std::max({ ex[0], ex[1], ex[2] });
            for (int k = 2; k >= 0; --k) if (ex[k] <= 1e-4 * extent && ex[k] < 0.05 * longest) b.axis = k;
            if (b.axis < 3) b.cell = (int64_t)std::floor(0.5 * (b.lo[b.axis] + b.hi[b.axis]) / std::max(1e-3 * extent, 1e-300) + 0.5);
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
        while (boxes.size() > (size_t)kLevel1Boxes) {
            size_t bi = 0, bj = 1; double best = INFINITY;
            for (size_t i = 0; i < boxes.size(); ++i)
                for (size_t j = i + 1; j < boxes.size(); ++j) {
                    const double grow = volume(join(boxes[i], boxes[j])) - volume(boxes[i]) - volume(boxes[j]);
                    if (grow < best) { best = grow; bi = i; bj = j; }
                }
            boxes[bi] = join(boxes[bi], boxes[bj]);
            boxes.erase(boxes.begin() + (std::ptrdiff_t)bj);
        }
        if (boxes.empty()) return;                                        // no record: condition (4) is the stretch alone
        Level1Cover V{};
        V.n = (int32_t)boxes.size();
        for (size_t j = 0; j < (size_t)kLevel1Boxes; ++j) {               // entries beyond n repeat the first: the kernel reads them all
            const Box& b = boxes[j < boxes.size() ? j : 0];
            V.r[j] = f_up(b.r + 2e-6); V.c[j] = f_up(b.c * (1.0 + 1e-5) + 1e-30);
            for (int k = 0; k < 3; ++k) { V.box[j][k] = f_down(b.lo[k]); V.box[j][3 + k] = f_up(b.hi[k]); }
            cover_rmin[j] = (float)b.rmin;                                // (a `reflective` value, exact)
        }
        P.level1_cover.assign(1, V);
    }
    // Condition (5)'s record (the lemma's mirror extension above), written wherever the cover is; n_panels = 0 where the condition is off.
    // Panels: non-emissive triangles with `reflective` > 0 (one with 0 mirrors only when unit_float(n1) is 0) are grouped by (value,
    // unit normal up to sign in steps of 1e-3, offset along it in steps of 1e-3 of the scene's extent); a group of at least two triangles
    // with at least a thousandth of the non-emissive area is a panel when its members lie within 1e-3 of the extent of their common plane
    // and their computed unit normals within 1e-3 of its normal.  Everything else goes to the rest boxes, one per value, merged by least
    // added volume down to kLevel1Rest.  Any grouping is valid; this one finds the walls of a room.
    void level1_mirror(const std::vector<char>& emits, double omax, double vmax, double vmax_inf, double delta1, double slab_slack) {
        if (P.level1_cover.empty()) return;
        const Level1Cull& L = P.level1;
        const double u = kLemmaU, eps = kLemmaEps;
        Level1Mirror M{};
        for (int j = 0; j < kLevel1Boxes; ++j) M.rmin[j] = cover_rmin[j];
        for (int j = 0; j < kLevel1Rest; ++j) M.rest[j][6] = -1.0f;        // (an unused rest box applies to no sample)
        P.level1_mirror.assign(1, M);                                      // off, until everything below has succeeded
        if (P.emitters.empty()) return;
        double slo[3] = { 1e300, 1e300, 1e300 }, shi[3] = { -1e300, -1e300, -1e300 };
        for (int32_t i = 0; i < sc.n_tris; ++i)
            for (const float* v : { sc.tris[i].v0, sc.tris[i].v1, sc.tris[i].v2 })
                for (int k = 0; k < 3; ++k) { slo[k] = std::min(slo[k], (double)v[k]); shi[k] = std::max(shi[k], (double)v[k]); }
        const double extent = std::max({ shi[0] - slo[0], shi[1] - slo[1], shi[2] - slo[2] });
        if (!(extent > 0.0)) return;
        // the exact normal of the kernels' triangle, its five points, and the bound on its COMPUTED unit normal: the fp32 cross product is
        // within 3.5u E1 E2 of n, its fp32 normalisation within 8u of the unit vector
        struct Tri { double n[3], nn, pts[5][3], dn_err, rho; };
        auto tri_of = [&](int32_t i) {
            const sq_tri& t = sc.tris[i];
            const TriNorms q = tri_norms(t);
            Tri r{};
            double e1[3], e2[3];
            for (int k = 0; k < 3; ++k) {
                e1[k] = (double)(t.v1[k] - t.v0[k]); e2[k] = (double)(t.v2[k] - t.v0[k]);
                r.pts[0][k] = t.v0[k]; r.pts[1][k] = t.v1[k]; r.pts[2][k] = t.v2[k]; r.pts[3][k] = (double)t.v0[k] + e1[k]; r.pts[4][k] = (double)t.v0[k] + e2[k];
            }
            const double n[3] = { e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0] };
            r.nn = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
            const bool ok = r.nn > 1e-4 * q.E1 * q.E2;
            int big = 0;
            for (int k = 1; k < 3; ++k) if (std::fabs(n[k]) > std::fabs(n[big])) big = k;
            for (int k = 0; k < 3; ++k) r.n[k] = ok ? n[k] / r.nn * (n[big] < 0 ? -1.0 : 1.0) : 0.0;
            r.dn_err = ok ? 4.0 * u * q.E1 * q.E2 / r.nn + 8.0 * u : 1.0;
            r.rho = lemma_rho(q, omax);
            return r;
        };
        std::map<std::array<int64_t, 5>, std::vector<int32_t>> groups;
        std::vector<int32_t> rest;
        double area_all = 0.0;
        for (int32_t i = 0; i < sc.n_tris; ++i) {
            if (emits[(size_t)i]) continue;
            const Tri t = tri_of(i);
            area_all += t.nn;
            const float val = P.surfs[(size_t)i].reflective;
            if (!(val > 0.0f) || t.dn_err >= 1.0) { rest.push_back(i); continue; }
            uint32_t vb; std::memcpy(&vb, &val, 4);
            const double d = t.n[0] * t.pts[0][0] + t.n[1] * t.pts[0][1] + t.n[2] * t.pts[0][2];
            groups[{ (int64_t)vb, (int64_t)std::floor(t.n[0] * 1e3 + 0.5), (int64_t)std::floor(t.n[1] * 1e3 + 0.5), (int64_t)std::floor(t.n[2] * 1e3 + 0.5),
                     (int64_t)std::floor(d / (1e-3 * extent) + 0.5) }].push_back(i);
        }
        struct Panel { std::vector<int32_t> tris; double n[3], d, h, delta, rho; float val; };
        std::vector<Panel> panels;
        for (auto& [key, members] : groups) {
            Panel p{}; p.val = P.surfs[(size_t)members[0]].reflective;
            double area = 0.0, lo = 1e300, hi = -1e300;
            for (int32_t i : members) { const Tri t = tri_of(i); area += t.nn; for (int k = 0; k < 3; ++k) p.n[k] += t.nn * t.n[k]; }
            const double len = std::sqrt(p.n[0] * p.n[0] + p.n[1] * p.n[1] + p.n[2] * p.n[2]);
            bool ok = members.size() >= 2 && area >= 1e-3 * area_all && len > 0.5 * area;
            if (ok) {
                for (int k = 0; k < 3; ++k) p.n[k] /= len;
                for (int32_t i : members) {
                    const Tri t = tri_of(i);
                    for (const auto& x : t.pts) { const double s = p.n[0] * x[0] + p.n[1] * x[1] + p.n[2] * x[2]; lo = std::min(lo, s); hi = std::max(hi, s); }
                    const double dv[3] = { t.n[0] - p.n[0], t.n[1] - p.n[1], t.n[2] - p.n[2] };
                    p.delta = std::max(p.delta, std::sqrt(dv[0] * dv[0] + dv[1] * dv[1] + dv[2] * dv[2]) + t.dn_err + 1e-12);
                    p.rho = std::max(p.rho, t.rho);
                }
                p.d = 0.5 * (lo + hi); p.h = 0.5 * (hi - lo) + 1e-12 * (vmax + 1.0);
                ok = p.delta <= 1e-3 && p.h <= 1e-3 * extent;
            }
            if (ok) { p.tris = members; panels.push_back(std::move(p)); }
            else rest.insert(rest.end(), members.begin(), members.end());
        }
        if (panels.empty() || panels.size() > (size_t)kLevel1Panels) return;
        // the determinant floor and the emitters' margin at it: the floor that makes the margin 2e-3 of the emitters' extent
        double em_ext = std::max({ L.em_hi[0] - L.em_lo[0], L.em_hi[1] - L.em_lo[1], L.em_hi[2] - L.em_lo[2] });
        if (!(em_ext > 0.0)) em_ext = extent;
        const double a0 = std::max(eps, L.em_rho * eps / (2e-3 * em_ext)), m0 = L.em_rho * (eps / a0) + L.em_add;
        // W and err
        struct Wk { double w[3], len; };
        std::vector<Wk> ws;
        double err = 0.0;
        for (const Panel& p : panels) {
            const double kappa = 4.01 * p.delta + 16.0 * u;
            for (int32_t e : P.emitters) {
                const sq_tri& t = sc.tris[e];
                const TriNorms q = tri_norms(t);
                double e1[3], e2[3];
                for (int k = 0; k < 3; ++k) { e1[k] = (double)(t.v1[k] - t.v0[k]); e2[k] = (double)(t.v2[k] - t.v0[k]); }
                const double nE[3] = { e2[1] * e1[2] - e2[2] * e1[1], e2[2] * e1[0] - e2[0] * e1[2], e2[0] * e1[1] - e2[1] * e1[0] };
                const double f = 2.0 * (p.n[0] * nE[0] + p.n[1] * nE[1] + p.n[2] * nE[2]);
                const double W[3] = { nE[0] - f * p.n[0], nE[1] - f * p.n[1], nE[2] - f * p.n[2] };
                const double nEl = std::sqrt(nE[0] * nE[0] + nE[1] * nE[1] + nE[2] * nE[2]);
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
                    dev = 2.0 * u * (nEl + w.len);
                    ws.push_back(w);
                }
                err = std::max(err, 4.1 * u * ws[at].len + dev + kappa * nEl * 1.0001 + 17.7 * u * q.E1 * q.E2 + 1e-30);
            }
        }
        if (ws.size() > (size_t)kLevel1W) return;
        // the boxes
        const double B_lo[3] = { L.em_lo[0] - m0, L.em_lo[1] - m0, L.em_lo[2] - m0 }, B_hi[3] = { L.em_hi[0] + m0, L.em_hi[1] + m0, L.em_hi[2] + m0 };
        bool finite_all = std::isfinite(a0) && std::isfinite(m0) && std::isfinite(err);
        for (size_t j = 0; j < panels.size(); ++j) {
            const Panel& p = panels[j];
            CoverBox b = cover_box_of(p.tris[0], omax, slab_slack);
            for (size_t i = 1; i < p.tris.size(); ++i) b = join(b, cover_box_of(p.tris[i], omax, slab_slack));
            double corner = 0.0, far2 = 0.0;
            for (int k = 0; k < 3; ++k) {
                const double c = std::max(std::fabs(b.lo[k]), std::fabs(b.hi[k])), f = std::max(std::fabs(b.hi[k] - B_lo[k]), std::fabs(B_hi[k] - b.lo[k]));
                corner += c * c; far2 += f * f;
            }
            const double reach = omax + std::sqrt(corner);
            const double e1 = delta1 + 1.25 * b.c + b.r * reach + 2.01 * u * 1.3 * (reach + 1.25 * b.c);
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
        std::vector<CoverBox> rb;                                          // (rmin holds the LARGEST value here)
        for (int32_t i : rest) {
            const sq_tri& t = sc.tris[i];
            double m = lemma_rho(tri_norms(t), omax);
            m += 8.0 * u * (vmax_inf + m + omax) + 1e-20;
            CoverBox b{}; b.count = 1; b.rmin = (double)P.surfs[(size_t)i].reflective;
            for (int k = 0; k < 3; ++k) {
                b.lo[k] = std::min({ (double)t.v0[k], (double)t.v1[k], (double)t.v2[k] }) - m; b.hi[k] = std::max({ (double)t.v0[k], (double)t.v1[k], (double)t.v2[k] }) + m;
            }
            size_t at = 0;
            while (at < rb.size() && rb[at].rmin != b.rmin) ++at;
            if (at == rb.size()) rb.push_back(b); else { const double v = b.rmin; rb[at] = join(rb[at], b); rb[at].rmin = v; }
        }
        while (rb.size() > (size_t)kLevel1Rest) {
            size_t bi = 0, bj = 1; double best = INFINITY;
            for (size_t i = 0; i < rb.size(); ++i)
                for (size_t j = i + 1; j < rb.size(); ++j) {
                    const double grow = volume(join(rb[i], rb[j])) - volume(rb[i]) - volume(rb[j]);
                    if (grow < best) { best = grow; bi = i; bj = j; }
                }
            const double v = std::max(rb[bi].rmin, rb[bj].rmin);
            rb[bi] = join(rb[bi], rb[bj]); rb[bi].rmin = v;
            rb.erase(rb.begin() + (std::ptrdiff_t)bj);
        }
        for (size_t j = 0; j < (size_t)kLevel1Rest && !rb.empty(); ++j) {
            const CoverBox& b = rb[j < rb.size() ? j : 0];
            for (int k = 0; k < 3; ++k) { M.rest[j][k] = f_down(b.lo[k]); M.rest[j][3 + k] = f_up(b.hi[k]); }
            M.rest[j][6] = (float)b.rmin;
        }
        if (!finite_all) return;
        for (size_t j = panels.size(); j < (size_t)kLevel1Panels; ++j) std::memcpy(M.panel[j], M.panel[0], sizeof M.panel[0]);
        for (size_t k = 0; k < (size_t)kLevel1W; ++k)
            for (int c = 0; c < 3; ++c) M.w[k][c] = (float)ws[k < ws.size() ? k : 0].w[c];
        M.n_panels = (int32_t)panels.size(); M.n_rest = (int32_t)rb.size(); M.n_w = (int32_t)ws.size();
        M.thr2 = f_up((a0 + err) * (a0 + err) * (1.0 + 1e-5));
        M.d2lo = f_up((double)L.d2min * 1.01); M.d2hi = f_down((double)L.d2max * 0.99);
        M.a0 = f_up(a0); M.m0 = f_up(m0);
        P.level1_mirror.assign(1, M);
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
    k.merged_records(); k.emitter_list(); k.geometry_flags(); k.level1_tables();
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

// Seeds [0, n_cover) that a scene's table of generator words holds for a w x h frame at `samples` (squigly_host.h): what the frame
// can use -- one past its largest seed, samples * (x + y * w) + samples - 1 at x = h - 1, y = w - 1 (src/Lib.hs:85-86) -- capped by
// the budget at 12 bytes per seed.  The product is taken in 128 bits: three factors below 2^31 reach 2^93.
extern "C" int64_t sq_rng_table_cover(int32_t w, int32_t h, int32_t samples, int64_t budget_bytes) {
    if (w < 1 || h < 1 || samples < 1 || budget_bytes < 12) return 0;
    const unsigned __int128 span = (unsigned __int128)samples * ((unsigned __int128)(w - 1) * (unsigned __int128)w + (unsigned __int128)h);
    const unsigned __int128 cap = (unsigned __int128)(budget_bytes / 12);
    return (int64_t)(span < cap ? span : cap);
}

// ----------------------------------------------------------------------------------------------
// Planning (sq_plan.h): what a render or query call decides before it touches the device.  Pure integer arithmetic on the scene's
// scalars, the options, the call's shape and the device's CU count; sq_device.hip allocates and enqueues by it.
// ----------------------------------------------------------------------------------------------
namespace sqd {
namespace {
// One row per option: how sq_set_option takes a value.  kAny: as it is; kRange: refused outside [lo, hi] with `refusal`; kBool: 0 or 1;
// kSign: -1 for a negative value, else 0 or 1; kIgnored: accepted, no effect.
enum OptionKind { kAny, kRange, kBool, kSign, kIgnored };
struct OptionRow { const char* name; int64_t Options::* member; OptionKind kind; int64_t lo, hi; const char* refusal; };
const OptionRow kOptionTable[] = {
    { "timing", &Options::timing, kAny, 0, 0, nullptr },
    { "variant", &Options::variant, kRange, 1, 2, "variant must be 1 (per-pixel kernel) or 2 (wavefront)" },
    { "slots", &Options::slots, kRange, 1, 512ll << 20, "slots must be in 1..2^29" },
    { "straggler_lanes", &Options::straggler_lanes, kRange, 0, 63, "straggler_lanes must be in 0..63" },
    { "resident", &Options::resident, kBool, 0, 1, nullptr },
    { "profile", &Options::profile, kBool, 0, 1, nullptr },
    { "lds_node_kb", &Options::lds_node_kb, kRange, 0, 128, "lds_node_kb must be in 0..128" },
    { "trace_blocks_per_cu", &Options::trace_blocks_per_cu, kRange, 0, 8, "trace_blocks_per_cu must be in 0..8" },
    { "overlap", &Options::overlap, kRange, 0, 2, "overlap must be 0, 1 or 2" },
    { "rng_table_mb", &Options::rng_table_mb, kRange, 0, 1ll << 20, "rng_table_mb must be in 0..2^20" },
    { "cast_wavefront", &Options::cast_wavefront, kBool, 0, 1, nullptr },
    { "deep", &Options::deep, kBool, 0, 1, nullptr },
    { "pool", &Options::pool, kBool, 0, 1, nullptr },
    { "guided", &Options::guided, kRange, 0, 3, "guided must be in 0..3" },
    { "primary_resident", &Options::primary_resident, kBool, 0, 1, nullptr },
    { "cull", &Options::cull, kBool, 0, 1, nullptr },
    { "level1_cull", &Options::level1_cull, kBool, 0, 1, nullptr },
    { "incremental", nullptr, kIgnored, 0, 0, nullptr },   // the incremental slab test was removed
    { "primary_tiles", &Options::primary_tiles, kBool, 0, 1, nullptr },
    { "primary_pooled", &Options::primary_pooled, kBool, 0, 1, nullptr },
    { "coresidency", &Options::coresidency, kBool, 0, 1, nullptr },
    { "aux_polite", &Options::aux_polite, kRange, 0, 8, "aux_polite must be in 0..8" },
    { "trace_prio", &Options::trace_prio, kRange, 0, 3, "trace_prio must be in 0..3" },
    { "aux_low_priority", &Options::aux_low_priority, kBool, 0, 1, nullptr },   // sq_set_option also drops the second stream
    { "descend_extra", &Options::descend_extra, kRange, 0, 16, "descend_extra must be in 0..16" },
    { "descend_lanes", &Options::descend_lanes, kRange, 1, 64, "descend_lanes must be in 1..64" },
    { "pixel_major", &Options::pixel_major, kSign, -1, 1, nullptr },
    { "refill_min", &Options::refill_min, kRange, 1, 64, "refill_min must be in 1..64" },
    { "flush_min", &Options::flush_min, kRange, 0, 64, "flush_min must be in 0..64" },
    { "aux_blocks_per_cu", &Options::aux_blocks_per_cu, kRange, 0, 16, "aux_blocks_per_cu must be in 0..16" },
};
}  // namespace

int set_option(Options& O, const char* key, int64_t value) {
    for (const OptionRow& r : kOptionTable) {
        if (std::strcmp(key, r.name)) continue;
        if (r.kind == kRange && (value < r.lo || value > r.hi)) return sq_set_error("%s", r.refusal);
        if (r.kind != kIgnored) O.*r.member = r.kind == kBool ? (value ? 1 : 0) : r.kind == kSign ? (value < 0 ? -1 : value != 0) : value;
        return 0;
    }
    return sq_set_error("unknown option '%s'", key);
}

int refuse_frame_size(int64_t n_views, int64_t rows, int64_t h, bool wavefront) {
    if (rows <= 0 || h <= 0 || n_views <= 0) return 0;
    const int64_t view_rows = n_views * rows;                           // each factor is below 2^31: below 2^62
    const bool huge = view_rows > kMaxCallPixels || view_rows * h > kMaxCallPixels;
    const int64_t pixels = huge ? 0 : view_rows * h;
    if (n_views > 1) {
        if (huge) return sq_set_error("%lld views of %lld x %lld pixels exceed 2^31 - 1 pixels in one call", (long long)n_views, (long long)rows, (long long)h);
        if (wavefront && pixels > kMaxWavefrontPixels)
            return sq_set_error("%lld views of %lld x %lld pixels exceed 2^29 pixels in one call of the wavefront form (variant 1 takes 2^31 - 1)", (long long)n_views, (long long)rows, (long long)h);
        return 0;
    }
    if (huge) return sq_set_error("%lld x %lld pixels exceed 2^31 - 1 pixels in one call", (long long)rows, (long long)h);
    if (wavefront && pixels > kMaxWavefrontPixels)
        return sq_set_error("%lld x %lld pixels exceed 2^29 pixels in one call of the wavefront form (variant 1 and cast frames take 2^31 - 1)", (long long)rows, (long long)h);
    return 0;
}

long long radiance_chunk_rays(long long n, long long slots, bool wavefront) {
    const long long cap = wavefront ? std::min<long long>(std::max<long long>(slots, 1), kMaxWavefrontPixels) : kLaneChunk;
    return std::min(n, cap);
}

namespace {
// Chooses the trace form -- resident, streaming six-wave or streaming plain -- its LDS layout and workgroups per CU, and fills the
// trace fields of the plan.  Refuses a tree whose stacks do not fit the streaming form's LDS.
int plan_trace(const PlanInputs& in, CallPlan& C) {
    const Options& o = in.opt; const SceneScalars& S = in.scene;
    const int n_cu = in.device.n_cu, stack_cap = C.stack_cap, stack_elem = S.stack_word;
    sq_plan& P = C.plan;
    // persistent trace kernel geometry.  Resident form: the whole scene (branches, leaves, unique vertices,
    // 16-bit indexed triangles) plus every lane's stack fits in the 160 KB of one CU -> one 1024-thread
    // workgroup per CU, no global traffic except ray fetch and hit store.  Streaming form otherwise.
    const size_t lds_budget = kLdsBudget;
    bool resident = false, dense = false;
    const bool pool = o.pool != 0;
    TraceLds L{};
    if (o.resident && S.has_trix) {
        L = trace_lds_layout(S.n_branches, true, S.n_verts, S.n_tris, kResidentBlock, stack_cap, stack_elem, pool);
        resident = L.total <= lds_budget && S.n_verts <= 4096;         // vertex byte offsets are 16-bit (ResidentTris)
    }
    int n_lds = S.n_branches, trace_blocks = 0, trace_threads = 0;
    if (resident) {
        trace_blocks = n_cu; trace_threads = kResidentBlock;
    } else {
        const size_t max_node_bytes = (size_t)o.lds_node_kb * 1024;     // top of the tree; the rest of LDS buys occupancy
        const int n_lds_want = (int)std::min<size_t>((size_t)S.n_branches, max_node_bytes / 48);
        const TraceLds L0 = trace_lds_layout(0, false, S.n_verts, S.n_tris, kTraceBlock, stack_cap, stack_elem, pool);   // stacks, live lists, window tables
        if (L0.total > lds_budget) return sq_set_error("BIH height %d needs %u B of LDS per workgroup (max %zu)", S.height, L0.total, lds_budget);
        // Three workgroups per CU (the six-wave build) when a third of the LDS holds a workgroup's stacks plus at least 4 KB of
        // the tree's top (or all of it); otherwise two, or one, with up to lds_node_kb of tree each.
        const size_t third = (lds_budget / 3) & ~(size_t)2047;            // 52 KB: the hardware allocates LDS in granules, and 3 x 53.3 KB rounded up does not fit
        const bool dense_fits = L0.total + std::min<size_t>((size_t)S.n_branches * 48, 4096) + 16 <= third;
        dense = pool && !o.profile && (o.trace_blocks_per_cu == 0 ? dense_fits : o.trace_blocks_per_cu == 3 && dense_fits);
        int per_cu;
        if (dense) {
            per_cu = 3;
            n_lds = (int)std::min<size_t>((size_t)n_lds_want, (third - L0.total - 16) / 48);
        } else {
            n_lds = n_lds_want;
            while (n_lds > 0 && trace_lds_layout(n_lds, false, S.n_verts, S.n_tris, kTraceBlock, stack_cap, stack_elem, pool).total > lds_budget) n_lds /= 2;
        }
        L = trace_lds_layout(n_lds, false, S.n_verts, S.n_tris, kTraceBlock, stack_cap, stack_elem, pool);
        if (!dense) {
            per_cu = (int)std::max<size_t>(1, std::min<size_t>(2, lds_budget / L.total));    // the plain build's 86 VGPRs allow four waves per SIMD = two workgroups
            if (o.trace_blocks_per_cu > 0) per_cu = (int)std::min<int64_t>(o.trace_blocks_per_cu, (int64_t)std::max<size_t>(1, lds_budget / L.total));
        }
        trace_blocks = n_cu * per_cu; trace_threads = kTraceBlock;
    }
    const size_t tr_lds = L.total;
    P.trace_form = resident ? SQ_FORM_RESIDENT : dense ? SQ_FORM_STREAMING_SIX_WAVE : SQ_FORM_STREAMING_PLAIN;
    P.blocks_per_cu = trace_blocks / n_cu; P.n_lds = n_lds; P.trace_lds_bytes = (int32_t)tr_lds;
    C.trace_form = P.trace_form; C.resident = resident; C.pool = pool; C.profile = o.profile != 0; C.dense = dense;
    C.n_lds = n_lds; C.trace_blocks = trace_blocks; C.trace_threads = trace_threads; C.tr_lds = tr_lds;
    return 0;
}
}  // namespace

int plan_call(const PlanInputs& in, CallPlan& C) {
    C = CallPlan{};
    C.in = in;
    const Options& o = in.opt; const SceneScalars& S = in.scene; const SceneState& st = in.state; const Call& F = in.call;
    const int n_cu = in.device.n_cu;
    if (!F.query && refuse_frame_size(F.n_views, F.local_rows, F.h, o.variant != 1 && (!F.cast || o.cast_wavefront))) return 1;
    // What a frame and an intersection query do first, alike: the options' view of the scene, the per-lane stacks' size, and the
    // fixed part of the plan.
    C.planned = true;
    C.cull_off = !o.cull;                                              // no ray is inside the culling limits: every leaf is tested
    C.nonneg_materials = S.nonneg_materials; C.n_emitters = S.n_emitters;
    const int stack_cap = std::max(S.height, 1);
    const size_t px_lds = (size_t)kBlock * stack_cap * (size_t)S.stack_word;
    C.stack_cap = stack_cap; C.px_lds = px_lds;
    sq_plan& P = C.plan;
    P.variant = (int32_t)o.variant; P.stack_word_bytes = S.stack_word; P.height = S.height; P.stack_cap = stack_cap;
    P.pixel_lds_bytes = (int32_t)px_lds; P.packed_leaves = S.packed_leaves; P.n_emitters = S.n_emitters;
    P.trace_form = SQ_FORM_PER_PIXEL; P.primary_form = SQ_PRIMARY_NONE;
    if (F.query) {
        // variant 1 runs the per-lane kernel; the default form runs chunks of stage -> one level of the trace kernel -> store
        if (o.variant == 1) {
            if (px_lds > kLdsBudget) return sq_set_error("BIH height %d needs %zu B of LDS stack per workgroup (max 163840)", S.height, px_lds);
            C.path = kPathQueryLanes; P.launched = 1;
            return 0;
        }
        if (plan_trace(in, C)) return 1;
        // Chunks of at most `slots` rays (and what the workspace holds; the option caps the slots at 2^29, so a chunk's queue positions and
        // the trace kernel's 32-bit cursor never overflow).  One slot per ray: 37 B, against 40 B of caller arrays per ray.
        C.path = kPathQueryWave; C.pixels = 1; C.slots = std::min<int64_t>(o.slots, F.n_rays); P.launched = 1;
        return 0;
    }
    // nonneg_materials bounds the radiance below an absorbing surface for the reference's depth.  A deeper path nests more products,
    // one of which may be inf where the bound still held: 0 * inf is NaN in the reference, so past the packer's shortcut_depth
    // (material_flags) the generic-depth kernels of this launch take no s == 0 shortcut.
    if (!F.cast && st.depth > 3 && st.depth > S.shortcut_depth) C.nonneg_materials = 0;
    // Under a sky neither the absorbing-surface shortcut nor the last ray's emitter pre-test is an identity as it stands (the last ray
    // adds the sky when it misses; 0 * sky is NaN for an infinite sky): this launch's generic-depth kernels take neither.
    const bool sky = !F.cast && st.sky_set;
    if (sky) { C.nonneg_materials = 0; C.n_emitters = -1; P.n_emitters = -1; }
    const long long pixels = (long long)F.n_views * F.local_rows * F.h;   // every view's pixels, view-major
    const long long px_blocks = (pixels + kBlock - 1) / kBlock;
    // a masked call (sq_render_rows_device_masked with a mask, second moments or counts) takes the AD instantiations of the kernels that
    // decide who is active, and clears no buffer; every other call takes the instantiations, and the memsets, it always took
    const bool ad = F.src == kSrcCamera && F.masked;
    const bool mom2 = ad && F.mom2;
    C.sky = sky; C.pixels = pixels; C.px_blocks = px_blocks; C.ad = ad; C.mom2 = mom2;
    if (px_blocks > 0x7fffffffLL) return sq_set_error("image too large for one launch");
    if (px_lds > kLdsBudget) return sq_set_error("BIH height %d needs %zu B of LDS stack per workgroup (max 163840)", S.height, px_lds);
    // a cast frame: the per-lane form, or (option "cast_wavefront" with variant 2) the wavefront form with the lights as its samples
    const bool cast_wave = F.cast && o.variant == 2 && o.cast_wavefront;
    const int n_lights = st.n_lights;
    // a path-traced frame or query under a depth other than 3 (or under option "deep"): the generic-depth kernels
    const int depth = st.depth;
    const bool deep = !F.cast && (depth != 3 || o.deep || sky);
    C.deep = deep;
    // The per-lane forms: one kernel, one lane per pixel.
    if (F.cast && !cast_wave && st.lights_set) { C.path = kPathLaneCast; P.launched = 1; return 0; }   // caller-given lights: sq_cast_pixels beside sq_render_pixels
    if (o.variant == 1 && deep) { C.path = kPathLaneDeep; P.launched = 1; return 0; }                   // a depth other than 3, or a sky: sq_render_pixels_deep
    if (o.variant == 1 || (F.cast && !cast_wave)) { C.path = kPathLanePlain; P.launched = 1; return 0; }
    // ---- wavefront pipeline ----
    // the samples this call renders (a whole frame: F.samples); in a cast frame the lights take the samples' place in the slots
    const int n_call = cast_wave ? n_lights : F.k_end - F.k_begin;
    // at least one sample of every pixel per batch, never more slots than the call has samples
    const int64_t slots = std::max<int64_t>(pixels, std::min<int64_t>(o.slots, (int64_t)pixels * n_call));
    C.n_call = n_call; C.slots = slots;
    if (plan_trace(in, C)) return 1;
    const int aux_blocks = n_cu * (int)(o.aux_blocks_per_cu ? o.aux_blocks_per_cu : 8);
    // sq_accumulate, by its loop form: the grouped loop when the shard has no more pixels than the launch has threads (every thread
    // at most one pixel)
    C.aux_blocks = aux_blocks; C.acc_grouped = pixels <= (long long)aux_blocks * kBlock;
    P.primary_form = (o.primary_pooled && C.pool) ? SQ_PRIMARY_POOLED : (C.resident && o.primary_resident) ? SQ_PRIMARY_RESIDENT : SQ_PRIMARY_PER_LANE;
    // the per-lane primary pass is one launch with a thread per tile lane, padding included (a narrow frame's edge tiles are mostly
    // padding: up to 64 lanes per pixel at h = 1), and a launch has at most 2^32 - 1 threads; the other two passes stride over a fixed grid
    const long long padded = primary_padded_lanes(F.local_rows, F.tile_rows, F.tiles_x);
    if (P.primary_form == SQ_PRIMARY_PER_LANE && (padded * F.n_views + kBlock - 1) / kBlock * kBlock > 0xffffffffLL)
        return sq_set_error("image too large for one launch of the primary rays (%lld tile lanes; at most 2^32 - 1)", padded * F.n_views);
    C.need_lights = cast_wave; C.need_sum2 = mom2; C.need_deep = deep;
    C.deep_slot_bytes = deep ? deep_slot_bytes(depth, sky) : 0;
    C.rng_table = !cast_wave; C.rng_grow = F.src != kSrcRays && !deep;
    // primary rays: once per pixel.  With a resident scene they are traced out of LDS as well
    if (P.primary_form == SQ_PRIMARY_RESIDENT) {
        const TraceLds Lp = trace_lds_layout(S.n_branches, true, S.n_verts, S.n_tris, kResidentBlock, stack_cap, S.stack_word, false);
        const long long need = (padded * F.n_views + kResidentBlock - 1) / kResidentBlock;
        C.primary_grid = std::min<long long>(n_cu, need); C.primary_lds = Lp.total;
    } else if (P.primary_form == SQ_PRIMARY_PER_LANE) {
        C.primary_grid = (padded * F.n_views + kBlock - 1) / kBlock; C.primary_lds = px_lds;
    }
    C.path = cast_wave ? kPathWaveCast : deep ? kPathWaveDeep : kPathPipeline;
    // Level-1 culling (level1_tables): the three-level pipeline only, and only with the shortcuts its lemma builds on
    if (C.path == kPathPipeline) {
        C.level1_cull = S.level1_on && o.level1_cull && C.n_emitters >= 0 && C.nonneg_materials && S.finite_geometry;
        P.level1_cull = C.level1_cull;
    }
    P.launched = 1;
    return 0;
}

Schedule plan_schedule(const CallPlan& C, int64_t have_slots) {
    Schedule D;
    const Options& o = C.in.opt;
    if (C.path == kPathQueryWave) { D.query_chunk = std::min<long long>(o.slots, have_slots); return D; }
    if (C.path != kPathWaveCast && C.path != kPathWaveDeep && C.path != kPathPipeline) return D;
    const long long pixels = C.pixels; const int n_call = C.n_call;
    // Overlapped schedule: the sample batches alternate between two halves of the workspace ("tracks"); every
    // trace launch stays on the caller's stream, in the order T1(a) T1(b) T2(a) T2(b), while the per-sample
    // kernels (RNG + bounce, shading, accumulation) run on a second stream beside them, ordered by events.
    // Opt-in (sq_set_option "overlap"): measured +3 % on the headline frame (105.5 -> 102.3 ms) -- the kernels do
    // run side by side, but the chip is VALU-bound as a whole, so each slows the other down by what it gains;
    // and trace-launch durations then include that interference, which blurs the per-kernel roofline figure.
    const bool overlap = o.overlap && C.path == kPathPipeline && n_call >= 2 && have_slots >= 2 * pixels;
    const int tracks = overlap ? 2 : 1;
    const int64_t track_slots = have_slots / tracks;
    // samples per batch: as many as a track holds, split evenly (few large launches: a small trace launch
    // wastes its ramp-up and drain, and the second-bounce launches only carry a few percent of the slots)
    const int max_batch = (int)std::max<int64_t>(1, std::min<int64_t>(n_call, track_slots / pixels));
    const int n_batches = std::max(tracks, (n_call + max_batch - 1) / max_batch);
    const int batch = (n_call + n_batches - 1) / n_batches;
    int n_real = 0;
    while (n_real < n_batches && std::max(0, std::min(batch, n_call - n_real * batch)) > 0) ++n_real;
    D.overlap = overlap; D.tracks = tracks; D.track_slots = track_slots; D.batch = batch; D.n_batches = n_batches; D.n_real = n_real;
    return D;
}

Grid2 pp_grid(const CallPlan& C, const Schedule& D, int kc) {
    const Options& o = C.in.opt; const int n_cu = C.in.device.n_cu; const long long pixels = C.pixels;
    // Overlapped schedules, option "aux_polite" = n > 0: the per-sample kernels get n workgroups per CU in all (grid-stride
    // loops do the rest), few enough that a trace workgroup -- 16 waves, all of the CU's LDS, 4 x 104 VGPRs per SIMD -- can
    // always be placed beside them, whichever kernel reaches a CU first.
    if (D.overlap && o.aux_polite > 0) return Grid2{ (unsigned)(n_cu * (int)o.aux_polite), 1u };
    // x covers the pixels, y splits a pixel's samples when the frame has too few pixels to fill the chip (one rank's share of a
    // frame, small frames)
    const long long bx = std::max<long long>(1, std::min<long long>((pixels + kBlock - 1) / kBlock, 1 << 20));
    const long long want_threads = (long long)n_cu * 2048 * 2;
    const long long ks = std::max<long long>(1, std::min<long long>(std::min(kc, 64), (want_threads + pixels - 1) / std::max<long long>(pixels, 1)));
    return Grid2{ (unsigned)bx, (unsigned)ks };
}

TraceLaunch trace_launch(const CallPlan& C, int64_t queue_rays, int kc, int level) {
    const Options& o = C.in.opt;
    const bool resident = C.resident;
    const int trace_blocks = C.trace_blocks, trace_threads = C.trace_threads;
    // a launch with few slots (the per-pixel mirror rays) takes small reservations, or only a few waves get any
    const int max_chunk = resident ? kChunkResident : kChunkStreaming;
    const int64_t per_wave = queue_rays * (int64_t)kc / std::max(1, trace_blocks * (trace_threads / 64));
    const int chunk = (int)std::min<int64_t>(max_chunk, std::max<int64_t>(64, (per_wave / 8) / 64 * 64));
    // queue order: a pixel's samples in a row pays once the triangles no longer fit the L2s (rays that start at one point
    // share their first leaves: 1M-triangle scene +2.5 %), and costs 1-7 % below that (strided queue reads)
    const bool pixel_major = o.pixel_major < 0 ? (!resident && (size_t)C.in.scene.n_tris * sizeof(DevTri) > ((size_t)4 << 20)) : o.pixel_major != 0;
    int guide_shift = 2;                                            // log2(4 x waves of the launch), rounded up
    while ((1ll << guide_shift) < 4ll * trace_blocks * (trace_threads / 64)) ++guide_shift;
    if (!((o.guided >> level) & 1)) guide_shift = 62;              // bit 0: first bounce level (and the mirror / primary launches), bit 1: second
    return TraceLaunch{ chunk, guide_shift, pixel_major };
}

int workspace_layout(int64_t pixels, int64_t slots, WorkLayout& W) {
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += al(bytes); return o; };
    W.cnt = take(128 * sizeof(int32_t)); W.stats = take(kStatSlots * sizeof(unsigned long long));
    W.pix = take(pixels * 4); W.t0 = take(pixels * 4); W.tri0 = take(pixels * 4); W.sum = take(pixels * 12);
    W.mt = take(pixels * 4); W.mtri = take(pixels * 4);
    // + pixels: the mirror rays' spare region behind the sample slots (state and the two ray quads)
    W.state = take(slots + pixels); W.org = take((slots + pixels) * 16); W.dir = take((slots + pixels) * 16); W.tri1 = take(slots * 4);
    W.carry = take(pixels * 12);                                    // behind everything else: no other array moves for it
    W.total = off;
    // every array has its own, ordered place in the block: a slip here would be a GPU fault, not an error code
    if (!(W.cnt < W.stats && W.stats < W.pix && W.pix < W.t0 && W.t0 < W.tri0 && W.tri0 < W.sum && W.sum < W.mt && W.mt < W.mtri &&
          W.mtri < W.state && W.state < W.org && W.org < W.dir && W.dir < W.tri1 && W.tri1 < W.carry && W.carry < off))
        return sq_set_error("internal error: frame workspace layout");
    return 0;
}

DeepLayout deep_layout(int depth, bool sky, long long cap) {
    DeepLayout L{};
    L.oxy = 0;                                                      // float2 per slot, from depth 4 on
    L.trail = depth >= 4 ? (size_t)cap * 8 : 0;                     // int32 per bounce level and slot
    L.has_tmiss = sky && depth >= 2;
    L.tmiss = L.has_tmiss ? L.trail + (size_t)(depth - 1) * cap * 4 : 0;
    return L;
}
}  // namespace sqd

// ---- the C-ABI window on the planner (include/squigly_host.h) ----
extern "C" int sq_plan_call(const char* const* in_names, const int64_t* in_values, int32_t n_in, int64_t have_slots,
                            sq_plan* plan, const char* const* out_names, int64_t* out_values, int32_t n_out) {
    using namespace sqd;
    if (!plan || n_in < 0 || n_out < 0 || (n_in > 0 && (!in_names || !in_values)) || (n_out > 0 && (!out_names || !out_values))) { sq_set_error("null argument"); return 2; }
    *plan = sq_plan{};
    for (int32_t i = 0; i < n_out; ++i) out_values[i] = 0;
    PlanInputs in;
    SceneScalars& S = in.scene; SceneState& st = in.state; Call& F = in.call;
    int64_t small_index = 0, trix = 0, sky = 0, lights_set = 0, cast = 0, masked = 0, mom2 = 0, query = 0, total_rays = 0;
    const struct { const char* name; int32_t* v32; int64_t* v64; } fields[] = {
        { "n_branches", &S.n_branches, nullptr }, { "n_verts", &S.n_verts, nullptr }, { "n_tris", &S.n_tris, nullptr }, { "height", &S.height, nullptr },
        { "trix", nullptr, &trix }, { "small_index", nullptr, &small_index }, { "packed_leaves", &S.packed_leaves, nullptr },
        { "n_emitters", &S.n_emitters, nullptr }, { "nonneg_materials", &S.nonneg_materials, nullptr }, { "finite_geometry", &S.finite_geometry, nullptr },
        { "shortcut_depth", &S.shortcut_depth, nullptr }, { "level1_on", &S.level1_on, nullptr }, { "n_cu", &in.device.n_cu, nullptr },
        { "depth", &st.depth, nullptr }, { "sky", nullptr, &sky }, { "lights_set", nullptr, &lights_set }, { "n_lights", &st.n_lights, nullptr },
        { "source", &F.src, nullptr }, { "cast", nullptr, &cast }, { "masked", nullptr, &masked }, { "mom2", nullptr, &mom2 },
        { "n_views", &F.n_views, nullptr }, { "local_rows", &F.local_rows, nullptr }, { "h", &F.h, nullptr }, { "tile_rows", &F.tile_rows, nullptr },
        { "tiles_x", &F.tiles_x, nullptr }, { "k_begin", &F.k_begin, nullptr }, { "k_end", &F.k_end, nullptr },
        { "query", nullptr, &query }, { "n_rays", nullptr, &F.n_rays }, { "total_rays", nullptr, &total_rays } };
    for (int32_t i = 0; i < n_in; ++i) {
        if (!in_names[i]) { sq_set_error("null argument"); return 2; }
        bool found = false;
        for (const auto& f : fields)
            if (!std::strcmp(in_names[i], f.name)) {
                if (f.v32 && (in_values[i] < INT32_MIN || in_values[i] > INT32_MAX)) { sq_set_error("%s = %lld is not a 32-bit value", f.name, (long long)in_values[i]); return 2; }
                if (f.v32) *f.v32 = (int32_t)in_values[i]; else *f.v64 = in_values[i];
                found = true;
            }
        if (!found && set_option(in.opt, in_names[i], in_values[i])) return 2;      // an option by sq_set_option's name, with its refusals
    }
    S.has_trix = trix != 0; S.stack_word = small_index ? 2 : 4;
    st.sky_set = sky != 0; st.lights_set = lights_set != 0;
    F.cast = cast != 0; F.masked = masked != 0; F.mom2 = mom2 != 0; F.query = query != 0;
    if (S.n_branches < 0 || S.n_verts < 0 || S.n_tris < 0 || S.height < 0 || in.device.n_cu < 1 || st.depth < 1 || st.depth > kDeepestPath || st.n_lights < 0 ||
        F.src < kSrcCamera || F.src > kSrcRays || F.n_views < 1 || F.local_rows < 1 || F.h < 1 || F.tile_rows < 1 || F.tiles_x < 1 ||
        F.k_begin < 0 || F.k_end <= F.k_begin || (F.query && F.n_rays < 1) || have_slots < 0 || total_rays < 0) {
        sq_set_error("bad planner input");
        return 2;
    }
    CallPlan C;
    const int rc = plan_call(in, C);
    *plan = C.plan;
    if (rc) { plan->launched = 0; return 1; }
    const int64_t have = have_slots ? have_slots : C.slots;            // 0: the workspace gave the slots the plan wanted
    const Schedule D = plan_schedule(C, have);
    WorkLayout W{};
    if (C.slots > 0 && workspace_layout(C.pixels, have, W)) return 1;
    const int tail_kc = D.n_real > 0 ? std::min(D.batch, C.n_call - (D.n_real - 1) * D.batch) : 0;
    const Grid2 g = pp_grid(C, D, D.batch), gt = pp_grid(C, D, tail_kc);
    const int64_t queue = C.path == kPathQueryWave ? std::min<int64_t>(D.query_chunk, F.n_rays) : C.pixels;
    const int kc = C.path == kPathQueryWave ? 1 : D.batch;
    const TraceLaunch t0 = trace_launch(C, queue, kc, 0), t1 = trace_launch(C, queue, kc, 1), tt = trace_launch(C, queue, tail_kc, 0), lone = trace_launch(C, C.pixels, 1, 0);
    const DeepLayout dl = deep_layout(st.depth, C.sky, have);
    const struct { const char* name; int64_t value; } all[] = {
        { "path", C.path }, { "ad", C.ad }, { "mom2", C.mom2 }, { "sky", C.sky }, { "deep", C.deep }, { "nonneg_materials", C.nonneg_materials },
        { "n_emitters", C.n_emitters }, { "cull_off", C.cull_off }, { "pixels", C.pixels }, { "px_blocks", C.px_blocks }, { "px_lds", (int64_t)C.px_lds },
        { "n_call", C.n_call }, { "slots", C.slots }, { "trace_form", C.trace_form }, { "resident", C.resident }, { "pool", C.pool }, { "profile", C.profile },
        { "dense", C.dense }, { "n_lds", C.n_lds }, { "stack_cap", C.stack_cap }, { "trace_blocks", C.trace_blocks }, { "trace_threads", C.trace_threads },
        { "tr_lds", (int64_t)C.tr_lds }, { "primary_grid", C.primary_grid }, { "primary_lds", (int64_t)C.primary_lds }, { "aux_blocks", C.aux_blocks },
        { "acc_grouped", C.acc_grouped }, { "level1_cull", C.level1_cull }, { "deep_slot_bytes", (int64_t)C.deep_slot_bytes }, { "need_lights", C.need_lights },
        { "need_sum2", C.need_sum2 }, { "need_deep", C.need_deep }, { "rng_table", C.rng_table }, { "rng_grow", C.rng_grow },
        { "chunk_rays", total_rays > 0 ? radiance_chunk_rays(total_rays, in.opt.slots, in.opt.variant != 1 && (!F.cast || in.opt.cast_wavefront)) : 0 },
        { "have_slots", have }, { "overlap", D.overlap }, { "tracks", D.tracks }, { "track_slots", D.track_slots }, { "batch", D.batch },
        { "n_batches", D.n_batches }, { "n_real", D.n_real }, { "query_chunk", D.query_chunk }, { "tail_kc", tail_kc },
        { "pp_grid_x", g.x }, { "pp_grid_y", g.y }, { "tail_pp_grid_x", gt.x }, { "tail_pp_grid_y", gt.y },
        { "chunk_0", t0.chunk }, { "chunk_1", t1.chunk }, { "guide_shift_0", t0.guide_shift }, { "guide_shift_1", t1.guide_shift },
        { "pixel_major", t0.pixel_major }, { "tail_chunk", tt.chunk }, { "lone_chunk", lone.chunk },
        { "ws_cnt", (int64_t)W.cnt }, { "ws_stats", (int64_t)W.stats }, { "ws_pix", (int64_t)W.pix }, { "ws_t0", (int64_t)W.t0 }, { "ws_tri0", (int64_t)W.tri0 },
        { "ws_sum", (int64_t)W.sum }, { "ws_mt", (int64_t)W.mt }, { "ws_mtri", (int64_t)W.mtri }, { "ws_state", (int64_t)W.state }, { "ws_org", (int64_t)W.org },
        { "ws_dir", (int64_t)W.dir }, { "ws_tri1", (int64_t)W.tri1 }, { "ws_carry", (int64_t)W.carry }, { "ws_total", (int64_t)W.total },
        { "deep_oxy", (int64_t)dl.oxy }, { "deep_trail", (int64_t)dl.trail }, { "deep_tmiss", dl.has_tmiss ? (int64_t)dl.tmiss : -1 } };
    for (int32_t i = 0; i < n_out; ++i) {
        bool found = false;
        for (const auto& s : all) if (out_names[i] && !std::strcmp(out_names[i], s.name)) { out_values[i] = s.value; found = true; }
        if (!found) { sq_set_error("no plan scalar '%s'", out_names[i] ? out_names[i] : "(null)"); return 2; }
    }
    return 0;
}
