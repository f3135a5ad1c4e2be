// moving_main.cpp — csrc/sq_temporal_pixel.h's accumulate, the text every lane of libsquigly_temporal.so's accumulate kernel compiles
// for the static and the moving call alike, as a program of its own over host memory, so that it can run under the sanitizers without anything else in the process
// (tests/test_moving.py builds it plainly and with -fsanitize=address,undefined and compares its output with the numpy restatement).
// Every table is a heap block of exactly its size, so a read through a wrong index is the sanitizer's to report.
//
//   moving_main IN OUT : IN is a file of 32-bit words --
//     rows cols has_prev has_alpha n_tris n_objects radius max_history   (int32; n_tris < 0: no tables; radius 0: no clamp)
//     k alpha_min sigma_p cos_n cam[12]                                  (float)
//     color[3n] var[n] tri[n] normal[3n] point[3n] (alpha[n]) (prev: color[3n] var[n] len[n] tri[n] normal[3n] point[3n])
//     (object[n_tris] back[12 n_objects])
//   OUT receives color[3n] var[n] len[n] flags[n] as 32-bit words.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../squigly-trace_amd/csrc/sq_temporal_pixel.h"

using temporalpix::Rec;

static std::vector<uint32_t> g_words;
static size_t g_at = 0;

template <class T>
static std::vector<T> take(size_t count) {
    static_assert(sizeof(T) == 4, "32-bit words");
    if (g_at + count > g_words.size()) { std::fprintf(stderr, "input too short\n"); std::exit(2); }
    std::vector<T> v(count);
    if (count) std::memcpy(v.data(), g_words.data() + g_at, 4 * count);
    g_at += count;
    return v;
}

int main(int argc, char** argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    std::FILE* in = std::fopen(argv[1], "rb");
    if (!in) { std::perror(argv[1]); return 2; }
    std::fseek(in, 0, SEEK_END);
    const long bytes = std::ftell(in);
    std::fseek(in, 0, SEEK_SET);
    g_words.resize((size_t)bytes / 4);
    if (std::fread(g_words.data(), 4, g_words.size(), in) != g_words.size()) { std::fprintf(stderr, "short read\n"); return 2; }
    std::fclose(in);

    const std::vector<int32_t> head = take<int32_t>(8);
    const int32_t rows = head[0], cols = head[1], n_tris = head[4], n_objects = head[5];
    const bool has_prev = head[2] != 0, has_alpha = head[3] != 0;
    const std::vector<float> fl = take<float>(16);
    const temporalpix::Clamp K{ head[6], fl[0] };
    const temporalpix::Params P{ fl[1], head[7], fl[2], fl[3] };
    const float* cam = fl.data() + 4;
    const size_t n = (size_t)rows * (size_t)cols;
    const std::vector<float> color = take<float>(3 * n), var = take<float>(n);
    const std::vector<int32_t> tri = take<int32_t>(n);
    const std::vector<float> normal = take<float>(3 * n), point = take<float>(3 * n);
    const std::vector<float> alpha = take<float>(has_alpha ? n : 0);
    std::vector<Rec> cv, nl, pt;
    if (has_prev) {
        const std::vector<float> pc = take<float>(3 * n), pv = take<float>(n);
        const std::vector<int32_t> plen = take<int32_t>(n), ptri = take<int32_t>(n);
        const std::vector<float> pn = take<float>(3 * n), pp = take<float>(3 * n);
        cv.resize(n); nl.resize(n); pt.resize(n);
        for (size_t p = 0; p < n; ++p) {
            cv[p] = Rec{ pc[3 * p], pc[3 * p + 1], pc[3 * p + 2], pv[p] };
            nl[p] = Rec{ pn[3 * p], pn[3 * p + 1], pn[3 * p + 2], temporalpix::int_bits(plen[p]) };
            pt[p] = Rec{ pp[3 * p], pp[3 * p + 1], pp[3 * p + 2], temporalpix::int_bits(ptri[p]) };
        }
    }
    const std::vector<int32_t> object = take<int32_t>(n_tris > 0 ? (size_t)n_tris : 0);
    const std::vector<float> back = take<float>(n_tris > 0 ? 12 * (size_t)n_objects : 0);
    if (g_at != g_words.size()) { std::fprintf(stderr, "input too long\n"); return 2; }

    std::vector<float> out_c(3 * n), out_v(n);
    std::vector<int32_t> out_len(n), out_flags(n);
    for (long long y = 0; y < rows; ++y)
        for (long long x = 0; x < cols; ++x) {
            const size_t p = (size_t)(y * cols + x);
            const int32_t tr = tri[p];
            const float* B = nullptr;                    // the kernel's lookup: an index outside its table is never read through
            bool moved = false;
            if (n_tris > 0 && has_prev && tr >= 0) {
                const int32_t o = tr < n_tris ? object[(size_t)tr] : -1;
                if (o >= 0 && o < n_objects) { B = back.data() + 12 * (size_t)o; moved = true; }
            }
            uint32_t flags;
            const temporalpix::Pixel r = temporalpix::accumulate(
                has_prev ? cv.data() : nullptr, nl.data(), pt.data(), rows, cols, cam, cam + 3, P, color[3 * p], color[3 * p + 1], color[3 * p + 2],
                var[p], tr, normal[3 * p], normal[3 * p + 1], normal[3 * p + 2], point[3 * p], point[3 * p + 1], point[3 * p + 2], has_alpha,
                has_alpha ? alpha[p] : -1.0f, moved, B, K.radius ? &K : nullptr,
                [&](int j, int i, float* c) {
                    const long long qy = y + j, qx = x + i;
                    if (qy < 0 || qy >= rows || qx < 0 || qx >= cols) return false;
                    const size_t q = (size_t)(qy * cols + qx);
                    if (tri[q] < 0) return false;
                    c[0] = color[3 * q]; c[1] = color[3 * q + 1]; c[2] = color[3 * q + 2];
                    return true;
                }, flags);
            out_c[3 * p] = r.r; out_c[3 * p + 1] = r.g; out_c[3 * p + 2] = r.b;
            out_v[p] = r.v; out_len[p] = r.len; out_flags[p] = (int32_t)flags;
        }
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!out) { std::perror(argv[2]); return 2; }
    std::fwrite(out_c.data(), 4, out_c.size(), out);
    std::fwrite(out_v.data(), 4, out_v.size(), out);
    std::fwrite(out_len.data(), 4, out_len.size(), out);
    std::fwrite(out_flags.data(), 4, out_flags.size(), out);
    return std::fclose(out) == 0 ? 0 : 2;
}
