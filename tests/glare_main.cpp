// glare_main.cpp — csrc/sq_glare_pixel.h, the text libsquigly_denoise.so's glare kernels compile, as a host program of its own, so that
// it can run under the sanitizers without anything else in the process (tests/test_glare.py builds it with g++ -ffp-contract=off, plainly
// and with -fsanitize=address,undefined, and runs each once).  Every float goes in and out as the hex word of its bits.
//
//   glare_main bright E G0 G1 G2 THRESHOLD CEILING R G B ...
//       prints a line a pixel: the three words of the exposed pixel x, then the three words of its bright pass b.
//   glare_main taps N
//       for every extent n = 1 .. N prints a line "d n o t0 t1 t2 t3" for every output o of the down step over a fine extent n, and a
//       line "u n v i0 i1 A B" for every fine coordinate v of the up step from the coarse extent (n + 1) / 2 (A, B: the weights' words).
//   glare_main frame ROWS COLS LEVELS E G0 G1 G2 THRESHOLD CEILING SPREAD STRENGTH R G B ...
//       the whole call over a ROWS x COLS frame, one level after the other as the library enqueues them: prints a line a pixel, the
//       three words of out.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../squigly-trace_amd/csrc/sq_glare_pixel.h"

namespace gp = glarepix;

static float word(const char* text) {
    const uint32_t u = (uint32_t)std::strtoul(text, nullptr, 16);
    float f;
    std::memcpy(&f, &u, sizeof f);
    return f;
}

static uint32_t bits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, sizeof u);
    return u;
}

// An image as the kernels' sources see one: S(j, i) is the pixel of row j and column i.  at() checks what the clamps promise.
struct Image {
    int32_t rows, cols;
    std::vector<sq::f3> px;
    Image(int32_t r, int32_t c) : rows(r), cols(c), px((size_t)r * (size_t)c) {}
    sq::f3 operator()(int32_t j, int32_t i) const { return px.at((size_t)j * (size_t)cols + (size_t)i); }
    sq::f3& set(int32_t j, int32_t i) { return px.at((size_t)j * (size_t)cols + (size_t)i); }
};

static Image down_image(const Image& fine) {
    Image out(gp::half_up(fine.rows), gp::half_up(fine.cols));
    for (int32_t y = 0; y < out.rows; ++y)
        for (int32_t x = 0; x < out.cols; ++x) out.set(y, x) = gp::down(fine, fine.rows, fine.cols, y, x);
    return out;
}

static int usage(const char* me) {
    std::fprintf(stderr, "usage: %s bright E G0 G1 G2 THRESHOLD CEILING (3 words a pixel)... | taps N | "
                         "frame ROWS COLS LEVELS E G0 G1 G2 THRESHOLD CEILING SPREAD STRENGTH (3 words a pixel)...\n", me);
    return 2;
}

int main(int argc, char** argv) {
    if (argc < 2) return usage(argv[0]);
    if (!std::strcmp(argv[1], "bright")) {
        if (argc < 8 || (argc - 8) % 3 != 0) return usage(argv[0]);
        const float e = word(argv[2]);
        const gp::Glare G{ { word(argv[3]), word(argv[4]), word(argv[5]) }, word(argv[6]), word(argv[7]), 0.0f, 0.0f };
        for (int a = 8; a + 3 <= argc; a += 3) {
            const sq::f3 x = gp::exposed(e, G, sq::mk(word(argv[a]), word(argv[a + 1]), word(argv[a + 2])));
            const sq::f3 b = gp::bright(G, x);
            std::printf("%08x %08x %08x %08x %08x %08x\n", bits(x.x), bits(x.y), bits(x.z), bits(b.x), bits(b.y), bits(b.z));
        }
        return 0;
    }
    if (!std::strcmp(argv[1], "taps")) {
        if (argc != 3) return usage(argv[0]);
        const int N = std::atoi(argv[2]);
        if (N < 1 || N > 1 << 20) return usage(argv[0]);
        for (int32_t n = 1; n <= N; ++n) {
            const int32_t half = gp::half_up(n);
            for (int32_t o = 0; o < half; ++o)
                std::printf("d %d %d %d %d %d %d\n", n, o, gp::down_tap(o, 0, n), gp::down_tap(o, 1, n), gp::down_tap(o, 2, n), gp::down_tap(o, 3, n));
            for (int32_t v = 0; v < n; ++v) {
                const gp::UpTap t = gp::up_tap(v, half);
                std::printf("u %d %d %d %d %08x %08x\n", n, v, t.i0, t.i1, bits(t.a), bits(t.b));
            }
        }
        return 0;
    }
    if (!std::strcmp(argv[1], "frame")) {
        if (argc < 13) return usage(argv[0]);
        const int32_t rows = std::atoi(argv[2]), cols = std::atoi(argv[3]), levels = std::atoi(argv[4]);
        if (rows < 1 || cols < 1 || (long long)rows * cols > 1 << 20 || levels < 0 || levels > gp::kMaxLevels
            || argc - 13 != 3 * rows * cols)
            return usage(argv[0]);
        const float e = word(argv[5]);
        const gp::Glare G{ { word(argv[6]), word(argv[7]), word(argv[8]) }, word(argv[9]), word(argv[10]), word(argv[11]), word(argv[12]) };
        Image x(rows, cols), b(rows, cols);
        for (int32_t p = 0; p < rows * cols; ++p) {
            const int a = 13 + 3 * p;
            x.px[p] = gp::exposed(e, G, sq::mk(word(argv[a]), word(argv[a + 1]), word(argv[a + 2])));
            b.px[p] = gp::bright(G, x.px[p]);
        }
        std::vector<Image> level;
        for (int k = 0; k < levels; ++k) level.push_back(down_image(k ? level[k - 1] : b));
        for (int k = levels - 2; k >= 0; --k)                            // in place, as the kernel: a pixel reads its own record alone
            for (int32_t y = 0; y < level[k].rows; ++y)
                for (int32_t xx = 0; xx < level[k].cols; ++xx)
                    level[k].set(y, xx) = gp::add_scaled(level[k](y, xx), G.spread, gp::up(level[k + 1], level[k + 1].rows, level[k + 1].cols, y, xx));
        for (int32_t y = 0; y < rows; ++y)
            for (int32_t xx = 0; xx < cols; ++xx) {
                sq::f3 o = x(y, xx);
                if (levels) o = gp::add_scaled(o, G.strength, gp::up(level[0], level[0].rows, level[0].cols, y, xx));
                std::printf("%08x %08x %08x\n", bits(o.x), bits(o.y), bits(o.z));
            }
        return 0;
    }
    return usage(argv[0]);
}
