// film_main.cpp — csrc/sq_film_pixel.h, the text libsquigly_film.so's kernels compile, as a host program of its own, so that it can
// run under the sanitizers without anything else in the process (tests/test_film.py builds it with g++ -ffp-contract=off, plainly and
// with -fsanitize=address,undefined, and runs each once).  Every float goes in and out as the hex word of its bits.
//
//   film_main develop CURVE DITHER COLS EXPOSURE WHITE NLUT L0 .. L(NLUT-1) R G B ...
//       prints a line a pixel: the three bytes (decimal), then the three display words (hex).  NLUT 0 = no table.
//   film_main slots R G B ...
//       prints a line a pixel: the histogram slot of its luminance.
//   film_main expose KEY PERMILLE E_MIN E_MAX RATE FALLBACK HAS_PREV PREV SLOT COUNT ...
//       prints the exposure word of the histogram that holds COUNT in SLOT (decimal pairs) and zero elsewhere.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../squigly-trace_amd/csrc/sq_film_pixel.h"

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

// The whole of sq_film_expose_device, one slot after the other, around the header's rank_of and exposure: what the kernel's scan
// must equal.
static float expose_serial(const uint32_t* hist, const filmpix::Meter& m, bool has_prev, float prev) {
    uint64_t M = 0;
    for (int i = 1; i < filmpix::kSlots - 1; ++i) M += hist[i];
    int s = 1;
    if (M) {
        const uint64_t rank = filmpix::rank_of(M, m.permille);
        uint64_t run = 0;
        for (s = 1; s < filmpix::kSlots - 1; ++s) { run += hist[s]; if (run >= rank) break; }
    }
    return filmpix::exposure(M, s, m, has_prev, prev);
}

// The header's pixel with its three template switches chosen at run time (the library chooses them per launch).
static void develop_any(int curve, bool lut, bool dither, const filmpix::Develop& D, float e, sq::f3 c, int y, int x, uint8_t* rgb, float* disp) {
    using namespace filmpix;
#define FILM_CASE(C)                                                                    \
    case C:                                                                             \
        if (lut && dither) develop<C, true, true>(D, e, c, y, x, rgb, disp);            \
        else if (lut) develop<C, true, false>(D, e, c, y, x, rgb, disp);                \
        else if (dither) develop<C, false, true>(D, e, c, y, x, rgb, disp);             \
        else develop<C, false, false>(D, e, c, y, x, rgb, disp);                        \
        break;
    switch (curve) {
        FILM_CASE(ATAN) FILM_CASE(REINHARD) FILM_CASE(FILMIC) FILM_CASE(LINEAR)
        default: develop<REFERENCE, false, false>(D, e, c, y, x, rgb, disp); break;
    }
#undef FILM_CASE
}

static int usage(const char* me) {
    std::fprintf(stderr, "usage: %s develop CURVE DITHER COLS EXPOSURE WHITE NLUT (table words) (3 words a pixel)... | slots (3 words a pixel)... | "
                         "expose KEY PERMILLE E_MIN E_MAX RATE FALLBACK HAS_PREV PREV (SLOT COUNT)...\n", me);
    return 2;
}

int main(int argc, char** argv) {
    if (argc < 2) return usage(argv[0]);
    if (!std::strcmp(argv[1], "develop")) {
        if (argc < 8) return usage(argv[0]);
        const int curve = std::atoi(argv[2]), dither = std::atoi(argv[3]), cols = std::atoi(argv[4]), n_lut = std::atoi(argv[7]);
        const float e = word(argv[5]), white = word(argv[6]);
        if (curve < 0 || curve >= filmpix::kCurves || cols < 1 || n_lut < 0 || n_lut == 1 || n_lut > 65536 || argc < 8 + n_lut
            || (argc - 8 - n_lut) % 3 != 0)
            return usage(argv[0]);
        std::vector<float> lut(n_lut);
        for (int i = 0; i < n_lut; ++i) lut[i] = word(argv[8 + i]);
        const filmpix::Develop D{ white, n_lut ? lut.data() : nullptr, n_lut };
        int p = 0;
        for (int a = 8 + n_lut; a + 3 <= argc; a += 3, ++p) {
            uint8_t rgb[3];
            float d[3];
            develop_any(curve, n_lut != 0, dither != 0, D, e, sq::mk(word(argv[a]), word(argv[a + 1]), word(argv[a + 2])), p / cols, p % cols,
                        rgb, d);
            std::printf("%d %d %d %08x %08x %08x\n", rgb[0], rgb[1], rgb[2], bits(d[0]), bits(d[1]), bits(d[2]));
        }
        return 0;
    }
    if (!std::strcmp(argv[1], "slots")) {
        if ((argc - 2) % 3 != 0) return usage(argv[0]);
        for (int a = 2; a + 3 <= argc; a += 3)
            std::printf("%d\n", filmpix::slot(filmpix::luminance(word(argv[a]), word(argv[a + 1]), word(argv[a + 2]))));
        return 0;
    }
    if (!std::strcmp(argv[1], "expose")) {
        if (argc < 10 || (argc - 10) % 2 != 0) return usage(argv[0]);
        const filmpix::Meter m{ word(argv[2]), std::atoi(argv[3]), word(argv[4]), word(argv[5]), word(argv[6]), word(argv[7]) };
        std::vector<uint32_t> hist(filmpix::kSlots, 0u);
        for (int a = 10; a + 2 <= argc; a += 2) {
            const int s = std::atoi(argv[a]);
            if (s < 0 || s >= filmpix::kSlots) return usage(argv[0]);
            hist[s] = (uint32_t)std::strtoul(argv[a + 1], nullptr, 10);
        }
        std::printf("%08x\n", bits(expose_serial(hist.data(), m, std::atoi(argv[8]) != 0, word(argv[9]))));
        return 0;
    }
    return usage(argv[0]);
}
