// temporal_main.cpp — csrc/sq_temporal_pixel.h's projection, the host code sq_temporal_project and the kernel share, as a program of
// its own, so that it can run under the sanitizers without anything else in the process (tests/test_temporal.py builds it with
// -fsanitize=address,undefined and runs it once).
//
//   temporal_main ROWS COLS C0 .. C11 P0 P1 P2 ... : the image's size (decimal), the camera's twelve 32-bit words (hex, the bits of
//   a float: pos, then rot row-major), then three words a point.
// Prints a line a point: 1 or 0 (projects or not), then the words of fx and fy, in hex.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../squigly-trace_amd/csrc/sq_temporal_pixel.h"

static float word(const char* text) {
    const uint32_t u = (uint32_t)std::strtoul(text, nullptr, 16);
    float f;
    std::memcpy(&f, &u, sizeof f);
    return f;
}

int main(int argc, char** argv) {
    if (argc < 15 || (argc - 15) % 3 != 0) {
        std::fprintf(stderr, "usage: %s ROWS COLS (12 hex words: pos rot) (3 hex words a point)...\n", argv[0]);
        return 2;
    }
    const int rows = std::atoi(argv[1]), cols = std::atoi(argv[2]);
    float cam[12];
    for (int i = 0; i < 12; ++i) cam[i] = word(argv[3 + i]);
    for (int a = 15; a + 3 <= argc; a += 3) {
        float fx, fy;
        const bool ok = temporalpix::project(cam, cam + 3, (float)rows, (float)cols, word(argv[a]), word(argv[a + 1]), word(argv[a + 2]), fx, fy);
        uint32_t ux, uy;
        std::memcpy(&ux, &fx, sizeof ux);
        std::memcpy(&uy, &fy, sizeof uy);
        std::printf("%d %08x %08x\n", ok ? 1 : 0, ux, uy);
    }
    return 0;
}
