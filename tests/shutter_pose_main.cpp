// shutter_pose_main.cpp — csrc/sq_shutter_pose.h, the pose of an instant of an exposure, as a program of its own, so that the host
// code sq_shutter_pose and the kernels share can run under the sanitizers without anything else in the process
// (tests/test_shutter.py builds it with -fsanitize=address,undefined and runs it once).
//
//   shutter_pose_main W0 W1 ... : thirteen 32-bit words (hex, the bits of a float) a case -- pos0, ang0, pos1, ang1, tt.
// Prints a line a case: the twelve words of pos and rot, in hex.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../squigly-trace_amd/csrc/sq_shutter_pose.h"

static float word(const char* text) {
    const uint32_t u = (uint32_t)std::strtoul(text, nullptr, 16);
    float f;
    std::memcpy(&f, &u, sizeof f);
    return f;
}

int main(int argc, char** argv) {
    if ((argc - 1) % 13 != 0) {
        std::fprintf(stderr, "usage: %s (13 hex words a case: pos0 ang0 pos1 ang1 tt)\n", argv[0]);
        return 2;
    }
    for (int a = 1; a + 13 <= argc; a += 13) {
        float v[13];
        for (int i = 0; i < 13; ++i) v[i] = word(argv[a + i]);
        const shutterpose::Motion M = shutterpose::motion_of(v, v + 3, v + 6, v + 9, 0.0f);
        float out[12];
        shutterpose::pose_at(M, v[12], out, out + 3);
        for (int i = 0; i < 12; ++i) {
            uint32_t u;
            std::memcpy(&u, &out[i], sizeof u);
            std::printf("%08x%c", u, i == 11 ? '\n' : ' ');
        }
    }
    return 0;
}
