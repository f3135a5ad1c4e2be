// acos_main.cpp — host sq::facos as a stand-alone program (tests/test_acos_series.py):
//   g++ -std=c++17 -O2 -ffp-contract=off tests/acos_main.cpp -o acos_main
//   ./acos_main in.f32 out.f32
// Reads binary32 values from the first file and writes sq::facos of each, in order, to the second.
#include <cstdio>
#include <vector>

#include "../squigly-trace_amd/csrc/sq_math.h"

int main(int argc, char** argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: %s in.f32 out.f32\n", argv[0]); return 2; }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 1; }
    std::vector<float> x;
    float buf[4096];
    for (size_t n; (n = std::fread(buf, sizeof(float), 4096, f)) > 0;) x.insert(x.end(), buf, buf + n);
    std::fclose(f);
    for (float& v : x) v = sq::facos(v);
    f = std::fopen(argv[2], "wb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[2]); return 1; }
    const bool ok = std::fwrite(x.data(), sizeof(float), x.size(), f) == x.size();
    return (std::fclose(f) == 0 && ok) ? 0 : 1;
}
