// upsample_main.cpp — csrc/sq_upsample_pixel.h, the text libsquigly_denoise.so's two sparse-frame kernels compile, as a host program
// of its own, so that it can run under the sanitizers without anything else in the process (tests/test_upsample.py builds it with
// g++ -ffp-contract=off, plainly and with -fsanitize=address,undefined, and runs each once per case).
//
//   upsample_main IN OUT
//       IN:  int32 rows, cols, s, oy, ox, has_var, has_mask; float32 sigma_p, cos_n; then the images, row-major: tri (int32),
//            normal, point, colour (3 float32 a pixel), with has_var the variance (float32), with has_mask a mask (uint8).
//       OUT: the mask of the guides (uint8), then the frame filled in under the given mask -- without one, under the mask just
//            computed: colour (3 float32 a pixel) and, with has_var, variance (float32).
// Every image is a heap block of exactly its size, so that a tap outside the image is a finding of the address sanitizer.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../squigly-trace_amd/csrc/sq_upsample_pixel.h"

template <class T>
static bool read_all(std::FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return std::fread(v.data(), sizeof(T), n, f) == n;
}

template <class T>
static bool write_all(std::FILE* f, const std::vector<T>& v) {
    return v.empty() || std::fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
}

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
        return 2;
    }
    std::FILE* in = std::fopen(argv[1], "rb");
    if (!in) return 2;
    std::vector<int32_t> head;
    std::vector<float> stops;
    if (!read_all(in, head, 7) || !read_all(in, stops, 2)) return 2;
    const upspix::Lattice L{ head[0], head[1], head[2], head[3], head[4] };
    const bool has_var = head[5] != 0, has_mask = head[6] != 0;
    if (L.rows < 1 || L.cols < 1 || (int64_t)L.rows * L.cols > (1 << 24) || L.s < 1 || L.s > upspix::kMaxStride || L.oy < 0 || L.oy >= L.s
        || L.ox < 0 || L.ox >= L.s)
        return 2;
    const upspix::Stops K{ stops[0], stops[1] };
    const size_t n = (size_t)L.rows * (size_t)L.cols;
    std::vector<int32_t> tri;
    std::vector<float> normal, point, color, var;
    std::vector<uint8_t> given;
    if (!read_all(in, tri, n) || !read_all(in, normal, 3 * n) || !read_all(in, point, 3 * n) || !read_all(in, color, 3 * n)) return 2;
    if (has_var && !read_all(in, var, n)) return 2;
    if (has_mask && !read_all(in, given, n)) return 2;
    std::fclose(in);

    const upspix::Guides G{ tri.data(), normal.data(), point.data() };
    const upspix::Image I{ color.data(), has_var ? var.data() : nullptr };
    std::vector<uint8_t> mask(n);
    for (int32_t y = 0; y < L.rows; ++y)
        for (int32_t x = 0; x < L.cols; ++x) mask[(size_t)y * L.cols + x] = upspix::live(L, K, G, y, x);
    const uint8_t* use = has_mask ? given.data() : mask.data();
    std::vector<float> out(3 * n), out_var(has_var ? n : 0);
    for (int32_t y = 0; y < L.rows; ++y)
        for (int32_t x = 0; x < L.cols; ++x) {
            const size_t p = (size_t)y * L.cols + x;
            float unused = 0.0f;
            if (has_var) upspix::upsample<true>(L, K, G, I, use, y, x, &out[3 * p], &out_var[p]);
            else upspix::upsample<false>(L, K, G, I, use, y, x, &out[3 * p], &unused);
        }
    std::FILE* o = std::fopen(argv[2], "wb");
    if (!o || !write_all(o, mask) || !write_all(o, out) || !write_all(o, out_var)) return 2;
    return std::fclose(o) == 0 ? 0 : 2;
}
