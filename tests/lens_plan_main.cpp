// lens_plan_main.cpp — the GPU-free part of libsquigly_lens.so (csrc/sq_lens_plan.h) as a stand-alone program, for the sanitizers
// (tests/test_lens.py compiles it with -fsanitize=address,undefined and runs it once).
//
//     lens_plan_main P r_begin r_end work_bytes [P r_begin r_end work_bytes ...]
//
// Per case one line: "plan <count>: r0-r1 r0-r1 ..." or "refused: <message>".  Every case is planned three times -- counted with no
// array, into an array of exactly the count, and into one that is a batch short with a guard entry behind it -- and the layouts of
// its batches are checked to lie inside work_bytes.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../squigly-trace_amd/csrc/sq_lens_plan.h"

int main(int argc, char** argv) {
    if (argc < 5 || (argc - 1) % 4 != 0) {
        std::fprintf(stderr, "usage: %s P r_begin r_end work_bytes ...\n", argv[0]);
        return 2;
    }
    for (int a = 1; a + 3 < argc; a += 4) {
        const long long P = std::atoll(argv[a]);
        const int32_t r0 = (int32_t)std::atoll(argv[a + 1]), r1 = (int32_t)std::atoll(argv[a + 2]);
        const size_t bytes = (size_t)std::strtoull(argv[a + 3], nullptr, 10);
        const int32_t count = lensplan::plan(P, r0, r1, bytes, nullptr, 0);
        if (count < 0) {
            std::printf("refused: %s\n", sq_error_buffer());
            continue;
        }
        const int32_t shown = count < 64 ? count : 64;                 // a plan of 2^31 one-sub-ray batches is counted, not listed
        std::vector<int32_t> out(2 * (size_t)shown);
        if (lensplan::plan(P, r0, r1, bytes, out.data(), shown) != count) return 3;
        if (shown > 1) {
            std::vector<int32_t> shorter(2 * (size_t)(shown - 1) + 1, -7);
            if (lensplan::plan(P, r0, r1, bytes, shorter.data(), shown - 1) != count) return 4;
            if (shorter.back() != -7 || std::memcmp(shorter.data(), out.data(), 2 * (size_t)(shown - 1) * sizeof(int32_t)) != 0) return 5;
        }
        // the batches a frame enqueues (csrc/sq_lens_frame.h walks batch_count / batch) are the ones plan() lists: every listed one,
        // and the last one of a plan too long to list, which must end the range
        const long long nb = lensplan::max_batch(P, bytes);
        if (lensplan::batch_count(r0, r1, nb) != count) return 7;
        for (int32_t i = 0; i < shown; ++i) {
            const lensplan::Batch b = lensplan::batch(r0, r1, nb, i);
            if (b.r0 != out[2 * i] || b.r1 != out[2 * i + 1] || b.r1 <= b.r0 || b.r1 - b.r0 > nb) return 8;
            if (b.r0 != (i == 0 ? r0 : out[2 * i - 1])) return 9;
        }
        if (lensplan::batch(r0, r1, nb, (int64_t)count - 1).r1 != r1) return 10;
        std::printf("plan %d:", count);
        for (int32_t i = 0; i < shown; ++i) {
            const lensplan::Layout L = lensplan::layout(P * (out[2 * i + 1] - out[2 * i]));
            if (L.total > bytes || L.total != lensplan::work_bytes(P, out[2 * i + 1] - out[2 * i]) || L.org % 16 || L.dir % 16 || L.sum % 16) return 6;
            std::printf(" %d-%d", out[2 * i], out[2 * i + 1]);
        }
        std::printf("\n");
    }
    return 0;
}
