// sq_lens_plan.h — the GPU-free part of libsquigly_lens.so (include/squigly_lens.h): the workspace layout of a batch of sub-rays
// and the batch plan of a frame.  Plain host C++: batch() is the one place that cuts a sub-ray range into batches, plan() lists
// its batches and sq_lens_frame.h's render_batches enqueues them (over the pixels of a shard for libsquigly_lens.so, over those of
// a list for libsquigly_mlens.so), and tests/lens_plan_main.cpp runs it under the sanitizers without a device.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "sq_error.h"

namespace lensplan {

constexpr long long kMaxIndex = 0x7fffffffLL;      // pixels of a call, and ray slots of a batch: 32-bit indices in the kernels

inline size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

// The workspace of a batch of n ray slots: seeds first (8-byte entries), then origins, directions and sub-ray sums, each array
// starting at a multiple of 16 bytes.
struct Layout { size_t seed, org, dir, sum, total; };
inline Layout layout(long long n) {
    Layout L;
    const size_t n8 = align16((size_t)n * 8), n12 = align16((size_t)n * 12);
    L.seed = 0; L.org = n8; L.dir = n8 + n12; L.sum = n8 + 2 * n12; L.total = n8 + 3 * n12;
    return L;
}

inline size_t work_bytes(long long P, long long nb) {
    if (P < 1 || nb < 1 || P > kMaxIndex || nb > kMaxIndex / P) return 0;
    return layout(P * nb).total;
}

// The largest nb with work_bytes(P, nb) <= bytes and P * nb <= kMaxIndex; 0 when not even one sub-ray fits.  1 <= P <= kMaxIndex.
inline long long max_batch(long long P, size_t bytes) {
    long long nb = (long long)(bytes / (44 * (size_t)P));          // without the padding; the padding can only cost a few sub-rays
    if (nb > kMaxIndex / P) nb = kMaxIndex / P;
    while (nb > 0 && work_bytes(P, nb) > bytes) --nb;
    return nb;
}

// The batches of the sub-rays [r_begin, r_end), nb >= 1 at a time: how many there are, and batch i of them.
struct Batch { int32_t r0, r1; };
inline int64_t batch_count(int32_t r_begin, int32_t r_end, long long nb) { return ((int64_t)r_end - r_begin + nb - 1) / nb; }
inline Batch batch(int32_t r_begin, int32_t r_end, long long nb, int64_t i) {
    const int64_t r0 = r_begin + i * nb;
    return { (int32_t)r0, (int32_t)(r0 + nb < r_end ? r0 + nb : r_end) };
}

// sq_lens_plan.
inline int32_t plan(long long P, int32_t r_begin, int32_t r_end, size_t bytes, int32_t* out_r, int32_t cap) {
    if (P < 1) { sq_set_error("P must be at least 1 (got %lld)", P); return -1; }
    if (P > kMaxIndex) { sq_set_error("%lld pixels exceed 2^31 - 1 pixels in one call", P); return -1; }
    if (r_begin < 0 || r_end <= r_begin) { sq_set_error("bad sub-ray range [%d, %d) (need 0 <= r_begin < r_end)", r_begin, r_end); return -1; }
    const long long nb = max_batch(P, bytes);
    if (nb < 1) {
        sq_set_error("work_bytes = %zu is too small: one sub-ray of %lld pixels needs %zu", bytes, P, work_bytes(P, 1));
        return -1;
    }
    const int64_t count = batch_count(r_begin, r_end, nb);
    for (int64_t i = 0; out_r && i < count && i < cap; ++i) {
        const Batch b = batch(r_begin, r_end, nb, i);
        out_r[2 * i] = b.r0;
        out_r[2 * i + 1] = b.r1;
    }
    return (int32_t)count;
}

}  // namespace lensplan
