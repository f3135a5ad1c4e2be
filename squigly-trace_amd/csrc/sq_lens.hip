// sq_lens.hip — libsquigly_lens.so (include/squigly_lens.h): jittered, thin-lens primary rays around the radiance query of
// libsquigly_hip.so.  The library is a client of that library's public C-ABI: a frame is, per batch of whole sub-rays,
//     sq_lens_rays     one lane per (sub-ray, pixel): the ray and its seed base into the caller's workspace
//     sq_raytrace_rays_device                          the n = S / R samples of every ray, folded per ray
//     sq_lens_fold     one lane per pixel: the sub-ray sums into the pixel's sum and sum2 in sub-ray order, avg and its tonemap
// and the batches are those of sq_lens_plan.h.  No allocation, no state.
//
// Both kernels are memory-bound on [n][3] float arrays.  A lane moves its 12 bytes with one dwordx3 access and the 64 lanes of a
// wave cover 768 consecutive bytes, so every cache line a wave touches is used whole; slots are sub-ray-major, so that holds for
// the fold's reads of one sub-ray's sums as well.
//
// The arithmetic is header's, operation by operation; -ffp-contract=off and the correctly rounded divide / sqrt keep it equal to
// the numpy restatement (tests/lens_restatement.py).  A sub-ray's own arithmetic is csrc/sq_lens_ray.h's, which libsquigly_mlens.so
// (sq_mlens.hip: the same frame for the pixels of a list) includes too.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <string>

#include "sq_call_checks.h"
#include "sq_math.h"
#include "sq_lens_plan.h"
#include "sq_lens_ray.h"
#include "../../include/squigly_lens.h"

#ifndef SQ_LENS_BUILD_ID
#define SQ_LENS_BUILD_ID "unknown"
#endif

namespace {

using sq::f3;
using sq::load3;
using lensray::check_frame;
using lensray::RayArgs;
using lensray::ray_args;
using lensray::refuse_slots;

constexpr int kBlock = 256;
constexpr int kMaxGrid = 4096;             // blocks of a launch; the kernels stride over their slots

// ---- the rays: one lane per (sub-ray, pixel), slot = sub-ray * P + pixel ----
__global__ __launch_bounds__(kBlock) void sq_lens_rays(const RayArgs A, float* __restrict__ org, float* __restrict__ dir,
                                                       long long* __restrict__ seed) {
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < A.slots; i += (long long)gridDim.x * kBlock) {
        const int b = (int)(i / A.P);
        const lensray::Ray ray = lensray::sub_ray(A, (int)(i - b * A.P), A.r_begin + b);     // THE CONTRACT, csrc/sq_lens_ray.h
        store3(org, i, ray.o);
        store3(dir, i, ray.d);
        seed[i] = ray.base;
    }
}

// ---- the fold: one lane per pixel, the sub-ray sums part[b][pixel] in the order of b ----
__global__ __launch_bounds__(kBlock) void sq_lens_fold(const long long P, const int nb, const int carry, const float inv_s,
                                                       const float* __restrict__ part, float* __restrict__ sum,
                                                       float* __restrict__ sum2, float* __restrict__ avg, uint8_t* __restrict__ rgb) {
    for (long long p = (long long)blockIdx.x * kBlock + threadIdx.x; p < P; p += (long long)gridDim.x * kBlock) {
        f3 s, q;
        int b = 0;
        if (carry) {
            s = load3(sum, p);
            q = sum2 ? load3(sum2, p) : sq::mk(0.0f, 0.0f, 0.0f);
        } else {
            s = load3(part, p);
            q = s * s;
            b = 1;
        }
        for (; b < nb; ++b) {
            const f3 t = load3(part, (long long)b * P + p);
            s = s + t;
            q = q + t * t;
        }
        store3(sum, p, s);
        if (sum2) store3(sum2, p, q);
        if (avg || rgb) {
            const f3 a = sq::scale(inv_s, s);
            if (avg) store3(avg, p, a);
            if (rgb) tonemap(a, rgb + 3 * p);
        }
    }
}

unsigned grid_for(long long units) {
    const long long blocks = (units + kBlock - 1) / kBlock;
    return (unsigned)(blocks < kMaxGrid ? blocks : kMaxGrid);
}

// Enqueues the ray kernel for the sub-rays [r0, r1).
int enqueue_rays(RayArgs A, int32_t r0, int32_t r1, float* d_org, float* d_dir, int64_t* d_seed, hipStream_t stream) {
    A.r_begin = r0;
    A.slots = (long long)(r1 - r0) * A.P;
    static_assert(sizeof(long long) == sizeof(int64_t), "seed bases are 64-bit");
    hipLaunchKernelGGL(sq_lens_rays, dim3(grid_for(A.slots)), dim3(kBlock), 0, stream, A, d_org, d_dir, (long long*)d_seed);
    SQ_HIP(hipGetLastError());
    return 0;
}

int enqueue_fold(long long P, int32_t S, int32_t r0, int32_t r1, const float* d_part, float* d_sum, float* d_sum2, float* d_avg,
                 uint8_t* d_rgb, hipStream_t stream) {
    hipLaunchKernelGGL(sq_lens_fold, dim3(grid_for(P)), dim3(kBlock), 0, stream, P, (int)(r1 - r0), r0 > 0 ? 1 : 0, 1.0f / (float)S,
                       d_part, d_sum, d_sum2, d_avg, d_rgb);
    SQ_HIP(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" const char* sq_lens_last_error(void) { return sq_error_buffer(); }
extern "C" const char* sq_lens_build_id(void) { return SQ_LENS_BUILD_ID; }
extern "C" size_t sq_lens_work_bytes(int64_t P, int32_t nb) { return lensplan::work_bytes((long long)P, nb); }
extern "C" int32_t sq_lens_plan(int64_t P, int32_t r_begin, int32_t r_end, size_t work_bytes, int32_t* out_r, int32_t cap) {
    return lensplan::plan((long long)P, r_begin, r_end, work_bytes, out_r, cap);
}

extern "C" int sq_lens_rays_device(int32_t device, const sq_camera* cam, const sq_lens* lens, int32_t S, int32_t R, int32_t r_begin,
                                   int32_t r_end, int32_t w, int32_t h, sq_shard sh, float* d_org, float* d_dir, int64_t* d_seed,
                                   void* hip_stream) {
    long long P = 0;
    if (check_frame(cam, lens, S, R, r_begin, r_end, w, h, sh, &P)) return 1;
    if (!d_org || !d_dir || !d_seed) return sq_set_error("null argument: d_org, d_dir and d_seed are required");
    if (P == 0) return 0;                       // an empty shard (more shards than row blocks) has no pixels
    const long long nb = (long long)r_end - r_begin;
    if (refuse_slots(P, nb)) return 1;
    const size_t n = (size_t)(P * nb);
    const NamedRange spans[3] = { { "d_org", d_org, 12 * n }, { "d_dir", d_dir, 12 * n }, { "d_seed", d_seed, 8 * n } };
    if (refuse_overlaps(spans, 3)) return 1;
    SQ_HIP(hipSetDevice(device));
    return enqueue_rays(ray_args(cam, lens, S, R, w, h, sh, P), r_begin, r_end, d_org, d_dir, d_seed, (hipStream_t)hip_stream);
}

extern "C" int sq_lens_fold_device(int32_t device, int64_t P, int32_t S, int32_t r_begin, int32_t r_end, const float* d_part,
                                   float* d_sum, float* d_sum2, float* d_avg, uint8_t* d_rgb, void* hip_stream) {
    if (!d_part || !d_sum) return sq_set_error("null argument: d_part and d_sum are required");
    if (P < 1) return sq_set_error("P must be at least 1 (got %lld)", (long long)P);
    if (S < 1) return sq_set_error("samples must be at least 1 (got S = %d)", S);
    if (r_begin < 0 || r_end <= r_begin || r_end > S)
        return sq_set_error("bad sub-ray range [%d, %d) (need 0 <= r_begin < r_end <= S = %d)", r_begin, r_end, S);
    if (P > lensplan::kMaxIndex) return sq_set_error("%lld pixels exceed 2^31 - 1 pixels in one call", (long long)P);
    const long long nb = (long long)r_end - r_begin;
    if (refuse_slots((long long)P, nb)) return 1;
    const size_t p = (size_t)P;
    const NamedRange spans[5] = { { "d_part", d_part, 12 * p * (size_t)nb }, { "d_sum", d_sum, 12 * p }, { "d_sum2", d_sum2, 12 * p },
                                  { "d_avg", d_avg, 12 * p }, { "d_rgb", d_rgb, 3 * p } };
    if (refuse_overlaps(spans, 5)) return 1;
    SQ_HIP(hipSetDevice(device));
    return enqueue_fold((long long)P, S, r_begin, r_end, d_part, d_sum, d_sum2, d_avg, d_rgb, (hipStream_t)hip_stream);
}

extern "C" int sq_lens_render_device(sq_device_scene* s, const sq_camera* cam, const sq_lens* lens, int32_t S, int32_t R,
                                     int32_t r_begin, int32_t r_end, int32_t w, int32_t h, sq_shard sh, void* d_work, size_t work_bytes,
                                     float* d_sum, float* d_sum2, float* d_avg, uint8_t* d_rgb, void* hip_stream) {
    if (!s) return sq_set_error("null argument: the scene is required");
    long long P = 0;
    if (check_frame(cam, lens, S, R, r_begin, r_end, w, h, sh, &P)) return 1;
    if (!d_work || !d_sum) return sq_set_error("null argument: d_work and d_sum are required");
    if (P == 0) return 0;
    const long long nb_max = lensplan::max_batch(P, work_bytes);
    if (nb_max < 1)
        return sq_set_error("work_bytes = %zu is too small: one sub-ray of %lld pixels needs %zu", work_bytes, P, lensplan::work_bytes(P, 1));
    if ((uintptr_t)d_work % 16 != 0) return sq_set_error("d_work must be 16-byte aligned");
    const size_t p = (size_t)P;
    const NamedRange spans[5] = { { "d_sum", d_sum, 12 * p }, { "d_sum2", d_sum2, 12 * p }, { "d_avg", d_avg, 12 * p },
                                  { "d_rgb", d_rgb, 3 * p }, { "d_work", d_work, work_bytes } };
    if (refuse_overlaps(spans, 5)) return 1;
    hipPointerAttribute_t attr;
    SQ_HIP(hipPointerGetAttributes(&attr, d_work));
    const int device = attr.device;
    hipStream_t stream = (hipStream_t)hip_stream;
    const RayArgs A = ray_args(cam, lens, S, R, w, h, sh, P);
    for (long long r0 = r_begin; r0 < r_end; r0 += nb_max) {           // sq_lens_plan's batches
        const int32_t b0 = (int32_t)r0, b1 = (int32_t)(r0 + nb_max < r_end ? r0 + nb_max : r_end);
        const long long slots = (long long)(b1 - b0) * P;
        const lensplan::Layout L = lensplan::layout(slots);
        char* base = (char*)d_work;
        float* org = (float*)(base + L.org);
        float* dir = (float*)(base + L.dir);
        float* part = (float*)(base + L.sum);
        int64_t* seed = (int64_t*)(base + L.seed);
        SQ_HIP(hipSetDevice(device));
        if (enqueue_rays(A, b0, b1, org, dir, seed, stream)) return 1;
        if (sq_raytrace_rays_device(s, org, dir, seed, slots, 0, S / R, part, nullptr, nullptr, hip_stream)) {
            const std::string why = sq_last_error();                  // the two libraries may or may not share the message buffer
            return sq_set_error("%s", why.c_str());
        }
        SQ_HIP(hipSetDevice(device));
        if (enqueue_fold(P, S, b0, b1, part, d_sum, d_sum2, b1 == r_end ? d_avg : nullptr, b1 == r_end ? d_rgb : nullptr, stream)) return 1;
    }
    return 0;
}
