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
// the numpy restatement (tests/lens_restatement.py).  This file holds the library's exports and their argument checks.  The kernel
// bodies, their launches and the batch loop are csrc/sq_lens_frame.h's, which libsquigly_mlens.so (sq_mlens.hip: the same frame for
// the pixels of a list) instantiates the other way; a sub-ray's own arithmetic is csrc/sq_lens_ray.h's.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "sq_call_checks.h"
#include "sq_lens_frame.h"
#include "sq_lens_plan.h"
#include "sq_lens_ray.h"
#include "../../include/squigly_lens.h"

#ifndef SQ_LENS_BUILD_ID
#define SQ_LENS_BUILD_ID "unknown"
#endif

namespace {

using lensframe::kBlock;
using lensframe::Pixels;
using lensray::check_frame;
using lensray::RayArgs;
using lensray::ray_args;
using lensray::refuse_slots;

// ---- the rays: one lane per (sub-ray, pixel), slot = sub-ray * P + pixel ----
__global__ __launch_bounds__(kBlock) void sq_lens_rays(const RayArgs A, float* __restrict__ org, float* __restrict__ dir,
                                                       long long* __restrict__ seed) {
    lensframe::rays_body<false>(A, A.P, nullptr, org, dir, seed, lensray::StaticRay{});
}

// ---- the fold: one lane per pixel, the sub-ray sums part[b][pixel] in the order of b ----
__global__ __launch_bounds__(kBlock) void sq_lens_fold(const long long P, const int nb, const int carry, const float inv_s,
                                                       const float* __restrict__ part, float* __restrict__ sum,
                                                       float* __restrict__ sum2, float* __restrict__ avg, uint8_t* __restrict__ rgb) {
    lensframe::fold_body<false>(P, P, nb, carry, 0, inv_s, nullptr, part, sum, sum2, nullptr, avg, rgb);
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
    return lensframe::enqueue_rays<false>(sq_lens_rays, ray_args(cam, lens, S, R, w, h, sh, P), Pixels{ P, P, nullptr }, r_begin, r_end, d_org,
                                          d_dir, d_seed, (hipStream_t)hip_stream);
}

extern "C" int sq_lens_fold_device(int32_t device, int64_t P, int32_t S, int32_t r_begin, int32_t r_end, const float* d_part,
                                   float* d_sum, float* d_sum2, float* d_avg, uint8_t* d_rgb, void* hip_stream) {
    if (lensray::check_fold(d_part, d_sum, (long long)P, S, nullptr, r_begin, r_end)) return 1;       // no R here: r_end <= S
    const long long nb = (long long)r_end - r_begin;
    if (refuse_slots((long long)P, nb)) return 1;
    const size_t p = (size_t)P;
    const NamedRange spans[5] = { { "d_part", d_part, 12 * p * (size_t)nb }, { "d_sum", d_sum, 12 * p }, { "d_sum2", d_sum2, 12 * p },
                                  { "d_avg", d_avg, 12 * p }, { "d_rgb", d_rgb, 3 * p } };
    if (refuse_overlaps(spans, 5)) return 1;
    SQ_HIP(hipSetDevice(device));
    return lensframe::enqueue_fold<false>(sq_lens_fold, Pixels{ (long long)P, (long long)P, nullptr }, r_begin, r_end, 1.0f / (float)S, d_part,
                                          d_sum, d_sum2, nullptr, d_avg, d_rgb, (hipStream_t)hip_stream);
}

extern "C" int sq_lens_render_device(sq_device_scene* s, const sq_camera* cam, const sq_lens* lens, int32_t S, int32_t R,
                                     int32_t r_begin, int32_t r_end, int32_t w, int32_t h, sq_shard sh, void* d_work, size_t work_bytes,
                                     float* d_sum, float* d_sum2, float* d_avg, uint8_t* d_rgb, void* hip_stream) {
    if (!s) return sq_set_error("null argument: the scene is required");
    long long P = 0;
    if (check_frame(cam, lens, S, R, r_begin, r_end, w, h, sh, &P)) return 1;
    if (!d_work || !d_sum) return sq_set_error("null argument: d_work and d_sum are required");
    if (P == 0) return 0;
    const size_t p = (size_t)P;
    const NamedRange spans[5] = { { "d_sum", d_sum, 12 * p }, { "d_sum2", d_sum2, 12 * p }, { "d_avg", d_avg, 12 * p },
                                  { "d_rgb", d_rgb, 3 * p }, { "d_work", d_work, work_bytes } };
    return lensframe::render_batches<false>(sq_lens_rays, sq_lens_fold, s, ray_args(cam, lens, S, R, w, h, sh, P), Pixels{ P, P, nullptr },
                                            r_begin, r_end, 1.0f / (float)S, d_work, work_bytes, spans, 5, d_sum, d_sum2, nullptr, d_avg,
                                            d_rgb, hip_stream);
}
