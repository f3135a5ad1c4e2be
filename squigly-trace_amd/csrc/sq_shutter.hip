// sq_shutter.hip — libsquigly_shutter.so (include/squigly_shutter.h): motion blur, the lens frame of libsquigly_lens.so and of
// libsquigly_mlens.so under a camera that moves while the shutter is open.  A client of libsquigly_hip.so's public C-ABI, as the two
// lens libraries are: a frame is, per batch of whole sub-rays,
//     sq_shutter_rays / _rays_listed    one lane per (sub-ray, pixel or list entry): the instant, the pose of that instant, and the
//                                       ray of csrc/sq_lens_ray.h under that pose, with its seed base, into the workspace
//     sq_raytrace_rays_device           the n = S / R samples of every ray, folded per ray
//     sq_shutter_fold / _fold_listed    csrc/sq_lens_frame.h's fold, dense or through the list
// and the batches are those of sq_lens_plan.h.  No allocation, no state.
//
// Every lane computes its own pose (csrc/sq_shutter_pose.h: three crd sine / cosine pairs and two 3 x 3 products): with
// time_jitter > 0 no two lanes share an instant, and with time_jitter = 0 the lanes of a sub-ray do, but a table of R poses would
// need a kernel, a buffer and a contract of its own for what DESIGN.md 4.23 measures as a small part of a frame.  The kernels stay
// memory-shaped as the lens kernels are: a lane's 12 bytes in one dwordx3, a wave's 768 bytes consecutive.
//
// This file holds the moving camera, the library's four kernels and its exports with their argument checks; the kernel bodies,
// their launches and the batch loop are csrc/sq_lens_frame.h's, instantiated here with csrc/sq_lens_ray.h's sub-ray under the moving camera.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "sq_call_checks.h"
#include "sq_lens_frame.h"
#include "sq_lens_plan.h"
#include "sq_lens_ray.h"
#include "sq_shutter_pose.h"
#include "../../include/squigly_shutter.h"

#ifndef SQ_SHUTTER_BUILD_ID
#define SQ_SHUTTER_BUILD_ID "unknown"
#endif

namespace {

using lensframe::kBlock;
using lensframe::Pixels;
using lensray::RayArgs;
using shutterpose::Motion;

// THE CONTRACT of include/squigly_shutter.h for one sub-ray's camera: the instant and its pose, what lensray::sub_ray is given.
struct MovingCamera {
    Motion M;
    __device__ __forceinline__ bool plain(const RayArgs& A) const { return A.jitter == 0.0f && A.aperture == 0.0f && M.time_jitter == 0.0f; }
    __device__ __forceinline__ lensray::Camera operator()(const RayArgs& A, int r, bool plain, const uint64_t* c, float* moved) const {
        const float u4 = plain ? 0.0f : sq::unit_float((uint32_t)c[2]);          // m4: the low half of the block's third word
        const float tt = shutterpose::instant(r, A.S / A.n, M.time_jitter, u4);
        shutterpose::pose_at(M, tt, moved, moved + 3);
        return lensray::Camera{ moved, moved + 3 };
    }
};
using MovingRay = lensray::RayUnder<MovingCamera>;

// ---- the rays: one lane per (sub-ray, pixel), slot = sub-ray * P + pixel; A.pos and A.rot are not read ----
__global__ __launch_bounds__(kBlock) void sq_shutter_rays(const RayArgs A, const Motion M, float* __restrict__ org, float* __restrict__ dir,
                                                          long long* __restrict__ seed) {
    lensframe::rays_body<false>(A, A.P, nullptr, org, dir, seed, MovingRay{ MovingCamera{ M } });
}

// ---- the rays of a list: one lane per (sub-ray, list entry), slot = sub-ray * L + entry ----
__global__ __launch_bounds__(kBlock) void sq_shutter_rays_listed(const RayArgs A, const Motion M, const long long L, const int* __restrict__ index,
                                                                 float* __restrict__ org, float* __restrict__ dir, long long* __restrict__ seed) {
    lensframe::rays_body<true>(A, L, index, org, dir, seed, MovingRay{ MovingCamera{ M } });
}

// ---- the folds: csrc/sq_lens_frame.h's, one lane per pixel or per list entry ----
__global__ __launch_bounds__(kBlock) void sq_shutter_fold(const long long P, const int nb, const int carry, const float inv_s,
                                                          const float* __restrict__ part, float* __restrict__ sum,
                                                          float* __restrict__ sum2, float* __restrict__ avg, uint8_t* __restrict__ rgb) {
    lensframe::fold_body<false>(P, P, nb, carry, 0, inv_s, nullptr, part, sum, sum2, nullptr, avg, rgb);
}

__global__ __launch_bounds__(kBlock) void sq_shutter_fold_listed(const long long P, const long long L, const int nb, const int carry,
                                                                 const int r_end, const float inv, const int* __restrict__ index,
                                                                 const float* __restrict__ part, float* __restrict__ sum,
                                                                 float* __restrict__ sum2, int* __restrict__ count, float* __restrict__ avg,
                                                                 uint8_t* __restrict__ rgb) {
    lensframe::fold_body<true>(P, L, nb, carry, r_end, inv, index, part, sum, sum2, count, avg, rgb);
}

// What lensframe::enqueue_rays launches for this library: the ray kernel with the motion behind RayArgs.
template <typename Kernel>
struct MovingLaunch {
    Kernel kernel;
    Motion M;
    template <typename... Rest>
    void operator()(unsigned grid, hipStream_t stream, const RayArgs& A, Rest... rest) const {
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), 0, stream, A, M, rest...);
    }
};
template <typename Kernel>
MovingLaunch<Kernel> moving(Kernel kernel, const Motion& M) { return MovingLaunch<Kernel>{ kernel, M }; }

Motion motion_args(const sq_motion* m) { return shutterpose::motion_of(m->pos0, m->ang0, m->pos1, m->ang1, m->time_jitter); }

// What both frame calls refuse about their frame: lensray::check_frame's list, then the time jitter.  The frame has no one camera:
// check_frame and ray_args get a camera of zeros, which the moving kernels never read.
const sq_camera kNoCamera = {};

int check_moving_frame(const sq_motion* motion, const sq_lens* lens, int32_t S, int32_t R, int32_t r_begin, int32_t r_end, int32_t w, int32_t h,
                       sq_shard sh, long long* P_out) {
    if (!motion || !lens) return sq_set_error("null argument: motion and lens are required");
    if (lensray::check_frame(&kNoCamera, lens, S, R, r_begin, r_end, w, h, sh, P_out)) return 1;
    if (!(motion->time_jitter >= 0.0f && motion->time_jitter <= 1.0f))
        return sq_set_error("time_jitter must be a number in [0, 1] (got %g)", (double)motion->time_jitter);
    return 0;
}

// What the list-taking forms refuse about their list; P >= 1.
int check_list(int64_t L, long long P) {
    if (L < 0 || L > P) return sq_set_error("the list must hold between 0 and P = %lld pixels (got L = %lld)", P, (long long)L);
    return 0;
}

}  // namespace

extern "C" const char* sq_shutter_last_error(void) { return sq_error_buffer(); }
extern "C" const char* sq_shutter_build_id(void) { return SQ_SHUTTER_BUILD_ID; }

extern "C" int sq_shutter_pose(const sq_motion* motion, float tt, sq_camera* out) {
    if (!motion || !out) return sq_set_error("null argument: motion and out are required");
    shutterpose::pose_at(motion_args(motion), tt, out->pos, out->rot);
    return 0;
}

extern "C" int sq_shutter_rays_device(int32_t device, const sq_motion* motion, const sq_lens* lens, int32_t S, int32_t R, int32_t r_begin,
                                      int32_t r_end, int32_t w, int32_t h, sq_shard sh, const int32_t* d_index, int64_t L, float* d_org,
                                      float* d_dir, int64_t* d_seed, void* hip_stream) {
    long long P = 0;
    if (check_moving_frame(motion, lens, S, R, r_begin, r_end, w, h, sh, &P)) return 1;
    if (!d_org || !d_dir || !d_seed) return sq_set_error("null argument: d_org, d_dir and d_seed are required");
    if (P == 0) return 0;                       // an empty shard (more shards than row blocks) has no pixels
    if (d_index && check_list(L, P)) return 1;
    const long long pixels = d_index ? (long long)L : P;
    if (pixels == 0) return 0;
    const long long nb = (long long)r_end - r_begin;
    if (lensray::refuse_slots(pixels, nb)) return 1;
    const size_t n = (size_t)(pixels * nb);
    const NamedRange spans[4] = { { "d_index", d_index, 4 * (size_t)(d_index ? L : 0) }, { "d_org", d_org, 12 * n }, { "d_dir", d_dir, 12 * n },
                                  { "d_seed", d_seed, 8 * n } };
    if (refuse_overlaps(spans, 4)) return 1;
    SQ_HIP(hipSetDevice(device));
    const RayArgs A = lensray::ray_args(&kNoCamera, lens, S, R, w, h, sh, P);
    const Motion M = motion_args(motion);
    if (d_index)
        return lensframe::enqueue_rays<true>(moving(sq_shutter_rays_listed, M), A, Pixels{ P, (long long)L, d_index }, r_begin, r_end, d_org,
                                             d_dir, d_seed, (hipStream_t)hip_stream);
    return lensframe::enqueue_rays<false>(moving(sq_shutter_rays, M), A, Pixels{ P, P, nullptr }, r_begin, r_end, d_org, d_dir, d_seed,
                                          (hipStream_t)hip_stream);
}

extern "C" int sq_shutter_render_device(sq_device_scene* s, const sq_motion* motion, const sq_lens* lens, int32_t S, int32_t R, int32_t r_begin,
                                        int32_t r_end, int32_t w, int32_t h, sq_shard sh, const int32_t* d_index, int64_t L, void* d_work,
                                        size_t work_bytes, float* d_sum, float* d_sum2, int32_t* d_count, float* d_avg, uint8_t* d_rgb,
                                        void* hip_stream) {
    if (!s) return sq_set_error("null argument: the scene is required");
    long long P = 0;
    if (check_moving_frame(motion, lens, S, R, r_begin, r_end, w, h, sh, &P)) return 1;
    if (!d_work || !d_sum) return sq_set_error("null argument: d_work and d_sum are required");
    if (!d_index && d_count) return sq_set_error("d_count needs a list: the dense frame counts nothing (d_index is NULL)");
    if (P == 0) return 0;
    if (d_index && check_list(L, P)) return 1;
    if (d_index && L == 0) return 0;
    const size_t p = (size_t)P;
    const NamedRange spans[7] = { { "d_index", d_index, 4 * (size_t)(d_index ? L : 0) }, { "d_sum", d_sum, 12 * p }, { "d_sum2", d_sum2, 12 * p },
                                  { "d_count", d_count, 4 * p }, { "d_avg", d_avg, 12 * p }, { "d_rgb", d_rgb, 3 * p }, { "d_work", d_work, work_bytes } };
    const RayArgs A = lensray::ray_args(&kNoCamera, lens, S, R, w, h, sh, P);
    const Motion M = motion_args(motion);
    if (d_index)
        return lensframe::render_batches<true>(moving(sq_shutter_rays_listed, M), sq_shutter_fold_listed, s, A, Pixels{ P, (long long)L, d_index },
                                               r_begin, r_end, 1.0f / (float)((long long)r_end * (S / R)), d_work, work_bytes, spans, 7, d_sum,
                                               d_sum2, d_count, d_avg, d_rgb, hip_stream);
    return lensframe::render_batches<false>(moving(sq_shutter_rays, M), sq_shutter_fold, s, A, Pixels{ P, P, nullptr }, r_begin, r_end,
                                            1.0f / (float)S, d_work, work_bytes, spans, 7, d_sum, d_sum2, nullptr, d_avg, d_rgb, hip_stream);
}
