// sq_mlens.hip — libsquigly_mlens.so (include/squigly_mlens.h): the lens frame of libsquigly_lens.so for the live pixels of a mask.
// A client of libsquigly_hip.so's public C-ABI, as sq_lens.hip is: a frame is, per batch of whole sub-rays of the L listed pixels,
//     sq_mlens_rays    one lane per (sub-ray, list entry): the ray of csrc/sq_lens_ray.h and its seed base into the workspace
//     sq_raytrace_rays_device                              the n = S / R samples of every ray, folded per ray
//     sq_mlens_fold    one lane per list entry: the sub-ray sums into the listed pixel's sum, sum2, count, avg and tonemap
// and the batches are those of sq_lens_plan.h over L.  The list comes from
//     sq_mlens_live    the ordered compaction of the live pixels.
// No allocation, no state.  This file holds the compaction and the library's exports with their argument checks; the bodies of
// the ray and fold kernels, their launches and the batch loop are csrc/sq_lens_frame.h's, instantiated here for a list.
//
// The ray slots are dense in list order, so org, dir, seed and part keep the dense frame's access shape (a lane's 12 bytes in one
// dwordx3, a wave's 768 bytes consecutive); the per-pixel side is a gather and a scatter through the list, whose ascending order
// keeps the pixels of a wave close.
//
// The compaction.  The call has no workspace and may write nothing but the first L entries of d_index and *d_n_live, so a
// workgroup's total has nowhere to go where another workgroup could read it.  Each workgroup therefore counts the live pixels in
// front of its own pixels itself -- a read of 1 byte a pixel, 5 when the counts take part, 16 pixels a lane and round in 16-byte
// loads that do not depend on each other -- and ranks its own kGroupPixels pixels behind that count: wave ballots and popcounts for
// the rank within a wave, LDS for the offsets of the waves.  One launch, no workgroup waits for another, and the list is the
// ascending one whatever order the workgroups run in.  The price is that the workgroups read P * groups / 2 pixels between them
// instead of P, and that the last one reads all of them alone: DESIGN.md 4.22 has the measured time.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "sq_call_checks.h"
#include "sq_lens_frame.h"
#include "sq_lens_plan.h"
#include "sq_lens_ray.h"
#include "../../include/squigly_mlens.h"

#ifndef SQ_MLENS_BUILD_ID
#define SQ_MLENS_BUILD_ID "unknown"
#endif

namespace {

using lensframe::kBlock;
using lensframe::Pixels;
using lensray::RayArgs;

constexpr int kLiveBlock = 1024;           // the compaction: 16 waves a workgroup,
constexpr int kLiveWaves = kLiveBlock / 64;
constexpr int kLiveSteps = 32;             // each ranking 32 x 64 consecutive pixels
constexpr int kGroupPixels = kLiveWaves * kLiveSteps * 64;       // 32768 pixels a workgroup
constexpr int kFrontLane = 16;             // pixels a lane counts per round of the front count: one 16-byte load of mask bytes
constexpr int kFrontRound = kLiveBlock * kFrontLane;
static_assert(kGroupPixels % kFrontRound == 0, "the pixels in front of a workgroup are whole rounds of the front count");

__device__ __forceinline__ bool live_pixel(long long p, int r_begin, const uint8_t* __restrict__ mask, const int* __restrict__ count) {
    if (mask && mask[p] == 0) return false;
    return r_begin == 0 || !count || count[p] == r_begin;
}

// ---- the list: workgroup g owns the pixels [g * kGroupPixels, (g + 1) * kGroupPixels) ----
__global__ __launch_bounds__(kLiveBlock) void sq_mlens_live(const long long P, const int r_begin, const uint8_t* __restrict__ mask,
                                                            const int* __restrict__ count, int* __restrict__ index, int* __restrict__ n_live, const int vec) {
    __shared__ int s_front[kLiveWaves], s_own[kLiveWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long g0 = (long long)blockIdx.x * kGroupPixels;
    // the live pixels in front of the workgroup's, per wave: g0 is a multiple of kFrontRound, so every lane is in every round
    int front = 0;
    const bool guard = r_begin != 0 && count;
    if (vec) {                             // both arrays 16-byte aligned: a lane's 16 pixels are one uint4 of mask bytes and four int4 of counts
        for (long long p = (long long)threadIdx.x * kFrontLane; p < g0; p += kFrontRound) {
            uint4 m = make_uint4(0x01010101u, 0x01010101u, 0x01010101u, 0x01010101u);
            if (mask) m = *reinterpret_cast<const uint4*>(mask + p);
            const unsigned mw[4] = { m.x, m.y, m.z, m.w };
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                int4 c = make_int4(r_begin, r_begin, r_begin, r_begin);
                if (guard) c = *reinterpret_cast<const int4*>(count + p + 4 * q);
                front += ((mw[q] & 0xffu) != 0 && c.x == r_begin) + ((mw[q] & 0xff00u) != 0 && c.y == r_begin)
                       + ((mw[q] & 0xff0000u) != 0 && c.z == r_begin) + ((mw[q] & 0xff000000u) != 0 && c.w == r_begin);
            }
        }
    } else {
        for (long long p = threadIdx.x; p < g0; p += kLiveBlock) front += live_pixel(p, r_begin, mask, count) ? 1 : 0;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) front += __shfl_xor(front, off);
    // the wave's own pixels [w0, w0 + kLiveSteps * 64): one ballot a step
    const long long w0 = g0 + (long long)wave * (kLiveSteps * 64);
    unsigned long long votes[kLiveSteps];
    int own = 0;
#pragma unroll
    for (int i = 0; i < kLiveSteps; ++i) {
        const long long p = w0 + i * 64 + lane;
        votes[i] = __ballot(p < P && live_pixel(p, r_begin, mask, count));
        own += __popcll(votes[i]);
    }
    if (lane == 0) { s_front[wave] = front; s_own[wave] = own; }
    __syncthreads();
    int out = 0, total = 0;                            // out: the live pixels in front of the wave's; total: in front of the next workgroup's
    for (int v = 0; v < kLiveWaves; ++v) {
        out += s_front[v] + (v < wave ? s_own[v] : 0);
        total += s_front[v] + s_own[v];
    }
    const unsigned long long below = (1ull << lane) - 1;
#pragma unroll
    for (int i = 0; i < kLiveSteps; ++i) {
        if ((votes[i] >> lane) & 1) index[out + __popcll(votes[i] & below)] = (int)(w0 + i * 64 + lane);
        out += __popcll(votes[i]);
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) *n_live = total;
}

// ---- the rays: one lane per (sub-ray, list entry), slot = sub-ray * L + entry ----
__global__ __launch_bounds__(kBlock) void sq_mlens_rays(const RayArgs A, const long long L, const int* __restrict__ index,
                                                        float* __restrict__ org, float* __restrict__ dir, long long* __restrict__ seed) {
    lensframe::rays_body<true>(A, L, index, org, dir, seed, lensray::StaticRay{});
}

// ---- the fold: one lane per list entry, the sub-ray sums part[b][entry] in the order of b, into the listed pixel ----
__global__ __launch_bounds__(kBlock) void sq_mlens_fold(const long long P, const long long L, const int nb, const int carry, const int r_end,
                                                        const float inv, const int* __restrict__ index, const float* __restrict__ part,
                                                        float* __restrict__ sum, float* __restrict__ sum2, int* __restrict__ count,
                                                        float* __restrict__ avg, uint8_t* __restrict__ rgb) {
    lensframe::fold_body<true>(P, L, nb, carry, r_end, inv, index, part, sum, sum2, count, avg, rgb);
}

// What the three list-taking calls refuse about their list; P >= 1.
int check_list(const int32_t* d_index, int64_t L, long long P) {
    if (!d_index) return sq_set_error("null argument: d_index is required");
    if (L < 0 || L > P) return sq_set_error("the list must hold between 0 and P = %lld pixels (got L = %lld)", P, (long long)L);
    return 0;
}

}  // namespace

extern "C" const char* sq_mlens_last_error(void) { return sq_error_buffer(); }
extern "C" const char* sq_mlens_build_id(void) { return SQ_MLENS_BUILD_ID; }

extern "C" int sq_mlens_live_device(int32_t device, int64_t P, int32_t r_begin, const uint8_t* d_mask, const int32_t* d_count,
                                    int32_t* d_index, int32_t* d_n_live, void* hip_stream) {
    if (!d_index || !d_n_live) return sq_set_error("null argument: d_index and d_n_live are required");
    if (P < 1) return sq_set_error("P must be at least 1 (got %lld)", (long long)P);
    if (P > lensplan::kMaxIndex) return sq_set_error("%lld pixels exceed 2^31 - 1 pixels in one call", (long long)P);
    if (r_begin < 0) return sq_set_error("r_begin must be at least 0 (got %d)", r_begin);
    const size_t p = (size_t)P;
    const NamedRange spans[4] = { { "d_mask", d_mask, p }, { "d_count", d_count, 4 * p }, { "d_index", d_index, 4 * p }, { "d_n_live", d_n_live, 4 } };
    if (refuse_overlaps(spans, 4)) return 1;
    SQ_HIP(hipSetDevice(device));
    const unsigned groups = (unsigned)((P + kGroupPixels - 1) / kGroupPixels);        // at most 2^16
    const int vec = ((uintptr_t)d_mask | (uintptr_t)d_count) % 16 == 0 ? 1 : 0;        // (NULL counts as aligned: it is not read)
    hipLaunchKernelGGL(sq_mlens_live, dim3(groups), dim3(kLiveBlock), 0, (hipStream_t)hip_stream, (long long)P, (int)r_begin, d_mask,
                       (const int*)d_count, (int*)d_index, (int*)d_n_live, vec);
    SQ_HIP(hipGetLastError());
    return 0;
}

extern "C" int sq_mlens_rays_device(int32_t device, const sq_camera* cam, const sq_lens* lens, int32_t S, int32_t R, int32_t r_begin,
                                    int32_t r_end, int32_t w, int32_t h, sq_shard sh, const int32_t* d_index, int64_t L, float* d_org,
                                    float* d_dir, int64_t* d_seed, void* hip_stream) {
    long long P = 0;
    if (lensray::check_frame(cam, lens, S, R, r_begin, r_end, w, h, sh, &P)) return 1;
    if (!d_org || !d_dir || !d_seed) return sq_set_error("null argument: d_org, d_dir and d_seed are required");
    if (P == 0) return 0;                       // an empty shard (more shards than row blocks) has no pixels
    if (check_list(d_index, L, P)) return 1;
    if (L == 0) return 0;
    const long long nb = (long long)r_end - r_begin;
    if (lensray::refuse_slots((long long)L, nb)) return 1;
    const size_t n = (size_t)(L * nb);
    const NamedRange spans[4] = { { "d_index", d_index, 4 * (size_t)L }, { "d_org", d_org, 12 * n }, { "d_dir", d_dir, 12 * n }, { "d_seed", d_seed, 8 * n } };
    if (refuse_overlaps(spans, 4)) return 1;
    SQ_HIP(hipSetDevice(device));
    return lensframe::enqueue_rays<true>(sq_mlens_rays, lensray::ray_args(cam, lens, S, R, w, h, sh, P), Pixels{ P, (long long)L, d_index },
                                         r_begin, r_end, d_org, d_dir, d_seed, (hipStream_t)hip_stream);
}

extern "C" int sq_mlens_fold_device(int32_t device, int64_t P, int32_t S, int32_t R, int32_t r_begin, int32_t r_end, const int32_t* d_index,
                                    int64_t L, const float* d_part, float* d_sum, float* d_sum2, int32_t* d_count, float* d_avg,
                                    uint8_t* d_rgb, void* hip_stream) {
    if (lensray::check_fold(d_part, d_sum, (long long)P, S, &R, r_begin, r_end)) return 1;           // r_end <= R, and R divides S
    if (check_list(d_index, L, (long long)P)) return 1;
    if (L == 0) return 0;
    const long long nb = (long long)r_end - r_begin;
    if (lensray::refuse_slots((long long)L, nb)) return 1;
    const size_t p = (size_t)P, l = (size_t)L;
    const NamedRange spans[7] = { { "d_index", d_index, 4 * l }, { "d_part", d_part, 12 * l * (size_t)nb }, { "d_sum", d_sum, 12 * p },
                                  { "d_sum2", d_sum2, 12 * p }, { "d_count", d_count, 4 * p }, { "d_avg", d_avg, 12 * p }, { "d_rgb", d_rgb, 3 * p } };
    if (refuse_overlaps(spans, 7)) return 1;
    SQ_HIP(hipSetDevice(device));
    return lensframe::enqueue_fold<true>(sq_mlens_fold, Pixels{ (long long)P, (long long)L, d_index }, r_begin, r_end,
                                         1.0f / (float)((long long)r_end * (S / R)), d_part, d_sum, d_sum2, d_count, d_avg, d_rgb,
                                         (hipStream_t)hip_stream);
}

extern "C" int sq_mlens_render_device(sq_device_scene* s, const sq_camera* cam, const sq_lens* lens, int32_t S, int32_t R, int32_t r_begin,
                                      int32_t r_end, int32_t w, int32_t h, sq_shard sh, const int32_t* d_index, int64_t L, void* d_work,
                                      size_t work_bytes, float* d_sum, float* d_sum2, int32_t* d_count, float* d_avg, uint8_t* d_rgb,
                                      void* hip_stream) {
    if (!s) return sq_set_error("null argument: the scene is required");
    long long P = 0;
    if (lensray::check_frame(cam, lens, S, R, r_begin, r_end, w, h, sh, &P)) return 1;
    if (!d_work || !d_sum) return sq_set_error("null argument: d_work and d_sum are required");
    if (P == 0) return 0;
    if (check_list(d_index, L, P)) return 1;
    if (L == 0) return 0;
    const size_t p = (size_t)P;
    const NamedRange spans[7] = { { "d_index", d_index, 4 * (size_t)L }, { "d_sum", d_sum, 12 * p }, { "d_sum2", d_sum2, 12 * p },
                                  { "d_count", d_count, 4 * p }, { "d_avg", d_avg, 12 * p }, { "d_rgb", d_rgb, 3 * p }, { "d_work", d_work, work_bytes } };
    return lensframe::render_batches<true>(sq_mlens_rays, sq_mlens_fold, s, lensray::ray_args(cam, lens, S, R, w, h, sh, P),
                                           Pixels{ P, (long long)L, d_index }, r_begin, r_end, 1.0f / (float)((long long)r_end * (S / R)), d_work,
                                           work_bytes, spans, 7, d_sum, d_sum2, d_count, d_avg, d_rgb, hip_stream);
}
