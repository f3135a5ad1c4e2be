// sq_lens_frame.h — what libsquigly_lens.so (sq_lens.hip) and libsquigly_mlens.so (sq_mlens.hip) enqueue for a lens frame, written
// once: the bodies of the ray kernel and of the fold kernel, their launches, and the batch loop of a frame.  HIP only.
//
// Listed = false is the frame over every pixel of a shard: slot -> pixel is the identity and L = P.  Listed = true is the frame
// over the first L entries of a list of pixels: the ray slots stay dense in list order, the per-pixel side is a gather and a
// scatter through the list, and the fold also stores the pixel's sub-ray count.  The choice is made when the kernel is compiled,
// so the dense kernels carry no load of an index, no bounds test and no count store.
//
// Each library defines its own two __global__ kernels as calls of the bodies and hands them to the functions below.  The ray of a
// lane is a parameter of the ray kernel's body, chosen when the kernel is compiled like Listed: lensray::StaticRay for the frame's
// one camera, libsquigly_shutter.so's own for a camera that moves during the exposure -- the static kernels carry none of that.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <type_traits>

#include "sq_call_checks.h"
#include "sq_lens_plan.h"
#include "sq_lens_ray.h"
#include "sq_math.h"
#include "../../include/squigly_hip.h"

namespace lensframe {

using lensray::RayArgs;
using sq::f3;
using sq::load3;

constexpr int kBlock = 256;
constexpr int kMaxGrid = 4096;             // blocks of a launch; the kernels stride over their slots

inline unsigned grid_for(long long units) {
    const long long blocks = (units + kBlock - 1) / kBlock;
    return (unsigned)(blocks < kMaxGrid ? blocks : kMaxGrid);
}

// ---- the rays: one lane per (sub-ray, entry), slot = sub-ray * L + entry; the entry is the pixel, or names it through the list ----
template <bool Listed, typename RayOf>
__device__ __forceinline__ void rays_body(const RayArgs& A, const long long L, const int* __restrict__ index, float* __restrict__ org,
                                          float* __restrict__ dir, long long* __restrict__ seed, const RayOf ray_of) {
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < A.slots; i += (long long)gridDim.x * kBlock) {
        const int b = (int)(i / L);
        lensray::Ray ray;
        if constexpr (Listed) {
            const int pixel = index[i - b * L];
            if (pixel < 0 || pixel >= A.P) {                     // a wrong list is no out-of-range pixel: a ray of zeros
                ray.o = ray.d = sq::mk(0.0f, 0.0f, 0.0f);
                ray.base = 0;
            } else {
                ray = ray_of(A, pixel, A.r_begin + b);                // THE CONTRACT, csrc/sq_lens_ray.h
            }
        } else {
            ray = ray_of(A, (int)(i - b * L), A.r_begin + b);
        }
        store3(org, i, ray.o);
        store3(dir, i, ray.d);
        seed[i] = ray.base;
    }
}

// ---- the fold: one lane per entry, the sub-ray sums part[b][entry] in the order of b, into the entry's pixel ----
template <bool Listed>
__device__ __forceinline__ void fold_body(const long long P, const long long L, const int nb, const int carry, const int r_end,
                                          const float inv, const int* __restrict__ index, const float* __restrict__ part,
                                          float* __restrict__ sum, float* __restrict__ sum2, int* __restrict__ count,
                                          float* __restrict__ avg, uint8_t* __restrict__ rgb) {
    for (long long j = (long long)blockIdx.x * kBlock + threadIdx.x; j < L; j += (long long)gridDim.x * kBlock) {
        long long p = j;
        if constexpr (Listed) {
            p = index[j];
            if (p < 0 || p >= P) continue;
        }
        f3 s, q;
        int b = 0;
        if (carry) {
            s = load3(sum, p);
            q = sum2 ? load3(sum2, p) : sq::mk(0.0f, 0.0f, 0.0f);
        } else {
            s = load3(part, j);
            q = s * s;
            b = 1;
        }
        for (; b < nb; ++b) {
            const f3 t = load3(part, (long long)b * L + j);
            s = s + t;
            q = q + t * t;
        }
        store3(sum, p, s);
        if (sum2) store3(sum2, p, q);
        if constexpr (Listed) {
            if (count) count[p] = r_end;
        }
        if (avg || rgb) {
            const f3 a = sq::scale(inv, s);
            if (avg) store3(avg, p, a);
            if (rgb) tonemap(a, rgb + 3 * p);
        }
    }
}

// What a frame is made over: the P pixels of the shard (L = P, index = NULL), or the first L entries of a list of them.
struct Pixels { long long P, L; const int32_t* index; };

// Launches a ray kernel.  `kernel` is the __global__ function itself when it takes RayArgs and the buffers only; a library whose
// ray kernel takes more (libsquigly_shutter.so: the motion) hands in an object that is called with the grid, the stream and those
// arguments, and launches its kernel itself.
template <typename Kernel, typename... Args>
void launch_rays(Kernel kernel, unsigned grid, hipStream_t stream, Args... args) {
    if constexpr (std::is_pointer_v<Kernel>)
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), 0, stream, args...);
    else
        kernel(grid, stream, args...);
}

// Enqueues `kernel`, the library's ray kernel, for the sub-rays [r0, r1).
template <bool Listed, typename Kernel>
int enqueue_rays(Kernel kernel, RayArgs A, Pixels px, int32_t r0, int32_t r1, float* d_org, float* d_dir, int64_t* d_seed, hipStream_t stream) {
    A.r_begin = r0;
    A.slots = (long long)(r1 - r0) * px.L;
    static_assert(sizeof(long long) == sizeof(int64_t), "seed bases are 64-bit");
    if constexpr (Listed)
        launch_rays(kernel, grid_for(A.slots), stream, A, px.L, (const int*)px.index, d_org, d_dir, (long long*)d_seed);
    else
        launch_rays(kernel, grid_for(A.slots), stream, A, d_org, d_dir, (long long*)d_seed);
    SQ_HIP(hipGetLastError());
    return 0;
}

// Enqueues `kernel`, the library's fold kernel, for the sub-rays [r0, r1).  inv: what avg is of sum -- the caller's, because the two
// headers define it differently.  d_count (Listed only), d_avg and d_rgb may be NULL.
template <bool Listed, typename Kernel>
int enqueue_fold(Kernel kernel, Pixels px, int32_t r0, int32_t r1, float inv, const float* d_part, float* d_sum, float* d_sum2,
                 int32_t* d_count, float* d_avg, uint8_t* d_rgb, hipStream_t stream) {
    const int nb = (int)(r1 - r0), carry = r0 > 0 ? 1 : 0;
    if constexpr (Listed)
        hipLaunchKernelGGL(kernel, dim3(grid_for(px.L)), dim3(kBlock), 0, stream, px.P, px.L, nb, carry, (int)r1, inv, (const int*)px.index,
                           d_part, d_sum, d_sum2, (int*)d_count, d_avg, d_rgb);
    else
        hipLaunchKernelGGL(kernel, dim3(grid_for(px.P)), dim3(kBlock), 0, stream, px.P, nb, carry, inv, d_part, d_sum, d_sum2, d_avg, d_rgb);
    SQ_HIP(hipGetLastError());
    return 0;
}

// The frame behind both _render_device calls, once their own arguments are checked: the sub-rays [r_begin, r_end) of px in
// sq_lens_plan.h's batches of as many whole sub-rays as the workspace holds -- rays, the radiance query, fold.  spans: the call's
// buffers, which must not overlap.  inv, d_count, d_avg and d_rgb are the last batch's only: it alone completes the range.
template <bool Listed, typename RayKernel, typename FoldKernel>
int render_batches(RayKernel rays, FoldKernel fold, sq_device_scene* s, const RayArgs& A, Pixels px, int32_t r_begin, int32_t r_end,
                   float inv, void* d_work, size_t work_bytes, const NamedRange* spans, int n_spans, float* d_sum, float* d_sum2,
                   int32_t* d_count, float* d_avg, uint8_t* d_rgb, void* hip_stream) {
    const long long nb_max = lensplan::max_batch(px.L, work_bytes);       // never more than 2^31 - 1 slots a batch
    if (nb_max < 1)
        return sq_set_error("work_bytes = %zu is too small: one sub-ray of %lld pixels needs %zu", work_bytes, px.L, lensplan::work_bytes(px.L, 1));
    if ((uintptr_t)d_work % 16 != 0) return sq_set_error("d_work must be 16-byte aligned");
    if (refuse_overlaps(spans, n_spans)) return 1;
    hipPointerAttribute_t attr;
    SQ_HIP(hipPointerGetAttributes(&attr, d_work));
    const int device = attr.device;
    hipStream_t stream = (hipStream_t)hip_stream;
    const int64_t batches = lensplan::batch_count(r_begin, r_end, nb_max);
    for (int64_t i = 0; i < batches; ++i) {
        const lensplan::Batch b = lensplan::batch(r_begin, r_end, nb_max, i);
        const long long slots = (long long)(b.r1 - b.r0) * px.L;
        const lensplan::Layout lay = lensplan::layout(slots);
        char* base = (char*)d_work;
        float* org = (float*)(base + lay.org);
        float* dir = (float*)(base + lay.dir);
        float* part = (float*)(base + lay.sum);
        int64_t* seed = (int64_t*)(base + lay.seed);
        const bool last = b.r1 == r_end;
        SQ_HIP(hipSetDevice(device));
        if (enqueue_rays<Listed>(rays, A, px, b.r0, b.r1, org, dir, seed, stream)) return 1;
        if (sq_raytrace_rays_device(s, org, dir, seed, slots, 0, A.n, part, nullptr, nullptr, hip_stream)) {
            const std::string why = sq_last_error();                  // the two libraries may or may not share the message buffer
            return sq_set_error("%s", why.c_str());
        }
        SQ_HIP(hipSetDevice(device));
        if (enqueue_fold<Listed>(fold, px, b.r0, b.r1, inv, part, d_sum, d_sum2, last ? d_count : nullptr, last ? d_avg : nullptr,
                                 last ? d_rgb : nullptr, stream)) return 1;
    }
    return 0;
}

}  // namespace lensframe
