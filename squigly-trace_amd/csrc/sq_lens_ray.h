// sq_lens_ray.h — what libsquigly_lens.so and libsquigly_mlens.so share about one sub-ray and about a call's arguments, written
// once: THE CONTRACT of include/squigly_lens.h for one (pixel, sub-ray) as a device function, the kernel arguments it reads, and
// the host checks of a frame's and of a fold's arguments.  The kernels that run it and the frame's batch loop are sq_lens_frame.h's.
//
// The arithmetic is the header's, operation by operation; -ffp-contract=off and the correctly rounded divide / sqrt keep it equal
// to the numpy restatement (tests/lens_restatement.py).
#pragma once
#include <stdint.h>

#include "sq_error.h"
#include "sq_lens_plan.h"
#include "sq_math.h"
#include "../../include/squigly_lens.h"

namespace lensray {

struct RayArgs {
    float pos[3], rot[9];
    float jitter, aperture, focus;
    int S, n, r_begin;                      // samples per pixel, samples per sub-ray, first sub-ray of the batch
    int w, h, row_block, shard, n_shards;
    long long P, slots;                     // pixels of the shard; ray slots of the batch
};

struct Ray { sq::f3 o, d; long long base; };

#if defined(__HIPCC__)
// The camera a sub-ray is made under.  The arithmetic of a sub-ray is one text (sub_ray below); whose camera it is under is a
// parameter chosen when the kernel is compiled:
//     camera.plain(A)                      whether the frame makes no draw at all
//     camera(A, r, plain, c, moved)        the Camera of sub-ray r; c is the Threefish block of ~base, drawn unless plain; moved is
//                                          12 floats of the lane's own a camera that depends on the sub-ray may return pointers into
struct Camera { const float* pos; const float* rot; };

// The frame's one camera: RayArgs' pos and rot, whatever the sub-ray.
struct StaticCamera {
    __device__ __forceinline__ bool plain(const RayArgs& A) const {
        return A.jitter == 0.0f && A.aperture == 0.0f;     // makeRay's ray: x + 0 * u is x for every draw u, so no draw is made
    }
    __device__ __forceinline__ Camera operator()(const RayArgs& A, int, bool, const uint64_t*, float*) const { return Camera{ A.pos, A.rot }; }
};

// o, d and base of sub-ray r of local pixel `pixel` of the shard.
template <typename CameraOf>
__device__ __forceinline__ Ray sub_ray(const RayArgs& A, int pixel, int r, const CameraOf& camera_of) {
    const float ww = (float)A.w, hh = (float)A.h;
    const bool plain = camera_of.plain(A);
    const int j = pixel / A.h, x = pixel - j * A.h;
    const int blk = j / A.row_block;     // sq::shard_global_row, written out: through the function the kernel's registers are allocated differently
    const int y = (blk * A.n_shards + A.shard) * A.row_block + (j - blk * A.row_block);
    Ray ray;
    ray.base = (long long)A.S * ((long long)x + (long long)y * A.w) + (long long)r * A.n;
    float xs = (float)x, ys = (float)y;
    float u2 = 0.0f, u3 = 0.0f;
    uint64_t c[4];
    if (!plain) {
        sq::threefish256_key_only(~(uint64_t)ray.base, c);
        xs = (float)x + A.jitter * sq::unit_float((uint32_t)c[0]);
        ys = (float)y + A.jitter * sq::unit_float((uint32_t)(c[0] >> 32));
        u2 = sq::unit_float((uint32_t)c[1]);
        u3 = sq::unit_float((uint32_t)(c[1] >> 32));
    }
    const float xoffs = (xs - (ww / 2)) / ww;
    const float yoffs = ((hh / 2) - ys) / hh;
    float moved[12];
    const Camera cam = camera_of(A, r, plain, c, moved);
    ray.o = sq::mk(cam.pos[0], cam.pos[1], cam.pos[2]);
    if (A.aperture == 0.0f) {
        ray.d = sq::rot_vert(1.0f, xoffs, yoffs, cam.rot);
    } else {
        const float rad = A.aperture * sq::fsqrt(u2);
        const float th = 2 * sq::kPi * u3;
        float sth, cth;
        sq::fsincos(th, sth, cth);
        const float lx = rad * cth, ly = rad * sth;
        ray.o = ray.o + sq::rot_vert(0.0f, lx, ly, cam.rot);
        ray.d = sq::rot_vert(1.0f, xoffs - lx / A.focus, yoffs - ly / A.focus, cam.rot);
    }
    return ray;
}

// The per-lane ray function lensframe::rays_body is given: sub_ray under the library's camera.
template <typename CameraOf>
struct RayUnder {
    CameraOf camera_of;
    __device__ __forceinline__ Ray operator()(const RayArgs& A, int pixel, int r) const { return sub_ray(A, pixel, r, camera_of); }
};
using StaticRay = RayUnder<StaticCamera>;
#endif

// What every ray-making call refuses about its frame, in the order of the header's list; *P_out = the shard's pixels (0: empty).
inline int check_frame(const sq_camera* cam, const sq_lens* lens, int32_t S, int32_t R, int32_t r_begin, int32_t r_end, int32_t w, int32_t h,
                       sq_shard sh, long long* P_out) {
    if (!cam || !lens) return sq_set_error("null argument: cam and lens are required");
    if (S < 1 || R < 1) return sq_set_error("samples and sub-rays must be at least 1 (got S = %d, R = %d)", S, R);
    if (S % R != 0) return sq_set_error("the sub-rays must divide the samples (got S = %d, R = %d)", S, R);
    if (r_begin < 0 || r_end <= r_begin || r_end > R)
        return sq_set_error("bad sub-ray range [%d, %d) (need 0 <= r_begin < r_end <= R = %d)", r_begin, r_end, R);
    if (!(lens->jitter >= 0.0f && lens->jitter <= 1.0f)) return sq_set_error("jitter must be a number in [0, 1] (got %g)", (double)lens->jitter);
    if (!(lens->aperture >= 0.0f && lens->aperture < __builtin_inff()))
        return sq_set_error("aperture must be a finite number >= 0 (got %g)", (double)lens->aperture);
    if (lens->aperture > 0.0f && !(lens->focus > 0.0f && lens->focus < __builtin_inff()))
        return sq_set_error("focus must be a finite number > 0 when the aperture is open (got %g)", (double)lens->focus);
    if (w < 1 || h < 1) return sq_set_error("w and h must be at least 1 (got %d x %d)", w, h);
    const int32_t rows = sq_shard_rows(w, sh);
    if (rows < 0) return sq_set_error("bad shard {row_block=%d, shard=%d, n_shards=%d}", sh.row_block, sh.shard, sh.n_shards);
    const long long P = (long long)rows * h;
    if (P > lensplan::kMaxIndex) return sq_set_error("%d x %d pixels exceed 2^31 - 1 pixels in one call", rows, h);
    *P_out = P;
    return 0;
}

// What both fold calls refuse about their frame, in the order of their headers' lists.  R: NULL for sq_lens_fold_device, which
// knows no R -- its range ends at S; sq_mlens_fold_device's ends at *R, which must divide S.
inline int check_fold(const void* d_part, const void* d_sum, long long P, int32_t S, const int32_t* R, int32_t r_begin, int32_t r_end) {
    if (!d_part || !d_sum) return sq_set_error("null argument: d_part and d_sum are required");
    if (P < 1) return sq_set_error("P must be at least 1 (got %lld)", P);
    if (!R && S < 1) return sq_set_error("samples must be at least 1 (got S = %d)", S);
    if (R && (S < 1 || *R < 1)) return sq_set_error("samples and sub-rays must be at least 1 (got S = %d, R = %d)", S, *R);
    if (R && S % *R != 0) return sq_set_error("the sub-rays must divide the samples (got S = %d, R = %d)", S, *R);
    const int32_t end = R ? *R : S;
    if (r_begin < 0 || r_end <= r_begin || r_end > end)
        return sq_set_error("bad sub-ray range [%d, %d) (need 0 <= r_begin < r_end <= %c = %d)", r_begin, r_end, R ? 'R' : 'S', end);
    if (P > lensplan::kMaxIndex) return sq_set_error("%lld pixels exceed 2^31 - 1 pixels in one call", P);
    return 0;
}

// INDEX WIDTHS: nb sub-rays of `pixels` pixels (of a shard, or of a list) are at most 2^31 - 1 ray slots.  pixels >= 1.
inline int refuse_slots(long long pixels, long long nb) {
    if (nb > lensplan::kMaxIndex / pixels)
        return sq_set_error("%lld sub-rays of %lld pixels exceed 2^31 - 1 ray slots in one batch", nb, pixels);
    return 0;
}

inline RayArgs ray_args(const sq_camera* cam, const sq_lens* lens, int32_t S, int32_t R, int32_t w, int32_t h, sq_shard sh, long long P) {
    RayArgs A{};
    for (int i = 0; i < 3; ++i) A.pos[i] = cam->pos[i];
    for (int i = 0; i < 9; ++i) A.rot[i] = cam->rot[i];
    A.jitter = lens->jitter; A.aperture = lens->aperture; A.focus = lens->focus;
    A.S = S; A.n = S / R;
    A.w = w; A.h = h; A.row_block = sh.row_block; A.shard = sh.shard; A.n_shards = sh.n_shards;
    A.P = P;
    return A;
}

}  // namespace lensray
