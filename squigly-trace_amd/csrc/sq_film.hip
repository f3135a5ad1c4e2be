// sq_film.hip — libsquigly_film.so (include/squigly_film.h): the display stage over device images.  It knows nothing of scenes:
// a frame in, a histogram, one float of exposure and an 8-bit image out, no state.
//
// Three kernels.
//  histogram  a workgroup counts into an 8 KB LDS histogram with LDS integer atomics over a grid-stride loop, then adds its non-zero
//             slots to d_hist with vector global atomics (atomicAdd from lanes).  Most of a rendered frame is one value -- two
//             thirds of the room's pixels see no surface and stay black at any sample count, and at 4 spp 97 % are still black
//              -- so a wave first folds the lanes that share its first lane's slot: one ballot, one
//             popcount, one lane adds (SQ_FILM_HIST_FOLD, below; the forms are measured in DESIGN.md 4.25).
//  expose     one workgroup: 256 lanes own eight slots each, a scan over their sums in LDS finds the lane that holds the rank, and
//             that lane alone reads *d_prev and writes *d_exposure (which may be the same float).
//  develop    12 bytes in and 3 bytes out per pixel.  Where the pointers allow it a lane takes four consecutive pixels: three
//             16-byte loads and three dword stores; otherwise a lane takes one pixel and writes three single bytes.  Curve, table
//             and dither are template arguments (the same for every pixel of a call), the pixel itself is csrc/sq_film_pixel.h.
//
// -ffp-contract=off and the correctly rounded divide keep the arithmetic equal to the numpy restatement.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "sq_call_checks.h"
#include "sq_film_pixel.h"
#include "../../include/squigly_film.h"

#ifndef SQ_FILM_BUILD_ID
#define SQ_FILM_BUILD_ID "unknown"
#endif
// How a wave folds equal slots before its LDS adds: 0 = not at all (every lane adds 1), 1 = the lanes of slot 0, 2 = the lanes that
// share the slot of the wave's first lane.  The counts are the same under all three.
#ifndef SQ_FILM_HIST_FOLD
#define SQ_FILM_HIST_FOLD 2
#endif

namespace {

using filmpix::Develop;
using filmpix::Meter;

constexpr int kBlock = 256;
constexpr long long kMaxPixels = 0x7fffffffLL;
constexpr int kMaxGrid = 2048;             // blocks of a launch: 8 per CU; the kernels stride over their pixels
constexpr int kSlots = filmpix::kSlots;
static_assert(kSlots == SQ_FILM_SLOTS && kSlots == 8 * kBlock, "a lane of the expose kernel owns eight slots");

template <int FOLD>
__global__ __launch_bounds__(kBlock) void sq_fm_histogram(const long long n, const float* __restrict__ color, uint32_t* __restrict__ hist) {
    __shared__ uint32_t h[kSlots];
    for (int i = threadIdx.x; i < kSlots; i += kBlock) h[i] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    // the bounds are the workgroup's, so that every lane of a wave reaches the ballot; a lane past the end holds slot -1
    for (long long base = (long long)blockIdx.x * kBlock; base < n; base += (long long)gridDim.x * kBlock) {
        const long long p = base + threadIdx.x;
        int s = -1;
        if (p < n) {
            const sq::f3 c = sq::load3(color, p);
            s = filmpix::slot(filmpix::luminance(c.x, c.y, c.z));
        }
        if (FOLD == 0) {
            if (s >= 0) atomicAdd(&h[s], 1u);
        } else {
            const int s0 = FOLD == 1 ? 0 : __builtin_amdgcn_readfirstlane(s);
            const unsigned long long equal = __ballot(s == s0);
            if (s == s0) {
                if (s0 >= 0 && (equal & ((1ull << lane) - 1ull)) == 0) atomicAdd(&h[s0], (uint32_t)__popcll(equal));
            } else if (s >= 0) {
                atomicAdd(&h[s], 1u);
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kSlots; i += kBlock) {
        const uint32_t v = h[i];
        if (v) atomicAdd(&hist[i], v);
    }
}

// d_prev may be d_exposure: only the lane that writes reads, and it reads first.
__global__ __launch_bounds__(kBlock) void sq_fm_expose(const uint32_t* __restrict__ hist, const Meter m, const float* prev, float* out) {
    __shared__ uint64_t part[kBlock];
    const int t = threadIdx.x;
    uint32_t v[8];
    uint64_t own = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int i = 8 * t + k;
        v[k] = (i >= 1 && i <= kSlots - 2) ? hist[i] : 0u;
        own += v[k];
    }
    part[t] = own;
    __syncthreads();
    for (int off = 1; off < kBlock; off <<= 1) {                   // an inclusive scan of the 256 sums
        const uint64_t add = t >= off ? part[t - off] : 0;
        __syncthreads();
        part[t] += add;
        __syncthreads();
    }
    const uint64_t M = part[kBlock - 1], incl = part[t], excl = incl - own;
    if (M == 0) {
        if (t == 0) *out = filmpix::exposure(0, 1, m, prev != nullptr, prev ? *prev : 0.0f);
        return;
    }
    const uint64_t rank = filmpix::rank_of(M, m.permille);
    if (!(excl < rank && rank <= incl)) return;                    // exactly one lane holds the rank
    uint64_t run = excl;
    int s = 8 * t + 7;
    bool found = false;
#pragma unroll
    for (int k = 0; k < 8; ++k) {                                  // the first of its eight slots whose running sum reaches the rank
        run += v[k];
        if (!found && run >= rank) { s = 8 * t + k; found = true; }
    }
    *out = filmpix::exposure(M, s, m, prev != nullptr, prev ? *prev : 0.0f);
}

SQ_HD void pixel_place(long long p, int cols, int& y, int& x) {
    const uint32_t q = (uint32_t)p / (uint32_t)cols;               // p <= 2^31 - 2
    y = (int)q;
    x = (int)((uint32_t)p - q * (uint32_t)cols);
}

// One pixel a lane.  Tensor views start anywhere: this form asks nothing of the pointers.
template <int CURVE, bool LUT, bool DITHER>
__global__ __launch_bounds__(kBlock) void sq_fm_develop1(const long long n, const int cols, const float* __restrict__ color,
                                                         const float* __restrict__ d_exposure, const float exposure, const Develop D,
                                                         uint8_t* __restrict__ rgb, float* __restrict__ display) {
    const float e = d_exposure ? *d_exposure : exposure;
    for (long long p = (long long)blockIdx.x * kBlock + threadIdx.x; p < n; p += (long long)gridDim.x * kBlock) {
        int y = 0, x = 0;
        if (DITHER) pixel_place(p, cols, y, x);
        uint8_t o[3];
        float d[3];
        filmpix::develop<CURVE, LUT, DITHER>(D, e, sq::load3(color, p), y, x, o, d);
        rgb[3 * p] = o[0]; rgb[3 * p + 1] = o[1]; rgb[3 * p + 2] = o[2];
        if (display) sq::store3(display, p, sq::mk(d[0], d[1], d[2]));
    }
}

// Four consecutive pixels a lane: color is 16-byte aligned and rgb 4-byte aligned.  display_wide: display is 16-byte aligned too.
// The n % 4 pixels at the end are taken one a lane by the first lanes of workgroup 0.
template <int CURVE, bool LUT, bool DITHER>
__global__ __launch_bounds__(kBlock) void sq_fm_develop4(const long long n, const int cols, const float* __restrict__ color,
                                                         const float* __restrict__ d_exposure, const float exposure, const Develop D,
                                                         uint8_t* __restrict__ rgb, float* __restrict__ display, const bool display_wide) {
    const float e = d_exposure ? *d_exposure : exposure;
    const long long quads = n / 4;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < quads; i += (long long)gridDim.x * kBlock) {
        const float4* src = reinterpret_cast<const float4*>(color) + 3 * i;
        const float4 a = src[0], b = src[1], c = src[2];
        const float in[12] = { a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w };
        uint8_t o[12];
        float d[12];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            int y = 0, x = 0;
            if (DITHER) pixel_place(4 * i + k, cols, y, x);
            filmpix::develop<CURVE, LUT, DITHER>(D, e, sq::mk(in[3 * k], in[3 * k + 1], in[3 * k + 2]), y, x, o + 3 * k, d + 3 * k);
        }
        uint32_t* dst = reinterpret_cast<uint32_t*>(rgb) + 3 * i;
#pragma unroll
        for (int k = 0; k < 3; ++k)
            dst[k] = (uint32_t)o[4 * k] | ((uint32_t)o[4 * k + 1] << 8) | ((uint32_t)o[4 * k + 2] << 16) | ((uint32_t)o[4 * k + 3] << 24);
        if (display) {
            if (display_wide) {
                float4* dd = reinterpret_cast<float4*>(display) + 3 * i;
                dd[0] = make_float4(d[0], d[1], d[2], d[3]);
                dd[1] = make_float4(d[4], d[5], d[6], d[7]);
                dd[2] = make_float4(d[8], d[9], d[10], d[11]);
            } else {
#pragma unroll
                for (int k = 0; k < 12; ++k) display[12 * i + k] = d[k];
            }
        }
    }
    const long long p = 4 * quads + threadIdx.x;
    if (blockIdx.x == 0 && p < n) {
        int y = 0, x = 0;
        if (DITHER) pixel_place(p, cols, y, x);
        uint8_t o[3];
        float d[3];
        filmpix::develop<CURVE, LUT, DITHER>(D, e, sq::load3(color, p), y, x, o, d);
        rgb[3 * p] = o[0]; rgb[3 * p + 1] = o[1]; rgb[3 * p + 2] = o[2];
        if (display) sq::store3(display, p, sq::mk(d[0], d[1], d[2]));
    }
}

int check_size(int32_t rows, int32_t cols) {
    if (rows < 1 || cols < 1) return sq_set_error("rows and cols must be at least 1 (got %d x %d)", rows, cols);
    if ((long long)rows * cols > kMaxPixels) return sq_set_error("%d x %d pixels exceed 2^31 - 1 pixels in one call", rows, cols);
    return 0;
}

bool finite_positive(float v) { return v > 0.0f && v < __builtin_inff(); }

unsigned grid_for(long long units) {
    const long long blocks = (units + kBlock - 1) / kBlock;
    return (unsigned)(blocks < 1 ? 1 : blocks < kMaxGrid ? blocks : kMaxGrid);
}

struct DevelopCall {
    long long n; int cols; const float* color; const float* d_exposure; float exposure; Develop D; uint8_t* rgb; float* display;
    hipStream_t stream;
};

template <int CURVE, bool LUT, bool DITHER> void launch_develop(const DevelopCall& a) {
    const bool wide = (uintptr_t)a.color % 16 == 0 && (uintptr_t)a.rgb % 4 == 0;
    if (wide)
        hipLaunchKernelGGL((sq_fm_develop4<CURVE, LUT, DITHER>), dim3(grid_for((a.n + 3) / 4)), dim3(kBlock), 0, a.stream, a.n, a.cols, a.color,
                           a.d_exposure, a.exposure, a.D, a.rgb, a.display, (uintptr_t)a.display % 16 == 0);
    else
        hipLaunchKernelGGL((sq_fm_develop1<CURVE, LUT, DITHER>), dim3(grid_for(a.n)), dim3(kBlock), 0, a.stream, a.n, a.cols, a.color,
                           a.d_exposure, a.exposure, a.D, a.rgb, a.display);
}

template <int CURVE> void launch_curve(bool lut, bool dither, const DevelopCall& a) {
    if (lut) { if (dither) launch_develop<CURVE, true, true>(a); else launch_develop<CURVE, true, false>(a); }
    else { if (dither) launch_develop<CURVE, false, true>(a); else launch_develop<CURVE, false, false>(a); }
}

}  // namespace

extern "C" const char* sq_film_last_error(void) { return sq_error_buffer(); }
extern "C" const char* sq_film_build_id(void) { return SQ_FILM_BUILD_ID; }

extern "C" int sq_film_histogram_device(int32_t device, int32_t rows, int32_t cols, const float* d_color, uint32_t* d_hist, void* hip_stream) {
    if (!d_color || !d_hist) return sq_set_error("null argument: d_color and d_hist are required");
    if (check_size(rows, cols)) return 1;
    if ((uintptr_t)d_hist % 4 != 0) return sq_set_error("d_hist must be 4-byte aligned");
    const size_t n = (size_t)rows * (size_t)cols;
    const NamedRange r[2] = { { "d_color", d_color, 12 * n }, { "d_hist", d_hist, 4 * (size_t)kSlots } };
    if (refuse_overlaps(r, 2)) return 1;
    SQ_HIP(hipSetDevice(device));
    SQ_HIP(hipMemsetAsync(d_hist, 0, 4 * (size_t)kSlots, (hipStream_t)hip_stream));
    hipLaunchKernelGGL(sq_fm_histogram<SQ_FILM_HIST_FOLD>, dim3(grid_for((long long)n)), dim3(kBlock), 0, (hipStream_t)hip_stream, (long long)n,
                       d_color, d_hist);
    SQ_HIP(hipGetLastError());
    return 0;
}

extern "C" int sq_film_expose_device(int32_t device, const uint32_t* d_hist, const sq_film_meter* meter, const float* d_prev,
                                     float* d_exposure, void* hip_stream) {
    if (!d_hist || !meter || !d_exposure) return sq_set_error("null argument: d_hist, meter and d_exposure are required");
    if ((uintptr_t)d_hist % 4 != 0) return sq_set_error("d_hist must be 4-byte aligned");
    if (meter->permille < 1 || meter->permille > 1000) return sq_set_error("permille must be in 1..1000 (got %d)", meter->permille);
    if (!finite_positive(meter->e_min) || !finite_positive(meter->e_max) || meter->e_min > meter->e_max)
        return sq_set_error("e_min and e_max must be finite with 0 < e_min <= e_max (got %g, %g)", (double)meter->e_min, (double)meter->e_max);
    if (!(meter->rate >= 0.0f && meter->rate <= 1.0f)) return sq_set_error("rate must be a number in 0..1 (got %g)", (double)meter->rate);
    if (!(meter->fallback > 0.0f)) return sq_set_error("fallback must be a number > 0 (got %g)", (double)meter->fallback);
    const NamedRange r[3] = { { "d_hist", d_hist, 4 * (size_t)kSlots }, { "d_prev", d_prev, 4 }, { "d_exposure", d_exposure, 4 } };
    const int twins[1][2] = { { 1, 2 } };                                        // d_prev == d_exposure
    if (refuse_overlaps(r, 3, " (only d_prev == d_exposure may share memory)", twins, 1)) return 1;
    SQ_HIP(hipSetDevice(device));
    const Meter m{ meter->key, meter->permille, meter->e_min, meter->e_max, meter->rate, meter->fallback };
    hipLaunchKernelGGL(sq_fm_expose, dim3(1), dim3(kBlock), 0, (hipStream_t)hip_stream, d_hist, m, d_prev, d_exposure);
    SQ_HIP(hipGetLastError());
    return 0;
}

extern "C" int sq_film_develop_device(int32_t device, int32_t rows, int32_t cols, const float* d_color, const float* d_exposure,
                                      const sq_film_params* params, const float* d_lut, uint8_t* d_rgb, float* d_display, void* hip_stream) {
    if (!d_color || !params || !d_rgb) return sq_set_error("null argument: d_color, params and d_rgb are required");
    if (check_size(rows, cols)) return 1;
    const sq_film_params P = *params;
    if (P.curve < 0 || P.curve >= filmpix::kCurves) return sq_set_error("curve must be in 0..4 (got %d)", P.curve);
    if (P.curve == filmpix::REINHARD && !(P.white > 0.0f)) return sq_set_error("white must be a number > 0 (got %g)", (double)P.white);
    if (d_lut && (P.n_lut < 2 || P.n_lut > 65536)) return sq_set_error("n_lut must be in 2..65536 (got %d)", P.n_lut);
    if (P.dither != 0 && P.dither != 1) return sq_set_error("dither must be 0 or 1 (got %d)", P.dither);
    if (P.curve == filmpix::REFERENCE && (d_lut || P.dither))
        return sq_set_error("the reference curve takes neither d_lut nor dither: it is the renderer's own conversion to bytes");
    const size_t n = (size_t)rows * (size_t)cols;
    const NamedRange r[5] = { { "d_color", d_color, 12 * n }, { "d_exposure", d_exposure, 4 }, { "d_lut", d_lut, d_lut ? 4 * (size_t)P.n_lut : 0 },
                              { "d_rgb", d_rgb, 3 * n }, { "d_display", d_display, 12 * n } };
    if (refuse_overlaps(r, 5)) return 1;
    SQ_HIP(hipSetDevice(device));
    const DevelopCall a{ (long long)n, cols, d_color, d_exposure, P.exposure, Develop{ P.white, d_lut, d_lut ? P.n_lut : 0 }, d_rgb, d_display,
                         (hipStream_t)hip_stream };
    const bool lut = d_lut != nullptr, dither = P.dither != 0;
    switch (P.curve) {
        case filmpix::REFERENCE: launch_develop<filmpix::REFERENCE, false, false>(a); break;
        case filmpix::ATAN: launch_curve<filmpix::ATAN>(lut, dither, a); break;
        case filmpix::REINHARD: launch_curve<filmpix::REINHARD>(lut, dither, a); break;
        case filmpix::FILMIC: launch_curve<filmpix::FILMIC>(lut, dither, a); break;
        default: launch_curve<filmpix::LINEAR>(lut, dither, a); break;
    }
    SQ_HIP(hipGetLastError());
    return 0;
}
