// sq_denoise.hip — libsquigly_denoise.so (include/squigly_denoise.h): a variance- and geometry-guided a-trous filter over device
// images.  It knows nothing of scenes: device images in, device images out, a caller-given workspace, no state.
//
// A call is a pack pre-pass and `passes` filter passes.  The pre-pass turns the five input images into 16-byte records, so that a
// tap is three dwordx4 loads instead of ten dword loads at a stride of 12 bytes:
//     NV  normal.xyz, validity (1 / 0 as an integer)
//     PT  point.xyz, 0
//     CV  colour.rgb, variance         two of them: pass i reads CV[i & 1] and writes CV[~i & 1], the last pass writes d_out
// Every input is read by the pre-pass alone, which is why d_out == d_color is allowed.
//
// The arithmetic of a pixel (filter_pixel) is written once, operation by operation as the header states it, and is the same for
// every kernel form: a form only decides how a tap's records reach the lane (Direct: from the workspace; Tiled: from an LDS image
// of the tile and its halo).  -ffp-contract=off and the correctly rounded divide / sqrt keep it equal to the numpy restatement.
//
// Sparse frames (sq_denoise_sparse_mask_device, sq_denoise_upsample_device) are two kernels of their own further down: no workspace,
// the caller's images as they are, and a pixel's arithmetic from sq_upsample_pixel.h, the text the host test program compiles too.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "sq_call_checks.h"
#include "sq_math.h"
#include "sq_glare_pixel.h"
#include "sq_upsample_pixel.h"
#include "../../include/squigly_denoise.h"

#ifndef SQ_DENOISE_BUILD_ID
#define SQ_DENOISE_BUILD_ID "unknown"
#endif

namespace {

constexpr int kBlock = 256;
constexpr long long kMaxPixels = 0x7fffffffLL;
constexpr int kMaxGrid = 1 << 16;          // blocks of a launch; the kernels stride over their tiles
// Direct form: a block is 4 rows of 64 pixels, a wave one row segment (a tap of a wave is 1 KiB of consecutive records)
constexpr int kDirW = 64, kDirH = 4;
// Tiled form: a block is a 16 x 16 tile; its LDS image has a halo of 2 * step pixels
constexpr int kTile = 16;
constexpr int kTiledMaxStep = 4;           // (16 + 4 * 4)^2 records * 48 B = 48 KiB: three blocks per CU

struct Filter { float sigma_l, eps_l, sigma_p; int squarings; };

__device__ __forceinline__ float lum(float r, float g, float b) { return (0.25f * r + 0.5f * g) + 0.25f * b; }
__device__ __forceinline__ bool rec_valid(const float4& nv) { return __float_as_int(nv.w) != 0; }

// The pixel arithmetic of include/squigly_denoise.h.  S gives the records of the pixel at an offset from p:
//   S.nv(oy, ox, nv)  false when that pixel is outside the image or not valid (nv is then undefined)
//   S.pt(oy, ox), S.cv(oy, ox)  of a pixel nv() said true for
// cvp: CV of p.  Returns CV of p after the pass.
template <bool VAR, class Src>
__device__ __forceinline__ float4 filter_pixel(const Src& S, const int s, const Filter& F, const float4 nvp, const float4 ptp, const float4 cvp) {
    float sd = 0.0f;
    if (VAR) {
        float gs = 0.0f, gw = 0.0f;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                float4 nq;
                if (!S.nv(dy, dx, nq)) continue;
                const float g = (dy == 0 ? 0.5f : 0.25f) * (dx == 0 ? 0.5f : 0.25f);
                gs = gs + g * S.cv(dy, dx).w;
                gw = gw + g;
            }
        }
        const float gv = gs / gw;
        sd = F.sigma_l * sq::fsqrt(gv) + F.eps_l;
    }
    const float lp = lum(cvp.x, cvp.y, cvp.z);
    float sw = 0.0f, scr = 0.0f, scg = 0.0f, scb = 0.0f, sv = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            float4 nq;
            if (!S.nv(dy * s, dx * s, nq)) continue;
            const float4 pq = S.pt(dy * s, dx * s);
            const float4 cq = S.cv(dy * s, dx * s);
            const float ky = dy == 0 ? 0.375f : (dy == 1 || dy == -1) ? 0.25f : 0.0625f;
            const float kx = dx == 0 ? 0.375f : (dx == 1 || dx == -1) ? 0.25f : 0.0625f;
            const float kw = ky * kx;
            const float dn = (nvp.x * nq.x + nvp.y * nq.y) + nvp.z * nq.z;
            float t = dn > 0.0f ? dn : 0.0f;
            for (int k = 0; k < F.squarings; ++k) t = t * t;
            const float ex = pq.x - ptp.x, ey = pq.y - ptp.y, ez = pq.z - ptp.z;
            const float pd = (nvp.x * ex + nvp.y * ey) + nvp.z * ez;
            const float a = pd / F.sigma_p;
            const float wz = 1.0f / (1.0f + a * a);
            float w = (kw * t) * wz;
            if (VAR) {
                const float b = (lum(cq.x, cq.y, cq.z) - lp) / sd;
                const float wl = 1.0f / (1.0f + b * b);
                w = w * wl;
            }
            sw = sw + w;
            scr = scr + w * cq.x;
            scg = scg + w * cq.y;
            scb = scb + w * cq.z;
            if (VAR) sv = sv + (w * w) * cq.w;
        }
    }
    if (sw > 0.0f) return make_float4(scr / sw, scg / sw, scb / sw, VAR ? sv / (sw * sw) : cvp.w);
    return cvp;
}

// Where a pass leaves a pixel: the other CV image, or (the last pass) the caller's outputs.
__device__ __forceinline__ void store_pixel(const long long p, const float4 cv, float4* cv_out, float* out, float* out_var) {
    if (out) {
        out[3 * p + 0] = cv.x; out[3 * p + 1] = cv.y; out[3 * p + 2] = cv.z;
        if (out_var) out_var[p] = cv.w;
    } else {
        cv_out[p] = cv;
    }
}

// ---- pack pre-pass ----
__global__ __launch_bounds__(kBlock) void sq_dn_pack(const long long n, const float* __restrict__ color, const float* __restrict__ var,
                                                     const int32_t* __restrict__ tri, const float* __restrict__ normal,
                                                     const float* __restrict__ point, float4* __restrict__ nv, float4* __restrict__ pt,
                                                     float4* __restrict__ cv) {
    for (long long p = (long long)blockIdx.x * kBlock + threadIdx.x; p < n; p += (long long)gridDim.x * kBlock) {
        nv[p] = make_float4(normal[3 * p], normal[3 * p + 1], normal[3 * p + 2], __int_as_float(tri[p] >= 0 ? 1 : 0));
        pt[p] = make_float4(point[3 * p], point[3 * p + 1], point[3 * p + 2], 0.0f);
        cv[p] = make_float4(color[3 * p], color[3 * p + 1], color[3 * p + 2], var ? var[p] : 0.0f);
    }
}

// ---- variance of the pixel mean's luminance ----
__global__ __launch_bounds__(kBlock) void sq_dn_variance(const long long n, const float* __restrict__ sum, const float* __restrict__ sum2,
                                                         const int32_t* __restrict__ count, float* __restrict__ var) {
    for (long long p = (long long)blockIdx.x * kBlock + threadIdx.x; p < n; p += (long long)gridDim.x * kBlock) {
        const int32_t c = count[p];
        float v = 0.0f;
        if (c >= 1) {
            const float nf = (float)c;
            float m[3], vc[3];
            for (int k = 0; k < 3; ++k) {
                m[k] = sum[3 * p + k] / nf;
                const float d = sum2[3 * p + k] / nf - m[k] * m[k];
                vc[k] = d > 0.0f ? d / (nf - 1.0f) : 0.0f;
            }
            if (c < 2) {
                const float l = lum(m[0], m[1], m[2]);
                v = l * l;
            } else {
                v = (0.0625f * vc[0] + 0.25f * vc[1]) + 0.0625f * vc[2];
            }
        }
        var[p] = v;
    }
}

// ---- direct form ----
struct DirectSrc {
    const float4* __restrict__ nv_; const float4* __restrict__ pt_; const float4* __restrict__ cv_;
    long long y, x; int rows, cols;
    __device__ __forceinline__ bool inside(int oy, int ox, long long& q) const {
        const long long qy = y + oy, qx = x + ox;
        q = qy * cols + qx;
        return qy >= 0 && qy < rows && qx >= 0 && qx < cols;
    }
    __device__ __forceinline__ bool nv(int oy, int ox, float4& r) const {
        long long q;
        if (!inside(oy, ox, q)) return false;
        r = nv_[q];
        return rec_valid(r);
    }
    __device__ __forceinline__ float4 pt(int oy, int ox) const { return pt_[(y + oy) * cols + (x + ox)]; }
    __device__ __forceinline__ float4 cv(int oy, int ox) const { return cv_[(y + oy) * cols + (x + ox)]; }
};

template <bool VAR>
__global__ __launch_bounds__(kBlock) void sq_dn_pass_direct(const int rows, const int cols, const int s, const Filter F,
                                                            const float4* __restrict__ nv, const float4* __restrict__ pt,
                                                            const float4* __restrict__ cv_in, float4* __restrict__ cv_out,
                                                            float* __restrict__ out, float* __restrict__ out_var,
                                                            const long long tiles, const long long tiles_x) {
    for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
        const long long ty = t / tiles_x, tx = t - ty * tiles_x;
        const long long x = tx * kDirW + (threadIdx.x & (kDirW - 1)), y = ty * kDirH + (threadIdx.x / kDirW);
        if (x >= cols || y >= rows) continue;
        const long long p = y * cols + x;
        const float4 nvp = nv[p], cvp = cv_in[p];
        float4 r = cvp;
        if (rec_valid(nvp)) {
            const DirectSrc S{ nv, pt, cv_in, y, x, rows, cols };
            r = filter_pixel<VAR>(S, s, F, nvp, pt[p], cvp);
        }
        store_pixel(p, r, cv_out, out, out_var);
    }
}

// ---- tiled form ----
// The LDS image: (16 + 4 s)^2 pixels, three arrays of records.  A pixel outside the image is stored as not valid, so a tap needs
// no bounds test of its own.
struct TiledSrc {
    const float4* nv_; const float4* pt_; const float4* cv_;
    int at, w;              // p's index in the LDS image; the image's width
    __device__ __forceinline__ bool nv(int oy, int ox, float4& r) const { r = nv_[at + oy * w + ox]; return rec_valid(r); }
    __device__ __forceinline__ float4 pt(int oy, int ox) const { return pt_[at + oy * w + ox]; }
    __device__ __forceinline__ float4 cv(int oy, int ox) const { return cv_[at + oy * w + ox]; }
};

template <bool VAR>
__global__ __launch_bounds__(kBlock) void sq_dn_pass_tiled(const int rows, const int cols, const int s, const Filter F,
                                                           const float4* __restrict__ nv, const float4* __restrict__ pt,
                                                           const float4* __restrict__ cv_in, float4* __restrict__ cv_out,
                                                           float* __restrict__ out, float* __restrict__ out_var,
                                                           const long long tiles, const long long tiles_x) {
    extern __shared__ float4 lds[];
    const int halo = 2 * s, w = kTile + 2 * halo, n = w * w;
    float4* l_nv = lds;
    float4* l_pt = lds + n;
    float4* l_cv = lds + 2 * n;
    const int lx = threadIdx.x & (kTile - 1), ly = threadIdx.x / kTile;
    for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
        const long long ty = t / tiles_x, tx = t - ty * tiles_x;
        const long long y0 = ty * kTile - halo, x0 = tx * kTile - halo;
        for (int i = threadIdx.x; i < n; i += kBlock) {
            const int iy = i / w, ix = i - iy * w;
            const long long gy = y0 + iy, gx = x0 + ix;
            float4 a = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(0)), b = make_float4(0.0f, 0.0f, 0.0f, 0.0f), c = b;
            if (gy >= 0 && gy < rows && gx >= 0 && gx < cols) {
                const long long q = gy * cols + gx;
                a = nv[q]; b = pt[q]; c = cv_in[q];
            }
            l_nv[i] = a; l_pt[i] = b; l_cv[i] = c;
        }
        __syncthreads();
        const long long y = ty * kTile + ly, x = tx * kTile + lx;
        if (x < cols && y < rows) {
            const int at = (ly + halo) * w + (lx + halo);
            const float4 nvp = l_nv[at], cvp = l_cv[at];
            float4 r = cvp;
            if (rec_valid(nvp)) {
                const TiledSrc S{ l_nv, l_pt, l_cv, at, w };
                r = filter_pixel<VAR>(S, s, F, nvp, l_pt[at], cvp);
            }
            store_pixel(y * cols + x, r, cv_out, out, out_var);
        }
        __syncthreads();        // the next tile's image overwrites this one
    }
}

// ---- sparse frames: which pixels to trace, and the others from their traced neighbours (sq_upsample_pixel.h) ----
// One lane per pixel, a wave on 64 consecutive columns of a row (the direct form's tiles): a lane's own guide loads are contiguous
// across the wave, and the four taps of s neighbouring lanes are the same lattice pixels, so their lines come from L1 / L2.
__global__ __launch_bounds__(kBlock) void sq_dn_sparse_mask(const upspix::Lattice L, const upspix::Stops K, const upspix::Guides G,
                                                            uint8_t* __restrict__ mask, const long long tiles, const long long tiles_x) {
    for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
        const long long ty = t / tiles_x, tx = t - ty * tiles_x;
        const long long x = tx * kDirW + (threadIdx.x & (kDirW - 1)), y = ty * kDirH + (threadIdx.x / kDirW);
        if (x >= L.cols || y >= L.rows) continue;
        mask[y * L.cols + x] = upspix::live(L, K, G, (int32_t)y, (int32_t)x);
    }
}

template <bool VAR>
__global__ __launch_bounds__(kBlock) void sq_dn_upsample(const upspix::Lattice L, const upspix::Stops K, const upspix::Guides G,
                                                         const upspix::Image I, const uint8_t* __restrict__ mask,
                                                         float* __restrict__ out, float* __restrict__ out_var, const long long tiles,
                                                         const long long tiles_x) {
    for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
        const long long ty = t / tiles_x, tx = t - ty * tiles_x;
        const long long x = tx * kDirW + (threadIdx.x & (kDirW - 1)), y = ty * kDirH + (threadIdx.x / kDirW);
        if (x >= L.cols || y >= L.rows) continue;
        const long long p = y * L.cols + x;
        float c[3], v = 0.0f;
        upspix::upsample<VAR>(L, K, G, I, mask, (int32_t)y, (int32_t)x, c, &v);
        out[3 * p + 0] = c[0]; out[3 * p + 1] = c[1]; out[3 * p + 2] = c[2];
        if (VAR && out_var) out_var[p] = v;
    }
}

// The form of pass `pass` when the caller leaves the choice (form = 0): the tiled form wherever its LDS image fits.  Measured at
// 1920 x 1080 (tools/gpu_denoise.py): 0.111 / 0.112 / 0.114 ms at steps 1 / 2 / 4 against 0.173 / 0.173 / 0.177 ms direct.
int auto_form(int pass) { return (1 << pass) <= kTiledMaxStep ? SQ_DENOISE_FORM_TILED : SQ_DENOISE_FORM_DIRECT; }

// Everything that can be refused, in the order of the header's list.  Touches neither the device nor a buffer.
int check_call(int32_t rows, int32_t cols, const float* d_color, const float* d_var, const int32_t* d_tri, const float* d_normal,
               const float* d_point, const sq_denoise_params* P, float* d_out, float* d_out_var, void* d_work, size_t work_bytes) {
    if (!d_color || !d_tri || !d_normal || !d_point || !P || !d_out || !d_work)
        return sq_set_error("null argument: d_color, d_tri, d_normal, d_point, params, d_out and d_work are required");
    if (rows < 1 || cols < 1) return sq_set_error("rows and cols must be at least 1 (got %d x %d)", rows, cols);
    if ((long long)rows * cols > kMaxPixels) return sq_set_error("%d x %d pixels exceed 2^31 - 1 pixels in one call", rows, cols);
    if (P->passes < 1 || P->passes > 8) return sq_set_error("passes must be in 1..8 (got %d)", P->passes);
    if (P->normal_squarings < 0 || P->normal_squarings > 8) return sq_set_error("normal_squarings must be in 0..8 (got %d)", P->normal_squarings);
    if (P->form < 0 || P->form > SQ_DENOISE_N_FORMS) return sq_set_error("form must be in 0..%d (got %d)", SQ_DENOISE_N_FORMS, P->form);
    if (!(P->sigma_l > 0.0f)) return sq_set_error("sigma_l must be a number > 0 (got %g)", (double)P->sigma_l);
    if (!(P->sigma_p > 0.0f)) return sq_set_error("sigma_p must be a number > 0 (got %g)", (double)P->sigma_p);
    if (!(P->eps_l >= 0.0f)) return sq_set_error("eps_l must be a number >= 0 (got %g)", (double)P->eps_l);
    if (d_out_var && !d_var) return sq_set_error("d_out_var needs d_var: without a variance image there is none to filter");
    const size_t need = sq_denoise_workspace_bytes(rows, cols);
    if (work_bytes < need) return sq_set_error("work_bytes = %zu is too small: a %d x %d image needs %zu", work_bytes, rows, cols, need);
    if ((uintptr_t)d_work % 16 != 0) return sq_set_error("d_work must be 16-byte aligned");
    const size_t n = (size_t)rows * (size_t)cols;
    const NamedRange r[8] = { { "d_color", d_color, 12 * n }, { "d_var", d_var, 4 * n }, { "d_tri", d_tri, 4 * n }, { "d_normal", d_normal, 12 * n },
                              { "d_point", d_point, 12 * n }, { "d_out", d_out, 12 * n }, { "d_out_var", d_out_var, 4 * n }, { "d_work", d_work, work_bytes } };
    const int twins[2][2] = { { 0, 5 }, { 1, 6 } };                              // d_out == d_color, d_out_var == d_var
    return refuse_overlaps(r, 8, " (only d_out == d_color and d_out_var == d_var may share memory)", twins, 2);
}

unsigned grid_for(long long units) { return (unsigned)(units < kMaxGrid ? units : kMaxGrid); }

// Enqueues the stages [first, last] of a checked call: -1 = the pack pre-pass, i = pass i.
int enqueue(int32_t device, int32_t rows, int32_t cols, const float* d_color, const float* d_var, const int32_t* d_tri,
            const float* d_normal, const float* d_point, const sq_denoise_params& P, float* d_out, float* d_out_var, void* d_work,
            void* hip_stream, int first, int last) {
    SQ_HIP(hipSetDevice(device));
    hipStream_t stream = (hipStream_t)hip_stream;
    const long long n = (long long)rows * cols;
    float4* nv = (float4*)d_work;
    float4* pt = nv + n;
    float4* cv[2] = { pt + n, pt + 2 * n };
    const Filter F{ P.sigma_l, P.eps_l, P.sigma_p, P.normal_squarings };
    for (int stage = first; stage <= last; ++stage) {
        if (stage < 0) {
            hipLaunchKernelGGL(sq_dn_pack, dim3(grid_for((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, n, d_color, d_var, d_tri,
                               d_normal, d_point, nv, pt, cv[0]);
            SQ_HIP(hipGetLastError());
            continue;
        }
        const int s = 1 << stage;
        const bool is_last = stage == P.passes - 1;
        const float4* in = cv[stage & 1];
        float4* out_cv = cv[(stage + 1) & 1];
        float* out = is_last ? d_out : nullptr;
        float* out_var = is_last ? d_out_var : nullptr;
        int form = P.form == SQ_DENOISE_FORM_AUTO ? auto_form(stage) : P.form;
        if (s > kTiledMaxStep) form = SQ_DENOISE_FORM_DIRECT;
        if (form == SQ_DENOISE_FORM_TILED) {
            const long long tx = ((long long)cols + kTile - 1) / kTile, ty = ((long long)rows + kTile - 1) / kTile;
            const int w = kTile + 4 * s;
            const size_t lds = (size_t)w * w * 3 * sizeof(float4);
            if (d_var) hipLaunchKernelGGL(sq_dn_pass_tiled<true>, dim3(grid_for(tx * ty)), dim3(kBlock), lds, stream, rows, cols, s, F, nv, pt, in, out_cv, out, out_var, tx * ty, tx);
            else       hipLaunchKernelGGL(sq_dn_pass_tiled<false>, dim3(grid_for(tx * ty)), dim3(kBlock), lds, stream, rows, cols, s, F, nv, pt, in, out_cv, out, out_var, tx * ty, tx);
        } else {
            const long long tx = ((long long)cols + kDirW - 1) / kDirW, ty = ((long long)rows + kDirH - 1) / kDirH;
            if (d_var) hipLaunchKernelGGL(sq_dn_pass_direct<true>, dim3(grid_for(tx * ty)), dim3(kBlock), 0, stream, rows, cols, s, F, nv, pt, in, out_cv, out, out_var, tx * ty, tx);
            else       hipLaunchKernelGGL(sq_dn_pass_direct<false>, dim3(grid_for(tx * ty)), dim3(kBlock), 0, stream, rows, cols, s, F, nv, pt, in, out_cv, out, out_var, tx * ty, tx);
        }
        SQ_HIP(hipGetLastError());
    }
    return 0;
}

// What both sparse calls refuse of the lattice, the stops and the guides; then the overlaps among r[0 .. count).
int check_sparse(int32_t rows, int32_t cols, int32_t s, int32_t oy, int32_t ox, const sq_denoise_sparse_params* P, const NamedRange* r, int count) {
    if (rows < 1 || cols < 1) return sq_set_error("rows and cols must be at least 1 (got %d x %d)", rows, cols);
    if ((long long)rows * cols > kMaxPixels) return sq_set_error("%d x %d pixels exceed 2^31 - 1 pixels in one call", rows, cols);
    if (s < 1 || s > upspix::kMaxStride) return sq_set_error("stride must be in 1..%d (got %d)", upspix::kMaxStride, s);
    if (oy < 0 || oy >= s || ox < 0 || ox >= s) return sq_set_error("offset must be in [0, stride) both ways (got (%d, %d) at stride %d)", oy, ox, s);
    if (!(P->sigma_p >= 0.0f)) return sq_set_error("sigma_p must be a number >= 0 (got %g)", (double)P->sigma_p);
    if (P->cos_n != P->cos_n) return sq_set_error("cos_n must be a number (got %g)", (double)P->cos_n);
    return refuse_overlaps(r, count);
}

int enqueue_sparse(int32_t device, int32_t rows, int32_t cols, int32_t s, int32_t oy, int32_t ox, const sq_denoise_sparse_params& P,
                   const int32_t* d_tri, const float* d_normal, const float* d_point, const float* d_color, const float* d_var,
                   const uint8_t* d_mask_in, uint8_t* d_mask_out, float* d_out, float* d_out_var, void* hip_stream) {
    SQ_HIP(hipSetDevice(device));
    hipStream_t stream = (hipStream_t)hip_stream;
    const upspix::Lattice L{ rows, cols, s, oy, ox };
    const upspix::Stops K{ P.sigma_p, P.cos_n };
    const upspix::Guides G{ d_tri, d_normal, d_point };
    const long long tx = ((long long)cols + kDirW - 1) / kDirW, ty = ((long long)rows + kDirH - 1) / kDirH;
    const dim3 grid(grid_for(tx * ty)), block(kBlock);
    if (d_mask_out) {
        hipLaunchKernelGGL(sq_dn_sparse_mask, grid, block, 0, stream, L, K, G, d_mask_out, tx * ty, tx);
    } else {
        const upspix::Image I{ d_color, d_var };
        if (d_var) hipLaunchKernelGGL(sq_dn_upsample<true>, grid, block, 0, stream, L, K, G, I, d_mask_in, d_out, d_out_var, tx * ty, tx);
        else       hipLaunchKernelGGL(sq_dn_upsample<false>, grid, block, 0, stream, L, K, G, I, d_mask_in, d_out, d_out_var, tx * ty, tx);
    }
    SQ_HIP(hipGetLastError());
    return 0;
}

// ---- glare: a bloom pyramid, and exposure and white balance, ahead of the film stage (sq_glare_pixel.h) ----
// The workspace holds the levels B_0 .. B_levels-1 one after the other, a 16-byte record (r, g, b, 0) per level pixel; the up steps
// turn B_k into A_k in place.  Five kernels:
//   down<BRIGHT = true>   colour -> B_0: exposure, gain and the bright pass of the 16 fine pixels of an output, then the down step
//   down<BRIGHT = false>  B_k-1 -> B_k: the down step over records
//   up_add                A_k+1, B_k -> A_k, in place on level k: a lane writes only the record it read
//   composite<true>       colour, A_0 -> d_out, four pixels a lane where d_color and d_out are 16-byte aligned, else one
//   composite<false>      levels = 0: exposure and gain alone
// The down kernels have two forms, which give the same bits because h(j, x) depends on the fine row and the output column alone:
//   direct  a lane gathers its 4 x 4 fine pixels itself (a wave on 64 consecutive output columns, as the direct filter pass)
//   tiled   a workgroup stages the 34 x 34 fine pixels of its 16 x 16 outputs in LDS once (bright-passed once each, not four times),
//           planar -- one float plane a channel, rows 35 floats apart so that the two fine rows a 32-lane group reads at stride 2
//           fall on banks of opposite parity -- then the horizontal four-tap into a second LDS image (rows 24 floats apart: the
//           two tile rows of a 32-lane group read rows 48 floats = 16 banks apart), then the vertical one.
namespace gp = glarepix;

constexpr int kGlTile = 16;                       // outputs of a tiled workgroup, both ways
constexpr int kGlIn = 2 * kGlTile + 2;            // fine pixels it stages, both ways: 2 * 16 and one more on either side
constexpr int kGlInStride = kGlIn + 1;            // odd
constexpr int kGlHStride = 24;

// The fine image of a down step: the bright pass of the caller's colour image, or the records of the level before.
struct BrightSrc {
    const float* __restrict__ color; float e; gp::Glare G; int32_t cols;
    __device__ __forceinline__ sq::f3 operator()(int32_t j, int32_t i) const {
        return gp::bright(G, gp::exposed(e, G, sq::load3(color, (long long)j * cols + i)));
    }
};
struct RecordSrc {
    const float4* __restrict__ rec; int32_t cols;
    __device__ __forceinline__ sq::f3 operator()(int32_t j, int32_t i) const {
        const float4 v = rec[(long long)j * cols + i];
        return sq::mk(v.x, v.y, v.z);
    }
};

template <bool BRIGHT>
__global__ __launch_bounds__(kBlock) void sq_gl_down_direct(const int32_t r, const int32_t c, const float* __restrict__ color,
                                                            const float* __restrict__ d_exposure, const float exposure, const gp::Glare G,
                                                            const float4* __restrict__ fine, float4* __restrict__ coarse,
                                                            const long long tiles, const long long tiles_x) {
    const int32_t R = gp::half_up(r), C = gp::half_up(c);
    const float e = BRIGHT ? (d_exposure ? *d_exposure : exposure) : 0.0f;
    for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
        const long long ty = t / tiles_x, tx = t - ty * tiles_x;
        const long long x = tx * kDirW + (threadIdx.x & (kDirW - 1)), y = ty * kDirH + (threadIdx.x / kDirW);
        if (x >= C || y >= R) continue;
        sq::f3 v;
        if (BRIGHT) v = gp::down(BrightSrc{ color, e, G, c }, r, c, (int32_t)y, (int32_t)x);
        else v = gp::down(RecordSrc{ fine, c }, r, c, (int32_t)y, (int32_t)x);
        coarse[y * C + x] = make_float4(v.x, v.y, v.z, 0.0f);
    }
}

template <bool BRIGHT>
__global__ __launch_bounds__(kBlock) void sq_gl_down_tiled(const int32_t r, const int32_t c, const float* __restrict__ color,
                                                           const float* __restrict__ d_exposure, const float exposure, const gp::Glare G,
                                                           const float4* __restrict__ fine, float4* __restrict__ coarse,
                                                           const long long tiles, const long long tiles_x) {
    __shared__ float l_in[3][kGlIn * kGlInStride];
    __shared__ float l_h[3][kGlIn * kGlHStride];
    const int32_t R = gp::half_up(r), C = gp::half_up(c);
    const float e = BRIGHT ? (d_exposure ? *d_exposure : exposure) : 0.0f;
    const int lx = threadIdx.x & (kGlTile - 1), ly = threadIdx.x / kGlTile;
    for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
        const long long ty = t / tiles_x, tx = t - ty * tiles_x;
        // cell (iy, ix) of the LDS image holds the fine pixel (y0 + iy, x0 + ix), clamped to the fine image as the taps are: a tap
        // then needs no clamp of its own, and no load leaves the image
        const long long y0 = 2 * ty * kGlTile - 1, x0 = 2 * tx * kGlTile - 1;
        for (int i = threadIdx.x; i < kGlIn * kGlIn; i += kBlock) {
            const int iy = i / kGlIn, ix = i - iy * kGlIn;
            const long long gy = y0 + iy, gx = x0 + ix;
            const int32_t j = (int32_t)(gy < 0 ? 0 : gy > r - 1 ? r - 1 : gy), k = (int32_t)(gx < 0 ? 0 : gx > c - 1 ? c - 1 : gx);
            sq::f3 v;
            if (BRIGHT) v = BrightSrc{ color, e, G, c }(j, k);
            else v = RecordSrc{ fine, c }(j, k);
            const int at = iy * kGlInStride + ix;
            l_in[0][at] = v.x; l_in[1][at] = v.y; l_in[2][at] = v.z;
        }
        __syncthreads();
        for (int i = threadIdx.x; i < kGlIn * kGlTile; i += kBlock) {          // h(j, x) of the 34 fine rows and 16 output columns
            const int iy = i / kGlTile, ox = i - iy * kGlTile;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const float* p = &l_in[ch][iy * kGlInStride + 2 * ox];
                l_h[ch][iy * kGlHStride + ox] = gp::tap4(p[0], p[1], p[2], p[3]);
            }
        }
        __syncthreads();
        const long long y = ty * kGlTile + ly, x = tx * kGlTile + lx;
        if (x < C && y < R) {
            float o[3];
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const float* q = &l_h[ch][2 * ly * kGlHStride + lx];
                o[ch] = gp::tap4(q[0], q[kGlHStride], q[2 * kGlHStride], q[3 * kGlHStride]);
            }
            coarse[y * C + x] = make_float4(o[0], o[1], o[2], 0.0f);
        }
        __syncthreads();        // the next tile's image overwrites this one
    }
}

// A_k = B_k + spread * U(A_k+1), in place on level k (r x c); the coarse level is R x C.
__global__ __launch_bounds__(kBlock) void sq_gl_up_add(const int32_t r, const int32_t c, const int32_t R, const int32_t C,
                                                       const float4* __restrict__ coarse, float4* __restrict__ fine, const float spread,
                                                       const long long tiles, const long long tiles_x) {
    for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
        const long long ty = t / tiles_x, tx = t - ty * tiles_x;
        const long long x = tx * kDirW + (threadIdx.x & (kDirW - 1)), y = ty * kDirH + (threadIdx.x / kDirW);
        if (x >= c || y >= r) continue;
        const sq::f3 u = gp::up(RecordSrc{ coarse, C }, R, C, (int32_t)y, (int32_t)x);
        const float4 b = fine[y * c + x];
        const sq::f3 a = gp::add_scaled(sq::mk(b.x, b.y, b.z), spread, u);
        fine[y * c + x] = make_float4(a.x, a.y, a.z, 0.0f);
    }
}

// One pixel of d_out from the colour c at pixel p: x + strength * U(A_0), or x alone.
template <bool GLARE>
__device__ __forceinline__ sq::f3 composite_pixel(const long long p, const int32_t cols, const float e, const gp::Glare& G, const sq::f3 c,
                                                  const float4* __restrict__ a0, const int32_t R, const int32_t C) {
    const sq::f3 x = gp::exposed(e, G, c);
    if (!GLARE) return x;
    const uint32_t y = (uint32_t)p / (uint32_t)cols;                // p <= 2^31 - 2
    const uint32_t xx = (uint32_t)p - y * (uint32_t)cols;
    return gp::add_scaled(x, G.strength, gp::up(RecordSrc{ a0, C }, R, C, (int32_t)y, (int32_t)xx));
}

// d_out may be d_color (no __restrict__ on either): a lane reads the colour of its own pixels alone, before it writes them.
// One pixel a lane: asks nothing of the pointers.
template <bool GLARE>
__global__ __launch_bounds__(kBlock) void sq_gl_composite1(const long long n, const int32_t cols, const float* color,
                                                           const float* __restrict__ d_exposure, const float exposure, const gp::Glare G,
                                                           const float4* __restrict__ a0, const int32_t R, const int32_t C, float* out) {
    const float e = d_exposure ? *d_exposure : exposure;
    for (long long p = (long long)blockIdx.x * kBlock + threadIdx.x; p < n; p += (long long)gridDim.x * kBlock)
        sq::store3(out, p, composite_pixel<GLARE>(p, cols, e, G, sq::load3(color, p), a0, R, C));
}

// Four consecutive pixels a lane: color and out are 16-byte aligned.  The n % 4 pixels at the end are taken one a lane by the first
// lanes of workgroup 0.
template <bool GLARE>
__global__ __launch_bounds__(kBlock) void sq_gl_composite4(const long long n, const int32_t cols, const float* color,
                                                           const float* __restrict__ d_exposure, const float exposure, const gp::Glare G,
                                                           const float4* __restrict__ a0, const int32_t R, const int32_t C, float* out) {
    const float e = d_exposure ? *d_exposure : exposure;
    const long long quads = n / 4;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < quads; i += (long long)gridDim.x * kBlock) {
        const float4* src = reinterpret_cast<const float4*>(color) + 3 * i;
        const float4 a = src[0], b = src[1], c = src[2];
        const float in[12] = { a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w };
        float o[12];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const sq::f3 v = composite_pixel<GLARE>(4 * i + k, cols, e, G, sq::mk(in[3 * k], in[3 * k + 1], in[3 * k + 2]), a0, R, C);
            o[3 * k] = v.x; o[3 * k + 1] = v.y; o[3 * k + 2] = v.z;
        }
        float4* dst = reinterpret_cast<float4*>(out) + 3 * i;
        dst[0] = make_float4(o[0], o[1], o[2], o[3]);
        dst[1] = make_float4(o[4], o[5], o[6], o[7]);
        dst[2] = make_float4(o[8], o[9], o[10], o[11]);
    }
    const long long p = 4 * quads + threadIdx.x;
    if (blockIdx.x == 0 && p < n) sq::store3(out, p, composite_pixel<GLARE>(p, cols, e, G, sq::load3(color, p), a0, R, C));
}

// The form of the down step into level k when the caller leaves the choice (form = 0).  Measured (tools/gpu_glare.py, DESIGN.md 4.27,
// three rounds in turn): bright-and-down with the composite takes 0.0508 ms tiled against 0.0590 ms direct at 1080 x 1920 and 0.401
// against 0.552 ms at 4320 x 7680, the direct form's own spread being 0.0003 and 0.0008 ms; the coarse levels together take 0.035 ms
// tiled against 0.030 ms direct and 0.137 against 0.133 ms: there the tiled form does not pay.
int auto_glare_form(int level) { return level == 0 ? SQ_DENOISE_FORM_TILED : SQ_DENOISE_FORM_DIRECT; }

struct GlareLevels { int32_t rows[gp::kMaxLevels], cols[gp::kMaxLevels]; size_t at[gp::kMaxLevels]; size_t bytes; };

// r_k, c_k, the byte offset of level k in the workspace, and the bytes of all of them.
GlareLevels glare_levels(int32_t rows, int32_t cols, int32_t levels) {
    GlareLevels L = {};
    int32_t r = rows, c = cols;
    for (int k = 0; k < levels; ++k) {
        r = gp::half_up(r); c = gp::half_up(c);
        L.rows[k] = r; L.cols[k] = c; L.at[k] = L.bytes;
        L.bytes += sizeof(float4) * (size_t)r * (size_t)c;
    }
    return L;
}

bool finite_nonneg(float v) { return v >= 0.0f && v < __builtin_inff(); }

// Everything sq_denoise_glare_device refuses, in the order of the header's list.  Touches neither the device nor a buffer.
int check_glare(int32_t rows, int32_t cols, const float* d_color, const float* d_exposure, const sq_denoise_glare_params* P, float* d_out,
                void* d_work, size_t work_bytes) {
    if (!d_color || !P || !d_out) return sq_set_error("null argument: d_color, params and d_out are required");
    if (rows < 1 || cols < 1) return sq_set_error("rows and cols must be at least 1 (got %d x %d)", rows, cols);
    if ((long long)rows * cols > kMaxPixels) return sq_set_error("%d x %d pixels exceed 2^31 - 1 pixels in one call", rows, cols);
    if (P->levels < 0 || P->levels > gp::kMaxLevels) return sq_set_error("levels must be in 0..%d (got %d)", gp::kMaxLevels, P->levels);
    if (P->form < 0 || P->form > SQ_DENOISE_N_FORMS) return sq_set_error("form must be in 0..%d (got %d)", SQ_DENOISE_N_FORMS, P->form);
    if (!finite_nonneg(P->threshold)) return sq_set_error("threshold must be a finite number >= 0 (got %g)", (double)P->threshold);
    if (!(P->ceiling > P->threshold && P->ceiling < __builtin_inff()))
        return sq_set_error("ceiling must be a finite number > threshold (got %g, threshold %g)", (double)P->ceiling, (double)P->threshold);
    if (!finite_nonneg(P->spread)) return sq_set_error("spread must be a finite number >= 0 (got %g)", (double)P->spread);
    if (!finite_nonneg(P->strength)) return sq_set_error("strength must be a finite number >= 0 (got %g)", (double)P->strength);
    if (P->levels >= 1) {
        if (!d_work) return sq_set_error("null argument: d_work is required with levels >= 1");
        const size_t need = sq_denoise_glare_work_bytes(rows, cols, P->levels);
        if (work_bytes < need)
            return sq_set_error("work_bytes = %zu is too small: %d levels of a %d x %d image need %zu", work_bytes, P->levels, rows, cols, need);
        if ((uintptr_t)d_work % 16 != 0) return sq_set_error("d_work must be 16-byte aligned");
    }
    const size_t n = (size_t)rows * (size_t)cols;
    const NamedRange r[4] = { { "d_color", d_color, 12 * n }, { "d_exposure", d_exposure, 4 }, { "d_out", d_out, 12 * n }, { "d_work", d_work, work_bytes } };
    const int twins[1][2] = { { 0, 2 } };                                        // d_out == d_color
    return refuse_overlaps(r, 4, " (only d_out == d_color may share memory)", twins, 1);
}

template <bool BRIGHT>
void launch_glare_down(int form, int32_t r, int32_t c, const float* color, const float* d_exposure, float exposure, const gp::Glare& G,
                       const float4* fine, float4* coarse, hipStream_t stream) {
    const long long R = gp::half_up(r), C = gp::half_up(c);
    if (form == SQ_DENOISE_FORM_TILED) {
        const long long tx = (C + kGlTile - 1) / kGlTile, ty = (R + kGlTile - 1) / kGlTile;
        hipLaunchKernelGGL(sq_gl_down_tiled<BRIGHT>, dim3(grid_for(tx * ty)), dim3(kBlock), 0, stream, r, c, color, d_exposure, exposure, G, fine,
                           coarse, tx * ty, tx);
    } else {
        const long long tx = (C + kDirW - 1) / kDirW, ty = (R + kDirH - 1) / kDirH;
        hipLaunchKernelGGL(sq_gl_down_direct<BRIGHT>, dim3(grid_for(tx * ty)), dim3(kBlock), 0, stream, r, c, color, d_exposure, exposure, G, fine,
                           coarse, tx * ty, tx);
    }
}

int enqueue_glare(int32_t device, int32_t rows, int32_t cols, const float* d_color, const float* d_exposure, const sq_denoise_glare_params& P,
                  float* d_out, void* d_work, void* hip_stream) {
    SQ_HIP(hipSetDevice(device));
    hipStream_t stream = (hipStream_t)hip_stream;
    const gp::Glare G{ { P.gain[0], P.gain[1], P.gain[2] }, P.threshold, P.ceiling, P.spread, P.strength };
    const long long n = (long long)rows * cols;
    const GlareLevels L = glare_levels(rows, cols, P.levels);
    float4* level[gp::kMaxLevels] = {};
    for (int k = 0; k < P.levels; ++k) level[k] = (float4*)((char*)d_work + L.at[k]);
    for (int k = 0; k < P.levels; ++k) {
        const int form = P.form == SQ_DENOISE_FORM_AUTO ? auto_glare_form(k) : P.form;
        if (k == 0) launch_glare_down<true>(form, rows, cols, d_color, d_exposure, P.exposure, G, nullptr, level[0], stream);
        else launch_glare_down<false>(form, L.rows[k - 1], L.cols[k - 1], nullptr, nullptr, 0.0f, G, level[k - 1], level[k], stream);
        SQ_HIP(hipGetLastError());
    }
    for (int k = P.levels - 2; k >= 0; --k) {
        const long long tx = ((long long)L.cols[k] + kDirW - 1) / kDirW, ty = ((long long)L.rows[k] + kDirH - 1) / kDirH;
        hipLaunchKernelGGL(sq_gl_up_add, dim3(grid_for(tx * ty)), dim3(kBlock), 0, stream, L.rows[k], L.cols[k], L.rows[k + 1], L.cols[k + 1],
                           level[k + 1], level[k], P.spread, tx * ty, tx);
        SQ_HIP(hipGetLastError());
    }
    const bool wide = (uintptr_t)d_color % 16 == 0 && (uintptr_t)d_out % 16 == 0;
    const long long lanes = wide ? (n + 3) / 4 : n;
    const dim3 grid(grid_for((lanes + kBlock - 1) / kBlock)), block(kBlock);
    const int32_t R0 = P.levels ? L.rows[0] : 0, C0 = P.levels ? L.cols[0] : 0;
    if (P.levels) {
        if (wide) hipLaunchKernelGGL(sq_gl_composite4<true>, grid, block, 0, stream, n, cols, d_color, d_exposure, P.exposure, G, level[0], R0, C0, d_out);
        else      hipLaunchKernelGGL(sq_gl_composite1<true>, grid, block, 0, stream, n, cols, d_color, d_exposure, P.exposure, G, level[0], R0, C0, d_out);
    } else {
        if (wide) hipLaunchKernelGGL(sq_gl_composite4<false>, grid, block, 0, stream, n, cols, d_color, d_exposure, P.exposure, G, level[0], R0, C0, d_out);
        else      hipLaunchKernelGGL(sq_gl_composite1<false>, grid, block, 0, stream, n, cols, d_color, d_exposure, P.exposure, G, level[0], R0, C0, d_out);
    }
    SQ_HIP(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" size_t sq_denoise_glare_work_bytes(int32_t rows, int32_t cols, int32_t levels) {
    if (rows < 1 || cols < 1 || (long long)rows * cols > kMaxPixels || levels < 0 || levels > gp::kMaxLevels) return 0;
    return glare_levels(rows, cols, levels).bytes;
}

extern "C" int sq_denoise_glare_device(int32_t device, int32_t rows, int32_t cols, const float* d_color, const float* d_exposure,
                                       const sq_denoise_glare_params* params, float* d_out, void* d_work, size_t work_bytes, void* hip_stream) {
    if (check_glare(rows, cols, d_color, d_exposure, params, d_out, d_work, work_bytes)) return 1;
    return enqueue_glare(device, rows, cols, d_color, d_exposure, *params, d_out, d_work, hip_stream);
}

extern "C" const char* sq_denoise_last_error(void) { return sq_error_buffer(); }
extern "C" const char* sq_denoise_build_id(void) { return SQ_DENOISE_BUILD_ID; }
extern "C" int32_t sq_denoise_pass_form(int32_t pass) { return pass < 0 || pass > 7 ? -1 : auto_form(pass); }

extern "C" size_t sq_denoise_workspace_bytes(int32_t rows, int32_t cols) {
    if (rows < 1 || cols < 1 || (long long)rows * cols > kMaxPixels) return 0;
    return (size_t)rows * (size_t)cols * 4 * sizeof(float4);
}

extern "C" int sq_denoise_variance_device(int32_t device, int64_t n_pixels, const float* d_sum, const float* d_sum2,
                                          const int32_t* d_count, float* d_var, void* hip_stream) {
    if (!d_sum || !d_sum2 || !d_count || !d_var) return sq_set_error("null argument: d_sum, d_sum2, d_count and d_var are required");
    if (n_pixels < 0) return sq_set_error("n_pixels must not be negative (got %lld)", (long long)n_pixels);
    if (n_pixels > (int64_t)1 << 56) return sq_set_error("n_pixels = %lld is more than any device holds", (long long)n_pixels);
    const size_t n = (size_t)n_pixels;
    const NamedRange in[3] = { { "d_sum", d_sum, 12 * n }, { "d_sum2", d_sum2, 12 * n }, { "d_count", d_count, 4 * n } };
    for (const NamedRange& s : in)
        if (ranges_overlap(d_var, 4 * n, s.p, s.bytes)) return sq_set_error("d_var and %s overlap", s.name);
    if (n_pixels == 0) return 0;
    SQ_HIP(hipSetDevice(device));
    hipLaunchKernelGGL(sq_dn_variance, dim3(grid_for(((long long)n_pixels + kBlock - 1) / kBlock)), dim3(kBlock), 0, (hipStream_t)hip_stream,
                       (long long)n_pixels, d_sum, d_sum2, d_count, d_var);
    SQ_HIP(hipGetLastError());
    return 0;
}

extern "C" int sq_denoise_device(int32_t device, int32_t rows, int32_t cols, const float* d_color, const float* d_var,
                                 const int32_t* d_tri, const float* d_normal, const float* d_point, const sq_denoise_params* params,
                                 float* d_out, float* d_out_var, void* d_work, size_t work_bytes, void* hip_stream) {
    if (check_call(rows, cols, d_color, d_var, d_tri, d_normal, d_point, params, d_out, d_out_var, d_work, work_bytes)) return 1;
    return enqueue(device, rows, cols, d_color, d_var, d_tri, d_normal, d_point, *params, d_out, d_out_var, d_work, hip_stream, -1, params->passes - 1);
}

extern "C" int sq_denoise_stage_device(int32_t device, int32_t rows, int32_t cols, const float* d_color, const float* d_var,
                                       const int32_t* d_tri, const float* d_normal, const float* d_point, const sq_denoise_params* params,
                                       float* d_out, float* d_out_var, void* d_work, size_t work_bytes, void* hip_stream, int32_t stage) {
    if (check_call(rows, cols, d_color, d_var, d_tri, d_normal, d_point, params, d_out, d_out_var, d_work, work_bytes)) return 1;
    if (stage < -1 || stage >= params->passes) return sq_set_error("stage must be in -1..%d (got %d)", params->passes - 1, stage);
    return enqueue(device, rows, cols, d_color, d_var, d_tri, d_normal, d_point, *params, d_out, d_out_var, d_work, hip_stream, stage, stage);
}

extern "C" int sq_denoise_sparse_mask_device(int32_t device, int32_t rows, int32_t cols, int32_t stride, int32_t oy, int32_t ox,
                                             const int32_t* d_tri, const float* d_normal, const float* d_point,
                                             const sq_denoise_sparse_params* params, uint8_t* d_mask, void* hip_stream) {
    if (!d_tri || !d_normal || !d_point || !params || !d_mask)
        return sq_set_error("null argument: d_tri, d_normal, d_point, params and d_mask are required");
    const size_t n = rows > 0 && cols > 0 ? (size_t)rows * (size_t)cols : 0;
    const NamedRange r[4] = { { "d_tri", d_tri, 4 * n }, { "d_normal", d_normal, 12 * n }, { "d_point", d_point, 12 * n }, { "d_mask", d_mask, n } };
    if (check_sparse(rows, cols, stride, oy, ox, params, r, 4)) return 1;
    return enqueue_sparse(device, rows, cols, stride, oy, ox, *params, d_tri, d_normal, d_point, nullptr, nullptr, nullptr, d_mask, nullptr,
                          nullptr, hip_stream);
}

extern "C" int sq_denoise_upsample_device(int32_t device, int32_t rows, int32_t cols, int32_t stride, int32_t oy, int32_t ox,
                                          const float* d_color, const float* d_var, const int32_t* d_tri, const float* d_normal,
                                          const float* d_point, const uint8_t* d_mask, const sq_denoise_sparse_params* params,
                                          float* d_out, float* d_out_var, void* hip_stream) {
    if (!d_color || !d_tri || !d_normal || !d_point || !d_mask || !params || !d_out)
        return sq_set_error("null argument: d_color, d_tri, d_normal, d_point, d_mask, params and d_out are required");
    if (d_out_var && !d_var) return sq_set_error("d_out_var needs d_var: without a variance image there is none to fill in");
    const size_t n = rows > 0 && cols > 0 ? (size_t)rows * (size_t)cols : 0;
    const NamedRange r[8] = { { "d_color", d_color, 12 * n }, { "d_var", d_var, 4 * n }, { "d_tri", d_tri, 4 * n }, { "d_normal", d_normal, 12 * n },
                              { "d_point", d_point, 12 * n }, { "d_mask", d_mask, n }, { "d_out", d_out, 12 * n }, { "d_out_var", d_out_var, 4 * n } };
    if (check_sparse(rows, cols, stride, oy, ox, params, r, 8)) return 1;
    return enqueue_sparse(device, rows, cols, stride, oy, ox, *params, d_tri, d_normal, d_point, d_color, d_var, d_mask, nullptr, d_out,
                          d_out_var, hip_stream);
}
