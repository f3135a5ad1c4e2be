// sq_temporal.hip — libsquigly_temporal.so (include/squigly_temporal.h): temporal accumulation over device images.  It knows nothing
// of scenes: device images and a caller-given history block in, device images and the next block out, no state.
//
// One kernel does a frame.  A thread is a pixel, a wave 64 consecutive columns of a row (a block is 4 such row segments), so that the
// plain reads and writes of a wave are one span of memory each and a tap's loads of one plane of the previous block are close to
// contiguous: under a slow camera the 64 lanes of a wave reproject into one or two row segments of the previous frame.  The block of
// a frame is three planes of 16-byte records (CV colour + variance, NL normal + length, PT point + triangle), so a tap is three
// dwordx4 loads, and the twelve loads of a pixel's four taps are issued together, before any tap is judged (sq_temporal_pixel.h).
// No LDS for the taps: the four taps of neighbouring lanes overlap, and L1 / L2 serve the re-reads.  (The moving call's clamp window
// is another matter: below.)
//
// The arithmetic of a pixel is csrc/sq_temporal_pixel.h: one `accumulate` for the static and the moving call, and `project`, the
// text the host's sq_temporal_project compiles too.  -ffp-contract=off and the correctly rounded divide keep it equal to the numpy
// restatements.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "sq_call_checks.h"
#include "sq_temporal_pixel.h"
#include "../../include/squigly_temporal.h"

#ifndef SQ_TEMPORAL_BUILD_ID
#define SQ_TEMPORAL_BUILD_ID "unknown"
#endif

namespace {

using temporalpix::Rec;

constexpr int kBlock = 256;
constexpr long long kMaxPixels = 0x7fffffffLL;
constexpr int kMaxGrid = 2048;             // blocks of a launch: 8 per CU; the kernels stride over their tiles
constexpr int kTileW = 64, kTileH = 4;     // a block is 4 rows of 64 pixels, a wave one row segment

struct Cam { float pos[3]; float rot[9]; };

// One kernel in four instantiations.  <kClampNone, false> is the static one, what a call without tables, flags and clamp runs: the
// tile, the pixel's own loads, the twelve tap loads, the stores; the table lookup, every read of M and the flags store are compiled
// out of it.  With kMoving, ahead of the twelve loads a moved pixel takes two dependent loads (its triangle's object, then the
// object's twelve floats, which a wave mostly shares).  The clamp's window is up to 49 taps of colour and triangle a pixel, in two
// forms that give the same bits (the window's order is pinned, sq_temporal_pixel.h): kClampDirect reads every tap from memory,
// kClampTiled stages the tile and its halo of `radius` pixels in LDS once -- (4 + 2r) x (64 + 2r) records of colour and a hit flag,
// 11200 bytes at r = 3 -- and reads the taps from there.  A tap that does not count (outside the image, or no hit) is staged with
// flag 0, so the image's borders need no second test.
constexpr int kClampNone = 0, kClampDirect = SQ_TEMPORAL_FORM_DIRECT, kClampTiled = SQ_TEMPORAL_FORM_TILED;
constexpr int kMaxRadius = 3;
constexpr int kHaloRecs = (kTileH + 2 * kMaxRadius) * (kTileW + 2 * kMaxRadius);

struct Moving {
    const int32_t* object; const float* back;      // both or neither
    int32_t n_tris, n_objects;
    temporalpix::Clamp clamp;                        // read by the clamped instantiations only
};

// d_color / d_out and d_var / d_out_var may be the same memory: a thread reads its own pixel of the inputs before it writes its
// own pixel of the outputs, and none of the four is __restrict__.
template <int kClamp, bool kMoving>
__global__ __launch_bounds__(kBlock) void sq_tp_accumulate(const int rows, const int cols, const float* color, const float* var,
                                                           const int32_t* __restrict__ tri, const float* __restrict__ normal,
                                                           const float* __restrict__ point, const float* __restrict__ alpha,
                                                           const Cam cam, const Rec* __restrict__ prev, const temporalpix::Params P,
                                                           const Moving M, Rec* __restrict__ next, float* out, float* out_var,
                                                           int32_t* __restrict__ out_len, uint8_t* __restrict__ out_flags,
                                                           const long long tiles, const long long tiles_x) {
    static_assert(kMoving || kClamp == kClampNone, "a clamp is the moving call's");
    __shared__ Rec halo[kClamp == kClampTiled ? kHaloRecs : 1];
    const long long n = (long long)rows * cols;
    const Rec* p_cv = prev;
    const Rec* p_nl = prev ? prev + n : nullptr;
    const Rec* p_pt = prev ? prev + 2 * n : nullptr;
    const int r = kClamp == kClampNone ? 0 : M.clamp.radius;
    const int halo_w = kTileW + 2 * r;
    const int lx = threadIdx.x & (kTileW - 1), ly = threadIdx.x / kTileW;
    for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {          // (the trip count is the block's: every thread meets every barrier)
        const long long ty = t / tiles_x, tx = t - ty * tiles_x;
        if (kClamp == kClampTiled) {
            __syncthreads();                                             // the last tile's taps have been read
            for (int e = threadIdx.x; e < halo_w * (kTileH + 2 * r); e += kBlock) {
                const int hy = e / halo_w, hx = e - hy * halo_w;
                const long long gy = ty * kTileH + hy - r, gx = tx * kTileW + hx - r;
                Rec c = { 0.0f, 0.0f, 0.0f, 0.0f };
                if (gy >= 0 && gy < rows && gx >= 0 && gx < cols) {
                    const long long q = gy * cols + gx;
                    if (tri[q] >= 0) c = Rec{ color[3 * q], color[3 * q + 1], color[3 * q + 2], 1.0f };
                }
                halo[e] = c;
            }
            __syncthreads();
        }
        const long long x = tx * kTileW + lx, y = ty * kTileH + ly;
        if (x >= cols || y >= rows) continue;
        const long long p = y * cols + x;
        const float cr = color[3 * p], cg = color[3 * p + 1], cb = color[3 * p + 2], v = var[p];
        const int32_t tr = tri[p];
        const float nx = normal[3 * p], ny = normal[3 * p + 1], nz = normal[3 * p + 2];
        const float px = point[3 * p], py = point[3 * p + 1], pz = point[3 * p + 2];
        const float al = alpha ? alpha[p] : -1.0f;
        float B[12];
        bool moved = false;
        if (kMoving && M.object && prev && tr >= 0) {                    // an index outside its table is never read through
            const int32_t o = tr < M.n_tris ? M.object[tr] : -1;
            if (o >= 0 && o < M.n_objects) {
                moved = true;
#pragma unroll
                for (int i = 0; i < 12; ++i) B[i] = M.back[12LL * o + i];
            }
        }
        uint32_t flags;
        temporalpix::Pixel res;
        if (kClamp == kClampTiled) {
            const Rec* centre = halo + (ly + r) * halo_w + (lx + r);
            res = temporalpix::accumulate(p_cv, p_nl, p_pt, rows, cols, cam.pos, cam.rot, P, cr, cg, cb, v, tr, nx, ny, nz, px, py, pz,
                                          alpha != nullptr, al, moved, B, &M.clamp,
                                          [&](int j, int i, float* c) {
                                              const Rec h = centre[j * halo_w + i];
                                              c[0] = h.x; c[1] = h.y; c[2] = h.z;
                                              return h.w != 0.0f;
                                          }, flags);
        } else {
            res = temporalpix::accumulate(p_cv, p_nl, p_pt, rows, cols, cam.pos, cam.rot, P, cr, cg, cb, v, tr, nx, ny, nz, px, py, pz,
                                          alpha != nullptr, al, moved, B, kClamp == kClampNone ? nullptr : &M.clamp,
                                          [&](int j, int i, float* c) {
                                              const long long qy = y + j, qx = x + i;
                                              if (qy < 0 || qy >= rows || qx < 0 || qx >= cols) return false;
                                              const long long q = qy * cols + qx;
                                              if (tri[q] < 0) return false;
                                              c[0] = color[3 * q]; c[1] = color[3 * q + 1]; c[2] = color[3 * q + 2];
                                              return true;
                                          }, flags);
        }
        next[p] = Rec{ res.r, res.g, res.b, res.v };
        next[n + p] = Rec{ nx, ny, nz, temporalpix::int_bits(res.len) };
        next[2 * n + p] = Rec{ px, py, pz, temporalpix::int_bits(tr) };
        out[3 * p] = res.r; out[3 * p + 1] = res.g; out[3 * p + 2] = res.b;
        out_var[p] = res.v;
        if (out_len) out_len[p] = res.len;
        if (kMoving && out_flags) out_flags[p] = (uint8_t)flags;
    }
}

__global__ __launch_bounds__(kBlock) void sq_tp_unpack(const long long n, const Rec* __restrict__ hist, float* __restrict__ color,
                                                       float* __restrict__ var, int32_t* __restrict__ len, int32_t* __restrict__ tri,
                                                       float* __restrict__ normal, float* __restrict__ point) {
    for (long long p = (long long)blockIdx.x * kBlock + threadIdx.x; p < n; p += (long long)gridDim.x * kBlock) {
        if (color || var) {
            const Rec cv = hist[p];
            if (color) { color[3 * p] = cv.x; color[3 * p + 1] = cv.y; color[3 * p + 2] = cv.z; }
            if (var) var[p] = cv.w;
        }
        if (normal || len) {
            const Rec nl = hist[n + p];
            if (normal) { normal[3 * p] = nl.x; normal[3 * p + 1] = nl.y; normal[3 * p + 2] = nl.z; }
            if (len) len[p] = temporalpix::bits_int(nl.w);
        }
        if (point || tri) {
            const Rec pt = hist[2 * n + p];
            if (point) { point[3 * p] = pt.x; point[3 * p + 1] = pt.y; point[3 * p + 2] = pt.z; }
            if (tri) tri[p] = temporalpix::bits_int(pt.w);
        }
    }
}

int check_size(int32_t rows, int32_t cols) {
    if (rows < 1 || cols < 1) return sq_set_error("rows and cols must be at least 1 (got %d x %d)", rows, cols);
    if ((long long)rows * cols > kMaxPixels) return sq_set_error("%d x %d pixels exceed 2^31 - 1 pixels in one call", rows, cols);
    return 0;
}

// The images and blocks both accumulate calls take, and what the moving call adds: the checks' argument, and the launch's.
struct Buffers {
    const float *d_color, *d_var; const int32_t* d_tri; const float *d_normal, *d_point, *d_alpha; const void* d_prev;
    void* d_next; float *d_out, *d_out_var; int32_t* d_out_len;
    const int32_t* d_object; const float* d_back; uint8_t* d_out_flags;      // NULL from the old entry point
};

// The table of a call's device buffers: the eleven both calls take, then the moving call's three.
constexpr int kSharedRanges = 11, kAllRanges = 14;
struct Ranges { NamedRange r[kAllRanges]; };
Ranges ranges_of(const Buffers& b, int32_t rows, int32_t cols, int32_t n_tris, int32_t n_objects) {
    const size_t n = (size_t)rows * (size_t)cols, hb = sq_temporal_history_bytes(rows, cols);
    return { { { "d_color", b.d_color, 12 * n }, { "d_var", b.d_var, 4 * n }, { "d_tri", b.d_tri, 4 * n }, { "d_normal", b.d_normal, 12 * n },
               { "d_point", b.d_point, 12 * n }, { "d_alpha", b.d_alpha, 4 * n }, { "d_prev", b.d_prev, hb }, { "d_next", b.d_next, hb },
               { "d_out", b.d_out, 12 * n }, { "d_out_var", b.d_out_var, 4 * n }, { "d_out_len", b.d_out_len, 4 * n },
               { "d_object", b.d_object, 4 * (size_t)n_tris }, { "d_back", b.d_back, 48 * (size_t)n_objects },
               { "d_out_flags", b.d_out_flags, n } } };
}

// Everything that can be refused, in the order of the header's list.  Touches neither the device nor a buffer.
int check_accumulate(int32_t rows, int32_t cols, const Buffers& b, const sq_camera* prev_cam, const sq_temporal_params* P) {
    if (!b.d_color || !b.d_var || !b.d_tri || !b.d_normal || !b.d_point || !P || !b.d_next || !b.d_out || !b.d_out_var)
        return sq_set_error("null argument: d_color, d_var, d_tri, d_normal, d_point, params, d_next, d_out and d_out_var are required");
    if (b.d_prev && !prev_cam) return sq_set_error("null argument: prev_cam is required with d_prev (the camera the previous block was rendered under)");
    if (check_size(rows, cols)) return 1;
    if (!(P->alpha_min >= 0.0f && P->alpha_min <= 1.0f)) return sq_set_error("alpha_min must be a number in 0..1 (got %g)", (double)P->alpha_min);
    if (P->max_history < 1 || P->max_history > 65536) return sq_set_error("max_history must be in 1..65536 (got %d)", P->max_history);
    if (!(P->sigma_p >= 0.0f)) return sq_set_error("sigma_p must be a number >= 0 (got %g)", (double)P->sigma_p);
    if (P->cos_n != P->cos_n) return sq_set_error("cos_n must be a number (got %g)", (double)P->cos_n);
    if ((uintptr_t)b.d_prev % 16 != 0) return sq_set_error("d_prev must be 16-byte aligned");
    if ((uintptr_t)b.d_next % 16 != 0) return sq_set_error("d_next must be 16-byte aligned");
    const int twins[2][2] = { { 0, 8 }, { 1, 9 } };                              // d_out == d_color, d_out_var == d_var
    return refuse_overlaps(ranges_of(b, rows, cols, 0, 0).r, kSharedRanges, " (only d_out == d_color and d_out_var == d_var may share memory)", twins, 2);
}

// Radius 3 is the widest window the tiled form's LDS holds; what the auto form is, is DESIGN.md 4.28's measurement.
int auto_clamp_form() { return SQ_TEMPORAL_FORM_TILED; }

// What the moving call refuses beyond check_accumulate, which has passed, in the order of the header's list.
int check_moving(int32_t rows, int32_t cols, const Buffers& b, int32_t n_tris, int32_t n_objects, const sq_temporal_clamp* clamp, int32_t form) {
    if (n_tris < 0 || n_objects < 0) return sq_set_error("n_tris and n_objects must not be negative (got %d and %d)", n_tris, n_objects);
    if ((b.d_object == nullptr) != (b.d_back == nullptr))
        return sq_set_error("d_object and d_back go together: both NULL (nothing moves) or both given");
    if (b.d_object && n_tris == 0) return sq_set_error("d_object is given with n_tris = 0");
    if (b.d_back && n_objects == 0) return sq_set_error("d_back is given with n_objects = 0");
    if (clamp) {
        if (clamp->radius < 1 || clamp->radius > kMaxRadius) return sq_set_error("clamp.radius must be in 1..3 (got %d)", clamp->radius);
        if (!(clamp->k >= 0.0f)) return sq_set_error("clamp.k must be a number >= 0 (got %g)", (double)clamp->k);
    }
    if (form < SQ_TEMPORAL_FORM_AUTO || form > SQ_TEMPORAL_N_FORMS) return sq_set_error("form must be in 0..%d (got %d)", SQ_TEMPORAL_N_FORMS, form);
    const int twins[2][2] = { { 1, 9 }, { 0, 8 } };                              // under a clamp neighbours' colours are read: only the first
    return refuse_overlaps(ranges_of(b, rows, cols, n_tris, n_objects).r, kAllRanges,
                           clamp ? " (under a clamp only d_out_var == d_var may share memory)"
                                 : " (only d_out == d_color and d_out_var == d_var may share memory)", twins, clamp ? 1 : 2);
}

unsigned grid_for(long long units) { return (unsigned)(units < kMaxGrid ? units : kMaxGrid); }

// A checked call, from either entry point, to its launch.  The instantiation follows from what the caller gave: the static one
// unless there are tables, flags to write, or a clamp that has history to hold.
int launch_accumulate(int32_t device, int32_t rows, int32_t cols, const Buffers& b, const sq_camera* prev_cam, const sq_temporal_params* params,
                      int32_t n_tris, int32_t n_objects, const sq_temporal_clamp* clamp, int32_t form, void* hip_stream) {
    SQ_HIP(hipSetDevice(device));
    Cam cam = {};
    if (b.d_prev) {
        for (int i = 0; i < 3; ++i) cam.pos[i] = prev_cam->pos[i];
        for (int i = 0; i < 9; ++i) cam.rot[i] = prev_cam->rot[i];
    }
    const temporalpix::Params P{ params->alpha_min, params->max_history, params->sigma_p, params->cos_n };
    const Moving M{ b.d_object, b.d_back, n_tris, n_objects, clamp ? temporalpix::Clamp{ clamp->radius, clamp->k } : temporalpix::Clamp{ 0, 0.0f } };
    // without history nothing is blended, so nothing is clamped: the window is not read at all
    const int how = !clamp || !b.d_prev ? kClampNone : form == SQ_TEMPORAL_FORM_AUTO ? auto_clamp_form() : form;
    const long long tx = ((long long)cols + kTileW - 1) / kTileW, ty = ((long long)rows + kTileH - 1) / kTileH;
    auto* kernel = how == kClampTiled ? sq_tp_accumulate<kClampTiled, true>
                 : how == kClampDirect ? sq_tp_accumulate<kClampDirect, true>
                 : b.d_object || b.d_out_flags ? sq_tp_accumulate<kClampNone, true> : sq_tp_accumulate<kClampNone, false>;
    hipLaunchKernelGGL(kernel, dim3(grid_for(tx * ty)), dim3(kBlock), 0, (hipStream_t)hip_stream, rows, cols, b.d_color, b.d_var, b.d_tri,
                       b.d_normal, b.d_point, b.d_alpha, cam, (const Rec*)b.d_prev, P, M, (Rec*)b.d_next, b.d_out, b.d_out_var, b.d_out_len,
                       b.d_out_flags, tx * ty, tx);
    SQ_HIP(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" const char* sq_temporal_last_error(void) { return sq_error_buffer(); }
extern "C" const char* sq_temporal_build_id(void) { return SQ_TEMPORAL_BUILD_ID; }

extern "C" size_t sq_temporal_history_bytes(int32_t rows, int32_t cols) {
    if (rows < 1 || cols < 1 || (long long)rows * cols > kMaxPixels) return 0;
    return (size_t)rows * (size_t)cols * 3 * sizeof(Rec);
}

extern "C" int sq_temporal_project(const sq_camera* prev, int32_t w, int32_t h, const float point[3], float* fx, float* fy) {
    if (!prev || !point || !fx || !fy) { sq_set_error("null argument: prev, point, fx and fy are required"); return -1; }
    if (w < 1 || h < 1) { sq_set_error("w and h must be at least 1 (got %d x %d)", w, h); return -1; }
    float x, y;
    const bool ok = temporalpix::project(prev->pos, prev->rot, (float)w, (float)h, point[0], point[1], point[2], x, y);
    *fx = x; *fy = y;
    return ok ? 1 : 0;
}

extern "C" int sq_temporal_accumulate_device(int32_t device, int32_t rows, int32_t cols, const float* d_color, const float* d_var,
                                             const int32_t* d_tri, const float* d_normal, const float* d_point, const float* d_alpha,
                                             const sq_camera* prev_cam, const void* d_prev, const sq_temporal_params* params,
                                             void* d_next, float* d_out, float* d_out_var, int32_t* d_out_len, void* hip_stream) {
    const Buffers b{ d_color, d_var, d_tri, d_normal, d_point, d_alpha, d_prev, d_next, d_out, d_out_var, d_out_len, nullptr, nullptr, nullptr };
    if (check_accumulate(rows, cols, b, prev_cam, params)) return 1;
    return launch_accumulate(device, rows, cols, b, prev_cam, params, 0, 0, nullptr, SQ_TEMPORAL_FORM_AUTO, hip_stream);
}

extern "C" int sq_temporal_accumulate_moving_device(int32_t device, int32_t rows, int32_t cols, const float* d_color, const float* d_var,
                                                    const int32_t* d_tri, const float* d_normal, const float* d_point, const float* d_alpha,
                                                    const sq_camera* prev_cam, const void* d_prev, const sq_temporal_params* params,
                                                    const int32_t* d_object, int32_t n_tris, const float* d_back, int32_t n_objects,
                                                    const sq_temporal_clamp* clamp, int32_t form, void* d_next, float* d_out,
                                                    float* d_out_var, int32_t* d_out_len, uint8_t* d_out_flags, void* hip_stream) {
    const Buffers b{ d_color, d_var, d_tri, d_normal, d_point, d_alpha, d_prev, d_next, d_out, d_out_var, d_out_len, d_object, d_back, d_out_flags };
    if (check_accumulate(rows, cols, b, prev_cam, params) || check_moving(rows, cols, b, n_tris, n_objects, clamp, form)) return 1;
    return launch_accumulate(device, rows, cols, b, prev_cam, params, n_tris, n_objects, clamp, form, hip_stream);
}

extern "C" int sq_temporal_unpack_device(int32_t device, int32_t rows, int32_t cols, const void* d_hist, float* d_color, float* d_var,
                                         int32_t* d_len, int32_t* d_tri, float* d_normal, float* d_point, void* hip_stream) {
    if (!d_hist) return sq_set_error("null argument: d_hist is required");
    if (!d_color && !d_var && !d_len && !d_tri && !d_normal && !d_point)
        return sq_set_error("no output: give at least one of d_color, d_var, d_len, d_tri, d_normal and d_point");
    if (check_size(rows, cols)) return 1;
    if ((uintptr_t)d_hist % 16 != 0) return sq_set_error("d_hist must be 16-byte aligned");
    const size_t n = (size_t)rows * (size_t)cols;
    const NamedRange r[7] = { { "d_hist", d_hist, sq_temporal_history_bytes(rows, cols) }, { "d_color", d_color, 12 * n }, { "d_var", d_var, 4 * n },
                              { "d_len", d_len, 4 * n }, { "d_tri", d_tri, 4 * n }, { "d_normal", d_normal, 12 * n }, { "d_point", d_point, 12 * n } };
    if (refuse_overlaps(r, 7)) return 1;
    SQ_HIP(hipSetDevice(device));
    hipLaunchKernelGGL(sq_tp_unpack, dim3(grid_for(((long long)n + kBlock - 1) / kBlock)), dim3(kBlock), 0, (hipStream_t)hip_stream,
                       (long long)n, (const Rec*)d_hist, d_color, d_var, d_len, d_tri, d_normal, d_point);
    SQ_HIP(hipGetLastError());
    return 0;
}
