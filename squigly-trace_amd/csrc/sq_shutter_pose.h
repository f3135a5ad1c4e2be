// sq_shutter_pose.h — the camera of one instant of an exposure (include/squigly_shutter.h), written once for the host and the
// device: sq_shutter_pose compiles this text with the host compiler, every lane of libsquigly_shutter.so's ray kernels with the
// device compiler, and tests/shutter_pose_main.cpp with g++ under the sanitizers.  Only the shutter library lists this header.
//
// Every operation is one fp32 operation in the order of the header's contract; the sines and cosines are sq::fsincos, the numeric
// spec's, and the matrix is bit for bit sq_rot_matrix_rads' (csrc/sq_host.cpp): yx = ry * rx, rot = rz * yx, an entry the fold
// r = a[i][k] * b[k][j] + r over k = 0, 1, 2 from r = +0.  Nothing here is skipped for a zero or a one: 0 * inf is NaN there too.
#pragma once
#include <stdint.h>

#include "sq_math.h"

namespace shutterpose {

// What the kernels take of an sq_motion, by value: the open pose, the two differences (taken by the host, in fp32) and time_jitter.
struct Motion {
    float pos0[3], dpos[3], ang0[3], dang[3];
    float time_jitter;
};

SQ_HD Motion motion_of(const float* pos0, const float* ang0, const float* pos1, const float* ang1, float time_jitter) {
    Motion M;
    for (int c = 0; c < 3; ++c) {
        M.pos0[c] = pos0[c]; M.dpos[c] = pos1[c] - pos0[c];
        M.ang0[c] = ang0[c]; M.dang[c] = ang1[c] - ang0[c];
    }
    M.time_jitter = time_jitter;
    return M;
}

SQ_HD void mul3(const float* a, const float* b, float* o) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            float r = 0.0f;
#pragma unroll
            for (int k = 0; k < 3; ++k) r = a[3 * i + k] * b[3 * k + j] + r;
            o[3 * i + j] = r;
        }
}

// rotMatrixRads: foldr1 (*) [rz alp, ry bet, rx gam] = rz * (ry * rx).
SQ_HD void rot_matrix_rads(float alp, float bet, float gam, float* out9) {
    float sa, ca, sb, cb, sg, cg;
    sq::fsincos(alp, sa, ca); sq::fsincos(bet, sb, cb); sq::fsincos(gam, sg, cg);
    const float rz[9] = { ca, -sa, 0, sa, ca, 0, 0, 0, 1 };
    const float ry[9] = { cb, 0, sb, 0, 1, 0, -sb, 0, cb };
    const float rx[9] = { 1, 0, 0, 0, cg, -sg, 0, sg, cg };
    float yx[9];
    mul3(ry, rx, yx);
    mul3(rz, yx, out9);
}

// tt of sub-ray r of R: u = random01 m4, or anything finite when time_jitter == 0 (0 * u is +0 and r + 0 is r: no draw is needed).
SQ_HD float instant(int r, int R, float time_jitter, float u) { return ((float)r + time_jitter * u) / (float)R; }

// pos and rot at the instant tt: x0 + tt * dx per component, then the matrix of the three angles.
SQ_HD void pose_at(const Motion& M, float tt, float* pos, float* rot) {
    float ang[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        pos[c] = M.pos0[c] + tt * M.dpos[c];
        ang[c] = M.ang0[c] + tt * M.dang[c];
    }
    rot_matrix_rads(ang[0], ang[1], ang[2], rot);
}

}  // namespace shutterpose
