// The back-projection of a depth pixel into the world that lift_queries.hip (step 5 of its rule) and fuse_views.hip (step 4) share:
// one definition, so the two stages cannot drift apart in the order of their operations.
//
// Contraction is the including file's choice.  hipcc contracts a multiply and an add into a fused multiply-add by default, and HIP's
// __fmul_rn / __fadd_rn / __fsub_rn / __fdiv_rn do not prevent it: they are defined as the plain operators (lift_queries.hip used to
// spell this sequence with them, and compiled to the same instructions as it does now).  The operators below stand in this header, so
// the `#pragma clang fp contract` state of the including file governs them.  fuse_views.hip, whose results must EQUAL a float32
// evaluation of its restatement, includes this header under `contract(off)`: there every operation is rounded on its own.
// lift_queries.hip includes it under the default, as its kernel was always compiled; its centres are tested to a tolerance.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// One view's camera: fx, fy, cx, cy in pixels of the depth image and the rows of the fp32 cam_to_world [R | t].
struct Sd3dCamera {
    float fx, fy, cx, cy;
    float r00, r01, r02, t0, r10, r11, r12, t1, r20, r21, r22, t2;
};
__device__ __forceinline__ Sd3dCamera sd3d_load_camera(const float* __restrict__ intr, const float* __restrict__ c2w, int64_t v) {
    const float* kk = intr + v * 4;
    const float* m = c2w + v * 12;
    return Sd3dCamera{kk[0], kk[1], kk[2], kk[3], m[0], m[1], m[2], m[3], m[4], m[5], m[6], m[7], m[8], m[9], m[10], m[11]};
}

// p_c = ((ui - cx) d / fx, (vi - cy) d / fy, d), w = R p_c + t, each component as ((r0 x + r1 y) + r2 d) + t, left to right.
__device__ __forceinline__ void sd3d_backproject(const Sd3dCamera& c, int vi, int ui, float d, float& wx, float& wy, float& wz) {
    const float x = (((float)ui - c.cx) * d) / c.fx, y = (((float)vi - c.cy) * d) / c.fy;
    wx = ((c.r00 * x + c.r01 * y) + c.r02 * d) + c.t0;
    wy = ((c.r10 * x + c.r11 * y) + c.r12 * d) + c.t1;
    wz = ((c.r20 * x + c.r21 * y) + c.r22 * d) + c.t2;
}
