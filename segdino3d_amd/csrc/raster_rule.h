// The arithmetic of the triangle rasteriser (the rule: include/segdino3d_hip.h, "Mesh rasteriser"; segdino3d_amd/raster.py has it in
// full), in ONE place: setup, both draw kernels and resolve of raster.hip call these functions and nothing else touches a coordinate,
// so the four cannot drift.  tests/raster_ref.py restates them in numpy and the kernels EQUAL it, bit for bit.
//
// The including file must have `#pragma clang fp contract(off)` in force: every fp32 and fp64 operation below is rounded on its own.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define RASTER_SUB 256                                  // sub-pixel steps per pixel: eight bits
#define RASTER_SUB_BITS 8
#define RASTER_LIMIT 16384.0f                           // |coordinate| and |u|, |v| must stay below 2^14

// the class of a (view, face) pair, in the order of the info vector; the precedence is BAD, NEAR, GUARD, EMPTY, DRAWN
enum { RASTER_DRAWN = 0, RASTER_NEAR = 1, RASTER_GUARD = 2, RASTER_EMPTY = 3, RASTER_BAD = 4 };

struct RasterView {
    float r[12];                                        // world_to_cam [3, 4], row-major
    float fx, fy, cx, cy;
};
struct RasterTri {
    int32_t idx[3];                                     // the face's vertex indices
    int32_t X[3], Y[3];                                 // snapped corners, |X|, |Y| <= 2^22
    double q[3];                                        // 1 / z_c per corner
    int64_t A;                                          // E(v0, v1, v2), signed
    int x0, x1, y0, y1;                                 // the bounding box clamped to the image, inclusive
};

__device__ __forceinline__ RasterView raster_view(const float* __restrict__ world_to_cam, const float* __restrict__ intrinsics, int64_t v) {
    RasterView c;
#pragma unroll
    for (int i = 0; i < 12; ++i) c.r[i] = world_to_cam[v * 12 + i];
    c.fx = intrinsics[v * 4 + 0]; c.fy = intrinsics[v * 4 + 1]; c.cx = intrinsics[v * 4 + 2]; c.cy = intrinsics[v * 4 + 3];
    return c;
}

// E(a, b, p): the differences fit 24 bits, so each product is one 32 x 32 -> 64 multiply
__device__ __forceinline__ int64_t raster_edge(int32_t ax, int32_t ay, int32_t bx, int32_t by, int32_t px, int32_t py) {
    return (int64_t)(bx - ax) * (int64_t)(py - ay) - (int64_t)(by - ay) * (int64_t)(px - ax);
}

// Steps 1 to 4 up to the bounding box: the class of face `f` in view `c`; `t` is complete iff the class is RASTER_DRAWN.
__device__ __forceinline__ int raster_setup(const float* __restrict__ vertices, int64_t Nv, const int32_t* __restrict__ faces, int64_t f,
                                            const RasterView& c, float near, int H, int W, RasterTri& t) {
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        t.idx[i] = faces[f * 3 + i];
        ok = ok && t.idx[i] >= 0 && (int64_t)t.idx[i] < Nv;
    }
    if (!ok) return RASTER_BAD;
    float p[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            p[i][a] = vertices[(int64_t)t.idx[i] * 3 + a];
            ok = ok && fabsf(p[i][a]) < RASTER_LIMIT;   // a NaN or an infinity fails
        }
    if (!ok) return RASTER_BAD;
    float xc[3], yc[3], zc[3];
    bool behind = false;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        xc[i] = ((c.r[0] * p[i][0] + c.r[1] * p[i][1]) + c.r[2] * p[i][2]) + c.r[3];
        yc[i] = ((c.r[4] * p[i][0] + c.r[5] * p[i][1]) + c.r[6] * p[i][2]) + c.r[7];
        zc[i] = ((c.r[8] * p[i][0] + c.r[9] * p[i][1]) + c.r[10] * p[i][2]) + c.r[11];
        behind = behind || zc[i] < near;
    }
    if (behind) return RASTER_NEAR;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float u = (c.fx * xc[i]) / zc[i] + c.cx, v = (c.fy * yc[i]) / zc[i] + c.cy;
        ok = ok && fabsf(u) < RASTER_LIMIT && fabsf(v) < RASTER_LIMIT;      // floats, before anything becomes an integer
        if (ok) {
            t.X[i] = (int32_t)rintf(u * (float)RASTER_SUB);
            t.Y[i] = (int32_t)rintf(v * (float)RASTER_SUB);
        }
        t.q[i] = 1.0 / (double)zc[i];
    }
    if (!ok) return RASTER_GUARD;
    t.A = raster_edge(t.X[0], t.Y[0], t.X[1], t.Y[1], t.X[2], t.Y[2]);
    const int32_t xlo = min(t.X[0], min(t.X[1], t.X[2])), xhi = max(t.X[0], max(t.X[1], t.X[2]));
    const int32_t ylo = min(t.Y[0], min(t.Y[1], t.Y[2])), yhi = max(t.Y[0], max(t.Y[1], t.Y[2]));
    // pixel centres lie at multiples of RASTER_SUB: the first at or after the low corner, the last at or before the high one
    t.x0 = max((xlo + (RASTER_SUB - 1)) >> RASTER_SUB_BITS, 0); t.x1 = min(xhi >> RASTER_SUB_BITS, W - 1);
    t.y0 = max((ylo + (RASTER_SUB - 1)) >> RASTER_SUB_BITS, 0); t.y1 = min(yhi >> RASTER_SUB_BITS, H - 1);
    if (t.A == 0 || t.x0 > t.x1 || t.y0 > t.y1) return RASTER_EMPTY;
    return RASTER_DRAWN;
}

// The clamped bounding-box area of a drawn face: what splits the records into the small and the large class.
__device__ __forceinline__ int64_t raster_box_pixels(const RasterTri& t) { return (int64_t)(t.x1 - t.x0 + 1) * (int64_t)(t.y1 - t.y0 + 1); }

// Step 4 at pixel (vi, ui): the three weights, w0 + w1 + w2 == |A|; covered iff none is negative (edges inclusive, both windings).
__device__ __forceinline__ bool raster_weights(const RasterTri& t, int ui, int vi, int64_t w[3]) {
    const int32_t px = ui << RASTER_SUB_BITS, py = vi << RASTER_SUB_BITS;
    const int64_t e0 = raster_edge(t.X[1], t.Y[1], t.X[2], t.Y[2], px, py), e1 = raster_edge(t.X[2], t.Y[2], t.X[0], t.Y[0], px, py),
                  e2 = raster_edge(t.X[0], t.Y[0], t.X[1], t.Y[1], px, py);
    const bool neg = t.A < 0;
    w[0] = neg ? -e0 : e0; w[1] = neg ? -e1 : e1; w[2] = neg ? -e2 : e2;
    return (w[0] | w[1] | w[2]) >= 0;
}

// Step 5: perspective-correct depth in float64, one rounding per operation, rounded once to fp32.
__device__ __forceinline__ float raster_depth(const RasterTri& t, const int64_t w[3]) {
    const double num = ((double)w[0] * t.q[0] + (double)w[1] * t.q[1]) + (double)w[2] * t.q[2];
    const double area = (double)(t.A < 0 ? -t.A : t.A);
    return (float)(area / num);
}

// Steps 4 to 6 at one pixel: the key of the sample, or false when the pixel is not covered or the depth is out of range.
__device__ __forceinline__ bool raster_sample(const RasterTri& t, int ui, int vi, float near, float far, uint32_t face, uint64_t& key) {
    int64_t w[3];
    if (!raster_weights(t, ui, vi, w)) return false;
    const float d = raster_depth(t, w);
    if (!(d >= near && d <= far)) return false;
    key = ((uint64_t)__float_as_uint(d) << 32) | (uint64_t)face;
    return true;
}

// Step 7: the corner with the largest weight, ties to the lowest corner.
__device__ __forceinline__ int raster_corner(const int64_t w[3]) {
    int best = 0;
    if (w[1] > w[best]) best = 1;
    if (w[2] > w[best]) best = 2;
    return best;
}
