// Multi-view lifting of posed 2D feature maps onto scene points (the producer of `points_2dfeats`; the reference only loads them
// from a per-scene dump and ships no code that makes them, so tests/lift2d_ref.py - a float64 restatement of the rule in
// include/segdino3d_hip.h - is what these kernels are pinned against).
//
//   sd3d_lift_visibility  lift_visibility_kernel  one thread per (point, group of 32 views): project, compare, read ONE depth pixel per
//                                                 surviving view, one plain store of the group's word of the point-major bit mask;
//                         lift_count_kernel       one thread per point: popcount of its words (added to or replacing `count`);
//   sd3d_lift_accumulate  lift_accumulate_kernel  one group of 8 / 16 / 32 / 64 lanes per point and 16 bytes of a feature row per lane.
//                                                 The group loads the point's running sum, walks the set bits of views [v0, v1) in
//                                                 ascending order, adds the four weighted taps of every view with four FMAs per channel
//                                                 and stores the sum back.  It alone touches that row of `sum`, so the result is the same
//                                                 sequential fp32 sum whatever the cut of the views into launches;
//   sd3d_lift_finish      lift_finish_kernel      mean = sum / count (0 where count == 0), added over the scales, divided by their number.
// No atomics, no LDS, no cross-lane traffic: a lane's channels never meet another lane's.  Every comparison that guards an index is
// made on floats first (a NaN fails it); the tap coordinates of sd3d_lift_accumulate are clamped as floats before they become
// integers, so a mask the caller made up cannot produce an address outside the maps either.
#include "common.h"
#include "depth_pixel.h"                                // the depth conversion alone, under the default contraction
#include <hip/hip_fp16.h>
#include <stdio.h>

#define LIFT_MAX_POINTS 0x7F000000ll
#define LIFT_MAX_VIEWS (1 << 20)                        // words per point stay below the 65535 of gridDim.y

struct LiftRule {
    float near, tol_abs, tol_rel, lo, hi_x, hi_y, depth_scale;
};

struct LiftProj {
    float z, u, v;
};

// p_c = R p + t, u = fx x / z + cx, v = fy y / z + cy.  One function for both kernels: the sample position of a visible pair is
// computed from the very numbers its visibility was decided on.
__device__ __forceinline__ LiftProj lift_project(const float* __restrict__ m, const float* __restrict__ k, float px, float py, float pz) {
    const float x = m[0] * px + m[1] * py + m[2] * pz + m[3];
    const float y = m[4] * px + m[5] * py + m[6] * pz + m[7];
    LiftProj p;
    p.z = m[8] * px + m[9] * py + m[10] * pz + m[11];
    p.u = k[0] * x / p.z + k[2];
    p.v = k[1] * y / p.z + k[3];
    return p;
}

template <typename D>
__global__ __launch_bounds__(256) void lift_visibility_kernel(const float* __restrict__ points, int64_t ld, int64_t N,
                                                              const float* __restrict__ w2c, const float* __restrict__ intr,
                                                              const D* __restrict__ depth, int V, int Hd, int Wd, LiftRule r, int W,
                                                              uint32_t* __restrict__ bits) {
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int w = blockIdx.y;
    if (n >= N) return;
    const float px = points[n * ld], py = points[n * ld + 1], pz = points[n * ld + 2];
    const int vbeg = w * 32, vend = min(V, vbeg + 32);
    uint32_t word = 0;
    for (int v = vbeg; v < vend; ++v) {
        const LiftProj p = lift_project(w2c + (int64_t)v * 12, intr + (int64_t)v * 4, px, py, pz);
        if (!(p.z > r.near)) continue;
        const float uf = floorf(p.u + 0.5f), vf = floorf(p.v + 0.5f);
        if (!(uf >= r.lo && uf < r.hi_x && vf >= r.lo && vf < r.hi_y)) continue;          // NaN and huge values stop here
        const int ui = (int)uf, vi = (int)vf;                                             // 0 <= ui < Wd, 0 <= vi < Hd
        const float d = sd3d_depth_metres(depth[((int64_t)v * Hd + vi) * Wd + ui], r.depth_scale);
        if (!(d > 0.0f)) continue;
        if (fabsf(d - p.z) <= r.tol_abs + r.tol_rel * d) word |= 1u << (v - vbeg);
    }
    bits[n * W + w] = word;
}

__global__ __launch_bounds__(256) void lift_count_kernel(const uint32_t* __restrict__ bits, int64_t N, int W, int add, int32_t* count) {
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    int c = add ? count[n] : 0;
    for (int w = 0; w < W; ++w) c += __popc(bits[n * W + w]);
    count[n] = c;
}

// 16 bytes of a feature row -> fp32
__device__ __forceinline__ void lift_load(const __half* p, float (&t)[8]) {
    const uint4 q = *(const uint4*)p;
    const __half2* h = (const __half2*)&q;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float2 f = __half22float2(h[i]);
        t[2 * i] = f.x;
        t[2 * i + 1] = f.y;
    }
}
__device__ __forceinline__ void lift_load(const float* p, float (&t)[4]) {
    const float4 q = *(const float4*)p;
    t[0] = q.x; t[1] = q.y; t[2] = q.z; t[3] = q.w;
}

// the part of word `w` of a point's mask that lies in views [v0, v1)
__device__ __forceinline__ uint32_t lift_clip(uint32_t word, int w, int v0, int v1) {
    const int lo = max(v0 - w * 32, 0), hi = min(v1 - w * 32, 32);                       // 0 <= lo < hi <= 32 for the words walked
    word &= 0xFFFFFFFFu << lo;
    if (hi < 32) word &= (1u << hi) - 1u;
    return word;
}

template <typename T, int LANES>
__global__ __launch_bounds__(256) void lift_accumulate_kernel(const float* __restrict__ points, int64_t ld, int64_t N,
                                                              const float* __restrict__ w2c, const float* __restrict__ intr, float sx,
                                                              float sy, const uint32_t* __restrict__ bits, int W,
                                                              const T* __restrict__ maps, int Hf, int Wf, int C, int v0, int v1,
                                                              float* sum) {
    constexpr int VEC = 16 / (int)sizeof(T);
    const int64_t n = ((int64_t)blockIdx.x * 256 + threadIdx.x) / LANES;
    const int c0 = ((int)blockIdx.y * LANES + (int)(threadIdx.x % LANES)) * VEC;
    if (n >= N || c0 >= C) return;                                                     // C is a multiple of 64: c0 + VEC <= C
    const int w0 = v0 >> 5, w1 = (v1 - 1) >> 5;
    uint32_t any = 0;
    for (int w = w0; w <= w1; ++w) any |= lift_clip(bits[n * W + w], w, v0, v1);
    if (!any) return;                                                                    // unseen in this range: its sum row is not touched
    const float px = points[n * ld], py = points[n * ld + 1], pz = points[n * ld + 2];
    float* srow = sum + n * C + c0;
    float acc[VEC];
#pragma unroll
    for (int i = 0; i < VEC; i += 4) {
        const float4 q = *(const float4*)(srow + i);
        acc[i] = q.x; acc[i + 1] = q.y; acc[i + 2] = q.z; acc[i + 3] = q.w;
    }
    const float xmax = (float)Wf, ymax = (float)Hf;
    for (int w = w0; w <= w1; ++w) {
        uint32_t word = lift_clip(bits[n * W + w], w, v0, v1);
        while (word) {
            const int v = w * 32 + __ffs(word) - 1;
            word &= word - 1;
            const LiftProj p = lift_project(w2c + (int64_t)v * 12, intr + (int64_t)v * 4, px, py, pz);
            // align_corners = False; a visible pair lies in [-0.5, Wf - 0.5); the clamp (NaN -> -1) is for masks that are not ours
            const float xf = fminf(fmaxf((p.u + 0.5f) * sx - 0.5f, -1.0f), xmax);
            const float yf = fminf(fmaxf((p.v + 0.5f) * sy - 0.5f, -1.0f), ymax);
            const float xb = floorf(xf), yb = floorf(yf);
            const float wx = xf - xb, wy = yf - yb;
            const int xi = (int)xb, yi = (int)yb;
            const int x0 = min(max(xi, 0), Wf - 1), x1 = min(max(xi + 1, 0), Wf - 1);
            const int y0 = min(max(yi, 0), Hf - 1), y1 = min(max(yi + 1, 0), Hf - 1);
            const T* base = maps + (int64_t)v * Hf * Wf * C + c0;
            float t00[VEC], t01[VEC], t10[VEC], t11[VEC];
            lift_load(base + ((int64_t)y0 * Wf + x0) * C, t00);
            lift_load(base + ((int64_t)y0 * Wf + x1) * C, t01);
            lift_load(base + ((int64_t)y1 * Wf + x0) * C, t10);
            lift_load(base + ((int64_t)y1 * Wf + x1) * C, t11);
            const float a00 = (1.0f - wy) * (1.0f - wx), a01 = (1.0f - wy) * wx, a10 = wy * (1.0f - wx), a11 = wy * wx;
#pragma unroll
            for (int i = 0; i < VEC; ++i) acc[i] = fmaf(a11, t11[i], fmaf(a10, t10[i], fmaf(a01, t01[i], fmaf(a00, t00[i], acc[i]))));
        }
    }
#pragma unroll
    for (int i = 0; i < VEC; i += 4) *(float4*)(srow + i) = make_float4(acc[i], acc[i + 1], acc[i + 2], acc[i + 3]);
}

__device__ __forceinline__ void lift_store4(float* out, int64_t i, float4 a) { *(float4*)(out + i) = a; }
__device__ __forceinline__ void lift_store4(__half* out, int64_t i, float4 a) {
    __half2 h[2] = {__floats2half2_rn(a.x, a.y), __floats2half2_rn(a.z, a.w)};
    *(uint2*)(out + i) = *(const uint2*)h;
}

template <typename O>
__global__ __launch_bounds__(256) void lift_finish_kernel(const float* __restrict__ sum, const int32_t* __restrict__ count, int64_t quads,
                                                          int C, int scale_index, int n_scales, float* acc, O* __restrict__ out) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= quads) return;
    const int64_t i = q * 4;
    const int cnt = count[i / C];
    float4 m = make_float4(0.f, 0.f, 0.f, 0.f);
    if (cnt > 0) {
        const float4 s = *(const float4*)(sum + i);
        const float c = (float)cnt;
        m = make_float4(s.x / c, s.y / c, s.z / c, s.w / c);
    }
    if (scale_index > 0) {
        const float4 a = *(const float4*)(acc + i);
        m = make_float4(a.x + m.x, a.y + m.y, a.z + m.z, a.w + m.w);
    }
    if (scale_index < n_scales - 1) {
        *(float4*)(acc + i) = m;
    } else {
        const float k = (float)n_scales;
        lift_store4(out, i, make_float4(m.x / k, m.y / k, m.z / k, m.w / k));
    }
}

// ---------------------------------------------------------------------------------------------- C entry points
static bool lift_bad_views(int64_t N, int64_t ld, int V, int Hd, int Wd) {
    return N < 0 || N > LIFT_MAX_POINTS || ld < 3 || V < 1 || V > LIFT_MAX_VIEWS || Hd < 1 || Hd > SD3D_MAX_IMAGE_DIM || Wd < 1 || Wd > SD3D_MAX_IMAGE_DIM;
}

extern "C" int sd3d_lift_visibility(const float* points, int64_t ld, int64_t N, const float* world_to_cam, const float* intrinsics,
                                    const void* depth, int depth_u16, float depth_scale, int V, int Hd, int Wd, float near, int border,
                                    float tol_abs, float tol_rel, uint32_t* bits, int32_t* count, int add_count, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (lift_bad_views(N, ld, V, Hd, Wd) || border < 0 || !(near >= 0.0f) || !(tol_abs >= 0.0f) || !(tol_rel >= 0.0f) ||
        (depth_u16 && !(depth_scale > 0.0f)))
        return sd3d_set_error(SD3D_ERR_ARG, "lift_visibility: 0 <= N <= 0x7F000000 points (ld >= 3), 1..2^20 views, depth images up to 16384 a "
                                            "side, border >= 0, near / tol_abs / tol_rel >= 0, depth_scale > 0 for uint16 depth");
    if (!world_to_cam || !intrinsics || !depth || (N > 0 && (!points || !bits || !count)))
        return sd3d_set_error(SD3D_ERR_ARG, "lift_visibility: NULL argument");
    if (N == 0) return SD3D_OK;
    const int W = (V + 31) / 32;
    LiftRule r;
    r.near = near; r.tol_abs = tol_abs; r.tol_rel = tol_rel;
    r.lo = (float)border; r.hi_x = (float)(Wd - border); r.hi_y = (float)(Hd - border);
    r.depth_scale = depth_u16 ? depth_scale : 1.0f;
    const dim3 grid((unsigned)cdiv(N, 256), (unsigned)W);
    if (depth_u16)
        hipLaunchKernelGGL(lift_visibility_kernel<uint16_t>, grid, dim3(256), 0, st, points, ld, N, world_to_cam, intrinsics,
                           (const uint16_t*)depth, V, Hd, Wd, r, W, bits);
    else
        hipLaunchKernelGGL(lift_visibility_kernel<float>, grid, dim3(256), 0, st, points, ld, N, world_to_cam, intrinsics, (const float*)depth,
                           V, Hd, Wd, r, W, bits);
    hipLaunchKernelGGL(lift_count_kernel, dim3((unsigned)cdiv(N, 256)), dim3(256), 0, st, bits, N, W, add_count ? 1 : 0, count);
    SD3D_CHECK_LAUNCH();
    return SD3D_OK;
}

template <typename T>
static void lift_launch_accumulate(hipStream_t st, const float* points, int64_t ld, int64_t N, const float* w2c, const float* intr, float sx,
                                   float sy, const uint32_t* bits, int W, const void* maps, int Hf, int Wf, int C, int v0, int v1,
                                   float* sum) {
    const int need = C / (16 / (int)sizeof(T));                                          // lanes that cover one row
#define LIFT_GO(L)                                                                                                                   \
    hipLaunchKernelGGL((lift_accumulate_kernel<T, L>), dim3((unsigned)cdiv(N * L, 256), (unsigned)cdiv(need, L)), dim3(256), 0, st, \
                       points, ld, N, w2c, intr, sx, sy, bits, W, (const T*)maps, Hf, Wf, C, v0, v1, sum)
    if (need <= 8) LIFT_GO(8);
    else if (need <= 16) LIFT_GO(16);
    else if (need <= 32) LIFT_GO(32);
    else LIFT_GO(64);
#undef LIFT_GO
}

extern "C" int sd3d_lift_accumulate(const float* points, int64_t ld, int64_t N, const float* world_to_cam, const float* intrinsics, int V,
                                    int Hd, int Wd, const uint32_t* bits, const void* maps, int maps_f16, int Hf, int Wf, int C, int v0,
                                    int v1, float* sum, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (lift_bad_views(N, ld, V, Hd, Wd) || Hf < 1 || Hf > SD3D_MAX_IMAGE_DIM || Wf < 1 || Wf > SD3D_MAX_IMAGE_DIM || v0 < 0 || v1 > V || v0 > v1)
        return sd3d_set_error(SD3D_ERR_ARG, "lift_accumulate: 0 <= N <= 0x7F000000 points (ld >= 3), 1..2^20 views, images and maps up to "
                                            "16384 a side, 0 <= v0 <= v1 <= V");
    if (C < 64 || C > 1024 || C % 64 != 0) return sd3d_set_error(SD3D_ERR_ARG, "lift_accumulate: C must be a multiple of 64 up to 1024");
    if (!world_to_cam || !intrinsics || !maps || (N > 0 && (!points || !bits || !sum)))
        return sd3d_set_error(SD3D_ERR_ARG, "lift_accumulate: NULL argument");
    if (((uintptr_t)maps | (uintptr_t)sum) & 15) return sd3d_set_error(SD3D_ERR_ARG, "lift_accumulate: maps and sum must be 16-byte aligned");
    if (N == 0 || v0 == v1) return SD3D_OK;
    const int W = (V + 31) / 32;
    const float sx = (float)Wf / (float)Wd, sy = (float)Hf / (float)Hd;
    if (maps_f16)
        lift_launch_accumulate<__half>(st, points, ld, N, world_to_cam, intrinsics, sx, sy, bits, W, maps, Hf, Wf, C, v0, v1, sum);
    else
        lift_launch_accumulate<float>(st, points, ld, N, world_to_cam, intrinsics, sx, sy, bits, W, maps, Hf, Wf, C, v0, v1, sum);
    SD3D_CHECK_LAUNCH();
    return SD3D_OK;
}

extern "C" int sd3d_lift_finish(const float* sum, const int32_t* count, int64_t N, int C, int scale_index, int n_scales, float* acc,
                                void* out, int out_f16, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (N < 0 || N > LIFT_MAX_POINTS || C < 64 || C > 1024 || C % 64 != 0 || n_scales < 1 || scale_index < 0 || scale_index >= n_scales)
        return sd3d_set_error(SD3D_ERR_ARG, "lift_finish: 0 <= N <= 0x7F000000, C a multiple of 64 up to 1024, 0 <= scale_index < n_scales");
    const bool last = scale_index == n_scales - 1;
    if (N > 0 && (!sum || !count || (n_scales > 1 && !acc) || (last && !out))) return sd3d_set_error(SD3D_ERR_ARG, "lift_finish: NULL argument");
    if (((uintptr_t)sum | (uintptr_t)acc | (uintptr_t)out) & 15)
        return sd3d_set_error(SD3D_ERR_ARG, "lift_finish: sum, acc and out must be 16-byte aligned");
    if (N == 0) return SD3D_OK;
    const int64_t quads = N * C / 4;
    const dim3 grid((unsigned)cdiv(quads, 256));
    if (out_f16)
        hipLaunchKernelGGL(lift_finish_kernel<__half>, grid, dim3(256), 0, st, sum, count, quads, C, scale_index, n_scales, acc, (__half*)out);
    else
        hipLaunchKernelGGL(lift_finish_kernel<float>, grid, dim3(256), 0, st, sum, count, quads, C, scale_index, n_scales, acc, (float*)out);
    SD3D_CHECK_LAUNCH();
    return SD3D_OK;
}
