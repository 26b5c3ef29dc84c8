// The front end every stage that starts from a posed depth pixel shares - fuse_views.hip, tsdf.hip, track.hip, transfer.hip and, for
// the depth conversion alone, lift_queries.hip and lift2d.hip: one definition, so that the stages cannot drift apart.  What follows a
// valid pixel is backproject.h, included here.
//
// The rule of a depth pixel (vi, ui), restated in numpy as depth_metres / valid_pixels of tests/fuse_views_ref.py; every decision is a
// single rounded fp32 operation:
//   step 2. d = (float)raw * depth_scale, one rounded multiply (fp32 depth as it is); valid iff d > 0, d >= near and d <= far; a NaN
//           fails;
//   step 3. unless edges are off: each of the 4 neighbours (vi +- 1, ui), (vi, ui +- 1) inside the image, whatever the stride, with
//           depth dn by step 2, is a jump iff !(dn > 0) or |dn - d| > edge_abs + edge_rel * d (one rounded multiply, one rounded add,
//           one rounded subtract); a pixel with any jump is dropped.
// The edge test reads its neighbours from global memory: a row of a tile is 64 contiguous bytes and the rows above and below are the
// neighbouring lanes' own pixels, so they come from the L1; nothing of the halo is staged in LDS.
//
// Contraction is the including file's choice, as in backproject.h: the operators below take the `#pragma clang fp contract` state of
// the includer.  The four includers of sd3d_depth_pixel, sd3d_world_cell and sd3d_lds_claim (fuse_views.hip, tsdf.hip, track.hip,
// transfer.hip) compile under `contract(off)`, where `edge_abs + edge_rel * d` is two roundings; lift_queries.hip and lift2d.hip take
// only sd3d_depth_metres, under the default, as they always were compiled (a lone multiply has nothing to contract with here).
#pragma once
#include "common.h"
#include "backproject.h"
#include "../../include/segdino3d_hip.h"
#include <stdio.h>

#define SD3D_MAX_IMAGE_DIM 16384                        // image extents and strides; (2 v + 1) * H stays below 2^30

// What steps 2 and 3 read: the extents of one depth image and the thresholds.  The *Geom struct of each stage embeds it.
// Step 2's members first: a kernel without step 3 (transfer.hip) then reads one contiguous run of its arguments.
struct Sd3dDepthRule {
    int Hd, Wd;
    float depth_scale, near, far;
    int use_edges;
    float edge_abs, edge_rel;
};

__device__ __forceinline__ float sd3d_depth_metres(uint16_t raw, float scale) { return (float)raw * scale; }
__device__ __forceinline__ float sd3d_depth_metres(float d, float) { return d; }

// Steps 2 and 3 for pixel (vi, ui), inside the image, of the view whose image starts at `img`: d, and whether the pixel is valid.
// EDGES = false: a stage that has no step 3 (its rule's use_edges is 0) compiles without the branch.
template <bool EDGES = true, typename D>
__device__ __forceinline__ bool sd3d_depth_pixel(const D* __restrict__ img, const Sd3dDepthRule& r, int vi, int ui, float& d) {
    const D* row = img + (int64_t)vi * r.Wd;
    d = sd3d_depth_metres(row[ui], r.depth_scale);
    bool ok = d > 0.0f && d >= r.near && d <= r.far;                                  // a NaN fails
    if (EDGES && ok && r.use_edges) {
        const float thr = r.edge_abs + r.edge_rel * d;
        const auto jump = [&](int at) {
            const float dn = sd3d_depth_metres(row[at], r.depth_scale);
            return !(dn > 0.0f) || fabsf(dn - d) > thr;
        };
        if (vi > 0) ok = ok && !jump(ui - r.Wd);
        if (vi + 1 < r.Hd) ok = ok && !jump(ui + r.Wd);
        if (ui > 0) ok = ok && !jump(ui - 1);
        if (ui + 1 < r.Wd) ok = ok && !jump(ui + 1);
    }
    return ok;
}

// The world range and the cell of a back-projected point (steps 4 and 5 of the fusion rule, step 2 of the TSDF rule): all |w_i| <
// 2^SD3D_FUSE_WORLD_BITS, which stops a NaN and the infinities, then c_i = floorf(w_i * inv_voxel), one rounded multiply, with
// -cells <= c_i < cells on all axes, compared as floats before anything becomes an integer.
__device__ __forceinline__ bool sd3d_world_cell(const float (&w)[3], float inv_voxel, float cells, float (&c)[3]) {
    const float lim = (float)(1 << SD3D_FUSE_WORLD_BITS);
    bool ok = fabsf(w[0]) < lim && fabsf(w[1]) < lim && fabsf(w[2]) < lim;
    c[0] = c[1] = c[2] = 0.0f;
    if (ok) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            c[i] = floorf(w[i] * inv_voxel);
            ok = ok && c[i] >= -cells && c[i] < cells;
        }
    }
    return ok;
}

// Puts `key` into the open-addressing set s_key[SLOTS] of a workgroup (LDS, SD3D_EMPTY_KEY = free) and returns its slot; `fresh` iff
// this call claimed the slot.  The probe starts at the top log2(SLOTS) bits of the hash - the global tables take the low ones - and
// ends only on a free slot or the key itself: the caller must keep the distinct keys of a workgroup below SLOTS.
template <int SLOTS>
__device__ __forceinline__ int sd3d_lds_claim(unsigned long long* s_key, unsigned long long key, bool& fresh) {
    static_assert(SLOTS >= 2 && (SLOTS & (SLOTS - 1)) == 0, "a power of two");
    int slot = (int)(hash_u64(key) >> (32 - __builtin_ctz(SLOTS)));
    for (;;) {
        const unsigned long long prev = atomicCAS(&s_key[slot], (unsigned long long)SD3D_EMPTY_KEY, key);
        fresh = prev == SD3D_EMPTY_KEY;
        if (fresh || prev == key) return slot;
        slot = (slot + 1) & (SLOTS - 1);
    }
}

// ---------------------------------------------------------------------------------------------- host side
// The argument checks the entry points of the four stages share, and the fill of the rule (fp32 depth ignores depth_scale).
static inline int sd3d_depth_rule(const char* who, int depth_u16, float depth_scale, int Hd, int Wd, float near, float far, float edge_abs,
                                  float edge_rel, int use_edges, Sd3dDepthRule& out) {
    if (Hd < 1 || Hd > SD3D_MAX_IMAGE_DIM || Wd < 1 || Wd > SD3D_MAX_IMAGE_DIM || (depth_u16 && !(depth_scale > 0.0f)) || !(near >= 0.0f) ||
        !(far >= near) || (use_edges && (!(edge_abs >= 0.0f) || !(edge_rel >= 0.0f)))) {
        char msg[192];                                  // sd3d_set_error copies it
        snprintf(msg, sizeof msg, "%s: images up to 16384 a side, depth_scale > 0 for uint16 depth, 0 <= near <= far, edge_abs, edge_rel >= 0",
                 who);
        return sd3d_set_error(SD3D_ERR_ARG, msg);
    }
    out.Hd = Hd; out.Wd = Wd; out.use_edges = use_edges ? 1 : 0;
    out.depth_scale = depth_u16 ? depth_scale : 1.0f;
    out.near = near; out.far = far; out.edge_abs = edge_abs; out.edge_rel = edge_rel;
    return SD3D_OK;
}

// Launches kernel<uint16_t> or kernel<float>, whose first argument is the depth image.
#define SD3D_LAUNCH_DEPTH(kernel, grid, block, st, depth_u16, depth, ...)                                                     \
    do {                                                                                                                      \
        if (depth_u16) hipLaunchKernelGGL(kernel<uint16_t>, grid, block, 0, st, (const uint16_t*)(depth), __VA_ARGS__);       \
        else hipLaunchKernelGGL(kernel<float>, grid, block, 0, st, (const float*)(depth), __VA_ARGS__);                       \
    } while (0)
