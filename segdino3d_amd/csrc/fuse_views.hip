// Fusion of posed RGB-D frames into the scene's point cloud (the producer of `points [N, 6]`, the input every other stage starts
// from; the reference reads it from a file made offline from a mesh and ships no code that makes it, so tests/fuse_views_ref.py - a
// numpy restatement of the rule in include/segdino3d_hip.h - is what these kernels are pinned against, bit for bit).
//
// The rule, per depth pixel (vi, ui) of view v; every decision is an integer one or a single rounded fp32 operation:
//   1. the pixel takes part iff vi % stride == 0 and ui % stride == 0; it reads colour pixel ((2 vi + 1) Hc) / (2 Hd),
//      ((2 ui + 1) Wc) / (2 Wd) (integer divisions);
//   2, 3. the depth d of the pixel, its validity and the edge test: depth_pixel.h, which states both steps;
//   4. w = the back-projection of backproject.h (step 5 of lift_queries); unless all three components are finite with
//      |w| < 2^SD3D_FUSE_WORLD_BITS the pixel is dropped and counted in out_of_range;
//   5. c_i = floorf(w_i * inv_voxel), one rounded multiply; unless -2^SD3D_FUSE_CELL_BITS <= c_i < 2^SD3D_FUSE_CELL_BITS on all
//      axes, compared as floats, the pixel is dropped and counted in out_of_range; key = ((c_x + 2^20) << 42) | ((c_y + 2^20) << 21)
//      | (c_z + 2^20);
//   6. per cell, integers only: n += 1, S_i += (int64)rint((double)w_i * 2^SD3D_FUSE_FIXED_BITS), C_j += colour byte j;
//   7. the cells with n >= min_obs in ascending key order: xyz_i = (float)((double)S_i / (double)n / 2^20), rgb_j =
//      (float)((double)C_j / (double)n), obs = n.
//
// The state between calls is an open-addressing table of `capacity` slots of SD3D_FUSE_SLOT_WORDS 64-bit words, 64 bytes = one
// memory segment: {key (SD3D_EMPTY_KEY = free), S_x, S_y, S_z, n, C_r, C_g, C_b}.  All sums are 64-bit integers: 2^28 observations of
// |w| < 2^14 at 20 fraction bits stay below 2^62.
//
//   sd3d_fuse_reset       fv_reset_kernel       16 bytes per lane.
//   sd3d_fuse_accumulate  fv_accumulate_kernel  one workgroup of 256 lanes takes a tile of FV_TILE_H x FV_TILE_W participating pixels of
//                                               one view, one pixel per lane.  Tens of neighbouring pixels share a cell, so the tile
//                                               is combined on chip first: an LDS table of FV_LDS_SLOTS slots (keys claimed by a
//                                               64-bit LDS compare-and-swap, sums by LDS integer adds), whose claimed slots are listed
//                                               as they are claimed.  Then eight lanes take one distinct cell of the tile: lane 0 of
//                                               the eight claims the key in the global table (atomicCAS, linear probing, at most
//                                               SD3D_FUSE_PROBE_LIMIT slots), lanes 1 to 7 add one word each, so that a wave's atomic
//                                               instruction covers eight slots of 56 contiguous bytes.  A cell that finds no slot is
//                                               dropped and its pixels counted in `overflow`.  No float atomics: integer adds have the
//                                               same bits in any order, so the table is a function of the SET of observations.
//   sd3d_fuse_emit        fv_emit_keys_kernel   slot -> its key if n >= min_obs, SD3D_EMPTY_KEY otherwise; counts N and the cells;
//                         sort_pairs_u64        all `capacity` keys (the count is only known on the device), the empty ones last;
//                         fv_emit_write_kernel  sorted position j < N -> points, obs, keys; lane 0 copies the counters.
#include "common.h"
// The kernels here must EQUAL a float32 evaluation of the restatement, so nothing in this file may be contracted into a fused
// multiply-add: hipcc contracts by default, and HIP's __fmul_rn / __fadd_rn / __fsub_rn are the plain operators, which it contracts
// too.  The pragma covers depth_pixel.h and backproject.h as they are compiled here and every expression below.
#pragma clang fp contract(off)
#include "depth_pixel.h"

#define FV_THREADS 256
#define FV_TILE_W 32
#define FV_TILE_H 8
#define FV_LDS_SLOTS 512                                // twice the pixels of a tile: the LDS probe always ends
#define FV_W SD3D_FUSE_SLOT_WORDS
typedef unsigned long long fv_u64;

struct FvGeom {
    Sd3dDepthRule px;
    int Hc, Wc, stride, Hs, Ws, tiles_x, tiles_per_view;
    float inv_voxel;
    uint32_t mask;                                      // capacity - 1
};
// the counters at the head of the workspace, 64-bit each
enum { FV_N = 0, FV_CELLS = 1, FV_USED = 2, FV_RANGE = 3, FV_OVERFLOW = 4, FV_COUNTERS = 5 };

template <typename D>
__global__ __launch_bounds__(FV_THREADS) void fv_accumulate_kernel(const D* __restrict__ depth, const float* __restrict__ intr,
                                                                   const float* __restrict__ c2w, const uint8_t* __restrict__ colors,
                                                                   FvGeom g, fv_u64* __restrict__ table, fv_u64* __restrict__ counters) {
    __shared__ fv_u64 s_key[FV_LDS_SLOTS];
    __shared__ fv_u64 s_sum[FV_LDS_SLOTS][3];
    __shared__ uint32_t s_cnt[FV_LDS_SLOTS][4];         // n, C_r, C_g, C_b: a tile has 256 pixels, 32 bits hold them
    __shared__ int s_list[FV_THREADS], s_ncells;
    const int t = threadIdx.x, lane = t & 63;
    const int v = blockIdx.x / g.tiles_per_view, tile = blockIdx.x - v * g.tiles_per_view;
    const int ty = tile / g.tiles_x, tx = tile - ty * g.tiles_x;

    for (int i = t; i < FV_LDS_SLOTS; i += FV_THREADS) {
        s_key[i] = SD3D_EMPTY_KEY;
        s_sum[i][0] = s_sum[i][1] = s_sum[i][2] = 0;
        s_cnt[i][0] = s_cnt[i][1] = s_cnt[i][2] = s_cnt[i][3] = 0;
    }
    if (t == 0) s_ncells = 0;
    __syncthreads();

    // ---- steps 1 to 6 for this lane's pixel, into the tile's table
    const int vs = ty * FV_TILE_H + (t >> 5), us = tx * FV_TILE_W + (t & 31);
    int dropped = 0;
    if (vs < g.Hs && us < g.Ws) {
        const int vi = vs * g.stride, ui = us * g.stride;                             // < Hd, < Wd: Hs = ceil(Hd / stride)
        float d;
        if (sd3d_depth_pixel(depth + (int64_t)v * g.px.Hd * g.px.Wd, g.px, vi, ui, d)) {
            const Sd3dCamera cam = sd3d_load_camera(intr, c2w, v);
            float w[3], c[3];
            sd3d_backproject(cam, vi, ui, d, w[0], w[1], w[2]);
            if (!sd3d_world_cell(w, g.inv_voxel, (float)(1 << SD3D_FUSE_CELL_BITS), c)) {
                dropped = 1;
            } else {
                const fv_u64 off = 1ull << SD3D_FUSE_CELL_BITS;
                const fv_u64 key = ((fv_u64)((long long)c[0] + (long long)off) << 42) | ((fv_u64)((long long)c[1] + (long long)off) << 21) |
                                   (fv_u64)((long long)c[2] + (long long)off);
                const int yc = (int)(((uint32_t)(2 * vi + 1) * (uint32_t)g.Hc) / (uint32_t)(2 * g.px.Hd));       // < Hc
                const int xc = (int)(((uint32_t)(2 * ui + 1) * (uint32_t)g.Wc) / (uint32_t)(2 * g.px.Wd));       // < Wc
                const uint8_t* px = colors + (((int64_t)v * g.Hc + yc) * g.Wc + xc) * 3;
                const uint32_t cr = px[0], cg = px[1], cb = px[2];
                bool fresh;
                const int slot = sd3d_lds_claim<FV_LDS_SLOTS>(s_key, key, fresh);       // at most 256 keys in 512 slots: it ends
                if (fresh) s_list[atomicAdd(&s_ncells, 1)] = slot;
                const double fixed = (double)(1 << SD3D_FUSE_FIXED_BITS);
#pragma unroll
                for (int i = 0; i < 3; ++i) atomicAdd(&s_sum[slot][i], (fv_u64)(long long)rint((double)w[i] * fixed));
                atomicAdd(&s_cnt[slot][0], 1u);
                atomicAdd(&s_cnt[slot][1], cr);
                atomicAdd(&s_cnt[slot][2], cg);
                atomicAdd(&s_cnt[slot][3], cb);
            }
        }
    }
    __syncthreads();

    // ---- one set of global updates per distinct cell of the tile, eight lanes per cell
    const int ncells = s_ncells, sub = t & 7;
    int used = 0, lost = 0;
    for (int base = 0; base < ncells; base += FV_THREADS / 8) {                       // uniform over the workgroup
        const int cidx = base + (t >> 3);
        const bool active = cidx < ncells;
        const int ls = active ? s_list[cidx] : 0;
        int gslot = -1;
        if (active && sub == 0) {
            const fv_u64 key = s_key[ls];
            uint32_t slot = hash_u64(key) & g.mask;
            for (int probe = 0; probe < SD3D_FUSE_PROBE_LIMIT; ++probe) {
                const fv_u64 prev = atomicCAS(&table[(size_t)slot * FV_W], (fv_u64)SD3D_EMPTY_KEY, key);
                if (prev == SD3D_EMPTY_KEY || prev == key) { gslot = (int)slot; break; }
                slot = (slot + 1) & g.mask;
            }
            if (gslot >= 0) used += (int)s_cnt[ls][0]; else lost += (int)s_cnt[ls][0];
        }
        gslot = __shfl(gslot, lane & ~7);
        if (active && gslot >= 0 && sub > 0) {                                        // 0 <= gslot <= mask: inside the table
            const fv_u64 val = sub < 4 ? s_sum[ls][sub - 1] : (fv_u64)s_cnt[ls][sub - 4];
            atomicAdd(&table[(size_t)gslot * FV_W + sub], val);
        }
    }
    used = wave_sum(used); lost = wave_sum(lost); dropped = wave_sum(dropped);
    if (lane == 0) {
        if (used) atomicAdd(&counters[FV_USED], (fv_u64)used);
        if (lost) atomicAdd(&counters[FV_OVERFLOW], (fv_u64)lost);
        if (dropped) atomicAdd(&counters[FV_RANGE], (fv_u64)dropped);
    }
}

// word 0 of every slot = SD3D_EMPTY_KEY, the rest 0; two words per lane
__global__ __launch_bounds__(256) void fv_reset_kernel(fv_u64* __restrict__ table, int64_t pairs) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= pairs) return;
    ((ulonglong2*)table)[i] = make_ulonglong2((i & (FV_W / 2 - 1)) == 0 ? SD3D_EMPTY_KEY : 0ull, 0ull);
}

__global__ __launch_bounds__(256) void fv_emit_keys_kernel(const fv_u64* __restrict__ table, int64_t capacity, fv_u64 min_obs,
                                                           uint64_t* __restrict__ keys, fv_u64* __restrict__ counters) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool occupied = false, pass = false;
    if (i < capacity) {
        const fv_u64 key = table[i * FV_W];
        occupied = key != SD3D_EMPTY_KEY;
        pass = occupied && table[i * FV_W + 4] >= min_obs;
        keys[i] = pass ? key : SD3D_EMPTY_KEY;
    }
    const int n_occ = wave_sum(occupied ? 1 : 0), n_pass = wave_sum(pass ? 1 : 0);
    if ((threadIdx.x & 63) == 0) {
        if (n_occ) atomicAdd(&counters[FV_CELLS], (fv_u64)n_occ);
        if (n_pass) atomicAdd(&counters[FV_N], (fv_u64)n_pass);
    }
}

__global__ __launch_bounds__(256) void fv_emit_write_kernel(const fv_u64* __restrict__ table, const uint64_t* __restrict__ skeys,
                                                            const uint32_t* __restrict__ sslot, int64_t capacity, int64_t out_cap,
                                                            float* __restrict__ points, int32_t* __restrict__ obs, int64_t* __restrict__ keys_out,
                                                            const fv_u64* __restrict__ counters, int64_t* __restrict__ info) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j == 0)
        for (int i = 0; i < FV_COUNTERS; ++i) info[i] = (int64_t)counters[i];
    if (j >= capacity || j >= out_cap) return;
    const uint64_t key = skeys[j];
    if (key == SD3D_EMPTY_KEY) return;                                                // the passing cells come first
    const int64_t slot = sslot[j];
    if (slot >= capacity) return;                                                     // never from the sort: a permutation of the slots
    const fv_u64* s = table + slot * FV_W;
    const double n = (double)s[4], fixed = (double)(1 << SD3D_FUSE_FIXED_BITS);
    float* p = points + j * 6;
#pragma unroll
    for (int i = 0; i < 3; ++i) p[i] = (float)((double)(long long)s[1 + i] / n / fixed);
#pragma unroll
    for (int i = 0; i < 3; ++i) p[3 + i] = (float)((double)s[5 + i] / n);
    obs[j] = (int32_t)(s[4] > 0x7FFFFFFFull ? 0x7FFFFFFFull : s[4]);
    if (keys_out) keys_out[j] = (int64_t)key;
}

// ---------------------------------------------------------------------------------------------- C entry points
// counters (256 bytes) | table [capacity][FV_W] | keys a, b uint64 [capacity] | slots a, b uint32 [capacity] | sort scratch
struct FvWs {
    fv_u64 *counters, *table;
    uint64_t *keys_a, *keys_b;
    uint32_t *vals_a, *vals_b;
    void* sort_ws;
    size_t sort_bytes, total;
};
static FvWs fv_ws(void* ws, int64_t capacity) {
    FvWs w;
    char* p = (char*)ws;
    size_t o = 0;
    const size_t m = (size_t)capacity;
    auto take = [&](size_t bytes) { char* q = p + o; o += align_up(bytes, 256); return (void*)q; };
    w.counters = (fv_u64*)take(FV_COUNTERS * 8);
    w.table = (fv_u64*)take(m * FV_W * 8);
    w.keys_a = (uint64_t*)take(m * 8); w.keys_b = (uint64_t*)take(m * 8);
    w.vals_a = (uint32_t*)take(m * 4); w.vals_b = (uint32_t*)take(m * 4);
    w.sort_bytes = sort_ws_bytes((int64_t)m); w.sort_ws = take(w.sort_bytes);
    w.total = o;
    return w;
}
static bool fv_capacity_ok(int64_t c) { return c >= SD3D_FUSE_MIN_CAPACITY && c <= SD3D_FUSE_MAX_CAPACITY && (c & (c - 1)) == 0; }
static int fv_check_ws(const char* who, void* ws, size_t ws_bytes, int64_t capacity, FvWs& w) {
    char msg[160];                                      // sd3d_set_error copies it
    if (!fv_capacity_ok(capacity)) {
        snprintf(msg, sizeof msg, "%s: capacity must be a power of two in [2^4, 2^24]", who);
        return sd3d_set_error(SD3D_ERR_ARG, msg);
    }
    if (!ws || ((uintptr_t)ws & 255) != 0) {
        snprintf(msg, sizeof msg, "%s: ws is required and must be 256-byte aligned", who);
        return sd3d_set_error(SD3D_ERR_ARG, msg);
    }
    w = fv_ws(ws, capacity);
    if (ws_bytes < w.total) {
        snprintf(msg, sizeof msg, "%s: workspace too small (sd3d_fuse_ws_bytes)", who);
        return sd3d_set_error(SD3D_ERR_WS, msg);
    }
    return SD3D_OK;
}

extern "C" size_t sd3d_fuse_ws_bytes(int64_t capacity) { return fv_capacity_ok(capacity) ? fv_ws(nullptr, capacity).total : 0; }

extern "C" int sd3d_fuse_reset(void* ws, size_t ws_bytes, int64_t capacity, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    FvWs w;
    if (int rc = fv_check_ws("fuse_reset", ws, ws_bytes, capacity, w)) return rc;
    if (hipMemsetAsync(w.counters, 0, FV_COUNTERS * 8, st) != hipSuccess) return sd3d_set_error(SD3D_ERR_LAUNCH, "fuse_reset: memset");
    const int64_t pairs = capacity * (FV_W / 2);
    hipLaunchKernelGGL(fv_reset_kernel, dim3((unsigned)cdiv(pairs, 256)), dim3(256), 0, st, w.table, pairs);
    SD3D_CHECK_LAUNCH();
    return SD3D_OK;
}

extern "C" int sd3d_fuse_accumulate(const void* depth, int depth_u16, float depth_scale, const float* intrinsics, const float* cam_to_world,
                                    const void* colors, int V, int Hd, int Wd, int Hc, int Wc, int stride, float near, float far,
                                    float edge_abs, float edge_rel, int use_edges, float inv_voxel, void* ws, size_t ws_bytes,
                                    int64_t capacity, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    FvGeom g;
    if (int rc = sd3d_depth_rule("fuse_accumulate", depth_u16, depth_scale, Hd, Wd, near, far, edge_abs, edge_rel, use_edges, g.px)) return rc;
    if (V < 0 || Hc < 1 || Hc > SD3D_MAX_IMAGE_DIM || Wc < 1 || Wc > SD3D_MAX_IMAGE_DIM || stride < 1 || stride > SD3D_MAX_IMAGE_DIM ||
        !(inv_voxel > 0.0f) || !(inv_voxel <= 3.0e38f))
        return sd3d_set_error(SD3D_ERR_ARG, "fuse_accumulate: V >= 0, colour images up to 16384 a side, 1 <= stride <= 16384, inv_voxel > 0 and "
                                            "finite");
    FvWs w;
    if (int rc = fv_check_ws("fuse_accumulate", ws, ws_bytes, capacity, w)) return rc;
    if (V == 0) return SD3D_OK;
    if (!depth || !intrinsics || !cam_to_world || !colors) return sd3d_set_error(SD3D_ERR_ARG, "fuse_accumulate: NULL argument");
    g.Hc = Hc; g.Wc = Wc; g.stride = stride;
    g.Hs = (Hd + stride - 1) / stride; g.Ws = (Wd + stride - 1) / stride;
    g.tiles_x = (g.Ws + FV_TILE_W - 1) / FV_TILE_W;
    g.tiles_per_view = g.tiles_x * ((g.Hs + FV_TILE_H - 1) / FV_TILE_H);
    g.inv_voxel = inv_voxel;
    g.mask = (uint32_t)(capacity - 1);
    const int64_t blocks = (int64_t)V * g.tiles_per_view;
    if (blocks > 0x7FFFFFFFll) return sd3d_set_error(SD3D_ERR_ARG, "fuse_accumulate: more than 2^31 - 1 tiles in one call; cut the views into several");
    const dim3 grid((unsigned)blocks), block(FV_THREADS);
    SD3D_LAUNCH_DEPTH(fv_accumulate_kernel, grid, block, st, depth_u16, depth, intrinsics, cam_to_world, (const uint8_t*)colors, g, w.table,
                      w.counters);
    SD3D_CHECK_LAUNCH();
    return SD3D_OK;
}

extern "C" int sd3d_fuse_emit(void* ws, size_t ws_bytes, int64_t capacity, int min_obs, float* points, int32_t* obs, int64_t* keys_out,
                              int64_t out_cap, int64_t* info, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    FvWs w;
    if (int rc = fv_check_ws("fuse_emit", ws, ws_bytes, capacity, w)) return rc;
    if (min_obs < 1 || out_cap < 0 || !info || (out_cap > 0 && (!points || !obs)))
        return sd3d_set_error(SD3D_ERR_ARG, "fuse_emit: min_obs >= 1, out_cap >= 0, info required, points and obs required when out_cap > 0");
    if (hipMemsetAsync(w.counters, 0, 2 * 8, st) != hipSuccess) return sd3d_set_error(SD3D_ERR_LAUNCH, "fuse_emit: memset");   // N and cells
    const dim3 grid((unsigned)cdiv(capacity, 256)), block(256);
    hipLaunchKernelGGL(fv_emit_keys_kernel, grid, block, 0, st, w.table, capacity, (fv_u64)min_obs, w.keys_a, w.counters);
    int landed = 0;
    if (int rc = sort_pairs_u64(w.keys_a, nullptr, w.keys_b, w.vals_b, capacity, 0, 64, w.sort_ws, w.sort_bytes, st, w.vals_a, &landed)) return rc;
    hipLaunchKernelGGL(fv_emit_write_kernel, grid, block, 0, st, w.table, landed ? w.keys_a : w.keys_b, landed ? w.vals_a : w.vals_b, capacity,
                       out_cap, points, obs, keys_out, w.counters, info);
    SD3D_CHECK_LAUNCH();
    return SD3D_OK;
}
