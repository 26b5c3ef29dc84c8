// Lifting of a 2D detector's queries to 3D centres (the producer of `query2d_feats` / `query2d_pos`; the reference only loads them
// from a per-scene dump and ships no code that makes them, so tests/lift_queries_ref.py - a float64 restatement of the rule in
// include/segdino3d_hip.h - is what these kernels are pinned against).
//
// The rule, per (view v, query q); every decision is an integer one or a single rounded fp32 operation:
//   1. depth pixel (vi, ui) reads mask pixel ym = ((2 vi + 1) Hm) / (2 Hd), xm = ((2 ui + 1) Wm) / (2 Wd) (integer divisions);
//   2. d = depth in fp32 metres (raw * depth_scale for uint16); require d > 0; t = d * 1000 + 0.5 (two rounded operations, never
//      contracted), require t < 65536; k = (int)floor(t), require 1 <= k <= far_mm;
//   3. k_med = the key of rank (n - 1) / 2 of the n valid masked pixels in ascending order (the lower median), exact;
//   4. keep a pixel iff 1000 |k - k_med| <= 1000 gate_mm + gate_permille k_med (integers);
//   5. p_c = ((ui - cx) d / fx, (vi - cy) d / fy, d), w = R p_c + t with the fp32 cam_to_world, each component as
//      ((r0 x + r1 y) + r2 z) + t, every operation rounded on its own; require every component finite and
//      |w| < 2^SD3D_LIFTQ_WORLD_BITS, otherwise the pixel is dropped and not counted;
//   6. sum += rint(w * 2^SD3D_LIFTQ_FIXED_BITS) as int64 per component, count = kept pixels,
//      centre = (float)((double)sum / (double)count / 2^SD3D_LIFTQ_FIXED_BITS), zero where count == 0;
//   7. (v, q) is valid iff score >= score_thr (a NaN fails) and count >= min_pixels; all valid rows, or the max_queries best by score
//      descending (ties to the lower row), are emitted in ascending row order;
//   8. the selected rows of feats (fp16 -> fp32 is exact) and of centre are gathered.
//
//   sd3d_lift_query_centres  lq_centre_kernel   one workgroup of 256 lanes owns one (view, query): no other workgroup touches its
//                                               outputs.  It finds the bounding box of the mask (one pass over the mask, 16 bytes per
//                                               lane where the extents allow), then sweeps the depth pixels under the box three
//                                               times: a 256-bin histogram of the key's high byte (per wave in LDS, counted in runs
//                                               per lane), one of the low byte inside the bin that holds the median's rank, and the
//                                               gated int64 fixed-point sums, reduced with wave_sum and added over the four waves
//                                               through LDS.  Integer sums have the same bits in any order.  <D, FAST>: FAST = mask
//                                               and depth of one size with a width that is a multiple of 16 - 16 mask bytes and 16
//                                               depth pixels per lane and step; otherwise four neighbouring depth pixels per lane and
//                                               step, the divisions of step 1 as multiply-shifts.
//   sd3d_lift_query_select   lq_flags_kernel, scan_exclusive_i32, and when a cap can bind: sd3d_keys_from_f32 (descending),
//                            lq_key_invalid_kernel (invalid rows behind every valid one), sort_pairs_u64 over 33 bits (stable: ties
//                            keep the lower row first), lq_mark_kernel, a second scan; lq_compact_kernel writes the ascending rows.
//   sd3d_lift_query_gather   lq_gather_kernel   16 bytes of a feats row per lane.
// All values are written with plain vector stores; no atomics but the LDS ones of the histograms.
#include "common.h"
#include "depth_pixel.h"                                // the depth conversion alone (and backproject.h), under the default contraction
#include <hip/hip_fp16.h>

#define LQ_THREADS 256
#define LQ_MAX_PIXELS (1 << 28)                         // 2^28 pixels * 2^(14 + 20) per addend < 2^63
#define LQ_MAX_ROWS 0x7F000000ll

// floor(n / d) as a multiplication, m = ceil(2^45 / d): exact while n d < 2^45 (e = m d - 2^45 < d, and n e < 2^45 is what it takes), and
// n m fits 64 bits while n / d < 2^18.  Here n < 2^29 and d <= 2^15 with quotients below 2^14: the sweeps divide per pixel, and a
// division by a number the compiler does not know costs some forty instructions.
#define LQ_MAGIC_SHIFT 45
__host__ __device__ static inline uint64_t lq_magic(uint32_t d) { return ((1ull << LQ_MAGIC_SHIFT) + d - 1) / d; }
__device__ __forceinline__ int lq_div(int n, uint64_t m) { return (int)(((uint64_t)(uint32_t)n * m) >> LQ_MAGIC_SHIFT); }

struct LqGeom {
    int Q, Hd, Wd, Hm, Wm, far_mm, gate_mm, gate_permille, vec_mask;
    float depth_scale;
    uint64_t magic_2hd, magic_2wd;                      // lq_magic(2 Hd), lq_magic(2 Wd): step 1
};
struct LqBox {                                          // depth pixels, inclusive; empty when v0 > v1
    int v0, v1, u0, u1;
    uint64_t magic_cols;                                // lq_magic(columns a sweep walks per row)
};

// 16 depth pixels from a 16-byte aligned address -> metres
__device__ __forceinline__ void lq_load16(const uint16_t* p, float scale, float (&d)[16]) {
    const uint4 a = ((const uint4*)p)[0], b = ((const uint4*)p)[1];
    const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
    for (int j = 0; j < 16; ++j) d[j] = sd3d_depth_metres((uint16_t)((w[j >> 1] >> (16 * (j & 1))) & 0xFFFFu), scale);
}
__device__ __forceinline__ void lq_load16(const float* p, float, float (&d)[16]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float4 q = ((const float4*)p)[i];
        d[4 * i] = q.x; d[4 * i + 1] = q.y; d[4 * i + 2] = q.z; d[4 * i + 3] = q.w;
    }
}

// step 2 -> the key in millimetres, 0 = invalid.  Compared as floats before anything becomes an integer.
__device__ __forceinline__ int lq_key(float d, int far_mm) {
    if (!(d > 0.0f)) return 0;
    const float t = __fadd_rn(__fmul_rn(d, 1000.0f), 0.5f);
    if (!(t < 65536.0f)) return 0;
    const int k = (int)floorf(t);
    return k >= 1 && k <= far_mm ? k : 0;
}

// f(vi, ui, d, k) for every depth pixel of `box` whose mask sample is set and whose key is valid.
// The fast path's unit: 16 mask bytes `m` (not all zero) and the 16 depth pixels at `at` of one row -> f for the set and valid ones.
template <typename D, typename F>
__device__ __forceinline__ void lq_chunk(const uint4 m, const D* __restrict__ depth, int64_t at, const LqGeom& g, int vi, int ub, F f) {
    const uint32_t mw[4] = {m.x, m.y, m.z, m.w};
    float dv[16];
    lq_load16(depth + at, g.depth_scale, dv);
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        if (!((mw[j >> 2] >> (8 * (j & 3))) & 0xFFu)) continue;
        const int k = lq_key(dv[j], g.far_mm);
        if (k) f(vi, ub + j, dv[j], k);
    }
}

#define LQ_COLS 4                                       // depth pixels of one row a lane takes per step on the general path
template <typename D, bool FAST, typename F>
__device__ __forceinline__ void lq_sweep(const uint8_t* __restrict__ mask, const D* __restrict__ depth, const LqGeom& g, const LqBox& b, F f) {
    if (b.v0 > b.v1) return;
    if (FAST) {                                                                      // Hm == Hd, Wm == Wd, Wd % 16 == 0
        const int c0 = b.u0 >> 4, cpr = (b.u1 >> 4) - c0 + 1, total = (b.v1 - b.v0 + 1) * cpr;
        for (int idx = threadIdx.x; idx < total; idx += LQ_THREADS) {
            const int rr = lq_div(idx, b.magic_cols), vi = b.v0 + rr, ub = (c0 + idx - rr * cpr) * 16;
            const int64_t at = (int64_t)vi * g.Wd + ub;
            const uint4 m = *(const uint4*)(mask + at);
            if (m.x | m.y | m.z | m.w) lq_chunk(m, depth, at, g, vi, ub, f);
        }
    } else {                                                                         // LQ_COLS neighbours per lane: their loads go out together
        const int groups = (b.u1 - b.u0 + LQ_COLS) / LQ_COLS, total = (b.v1 - b.v0 + 1) * groups;
        for (int idx = threadIdx.x; idx < total; idx += LQ_THREADS) {
            const int rr = lq_div(idx, b.magic_cols), vi = b.v0 + rr, ug = b.u0 + (idx - rr * groups) * LQ_COLS;
            const int ym = lq_div((2 * vi + 1) * g.Hm, g.magic_2hd);                  // < Hm
            const uint8_t* mrow = mask + (int64_t)ym * g.Wm;
            const D* drow = depth + (int64_t)vi * g.Wd;
            uint8_t mk[LQ_COLS];
            D dv[LQ_COLS];
#pragma unroll
            for (int j = 0; j < LQ_COLS; ++j) {
                const int ui = min(ug + j, b.u1), xm = lq_div((2 * ui + 1) * g.Wm, g.magic_2wd);              // <= u1 < Wd, xm < Wm
                mk[j] = ug + j <= b.u1 ? mrow[xm] : (uint8_t)0;
            }
#pragma unroll
            for (int j = 0; j < LQ_COLS; ++j) dv[j] = mk[j] ? drow[ug + j] : (D)0;    // mk[j] != 0 only where ug + j <= u1
#pragma unroll
            for (int j = 0; j < LQ_COLS; ++j) {
                if (!mk[j]) continue;
                const float d = sd3d_depth_metres(dv[j], g.depth_scale);
                const int k = lq_key(d, g.far_mm);
                if (k) f(vi, ug + j, d, k);
            }
        }
    }
}

// Counts into this wave's histogram, run-length coded per lane.  Depth under one mask clusters and a lane walks neighbouring pixels, so
// most pixels only extend the lane's current run: one compare and one add instead of an LDS atomic each (the sweeps are bound by
// instruction issue, not by memory).  `flush` after the sweep.
struct LqRuns {
    int* h;
    int bin, run;
    __device__ __forceinline__ void add(int b) {
        if (b == bin) { ++run; return; }
        if (run) atomicAdd(&h[bin], run);
        bin = b; run = 1;
    }
    __device__ __forceinline__ void flush() { if (run) atomicAdd(&h[bin], run); run = 0; }
};

// The bin that holds rank `r` of the 4 x 256 per-wave histogram -> s_sel[0] = bin, s_sel[1] = rank inside it, s_sel[2] = total.
// r < 0: only the total is wanted (the caller derives r from it).  All 256 threads call; ends synchronised.
__device__ __forceinline__ void lq_select_bin(const int (*hist)[256], int r, int* s_wave, int* s_sel) {
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int c = hist[0][t] + hist[1][t] + hist[2][t] + hist[3][t];
    const int inc = wave_scan_incl(c, lane);
    if (lane == 63) s_wave[w] = inc;
    __syncthreads();
    int base = 0;
    for (int i = 0; i < w; ++i) base += s_wave[i];
    const int total = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    const int excl = base + inc - c;
    if (r < 0) r = total > 0 ? (total - 1) / 2 : 0;
    if (t == 0) s_sel[2] = total;
    if (c > 0 && excl <= r && r < excl + c) {                                        // exactly one thread when total > 0
        s_sel[0] = t;
        s_sel[1] = r - excl;
    }
    __syncthreads();
}

template <typename D, bool FAST>
__global__ __launch_bounds__(LQ_THREADS) void lq_centre_kernel(const D* __restrict__ depth, const float* __restrict__ intr,
                                                               const float* __restrict__ c2w, const uint8_t* __restrict__ masks, LqGeom g,
                                                               float* __restrict__ centre, int32_t* __restrict__ count,
                                                               int32_t* __restrict__ median_mm) {
    __shared__ int hist[4][256];
    __shared__ int s_wave[4], s_sel[3], s_box[4];
    __shared__ long long s_sum[4][3];
    __shared__ int s_cnt[4];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int64_t row = blockIdx.x;                                                   // v * Q + q
    const int v = (int)(row / g.Q);
    const uint8_t* mask = masks + row * ((int64_t)g.Hm * g.Wm);
    depth += (int64_t)v * g.Hd * g.Wd;

    // ---- the mask's bounding rows and columns (mask pixels).  (Histogramming the high byte in this pass on the fast path, which needs
    //      no box, saves a sweep and measured slower, 3.76 against 3.42 ms per scene: few chunks of a mask are set, so the lanes
    //      that hold one work through its 16 pixels while the rest of their wave idles.)
    if (t < 4) s_box[t] = t < 2 ? 0x7FFFFFFF : -1;
    for (int i = t; i < 4 * 256; i += LQ_THREADS) (&hist[0][0])[i] = 0;
    __syncthreads();
    LqRuns runs = {hist[w], 0, 0};
    int ymin = g.Hm, ymax = -1, xmin = g.Wm, xmax = -1;
    const int npix = g.Hm * g.Wm;
    if (g.vec_mask) {                                                                 // Wm % 16 == 0: a chunk of 16 lies in one row
        const int n16 = npix / 16;
        const uint4 none = make_uint4(0u, 0u, 0u, 0u);
        for (int i0 = t; i0 < n16; i0 += 4 * LQ_THREADS) {                            // four loads in flight per lane
            uint4 m[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) m[j] = i0 + j * LQ_THREADS < n16 ? ((const uint4*)mask)[i0 + j * LQ_THREADS] : none;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (!(m[j].x | m[j].y | m[j].z | m[j].w)) continue;
                const int i = i0 + j * LQ_THREADS, y = (i * 16) / g.Wm, x = i * 16 - y * g.Wm;
                ymin = min(ymin, y); ymax = max(ymax, y); xmin = min(xmin, x); xmax = max(xmax, x + 15);
            }
        }
    } else {
        for (int i = t; i < npix; i += LQ_THREADS) {
            if (!mask[i]) continue;
            const int y = i / g.Wm, x = i % g.Wm;
            ymin = min(ymin, y); ymax = max(ymax, y); xmin = min(xmin, x); xmax = max(xmax, x);
        }
    }
    ymin = wave_min(ymin); xmin = wave_min(xmin); ymax = wave_max(ymax); xmax = wave_max(xmax);
    if (lane == 0) {
        atomicMin(&s_box[0], ymin); atomicMin(&s_box[1], xmin); atomicMax(&s_box[2], ymax); atomicMax(&s_box[3], xmax);
    }
    __syncthreads();
    ymin = s_box[0]; xmin = s_box[1]; ymax = s_box[2]; xmax = s_box[3];
    // the depth pixels whose sample can fall inside: ym(vi) >= ymin needs vi >= Hd ymin / Hm - 1/2, ym(vi) <= ymax needs
    // vi < Hd (ymax + 1) / Hm - 1/2; one pixel of slack either way, the sweeps test the mask itself
    LqBox b;
    if (ymax < 0) {
        b.v0 = b.u0 = 0; b.v1 = b.u1 = -1;
    } else if (FAST) {
        b.v0 = ymin; b.v1 = ymax; b.u0 = xmin; b.u1 = xmax;
    } else {
        b.v0 = max((int)(((int64_t)ymin * g.Hd) / g.Hm) - 1, 0);
        b.v1 = min((int)(((int64_t)(ymax + 1) * g.Hd) / g.Hm), g.Hd - 1);
        b.u0 = max((int)(((int64_t)xmin * g.Wd) / g.Wm) - 1, 0);
        b.u1 = min((int)(((int64_t)(xmax + 1) * g.Wd) / g.Wm), g.Wd - 1);
    }
    b.magic_cols = ymax < 0 ? 0 : lq_magic((uint32_t)(FAST ? (b.u1 >> 4) - (b.u0 >> 4) + 1 : (b.u1 - b.u0 + LQ_COLS) / LQ_COLS));

    // ---- the exact lower median of the keys: radix select, high byte then low byte
    lq_sweep<D, FAST>(mask, depth, g, b, [&](int, int, float, int k) { runs.add(k >> 8); });
    runs.flush();
    __syncthreads();
    lq_select_bin(hist, -1, s_wave, s_sel);
    const int n = s_sel[2];
    if (n == 0) {                                                                     // uniform: nothing valid under the mask
        if (t == 0) {
            centre[row * 3] = 0.0f; centre[row * 3 + 1] = 0.0f; centre[row * 3 + 2] = 0.0f;
            count[row] = 0;
            median_mm[row] = 0;
        }
        return;
    }
    const int hi = s_sel[0], r_lo = s_sel[1];
    __syncthreads();
    for (int i = t; i < 4 * 256; i += LQ_THREADS) (&hist[0][0])[i] = 0;
    __syncthreads();
    lq_sweep<D, FAST>(mask, depth, g, b, [&](int, int, float, int k) { if ((k >> 8) == hi) runs.add(k & 255); });
    runs.flush();
    __syncthreads();
    lq_select_bin(hist, r_lo, s_wave, s_sel);
    const int k_med = (hi << 8) | s_sel[0];

    // ---- gate, back-project, fixed-point sums
    const Sd3dCamera cam = sd3d_load_camera(intr, c2w, v);
    const int64_t slack = 1000ll * g.gate_mm + (int64_t)g.gate_permille * k_med;
    const float lim = (float)(1 << SD3D_LIFTQ_WORLD_BITS), fixed = (float)(1 << SD3D_LIFTQ_FIXED_BITS);
    long long sx = 0, sy = 0, sz = 0;
    int cnt = 0;
    lq_sweep<D, FAST>(mask, depth, g, b, [&](int vi, int ui, float d, int k) {
        if (1000ll * abs(k - k_med) > slack) return;
        float wx, wy, wz;
        sd3d_backproject(cam, vi, ui, d, wx, wy, wz);                                  // step 5: backproject.h, shared with fuse_views.hip
        if (!(fabsf(wx) < lim && fabsf(wy) < lim && fabsf(wz) < lim)) return;          // NaN and infinities stop here
        sx += (long long)rintf(wx * fixed);
        sy += (long long)rintf(wy * fixed);
        sz += (long long)rintf(wz * fixed);
        ++cnt;
    });
    sx = wave_sum(sx); sy = wave_sum(sy); sz = wave_sum(sz); cnt = wave_sum(cnt);
    if (lane == 0) { s_sum[w][0] = sx; s_sum[w][1] = sy; s_sum[w][2] = sz; s_cnt[w] = cnt; }
    __syncthreads();
    if (t == 0) {
        const int c = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        float out[3] = {0.0f, 0.0f, 0.0f};
        if (c > 0)
            for (int i = 0; i < 3; ++i)
                out[i] = (float)((double)(s_sum[0][i] + s_sum[1][i] + s_sum[2][i] + s_sum[3][i]) / (double)c / (double)(1 << SD3D_LIFTQ_FIXED_BITS));
        centre[row * 3] = out[0]; centre[row * 3 + 1] = out[1]; centre[row * 3 + 2] = out[2];
        count[row] = c;
        median_mm[row] = k_med;
    }
}

// ---------------------------------------------------------------------------------------------- selection
__global__ __launch_bounds__(256) void lq_flags_kernel(const float* __restrict__ scores, const int32_t* __restrict__ count, int64_t n,
                                                       float score_thr, int min_pixels, int32_t* __restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) flags[i] = scores[i] >= score_thr && count[i] >= min_pixels ? 1 : 0;   // a NaN score fails
}

// the keys of sd3d_keys_from_f32 use 32 bits: bit 32 puts the invalid rows behind every valid one
__global__ __launch_bounds__(256) void lq_key_invalid_kernel(uint64_t* __restrict__ keys, const int32_t* __restrict__ flags, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n && !flags[i]) keys[i] |= 1ull << 32;
}

// sorted position j holds row order[j] (a permutation: every flag is written once): the first min(cap, n_valid) are taken
__global__ __launch_bounds__(256) void lq_mark_kernel(const uint32_t* __restrict__ order, int64_t n, const int32_t* __restrict__ n_valid,
                                                      int64_t cap, int32_t* __restrict__ flags) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const uint32_t r = order[j];
    if (r < n) flags[r] = j < min(cap, (int64_t)*n_valid) ? 1 : 0;
}

__global__ __launch_bounds__(256) void lq_compact_kernel(const int32_t* __restrict__ flags, const int32_t* __restrict__ pos, int64_t n,
                                                         int64_t rows_cap, int32_t* __restrict__ rows) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n && flags[i] && pos[i] >= 0 && pos[i] < rows_cap) rows[pos[i]] = (int32_t)i;
}

// ---------------------------------------------------------------------------------------------- gather
__device__ __forceinline__ void lq_row16(const __half* p, float* out) {              // 16 bytes = 8 channels
    const uint4 q = *(const uint4*)p;
    const __half2* h = (const __half2*)&q;
    const float2 a = __half22float2(h[0]), b = __half22float2(h[1]), c = __half22float2(h[2]), d = __half22float2(h[3]);
    *(float4*)out = make_float4(a.x, a.y, b.x, b.y);
    *(float4*)(out + 4) = make_float4(c.x, c.y, d.x, d.y);
}
__device__ __forceinline__ void lq_row16(const float* p, float* out) { *(float4*)out = *(const float4*)p; }      // 4 channels

template <typename T>
__global__ __launch_bounds__(256) void lq_gather_kernel(const T* __restrict__ feats, const float* __restrict__ centre,
                                                        const int32_t* __restrict__ rows, int64_t n, int64_t M, int C,
                                                        float* __restrict__ out_feats, float* __restrict__ out_pos) {
    constexpr int VEC = 16 / (int)sizeof(T);
    const int lpr = C / VEC;                                                          // lanes per row
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t j = i / lpr;
    if (j >= M) return;
    const int part = (int)(i % lpr);
    const int64_t r = rows[j];
    if (r < 0 || r >= n) return;                                                      // not a row of the stores: never from lq_compact_kernel
    lq_row16(feats + r * C + part * VEC, out_feats + j * C + part * VEC);
    if (part == 0) {
        out_pos[j * 3] = centre[r * 3]; out_pos[j * 3 + 1] = centre[r * 3 + 1]; out_pos[j * 3 + 2] = centre[r * 3 + 2];
    }
}

// ---------------------------------------------------------------------------------------------- C entry points
extern "C" int sd3d_lift_query_centres(const void* depth, int depth_u16, float depth_scale, const float* intrinsics,
                                       const float* cam_to_world, const void* masks, int V, int Q, int Hd, int Wd, int Hm, int Wm,
                                       int far_mm, int gate_mm, int gate_permille, float* centre, int32_t* count, int32_t* median_mm,
                                       void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (V < 0 || Q < 0 || (int64_t)V * Q > LQ_MAX_ROWS || Hd < 1 || Hd > SD3D_MAX_IMAGE_DIM || Wd < 1 || Wd > SD3D_MAX_IMAGE_DIM || Hm < 1 ||
        Hm > SD3D_MAX_IMAGE_DIM || Wm < 1 || Wm > SD3D_MAX_IMAGE_DIM || (int64_t)Hd * Wd > LQ_MAX_PIXELS || (int64_t)Hm * Wm > LQ_MAX_PIXELS || far_mm < 1 ||
        far_mm > 65535 || gate_mm < 0 || gate_mm > 65535 || gate_permille < 0 || gate_permille > 65535 || (depth_u16 && !(depth_scale > 0.0f)))
        return sd3d_set_error(SD3D_ERR_ARG, "lift_query_centres: V * Q <= 0x7F000000 rows, images and masks up to 16384 a side and 2^28 pixels, "
                                            "1 <= far_mm <= 65535, 0 <= gate_mm, gate_permille <= 65535, depth_scale > 0 for uint16 depth");
    if (V == 0 || Q == 0) return SD3D_OK;
    if (!depth || !intrinsics || !cam_to_world || !masks || !centre || !count || !median_mm)
        return sd3d_set_error(SD3D_ERR_ARG, "lift_query_centres: NULL argument");
    LqGeom g;
    g.Q = Q; g.Hd = Hd; g.Wd = Wd; g.Hm = Hm; g.Wm = Wm; g.far_mm = far_mm; g.gate_mm = gate_mm; g.gate_permille = gate_permille;
    g.depth_scale = depth_u16 ? depth_scale : 1.0f;
    g.magic_2hd = lq_magic(2u * (uint32_t)Hd); g.magic_2wd = lq_magic(2u * (uint32_t)Wd);
    // 16-byte loads need rows of whole chunks; every mask and depth image then starts on a multiple of 16 elements
    const bool mask16 = Wm % 16 == 0 && ((uintptr_t)masks & 15) == 0;
    const bool fast = Hm == Hd && Wm == Wd && mask16 && ((uintptr_t)depth & 15) == 0;
    g.vec_mask = mask16 ? 1 : 0;
    const dim3 grid((unsigned)((int64_t)V * Q)), block(LQ_THREADS);
    const uint8_t* mk = (const uint8_t*)masks;
#define LQ_GO(D, FAST) \
    hipLaunchKernelGGL((lq_centre_kernel<D, FAST>), grid, block, 0, st, (const D*)depth, intrinsics, cam_to_world, mk, g, centre, count, median_mm)
    if (depth_u16) { if (fast) LQ_GO(uint16_t, true); else LQ_GO(uint16_t, false); }
    else { if (fast) LQ_GO(float, true); else LQ_GO(float, false); }
#undef LQ_GO
    SD3D_CHECK_LAUNCH();
    return SD3D_OK;
}

// flags, pos: int32 [n]; keys a, b: uint64 [n]; vals a, b: uint32 [n]; n_valid: int32; scan and sort scratch
struct LqSelectWs {
    int32_t *flags, *pos, *n_valid;
    uint64_t *keys_a, *keys_b;
    uint32_t *vals_a, *vals_b;
    void *scan_ws, *sort_ws;
    size_t scan_bytes, sort_bytes, total;
};
static LqSelectWs lq_select_ws(void* ws, int64_t n) {
    LqSelectWs w;
    char* p = (char*)ws;
    size_t o = 0;
    const size_t m = (size_t)(n > 0 ? n : 1);
    auto take = [&](size_t bytes) { char* q = p + o; o += align_up(bytes, 256); return (void*)q; };
    w.keys_a = (uint64_t*)take(m * 8); w.keys_b = (uint64_t*)take(m * 8);
    w.flags = (int32_t*)take(m * 4); w.pos = (int32_t*)take(m * 4);
    w.vals_a = (uint32_t*)take(m * 4); w.vals_b = (uint32_t*)take(m * 4);
    w.n_valid = (int32_t*)take(4);
    w.scan_bytes = scan_ws_bytes(m); w.scan_ws = take(w.scan_bytes);
    w.sort_bytes = sort_ws_bytes(m); w.sort_ws = take(w.sort_bytes);
    w.total = o;
    return w;
}
extern "C" size_t sd3d_lift_query_select_ws_bytes(int64_t n) { return lq_select_ws(nullptr, n).total; }

extern "C" int sd3d_lift_query_select(const float* scores, const int32_t* count, int64_t n, float score_thr, int min_pixels,
                                      int64_t max_queries, int32_t* rows, int64_t rows_cap, int32_t* m_dev, void* ws, size_t ws_bytes,
                                      void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (n < 0 || n > LQ_MAX_ROWS || min_pixels < 1 || rows_cap < 0 || !m_dev)
        return sd3d_set_error(SD3D_ERR_ARG, "lift_query_select: 0 <= n <= 0x7F000000 rows, min_pixels >= 1, rows_cap >= 0, m_dev required");
    const int64_t cap = max_queries < 0 ? n : max_queries;
    if (rows_cap < (cap < n ? cap : n)) return sd3d_set_error(SD3D_ERR_ARG, "lift_query_select: rows must hold min(max_queries, n) entries");
    if (n == 0 || cap == 0) {
        if (hipMemsetAsync(m_dev, 0, sizeof(int32_t), st) != hipSuccess) return sd3d_set_error(SD3D_ERR_LAUNCH, "lift_query_select: memset");
        return SD3D_OK;
    }
    if (!scores || !count || !rows || !ws) return sd3d_set_error(SD3D_ERR_ARG, "lift_query_select: NULL argument");
    if (((uintptr_t)ws & 255) != 0) return sd3d_set_error(SD3D_ERR_ARG, "lift_query_select: ws must be 256-byte aligned");
    const LqSelectWs w = lq_select_ws(ws, n);
    if (ws_bytes < w.total) return sd3d_set_error(SD3D_ERR_WS, "lift_query_select: workspace too small");
    const dim3 grid((unsigned)cdiv(n, 256)), block(256);
    hipLaunchKernelGGL(lq_flags_kernel, grid, block, 0, st, scores, count, n, score_thr, min_pixels, w.flags);
    if (cap >= n) {                                                                   // the cap cannot bind
        if (int rc = scan_exclusive_i32(w.flags, w.pos, n, nullptr, m_dev, w.scan_ws, w.scan_bytes, st)) return rc;
    } else {
        if (int rc = scan_exclusive_i32(w.flags, w.pos, n, nullptr, w.n_valid, w.scan_ws, w.scan_bytes, st)) return rc;
        if (int rc = sd3d_keys_from_f32(scores, n, 1, w.keys_a, stream)) return rc;
        hipLaunchKernelGGL(lq_key_invalid_kernel, grid, block, 0, st, w.keys_a, w.flags, n);
        int landed = 0;
        if (int rc = sort_pairs_u64(w.keys_a, nullptr, w.keys_b, w.vals_b, n, 0, 33, w.sort_ws, w.sort_bytes, st, w.vals_a, &landed)) return rc;
        hipLaunchKernelGGL(lq_mark_kernel, grid, block, 0, st, landed ? w.vals_a : w.vals_b, n, w.n_valid, cap, w.flags);
        if (int rc = scan_exclusive_i32(w.flags, w.pos, n, nullptr, m_dev, w.scan_ws, w.scan_bytes, st)) return rc;
    }
    hipLaunchKernelGGL(lq_compact_kernel, grid, block, 0, st, w.flags, w.pos, n, rows_cap, rows);
    SD3D_CHECK_LAUNCH();
    return SD3D_OK;
}

extern "C" int sd3d_lift_query_gather(const void* feats, int feats_f16, const float* centre, const int32_t* rows, int64_t n, int64_t M,
                                      int C, float* out_feats, float* out_pos, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (n < 0 || n > LQ_MAX_ROWS || M < 0 || M > n || C < 8 || C > 65536 || C % 8 != 0)
        return sd3d_set_error(SD3D_ERR_ARG, "lift_query_gather: 0 <= M <= n <= 0x7F000000 rows, C a multiple of 8 up to 65536");
    if (M == 0) return SD3D_OK;
    if (!feats || !centre || !rows || !out_feats || !out_pos) return sd3d_set_error(SD3D_ERR_ARG, "lift_query_gather: NULL argument");
    if (((uintptr_t)feats | (uintptr_t)out_feats) & 15) return sd3d_set_error(SD3D_ERR_ARG, "lift_query_gather: feats and out_feats must be 16-byte aligned");
    if (feats_f16) {
        const int64_t threads = M * (C / 8);
        hipLaunchKernelGGL(lq_gather_kernel<__half>, dim3((unsigned)cdiv(threads, 256)), dim3(256), 0, st, (const __half*)feats, centre, rows, n,
                           M, C, out_feats, out_pos);
    } else {
        const int64_t threads = M * (C / 4);
        hipLaunchKernelGGL(lq_gather_kernel<float>, dim3((unsigned)cdiv(threads, 256)), dim3(256), 0, st, (const float*)feats, centre, rows, n, M,
                           C, out_feats, out_pos);
    }
    SD3D_CHECK_LAUNCH();
    return SD3D_OK;
}
