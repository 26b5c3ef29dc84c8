// Benchmark submission text on the device: the bytes `np.savetxt(path, x, fmt='%d')` writes for a mask row and for a label vector
// (the reference's format_results_semantic / save_single_instance, evaluator_3d.py:351-396).  The host only copies and write()s.
//
//   sd3d_mask_text    mt_kernel        one lane per 8 points: an 8-byte load of mask bytes (two aligned ones and a funnel shift where
//                                      a row starts off an 8-byte boundary) -> "0\n" / "1\n" x 8 = one aligned 16-byte store.  A row
//                                      starts at a multiple of `pitch` (a multiple of 16), so every full store is aligned whatever N
//                                      is; the last lane of a row writes its 1..7 points with 2-byte stores and nothing behind 2 N.
//                                      Store-bound: 2 bytes out per byte in, no LDS, no atomics.
//   sd3d_label_text   lt_count_kernel  LT_TILE values per workgroup: table lookup, range status, decimal length -> bytes per tile;
//                     scan             sd3d_scan_exclusive_i32 over the tile totals = where every tile's text starts, and the length;
//                     lt_write_kernel  the tile's lines are rebuilt in LDS at the position their first byte has modulo 16, so that
//                                      16-byte chunk k of the LDS image IS an aligned 16-byte chunk of the output: interior chunks go
//                                      out as one 16-byte store per lane, the two ragged ends of a tile byte by byte.
// Status word (info[1]), as in targets.hip: a value that cannot be printed contributes NO bytes and sets a bit (no clamp, no wrap); a
// text longer than out_cap sets a bit and is cut at out_cap.  One atomic per workgroup, and only when it has a bit to set.
#include "common.h"
#include "../../include/segdino3d_hip.h"
#include <stdio.h>

#define MT_PTS 8                                        // points per lane
#define LT_TILE 256                                     // values per workgroup: one per thread
#define LT_LINE 12                                      // longest line: "-2147483648\n"
#define LT_MAX_N (0x7FFFFFFFll / LT_LINE)               // every byte offset fits int32 (the scan is int32)

// 1 in every byte of w that is non-zero
__device__ static inline uint64_t mt_nonzero_bytes(uint64_t w) {
    const uint64_t m = 0x7F7F7F7F7F7F7F7Full;
    return ((((w & m) + m) | w) >> 7) & 0x0101010101010101ull;
}
// four flag bytes -> "f\n" x 4 as two little-endian 32-bit words
__device__ static inline uint2 mt_expand4(uint32_t f) {
    uint2 r;
    r.x = 0x0A300A30u + (f & 1u) + ((f & 0x100u) << 8);
    r.y = 0x0A300A30u + ((f >> 16) & 1u) + ((f >> 8) & 0x10000u);
    return r;
}

__global__ __launch_bounds__(256) void mt_kernel(const uint8_t* __restrict__ masks, int64_t N, const int32_t* __restrict__ rows, int64_t bpr,
                                                 uint8_t* __restrict__ out, int64_t pitch) {
    const int64_t i = blockIdx.x / bpr;                                             // output row
    const int64_t p0 = ((int64_t)(blockIdx.x - i * bpr) * 256 + threadIdx.x) * MT_PTS;
    if (p0 >= N) return;
    const int64_t r = rows ? rows[i] : i;
    const uint8_t* src = masks + r * N + p0;
    uint8_t* dst = out + i * pitch + 2 * p0;                                        // 16-byte aligned: out and pitch are, 2 p0 = 16 k
    if (p0 + MT_PTS <= N) {
        uint64_t w;
        const uint32_t k8 = 8u * (uint32_t)((uintptr_t)src & 7);
        if (k8 == 0) {
            w = *(const uint64_t*)src;
        } else if (p0 + 2 * MT_PTS <= N) {
            // rows of an odd length start anywhere: the two aligned words around the 8 bytes.  Each holds at least one of them (so it
            // lies in memory the row lies in), and the second ends before p0 + 16 <= N, inside the row.
            const uint64_t* al = (const uint64_t*)((uintptr_t)src & ~(uintptr_t)7);
            w = (al[0] >> k8) | (al[1] << (64u - k8));
        } else {
            w = 0;
#pragma unroll
            for (int j = 0; j < MT_PTS; ++j) w |= (uint64_t)src[j] << (8 * j);
        }
        const uint64_t f = mt_nonzero_bytes(w);
        const uint2 lo = mt_expand4((uint32_t)f), hi = mt_expand4((uint32_t)(f >> 32));
        *(uint4*)dst = make_uint4(lo.x, lo.y, hi.x, hi.y);
    } else {
        for (int j = 0; p0 + j < N; ++j) *(uint16_t*)(dst + 2 * j) = (uint16_t)(0x0A30u + (src[j] != 0));
    }
}

extern "C" int sd3d_mask_text(const uint8_t* masks, int64_t N, const int32_t* rows, int n_rows, uint8_t* out, int64_t pitch, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (N <= 0 || n_rows < 0) return sd3d_set_error(SD3D_ERR_ARG, "mask_text: N >= 1 points and n_rows >= 0");
    if (pitch < 2 * N || (pitch & 15)) return sd3d_set_error(SD3D_ERR_ARG, "mask_text: pitch must be a multiple of 16 and at least 2 N");
    if (n_rows == 0) return SD3D_OK;
    if (!masks || !out || ((uintptr_t)out & 15)) return sd3d_set_error(SD3D_ERR_ARG, "mask_text: NULL argument or `out` not 16-byte aligned");
    const int64_t bpr = cdiv(cdiv(N, MT_PTS), 256);
    if (bpr * n_rows > 0x7FFFFFFFll) return sd3d_set_error(SD3D_ERR_ARG, "mask_text: more than 2^31 workgroups; split the rows");
    hipLaunchKernelGGL(mt_kernel, dim3((unsigned)(bpr * n_rows)), dim3(256), 0, st, masks, N, rows, bpr, out, pitch);
    SD3D_CHECK_LAUNCH();
    return SD3D_OK;
}

// ---------------------------------------------------------------------------------------------- label text
// The value line i prints, or a status bit.  `ok` false: the line has no bytes.
__device__ static inline int32_t lt_value(const int64_t* __restrict__ values, int64_t i, const int32_t* __restrict__ lut, int lut_len, bool& ok,
                                          int& status) {
    const int64_t v = values[i];
    if (lut) {
        ok = v >= 0 && v < lut_len;
        if (!ok) { status |= SD3D_LABEL_TEXT_BAD_INDEX; return 0; }
        return lut[v];
    }
    ok = v >= -2147483648ll && v <= 2147483647ll;
    if (!ok) status |= SD3D_LABEL_TEXT_BAD_VALUE;
    return (int32_t)v;
}
// bytes of "%d\n"
__device__ static inline int lt_length(int32_t v) {
    const uint32_t a = v < 0 ? 0u - (uint32_t)v : (uint32_t)v;
    int d = 1;
    d += a >= 10u; d += a >= 100u; d += a >= 1000u; d += a >= 10000u; d += a >= 100000u;
    d += a >= 1000000u; d += a >= 10000000u; d += a >= 100000000u; d += a >= 1000000000u;
    return d + (v < 0) + 1;
}

__device__ static inline void lt_flush_status(int status, int32_t* info, int* red4) {
    status = wave_or(status);
    if ((threadIdx.x & 63) == 0) red4[threadIdx.x >> 6] = status;
    __syncthreads();
    if (threadIdx.x == 0) {
        status = red4[0] | red4[1] | red4[2] | red4[3];
        if (status) atomicOr(&info[1], status);
    }
}

__global__ __launch_bounds__(LT_TILE) void lt_count_kernel(const int64_t* __restrict__ values, int64_t N, const int32_t* __restrict__ lut, int lut_len,
                                                          int32_t* __restrict__ tile_bytes, int32_t* info) {
    __shared__ int red[4], sred[4];
    const int64_t i = (int64_t)blockIdx.x * LT_TILE + threadIdx.x;
    int status = 0, len = 0;
    if (i < N) {
        bool ok;
        const int32_t v = lt_value(values, i, lut, lut_len, ok, status);
        if (ok) len = lt_length(v);
    }
    len = wave_sum(len);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = len;
    lt_flush_status(status, info, sred);                                            // (has the barrier red[] needs)
    if (threadIdx.x == 0) tile_bytes[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

__global__ __launch_bounds__(LT_TILE) void lt_write_kernel(const int64_t* __restrict__ values, int64_t N, const int32_t* __restrict__ lut, int lut_len,
                                                          const int32_t* __restrict__ tile_start, uint8_t* __restrict__ out, int64_t out_cap,
                                                          int32_t* info) {
    __shared__ __attribute__((aligned(16))) uint8_t text[LT_TILE * LT_LINE + 16];
    __shared__ int wsum[4], sred[4];
    const int64_t i = (int64_t)blockIdx.x * LT_TILE + threadIdx.x;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int status = 0, len = 0;
    int32_t v = 0;
    if (i < N) {
        bool ok;
        v = lt_value(values, i, lut, lut_len, ok, status);
        if (ok) len = lt_length(v);
    }
    status = 0;                                                                     // the range bits were set by lt_count_kernel
    int inc = wave_scan_incl(len, lane);
    if (lane == 63) wsum[wv] = inc;
    __syncthreads();
    int at = inc - len;
    for (int k = 0; k < wv; ++k) at += wsum[k];
    const int total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    const int64_t start = tile_start[blockIdx.x];
    const int lead = (int)(start & 15);                                             // LDS byte j <-> output byte start - lead + j
    if (len > 0) {
        uint8_t* q = text + lead + at;
        uint32_t a = v < 0 ? 0u - (uint32_t)v : (uint32_t)v;
        q[len - 1] = '\n';
        for (int k = len - 2; k >= (v < 0); --k) { q[k] = (uint8_t)('0' + a % 10u); a /= 10u; }
        if (v < 0) q[0] = '-';
    }
    __syncthreads();
    int64_t end = start + total;
    if (end > out_cap) { status = SD3D_LABEL_TEXT_OVERFLOW; end = out_cap; }
    const int64_t g0 = start - lead;                                                // 16-byte aligned (out is)
    const int chunks = (lead + total + 15) >> 4;
    for (int c = threadIdx.x; c < chunks; c += LT_TILE) {
        const int64_t g = g0 + 16 * (int64_t)c;
        if (g >= start && g + 16 <= end) {
            *(uint4*)(out + g) = *(const uint4*)(text + 16 * c);
        } else {
            for (int k = 0; k < 16; ++k)
                if (g + k >= start && g + k < end) out[g + k] = text[16 * c + k];
        }
    }
    lt_flush_status(status, info, sred);
}

struct LtWs {
    int32_t *tile_bytes, *tile_start;
    void* scan_ws;
    size_t scan_ws_bytes, total;
};
static LtWs lt_carve(void* ws, int64_t n) {
    LtWs w;
    const int64_t nt = cdiv(n, LT_TILE);
    char* p = (char*)ws;
    auto take = [&](size_t bytes) { char* q = p; p += align_up(bytes, 256); return q; };
    w.tile_bytes = (int32_t*)take((size_t)nt * 4);
    w.tile_start = (int32_t*)take((size_t)nt * 4);
    w.scan_ws_bytes = scan_ws_bytes(nt);
    w.scan_ws = take(w.scan_ws_bytes);
    w.total = (size_t)(p - (char*)ws);
    return w;
}

extern "C" size_t sd3d_label_text_ws_bytes(int64_t N) { return lt_carve(nullptr, N > 0 ? N : 1).total; }

extern "C" int sd3d_label_text(const int64_t* values, int64_t N, const int32_t* lut, int lut_len, uint8_t* out, int64_t out_cap, int32_t* info,
                               void* ws, size_t ws_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (N < 0 || N > LT_MAX_N || out_cap < 0 || lut_len < 0 || !info)
        return sd3d_set_error(SD3D_ERR_ARG, "label_text: 0 <= N <= (2^31 - 1) / 12 values, out_cap >= 0, lut_len >= 0, info given");
    if (hipMemsetAsync(info, 0, 2 * sizeof(int32_t), st) != hipSuccess) return sd3d_set_error(SD3D_ERR_LAUNCH, "label_text: memset failed");
    if (N == 0) return SD3D_OK;
    if (!values || !ws || (out_cap > 0 && !out) || ((uintptr_t)out & 15))
        return sd3d_set_error(SD3D_ERR_ARG, "label_text: NULL argument or `out` not 16-byte aligned");
    const LtWs w = lt_carve(ws, N);
    if (ws_bytes < w.total) return sd3d_set_error(SD3D_ERR_WS, "label_text: workspace too small");
    const int64_t nt = cdiv(N, LT_TILE);
    hipLaunchKernelGGL(lt_count_kernel, dim3((unsigned)nt), dim3(LT_TILE), 0, st, values, N, lut, lut_len, w.tile_bytes, info);
    SD3D_CHECK_LAUNCH();
    if (int rc = sd3d_scan_exclusive_i32(w.tile_bytes, w.tile_start, nt, info, w.scan_ws, w.scan_ws_bytes, stream)) return rc;
    hipLaunchKernelGGL(lt_write_kernel, dim3((unsigned)nt), dim3(LT_TILE), 0, st, values, N, lut, lut_len, w.tile_start, out, out_cap, info);
    SD3D_CHECK_LAUNCH();
    return SD3D_OK;
}
