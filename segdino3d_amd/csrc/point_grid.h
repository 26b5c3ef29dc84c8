// The hashed grid of fixed-point cells that superpoints.hip (sd3d_knn_graph: a cloud against itself) and transfer.hip (a cloud against
// other queries) both search: one definition of the cell, the bucket, the workspace and the two kernels that build the index, so the
// two searches cannot drift apart.  The grid only chooses WHICH pairs are evaluated; why it cannot lose a pair with d2 <= r2 is argued
// above the kernels that walk it (superpoints.hip for the self case, transfer.hip for the cross-set case).
//
//   knn_key_kernel      one thread per point: its bucket as the sort key; an invalid point gets the key B and sorts behind all others.
//   knn_gather_kernel   after sort_pairs_u64 with "value = original index": per sorted position (x, y, z, index) side by side and the
//                       first / one-past-last position of every bucket (zeroed before: an empty bucket is [0, 0)).
//   knn_build_index     the memsets, the two kernels and the sort between them, enqueued on one stream.
//
// Nothing here multiplies and adds floats in one expression, so the including file's `#pragma clang fp contract` state does not matter
// to this header; both users include it under contract(off) all the same.
#pragma once
#include "common.h"

#define KNN_BIAS (1 << 24)

// the scene of element i < off[S]: the last s with off[s] <= i (off ascends from 0; empty scenes repeat a value)
__device__ __forceinline__ int sp_scene_of(const int64_t* __restrict__ off, int S, int64_t i) {
    int lo = 0, hi = S - 1;                                                           // at most 17 rounds
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= i) lo = mid; else hi = mid - 1;
    }
    return lo;
}

struct KnnWs {
    uint64_t *keys_a, *keys_b;                          // [N]
    uint32_t *vals_a, *vals_b;                          // [N]
    float4* sorted;                                     // [N]
    int32_t *cell_lo, *cell_hi;                         // [B]
    void* sort_ws;
    size_t sort_bytes, total_bytes;
};
static inline int knn_bucket_bits(int64_t N) {
    int bits = 10;
    while (bits < 26 && (1ll << bits) < 2 * N) ++bits;
    return bits;
}
static inline KnnWs knn_ws(void* ws, int64_t N) {
    KnnWs w;
    char* p = (char*)ws;
    size_t o = 0;
    auto take = [&](size_t bytes) { char* q = p + o; o += align_up(bytes, 256); return (void*)q; };
    const size_t n = (size_t)(N > 0 ? N : 1), b = (size_t)1 << knn_bucket_bits(N);
    w.keys_a = (uint64_t*)take(n * 8); w.keys_b = (uint64_t*)take(n * 8);
    w.vals_a = (uint32_t*)take(n * 4); w.vals_b = (uint32_t*)take(n * 4);
    w.sorted = (float4*)take(n * 16);
    w.cell_lo = (int32_t*)take(b * 4); w.cell_hi = (int32_t*)take(b * 4);
    w.sort_bytes = sort_ws_bytes((int64_t)n); w.sort_ws = take(w.sort_bytes);
    w.total_bytes = o;
    return w;
}
// the cell edge in fixed-point units of 2^-10: radius 2^10 is exact for radius <= 4; 3 <= H <= 4098
static inline int knn_cell_units(float radius) { return (int)ceilf(radius * 1024.0f) + 2; }

__device__ __forceinline__ bool knn_valid(float x, float y, float z) {
    return fabsf(x) < 16384.0f && fabsf(y) < 16384.0f && fabsf(z) < 16384.0f;         // a NaN or an infinity is not
}
__device__ __forceinline__ int knn_cell(float c, int H) { return ((int)rintf(c * 1024.0f) + KNN_BIAS) / H; }     // 0 <= q + 2^24 <= 2^25
__device__ __forceinline__ uint32_t knn_bucket(int cx, int cy, int cz, int s, int bucket_bits) {
    const uint32_t h = hash_u64(((uint64_t)(uint32_t)cx << 32) | (uint32_t)cy);
    return hash_u64(((uint64_t)h << 32) ^ ((uint64_t)(uint32_t)s << 40) ^ (uint32_t)cz) & ((1u << bucket_bits) - 1u);
}

// voff == NULL: one scene, every point in scene 0
static __global__ __launch_bounds__(256) void knn_key_kernel(const float* __restrict__ pts, const int64_t* __restrict__ voff, int S, int64_t N,
                                                             int H, int bucket_bits, uint64_t* __restrict__ keys) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const float x = pts[i * 3], y = pts[i * 3 + 1], z = pts[i * 3 + 2];
    uint64_t key = 1ull << bucket_bits;
    if (knn_valid(x, y, z)) key = knn_bucket(knn_cell(x, H), knn_cell(y, H), knn_cell(z, H), voff ? sp_scene_of(voff, S, i) : 0, bucket_bits);
    keys[i] = key;
}

static __global__ __launch_bounds__(256) void knn_gather_kernel(const float* __restrict__ pts, const uint64_t* __restrict__ keys,
                                                                const uint32_t* __restrict__ idx, int64_t N, int bucket_bits,
                                                                float4* __restrict__ sorted, int32_t* __restrict__ cell_lo,
                                                                int32_t* __restrict__ cell_hi) {
    const int64_t pos = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (pos >= N) return;
    const int64_t i = (int64_t)idx[pos];
    sorted[pos] = make_float4(pts[i * 3], pts[i * 3 + 1], pts[i * 3 + 2], __uint_as_float((uint32_t)i));
    const uint64_t key = keys[pos];
    if (key >> bucket_bits) return;                                                   // an invalid point: in no bucket
    if (pos == 0 || keys[pos - 1] != key) cell_lo[key] = (int32_t)pos;
    if (pos == N - 1 || keys[pos + 1] != key) cell_hi[key] = (int32_t)(pos + 1);
}

// Fills w.sorted, w.cell_lo and w.cell_hi for N >= 0 points [N, 3]; *keys_out = the sorted keys (one of w.keys_a / w.keys_b).
static inline int knn_build_index(const float* points, const int64_t* voff, int S, int64_t N, int H, int bucket_bits, const KnnWs& w,
                                  hipStream_t st, const uint64_t** keys_out) {
    if (hipMemsetAsync(w.cell_lo, 0, (size_t)4 << bucket_bits, st) != hipSuccess || hipMemsetAsync(w.cell_hi, 0, (size_t)4 << bucket_bits, st) != hipSuccess)
        return sd3d_set_error(SD3D_ERR_LAUNCH, "point grid: memset");
    *keys_out = w.keys_a;
    if (N == 0) return SD3D_OK;
    const dim3 b256(256), gv((unsigned)cdiv(N, 256));
    hipLaunchKernelGGL(knn_key_kernel, gv, b256, 0, st, points, voff, S, N, H, bucket_bits, w.keys_a);
    int landed = 0;
    if (int rc = sort_pairs_u64(w.keys_a, nullptr, w.keys_b, w.vals_b, N, 0, bucket_bits + 1, w.sort_ws, w.sort_bytes, st, w.vals_a, &landed)) return rc;
    const uint64_t* keys = landed ? w.keys_a : w.keys_b;
    const uint32_t* idx = landed ? w.vals_a : w.vals_b;
    hipLaunchKernelGGL(knn_gather_kernel, gv, b256, 0, st, points, keys, idx, N, bucket_bits, w.sorted, w.cell_lo, w.cell_hi);
    SD3D_CHECK_LAUNCH();
    *keys_out = keys;
    return SD3D_OK;
}
