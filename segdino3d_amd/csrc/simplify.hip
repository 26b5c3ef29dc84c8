// Mesh decimation by vertex clustering: the vertices of one grid cell become one vertex, faces follow their corners, collapsed and
// duplicate faces go (the rule: include/segdino3d_hip.h, "Mesh decimation"; segdino3d_amd/simplify.py has it in full).  It is the stage
// between TsdfVolume.mesh() and mesh_superpoints that brings a 2 cm surface-net mesh down to the vertex density the model was trained
// on, and its vertex_map carries a forward's per-vertex result back onto the full mesh.  The reference has no counterpart (its meshes
// were decimated offline), so tests/simplify_ref.py - a numpy restatement of the rule - is what these kernels are pinned against, bit
// for bit.
//
// Every sum is a 64-bit integer sum of fixed-point channels and every choice is a minimum over a set of integer keys, so a cell is a
// function of the SET of its vertices and a face of the SET of faces with its oriented triple: nothing depends on the order of the
// atomics, on the cut into waves, or on the stream.  The only global atomics are 64-bit integer sums and minima.
//
//   sm_vkey_kernel      one lane per 8 vertices: step 1 (all channels |c| < 2^14) and step 2 (the cell key; a bad vertex gets the empty key,
//                       which sorts last).  sort_pairs_u64 with "value = original index": a cell's members become one run.
//   sm_vheads_kernel    one lane per sorted position: the run heads.  scan_exclusive_i32 over them numbers the cells in ascending key.
//   sm_reduce_kernel    one lane per sorted position: vertex_map = the cell, and step 3: the channels in fixed point, reduced over the 64
//                       sorted entries of a wave by a segmented scan (a run is contiguous), one 64-bit atomicAdd per (wave, run, channel)
//                       at the run's last lane in the wave.  A run of all V vertices costs V / 64 atomics per channel, not V steps.
//   sm_nearest_kernel   placement "nearest": per sorted position d2 against the cell's fp32 mean, the same segmented scan with a minimum
//                       of (bits of d2 << 32) | vertex, one 64-bit atomicMin per (wave, run).
//   sm_fkey_kernel      one lane per 8 faces: step 5 up to the rotated triple, packed into one 63-bit key (bad and collapsed faces get the
//                       empty key).  sort_pairs_u64 with "value = original index": the head of a run is the lowest original face.
//   sm_fheads_kernel    one lane per 8 sorted positions: a run head flags its face at the face's ORIGINAL position and marks its three
//                       cells as referenced; the others count as duplicates.  Two scans: the kept faces, the referenced cells.
//   sm_faces_kernel     one lane per face: a kept face writes its rotated triple (renumbered when unreferenced cells are dropped) and
//                       its source at the scanned position: ascending original face index.
//   sm_vmap_kernel      keep_unreferenced = 0: vertex_map through the renumbering.
//   sm_cells_kernel     one lane per cell: step 4, the output row at the cell's final number; lane 0 of the grid writes the counters.
// The three kernels that count (bad vertices; bad and collapsed faces; duplicates) give a workgroup 2048 elements and one atomic per
// counter: same-address atomics serialise at the L2 (profiles/raster.md), and nearly every workgroup of faces has a collapsed one.
// All values are written with plain vector stores.
#include "common.h"
// The kernels here must EQUAL the restatement, so nothing in this file may be contracted into a fused multiply-add (see
// fuse_views.hip).
#pragma clang fp contract(off)
#include "../../include/segdino3d_hip.h"

#define SM_THREADS 256
#define SM_WAVES (SM_THREADS / 64)
#define SM_ITEMS 8                                      // elements per lane in the kernels that count
#define SM_LIMIT 16384.0f                               // |c| < 2^14
#define SM_FIXED 65536.0f                               // 16 fractional bits: |c * 2^16| < 2^30, the product is exact
#define SM_OFFSET 1048576                               // 2^20: cell indices lie in [-2^20, 2^20)
#define SM_MASK21 0x1FFFFFull
// the device counters: int32 ncells, nfaces, nref | int64 bad_vertices, bad_faces, collapsed, duplicates
enum { SM_NCELLS = 0, SM_NFACES = 1, SM_NREF = 2 };
enum { SM_BAD_V = 0, SM_BAD_F = 1, SM_COLLAPSED = 2, SM_DUPLICATES = 3 };

struct SmWs {
    uint64_t *keys_a, *keys_b;                          // [max(V, F)]: the vertex sort, then the face sort
    uint32_t *idx_a, *idx_b;
    int32_t *vhead, *vexcl;                             // [V]: run heads of the sorted vertices, their exclusive scan
    int64_t* sums;                                      // [V][C + 1]: per cell the C channel sums and the count
    uint64_t* best;                                     // [V]: per cell the minimum of (bits of d2 << 32) | vertex
    int32_t *ref, *rexcl;                               // [V]: per cell referenced by a kept face, the exclusive scan
    int32_t *keep, *fexcl;                              // [F]: per ORIGINAL face kept, the exclusive scan
    int32_t* ints;                                      // SM_NCELLS ..
    int64_t* counts;                                    // SM_BAD_V ..
    void *sort_ws, *scan_ws;
    size_t sort_bytes, scan_bytes, total;
};
static SmWs sm_ws(void* ws, int64_t V, int64_t F, int C) {
    SmWs w;
    char* p = (char*)ws;
    size_t o = 0;
    const size_t v = (size_t)(V > 0 ? V : 1), f = (size_t)(F > 0 ? F : 1), m = v > f ? v : f;
    auto take = [&](size_t bytes) { char* q = p + o; o += align_up(bytes, 256); return (void*)q; };
    w.keys_a = (uint64_t*)take(m * 8); w.keys_b = (uint64_t*)take(m * 8);
    w.idx_a = (uint32_t*)take(m * 4); w.idx_b = (uint32_t*)take(m * 4);
    w.vhead = (int32_t*)take(v * 4); w.vexcl = (int32_t*)take(v * 4);
    w.sums = (int64_t*)take(v * (size_t)(C + 1) * 8);
    w.best = (uint64_t*)take(v * 8);
    w.ref = (int32_t*)take(v * 4); w.rexcl = (int32_t*)take(v * 4);
    w.keep = (int32_t*)take(f * 4); w.fexcl = (int32_t*)take(f * 4);
    w.ints = (int32_t*)take(16);
    w.counts = (int64_t*)take(32);
    w.sort_bytes = sort_ws_bytes((int64_t)m); w.sort_ws = take(w.sort_bytes);
    w.scan_bytes = scan_ws_bytes((int64_t)m); w.scan_ws = take(w.scan_bytes);
    w.total = o;
    return w;
}

// One integer sum per class and workgroup: a lane counts its own SM_ITEMS elements, wave_sum, the waves through LDS, then one atomic
// where the class occurs.  Same-address atomics serialise at the L2, so a workgroup covers 2048 elements and issues one per counter.
template <int K>
__device__ __forceinline__ void sm_count(const int (&mine)[K], int64_t* __restrict__ counts, const int (&slot)[K]) {
    __shared__ int part[SM_WAVES][K];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int s = wave_sum(mine[k]);
        if (lane == 0) part[wv][k] = s;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k)
        if (threadIdx.x == k) {
            int s = 0;
#pragma unroll
            for (int i = 0; i < SM_WAVES; ++i) s += part[i][k];
            if (s) atomicAdd((unsigned long long*)&counts[slot[k]], (unsigned long long)s);
        }
}
// element `it` of this lane in a counting kernel: a workgroup covers SM_THREADS * SM_ITEMS consecutive elements, a wave 64 adjacent ones at a time
__device__ __forceinline__ int64_t sm_item(int it) { return ((int64_t)blockIdx.x * SM_ITEMS + it) * SM_THREADS + threadIdx.x; }
static inline unsigned sm_item_blocks(int64_t n) { return (unsigned)cdiv(n > 0 ? n : 1, (int64_t)SM_THREADS * SM_ITEMS); }

__global__ __launch_bounds__(SM_THREADS) void sm_vkey_kernel(const float* __restrict__ vertices, int64_t V, int C, float inv_cell,
                                                             uint64_t* __restrict__ keys, int64_t* __restrict__ counts) {
    int bad[1] = {0};
#pragma unroll 2
    for (int it = 0; it < SM_ITEMS; ++it) {
        const int64_t i = sm_item(it);
        if (i >= V) break;
        const float* row = vertices + i * C;
        bool ok = true;
        for (int j = 0; j < C; ++j) ok = ok && fabsf(row[j]) < SM_LIMIT;                // a NaN fails
        uint64_t key = SD3D_EMPTY_KEY;
        if (ok) {
            // |x| < 2^14 and inv_cell <= 64: floorf lies in [-2^20, 2^20)
            const int kx = (int)floorf(row[0] * inv_cell), ky = (int)floorf(row[1] * inv_cell), kz = (int)floorf(row[2] * inv_cell);
            key = ((uint64_t)(uint32_t)(kx + SM_OFFSET) << 42) | ((uint64_t)(uint32_t)(ky + SM_OFFSET) << 21) | (uint64_t)(uint32_t)(kz + SM_OFFSET);
        }
        keys[i] = key;
        bad[0] += !ok;
    }
    const int slot[1] = {SM_BAD_V};
    sm_count<1>(bad, counts, slot);
}

__global__ __launch_bounds__(SM_THREADS) void sm_vheads_kernel(const uint64_t* __restrict__ keys, int64_t V, int32_t* __restrict__ head) {
    const int64_t p = (int64_t)blockIdx.x * SM_THREADS + threadIdx.x;
    if (p >= V) return;
    const uint64_t k = keys[p];
    head[p] = k != SD3D_EMPTY_KEY && (p == 0 || keys[p - 1] != k);
}

// The runs of one wave: `cell` is this lane's run (-1: none; the lanes of a run are adjacent).  start = the first lane of this lane's
// run within the wave, last = whether this lane is the run's last in the wave.
__device__ __forceinline__ void sm_segments(int cell, int lane, int& start, bool& last) {
    const int prev = __shfl_up(cell, 1);
    const unsigned long long heads = __ballot(lane == 0 || prev != cell);              // bit 0 is always set
    start = 63 - __clzll(heads & (~0ull >> (63 - lane)));
    last = lane == 63 || (((heads >> lane) >> 1) & 1ull);
}
// inclusive segmented scans over the wave: lane l ends with the sum / minimum over the lanes start .. l of its run
__device__ __forceinline__ int64_t sm_seg_sum(int64_t v, int lane, int start) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int64_t t = __shfl_up(v, d);
        if (lane - d >= start) v += t;
    }
    return v;
}
__device__ __forceinline__ uint64_t sm_seg_min(uint64_t v, int lane, int start) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t t = __shfl_up(v, d);
        if (lane - d >= start && t < v) v = t;
    }
    return v;
}

__global__ __launch_bounds__(SM_THREADS) void sm_reduce_kernel(const float* __restrict__ vertices, int64_t V, int C,
                                                               const uint64_t* __restrict__ keys, const uint32_t* __restrict__ idx,
                                                               const int32_t* __restrict__ head, const int32_t* __restrict__ excl,
                                                               int32_t* __restrict__ vertex_map, int64_t* __restrict__ sums) {
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * SM_THREADS + threadIdx.x;
    int cell = -1;
    int64_t v = 0;
    if (p < V) {
        v = (int64_t)idx[p];
        if (keys[p] != SD3D_EMPTY_KEY) cell = excl[p] + head[p] - 1;
        vertex_map[v] = cell;
    }
    int start;
    bool last;
    sm_segments(cell, lane, start, last);
    const bool emit = last && cell >= 0;
    int64_t* out = sums + (int64_t)(cell >= 0 ? cell : 0) * (C + 1);
    for (int j = 0; j < C; ++j) {
        const int64_t q = cell >= 0 ? (int64_t)rintf(vertices[v * C + j] * SM_FIXED) : 0;
        const int64_t s = sm_seg_sum(q, lane, start);
        if (emit) atomicAdd((unsigned long long*)&out[j], (unsigned long long)s);
    }
    const int64_t n = sm_seg_sum(cell >= 0 ? 1 : 0, lane, start);
    if (emit) atomicAdd((unsigned long long*)&out[C], (unsigned long long)n);
}

// channel j of a cell: float32((double) S_j / ((double) n * 65536.0))
__device__ __forceinline__ float sm_mean(const int64_t* __restrict__ cell_sums, int j, int C) {
    return (float)((double)cell_sums[j] / ((double)cell_sums[C] * 65536.0));
}

__global__ __launch_bounds__(SM_THREADS) void sm_nearest_kernel(const float* __restrict__ vertices, int64_t V, int C,
                                                                const uint32_t* __restrict__ idx, const int32_t* __restrict__ vertex_map,
                                                                const int64_t* __restrict__ sums, uint64_t* __restrict__ best) {
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * SM_THREADS + threadIdx.x;
    int cell = -1;
    uint64_t key = SD3D_EMPTY_KEY;
    if (p < V) {
        const int64_t v = (int64_t)idx[p];
        cell = vertex_map[v];
        if (cell >= 0) {
            const int64_t* s = sums + (int64_t)cell * (C + 1);
            const float* row = vertices + v * C;
            const float dx = row[0] - sm_mean(s, 0, C), dy = row[1] - sm_mean(s, 1, C), dz = row[2] - sm_mean(s, 2, C);
            const float d2 = (dx * dx + dy * dy) + dz * dz;
            key = ((uint64_t)__float_as_uint(d2) << 32) | (uint64_t)v;
        }
    }
    int start;
    bool last;
    sm_segments(cell, lane, start, last);
    const uint64_t m = sm_seg_min(key, lane, start);
    if (last && cell >= 0) atomicMin((unsigned long long*)&best[cell], (unsigned long long)m);
}

// Step 5 for one face: 1 = bad, 2 = collapsed, 0 = (a, b, c) is the mapped triple rotated so that its smallest index comes first.
__device__ __forceinline__ int sm_triple(const int32_t* __restrict__ faces, int64_t f, int64_t V, const int32_t* __restrict__ vertex_map, int& a,
                                         int& b, int& c) {
    const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    if (i0 < 0 || i0 >= V || i1 < 0 || i1 >= V || i2 < 0 || i2 >= V) return 1;
    const int m0 = vertex_map[i0], m1 = vertex_map[i1], m2 = vertex_map[i2];
    if (m0 < 0 || m1 < 0 || m2 < 0) return 1;
    if (m0 == m1 || m1 == m2 || m0 == m2) return 2;
    if (m0 < m1 && m0 < m2) { a = m0; b = m1; c = m2; }
    else if (m1 < m2) { a = m1; b = m2; c = m0; }
    else { a = m2; b = m0; c = m1; }
    return 0;
}

__global__ __launch_bounds__(SM_THREADS) void sm_fkey_kernel(const int32_t* __restrict__ faces, int64_t F, int64_t V,
                                                             const int32_t* __restrict__ vertex_map, uint64_t* __restrict__ keys,
                                                             int64_t* __restrict__ counts) {
    int n[2] = {0, 0};                                                                  // bad, collapsed
#pragma unroll 2
    for (int it = 0; it < SM_ITEMS; ++it) {
        const int64_t f = sm_item(it);
        if (f >= F) break;
        int a = 0, b = 0, c = 0;
        const int r = sm_triple(faces, f, V, vertex_map, a, b, c);
        // at most 2^21 cells (the host refuses more): three 21-bit numbers
        keys[f] = r ? SD3D_EMPTY_KEY : (((uint64_t)a & SM_MASK21) << 42) | (((uint64_t)b & SM_MASK21) << 21) | ((uint64_t)c & SM_MASK21);
        n[0] += r == 1;
        n[1] += r == 2;
    }
    const int slot[2] = {SM_BAD_F, SM_COLLAPSED};
    sm_count<2>(n, counts, slot);
}

__global__ __launch_bounds__(SM_THREADS) void sm_fheads_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ idx, int64_t F,
                                                               int64_t V, int32_t* __restrict__ keep, int32_t* __restrict__ ref,
                                                               int64_t* __restrict__ counts) {
    int dup[1] = {0};
#pragma unroll 2
    for (int it = 0; it < SM_ITEMS; ++it) {
        const int64_t p = sm_item(it);
        if (p >= F) break;
        const uint64_t k = keys[p];
        if (k == SD3D_EMPTY_KEY) continue;
        if (p == 0 || keys[p - 1] != k) {
            keep[idx[p]] = 1;
            const int64_t a = (int64_t)(k >> 42), b = (int64_t)((k >> 21) & SM_MASK21), c = (int64_t)(k & SM_MASK21);
            // (with more than 2^21 cells - refused by the host after this call - a masked number is still below V or is left alone)
            if (a < V) ref[a] = 1;
            if (b < V) ref[b] = 1;
            if (c < V) ref[c] = 1;
        } else {
            dup[0] += 1;
        }
    }
    const int slot[1] = {SM_DUPLICATES};
    sm_count<1>(dup, counts, slot);
}

__global__ __launch_bounds__(SM_THREADS) void sm_faces_kernel(const int32_t* __restrict__ faces, int64_t F, int64_t V,
                                                              const int32_t* __restrict__ vertex_map, const int32_t* __restrict__ keep,
                                                              const int32_t* __restrict__ fexcl, const int32_t* __restrict__ rexcl, int keep_unref,
                                                              int32_t* __restrict__ faces_out, int32_t* __restrict__ face_source) {
    const int64_t f = (int64_t)blockIdx.x * SM_THREADS + threadIdx.x;
    if (f >= F || !keep[f]) return;
    int a = 0, b = 0, c = 0;
    if (sm_triple(faces, f, V, vertex_map, a, b, c)) return;                           // a kept face is neither bad nor collapsed
    if (!keep_unref) { a = rexcl[a]; b = rexcl[b]; c = rexcl[c]; }                      // the numbering keeps the order: a stays the smallest
    const int64_t o = (int64_t)fexcl[f];
    faces_out[3 * o] = a; faces_out[3 * o + 1] = b; faces_out[3 * o + 2] = c;
    face_source[o] = (int32_t)f;
}

// keep_unreferenced = 0, after sm_faces_kernel (which reads the cells): old vertex -> the cell's new number, or -1
__global__ __launch_bounds__(SM_THREADS) void sm_vmap_kernel(int64_t V, const int32_t* __restrict__ ref, const int32_t* __restrict__ rexcl,
                                                             int32_t* __restrict__ vertex_map) {
    const int64_t v = (int64_t)blockIdx.x * SM_THREADS + threadIdx.x;
    if (v >= V) return;
    const int cell = vertex_map[v];
    if (cell >= 0) vertex_map[v] = ref[cell] ? rexcl[cell] : -1;
}

__global__ __launch_bounds__(SM_THREADS) void sm_cells_kernel(const float* __restrict__ vertices, int64_t V, int C, int nearest, int keep_unref,
                                                              const int64_t* __restrict__ sums, const uint64_t* __restrict__ best,
                                                              const int32_t* __restrict__ ref, const int32_t* __restrict__ rexcl,
                                                              const int32_t* __restrict__ ints, const int64_t* __restrict__ counts,
                                                              float* __restrict__ vertices_out, int64_t* __restrict__ info) {
    const int64_t cell = (int64_t)blockIdx.x * SM_THREADS + threadIdx.x;
    const int ncells = ints[SM_NCELLS];
    if (cell == 0) {
        const int nref = ints[SM_NREF];
        info[0] = keep_unref ? ncells : nref;
        info[1] = ints[SM_NFACES];
        info[2] = counts[SM_BAD_V]; info[3] = counts[SM_BAD_F]; info[4] = counts[SM_COLLAPSED]; info[5] = counts[SM_DUPLICATES];
        info[6] = ncells - nref;
    }
    if (cell >= V || cell >= ncells) return;
    const int64_t o = keep_unref ? cell : (ref[cell] ? (int64_t)rexcl[cell] : -1);
    if (o < 0) return;
    float* out = vertices_out + o * C;
    if (nearest) {
        const uint32_t* row = (const uint32_t*)vertices + (int64_t)(uint32_t)best[cell] * C;        // the member's row, bit for bit
        for (int j = 0; j < C; ++j) ((uint32_t*)out)[j] = row[j];
    } else {
        const int64_t* s = sums + cell * (C + 1);
        for (int j = 0; j < C; ++j) out[j] = sm_mean(s, j, C);
    }
}

// ---------------------------------------------------------------------------------------------- C entry points
static bool sm_size_ok(int64_t n) { return n >= 0 && n <= 0x7FFFFFFFll; }
static bool sm_channels_ok(int C) { return C >= 3 && C <= SD3D_SIMPLIFY_MAX_CHANNELS; }

extern "C" size_t sd3d_simplify_ws_bytes(int64_t n_vertices, int64_t n_faces, int n_channels) {
    if (!sm_size_ok(n_vertices) || !sm_size_ok(n_faces) || !sm_channels_ok(n_channels)) return 0;
    return sm_ws(nullptr, n_vertices, n_faces, n_channels).total;
}

extern "C" int sd3d_simplify_mesh(const float* vertices, int64_t n_vertices, int n_channels, const int32_t* faces, int64_t n_faces, float inv_cell,
                                  int nearest, int keep_unreferenced, float* vertices_out, int32_t* faces_out, int32_t* vertex_map,
                                  int32_t* face_source, int64_t* info, void* ws, size_t ws_bytes, void* stream) {
    const int64_t V = n_vertices, F = n_faces;
    const int C = n_channels;
    if (!sm_size_ok(V) || !sm_size_ok(F)) return sd3d_set_error(SD3D_ERR_ARG, "simplify_mesh: 0 <= n_vertices, n_faces < 2^31");
    if (!sm_channels_ok(C)) return sd3d_set_error(SD3D_ERR_ARG, "simplify_mesh: 3 <= n_channels <= 11");
    if (!(inv_cell > 0.0f) || !(inv_cell <= 64.0f)) return sd3d_set_error(SD3D_ERR_ARG, "simplify_mesh: 0 < inv_cell <= 64 (cell >= 2^-6)");
    if (!info) return sd3d_set_error(SD3D_ERR_ARG, "simplify_mesh: info is required");
    if (!ws || ((uintptr_t)ws & 255) != 0) return sd3d_set_error(SD3D_ERR_ARG, "simplify_mesh: ws is required and must be 256-byte aligned");
    const SmWs w = sm_ws(ws, V, F, C);
    if (ws_bytes < w.total) return sd3d_set_error(SD3D_ERR_WS, "simplify_mesh: workspace too small (sd3d_simplify_ws_bytes)");
    if ((V > 0 && (!vertices || !vertices_out || !vertex_map)) || (F > 0 && (!faces || !faces_out || !face_source)))
        return sd3d_set_error(SD3D_ERR_ARG, "simplify_mesh: NULL argument");
    const hipStream_t st = (hipStream_t)stream;
    bool ok = hipMemsetAsync(w.ints, 0, 16, st) == hipSuccess && hipMemsetAsync(w.counts, 0, 32, st) == hipSuccess;
    if (V > 0) {
        ok = ok && hipMemsetAsync(w.sums, 0, (size_t)V * (C + 1) * 8, st) == hipSuccess && hipMemsetAsync(w.ref, 0, (size_t)V * 4, st) == hipSuccess;
        if (nearest) ok = ok && hipMemsetAsync(w.best, 0xFF, (size_t)V * 8, st) == hipSuccess;
    }
    if (F > 0) ok = ok && hipMemsetAsync(w.keep, 0, (size_t)F * 4, st) == hipSuccess;
    if (!ok) return sd3d_set_error(SD3D_ERR_LAUNCH, "simplify_mesh: hipMemsetAsync failed");
    const dim3 block(SM_THREADS), vgrid((unsigned)cdiv(V > 0 ? V : 1, SM_THREADS)), fgrid((unsigned)cdiv(F > 0 ? F : 1, SM_THREADS));
    if (V > 0) {
        hipLaunchKernelGGL(sm_vkey_kernel, dim3(sm_item_blocks(V)), block, 0, st, vertices, V, C, inv_cell, w.keys_a, w.counts);
        int landed = 0;
        if (int rc = sort_pairs_u64(w.keys_a, nullptr, w.keys_b, w.idx_b, V, 0, 64, w.sort_ws, w.sort_bytes, st, w.idx_a, &landed)) return rc;
        const uint64_t* keys = landed ? w.keys_a : w.keys_b;
        const uint32_t* idx = landed ? w.idx_a : w.idx_b;
        hipLaunchKernelGGL(sm_vheads_kernel, vgrid, block, 0, st, keys, V, w.vhead);
        if (int rc = scan_exclusive_i32(w.vhead, w.vexcl, V, nullptr, &w.ints[SM_NCELLS], w.scan_ws, w.scan_bytes, st)) return rc;
        hipLaunchKernelGGL(sm_reduce_kernel, vgrid, block, 0, st, vertices, V, C, keys, idx, w.vhead, w.vexcl, vertex_map, w.sums);
        if (nearest) hipLaunchKernelGGL(sm_nearest_kernel, vgrid, block, 0, st, vertices, V, C, idx, vertex_map, w.sums, w.best);
        SD3D_CHECK_LAUNCH();
    }
    if (F > 0) {
        hipLaunchKernelGGL(sm_fkey_kernel, dim3(sm_item_blocks(F)), block, 0, st, faces, F, V, vertex_map, w.keys_a, w.counts);
        int landed = 0;
        if (int rc = sort_pairs_u64(w.keys_a, nullptr, w.keys_b, w.idx_b, F, 0, 64, w.sort_ws, w.sort_bytes, st, w.idx_a, &landed)) return rc;
        hipLaunchKernelGGL(sm_fheads_kernel, dim3(sm_item_blocks(F)), block, 0, st, landed ? w.keys_a : w.keys_b, landed ? w.idx_a : w.idx_b, F, V, w.keep, w.ref,
                           w.counts);
        if (int rc = scan_exclusive_i32(w.keep, w.fexcl, F, nullptr, &w.ints[SM_NFACES], w.scan_ws, w.scan_bytes, st)) return rc;
    }
    if (V > 0)
        if (int rc = scan_exclusive_i32(w.ref, w.rexcl, V, nullptr, &w.ints[SM_NREF], w.scan_ws, w.scan_bytes, st)) return rc;
    if (F > 0)
        hipLaunchKernelGGL(sm_faces_kernel, fgrid, block, 0, st, faces, F, V, vertex_map, w.keep, w.fexcl, w.rexcl, keep_unreferenced, faces_out,
                           face_source);
    if (V > 0 && !keep_unreferenced) hipLaunchKernelGGL(sm_vmap_kernel, vgrid, block, 0, st, V, w.ref, w.rexcl, vertex_map);
    hipLaunchKernelGGL(sm_cells_kernel, vgrid, block, 0, st, vertices, V, C, nearest, keep_unreferenced, w.sums, w.best, w.ref, w.rexcl, w.ints,
                       w.counts, vertices_out, info);
    SD3D_CHECK_LAUNCH();
    return SD3D_OK;
}
