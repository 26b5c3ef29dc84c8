// Carrying per-point results onto other points and onto depth frames: the exact nearest source point of a query within a radius (the
// rule: include/segdino3d_hip.h, "Nearest point").  The reference has no counterpart (it evaluates on the points it loaded), so
// tests/transfer_ref.py - a numpy restatement of the rule - is what these kernels are pinned against, bit for bit.
//
// The rule, per query q against the source cloud P [N, 3], r2 = fl32(r r):
//   1. q and a source point are valid iff |c| < 2^14 on all three axes, compared as floats (a NaN or an infinity fails); an invalid
//      query answers -1, an invalid source point is never a candidate;
//   2. dx = P[j].x - q.x (dy, dz alike), d2 = (dx dx + dy dy) + dz dz, one fp32 rounding per operation; j is a candidate iff d2 <= r2;
//   3. the answer is the candidate with the smallest key (bits of d2 << 32) | j: the nearest, ties to the lower index; -1 / +inf if
//      there is none;
//   4. a pixel query is the back-projection of backproject.h of a depth pixel whose depth passes step 2 of the fusion rule
//      (depth_pixel.h, the edge test off);
//   5. out[l, query] = labels[l, idx], or `fill` where idx < 0, written by the kernel that found idx.
// The answer is a minimum over a SET of keys, so it is a pure function of the cloud and the query: nothing depends on the order in
// which candidates are met, on how the views are cut into calls, or on the stream.  No atomics touch global memory.
//
// The grid (point_grid.h, the index sd3d_knn_graph builds) only chooses WHICH source points are evaluated.  It is conservative for the
// cross-set case by the argument of superpoints.hip, which uses nothing but "both points are valid and d2 <= r2": a valid coordinate has
// |c| < 2^14, so c 2^10 is exact in fp32, and u = rint(c 2^10) is an integer with |u - c 2^10| <= 1/2.  If d2 <= r2 then
// fl(dx dx) <= d2 <= r2 = fl(r r) (sums of non-negative terms round monotonically), so |dx| <= r (1 + 2^-23), and the exact difference
// of the two coordinates is within a factor 1 + 2^-24 of its rounding dx: |P[j].x - q.x| <= r (1 + 2^-22) < r + 2^-20 for r <= 4.
// Hence |u_j - u_q| <= 2^10 r + 2^-10 + 1 < ceil(2^10 r) + 2 = H, and with cells of H units, cell = (u + 2^24) / H, the source
// point lies at most one cell from the query's on every axis: the 27 cells around the query's own hold every candidate.  Whether q is
// itself a point of P plays no part.  Cells are hashed into buckets; a bucket may hold points of other cells, and two of the 27 cells
// may share a bucket.  Both only add evaluations: a far point fails d2 <= r2, and a candidate met twice leaves a minimum unchanged, so
// the k-NN kernel's de-duplication of the 27 buckets is not needed here.
//
//   sd3d_point_index_build   knn_key_kernel, sort_pairs_u64, knn_gather_kernel of point_grid.h, once per source cloud, into a
//                            caller-owned workspace; the queries below only read it.
//   sd3d_nearest_points      tq_point_kernel   one thread per query: 27 bucket ranges from global memory, their points one by one.
//   sd3d_nearest_pixels      tq_pixel_kernel   one workgroup of 256 lanes takes a tile of TQ_TILE_H x TQ_TILE_W pixels of one view, one
//                                              pixel per lane.  The pixels of a tile see a patch of one surface, so their 27-cell
//                                              neighbourhoods overlap almost entirely: the tile takes the box of cells around its valid
//                                              queries (a min / max butterfly per wave, then one LDS atomic per wave), and when the box has at most TQ_CELLS cells it looks each
//                                              cell's bucket up ONCE, one cell per lane, and when the ranges hold at most TQ_POINTS points
//                                              it copies them into LDS once.  A lane then walks its 27 cells out of LDS: no hash, no
//                                              global load.  A tile whose box is too large (a depth discontinuity) walks global memory as
//                                              the point form does; a tile whose ranges are too long keeps the ranges in LDS and reads
//                                              the points from global memory.  All three paths evaluate supersets of the candidates and
//                                              take the same minimum.
//   sd3d_instance_map        tq_instance_map_kernel   four points per lane; a mask row is read with one 32-bit load per lane where
//                                              the alignment allows, and a row whose score fails the threshold is not read at all.
// All values are written with plain vector stores.
#include "common.h"
// The kernels here must EQUAL a float32 evaluation of the restatement, so nothing in this file may be contracted into a fused
// multiply-add (see fuse_views.hip).  The pragma covers depth_pixel.h, backproject.h and point_grid.h as they are compiled here.
#pragma clang fp contract(off)
#include "depth_pixel.h"
#include "point_grid.h"
#include <climits>

#define TQ_THREADS 256
#define TQ_TILE_W 32
#define TQ_TILE_H 8
#define TQ_CELLS 512                                    // cells of a tile's box whose bucket ranges are staged in LDS
#define TQ_POINTS 1536                                  // source points of a tile's box staged in LDS (16 bytes each)
#define TQ_NO_KEY 0xFFFFFFFFFFFFFFFFull
#define TQ_MAP_ROWS 8                                   // mask rows the instance map reads before it uses any

struct TqIndex {
    const float4* sorted;                               // [N] (x, y, z, index) in bucket order
    const int32_t *cell_lo, *cell_hi;                   // [B]
    int64_t N;
    int H, bucket_bits;
    float r2;
};
struct TqOut {
    const int32_t* labels;                              // [L, N] or NULL
    int32_t *idx, *out;                                 // [M] or NULL, [L, M] or NULL
    float* d2;                                          // [M] or NULL
    int64_t M, N;                                       // queries = the pitch of `out`; source points = the pitch of `labels`
    int L;
    int32_t fill;
};
struct TqGeom {
    int tiles_x, tiles_per_view;                        // before the rule: what the kernel reads is then one run of 28 bytes
    Sd3dDepthRule px;                                   // use_edges = 0: step 2 alone
};

// the points p[0 .. n) against the query: step 2 and the running minimum of step 3 (P = a global or an LDS pointer, after inlining)
template <typename P>
__device__ __forceinline__ void tq_scan(P p, int n, float qx, float qy, float qz, float r2, uint64_t& best) {
    for (int j = 0; j < n; ++j) {
        const float4 c = p[j];
        const float dx = c.x - qx, dy = c.y - qy, dz = c.z - qz;
        const float d2 = (dx * dx + dy * dy) + dz * dz;                               // >= +0: its bits order as the floats do
        if (d2 <= r2) {
            const uint64_t key = ((uint64_t)__float_as_uint(d2) << 32) | __float_as_uint(c.w);
            best = key < best ? key : best;
        }
    }
}

// the range of bucket b, inside [0, N] whatever the workspace holds
__device__ __forceinline__ void tq_range(const TqIndex& ix, uint32_t b, int& lo, int& n) {
    const int64_t l = ix.cell_lo[b], h = ix.cell_hi[b];
    lo = (int)(l < 0 ? 0 : (l > ix.N ? ix.N : l));
    n = h > ix.N ? (int)(ix.N - lo) : (int)(h - lo);
    if (n < 0) n = 0;
}

__device__ __forceinline__ uint64_t tq_walk_global(const TqIndex& ix, float qx, float qy, float qz) {
    const int cx = knn_cell(qx, ix.H), cy = knn_cell(qy, ix.H), cz = knn_cell(qz, ix.H);
    uint64_t best = TQ_NO_KEY;
    for (int m = 0; m < 27; ++m) {
        const uint32_t b = knn_bucket(cx + m % 3 - 1, cy + (m / 3) % 3 - 1, cz + m / 9 - 1, 0, ix.bucket_bits);
        int lo, n;
        tq_range(ix, b, lo, n);
        tq_scan(ix.sorted + lo, n, qx, qy, qz, ix.r2, best);
    }
    return best;
}

// steps 3 and 5 for query q
__device__ __forceinline__ void tq_emit(const TqOut& o, int64_t q, uint64_t best) {
    const bool none = best == TQ_NO_KEY;
    const int64_t j = (int64_t)(uint32_t)best;                                        // < N: an index the gather stored
    if (o.idx) o.idx[q] = none ? -1 : (int32_t)j;
    if (o.d2) o.d2[q] = none ? __builtin_inff() : __uint_as_float((uint32_t)(best >> 32));
    for (int l = 0; l < o.L; ++l) o.out[(int64_t)l * o.M + q] = none || j >= o.N ? o.fill : o.labels[(int64_t)l * o.N + j];
}

__global__ __launch_bounds__(TQ_THREADS) void tq_point_kernel(const float* __restrict__ queries, TqIndex ix, TqOut o) {
    const int64_t q = (int64_t)blockIdx.x * TQ_THREADS + threadIdx.x;
    if (q >= o.M) return;
    const float x = queries[q * 3], y = queries[q * 3 + 1], z = queries[q * 3 + 2];
    tq_emit(o, q, knn_valid(x, y, z) ? tq_walk_global(ix, x, y, z) : TQ_NO_KEY);
}

template <typename D>
__global__ __launch_bounds__(TQ_THREADS) void tq_pixel_kernel(const D* __restrict__ depth, const float* __restrict__ intr,
                                                              const float* __restrict__ c2w, TqGeom g, TqIndex ix, TqOut o) {
    __shared__ int s_min[3], s_max[3], s_total;
    __shared__ int s_lo[TQ_CELLS], s_len[TQ_CELLS], s_off[TQ_CELLS];
    __shared__ float4 s_pts[TQ_POINTS];
    const int t = threadIdx.x, lane = t & 63;
    const int v = blockIdx.x / g.tiles_per_view, tile = blockIdx.x - v * g.tiles_per_view;
    const int ty = tile / g.tiles_x, tx = tile - ty * g.tiles_x;
    if (t < 3) { s_min[t] = INT_MAX; s_max[t] = INT_MIN; }
    if (t == 0) s_total = 0;
    __syncthreads();

    // ---- step 4: this lane's pixel as a query, and the tile's box of cells
    const int vi = ty * TQ_TILE_H + (t >> 5), ui = tx * TQ_TILE_W + (t & 31);
    const bool inside = vi < g.px.Hd && ui < g.px.Wd;
    bool ok = false;
    float w[3] = {0.0f, 0.0f, 0.0f};
    int c[3] = {0, 0, 0};
    if (inside) {
        float d;
        ok = sd3d_depth_pixel<false>(depth + (int64_t)v * g.px.Hd * g.px.Wd, g.px, vi, ui, d);
        if (ok) {
            const Sd3dCamera cam = sd3d_load_camera(intr, c2w, v);
            sd3d_backproject(cam, vi, ui, d, w[0], w[1], w[2]);
            ok = knn_valid(w[0], w[1], w[2]);
        }
        if (ok) {
#pragma unroll
            for (int i = 0; i < 3; ++i) c[i] = knn_cell(w[i], ix.H);
        }
    }
    // the box: a butterfly over the wave first, so that one lane per wave touches the shared words (256 atomics on one LDS address
    // take their turns one by one)
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int lo = wave_min(ok ? c[i] : INT_MAX), hi = wave_max(ok ? c[i] : INT_MIN);
        if (lane == 0 && lo <= hi) {
            atomicMin(&s_min[i], lo);
            atomicMax(&s_max[i], hi);
        }
    }
    __syncthreads();
    // everything from here to the walk is uniform over the workgroup
    const int x0 = s_min[0] - 1, y0 = s_min[1] - 1, z0 = s_min[2] - 1;
    const bool any = s_min[0] <= s_max[0];
    const int nx = any ? s_max[0] - s_min[0] + 3 : 0, ny = any ? s_max[1] - s_min[1] + 3 : 0, nz = any ? s_max[2] - s_min[2] + 3 : 0;
    const bool small = any && nx <= TQ_CELLS && ny <= TQ_CELLS && nz <= TQ_CELLS && nx * ny * nz <= TQ_CELLS;   // each <= 2^9 first: no overflow
    const int ncell = small ? nx * ny * nz : 0;
    bool staged = false;
    if (small) {
        for (int k0 = 0; k0 < ncell; k0 += TQ_THREADS) {                               // whole waves: the scan needs every lane
            const int k = k0 + t;
            int lo = 0, n = 0;
            if (k < ncell) {
                const int kx = k % nx, ky = (k / nx) % ny, kz = k / (nx * ny);
                tq_range(ix, knn_bucket(x0 + kx, y0 + ky, z0 + kz, 0, ix.bucket_bits), lo, n);
                s_lo[k] = lo;
                s_len[k] = n;
            }
            // room in the tile's copy: a scan over the wave, then one add per wave.  The sum only decides whether the points fit: a long
            // range counts as "too many", which keeps it far below 2^31.  The order of the copy is of no account to a minimum.
            const int want = n > TQ_POINTS ? TQ_POINTS + 1 : n;
            const int incl = wave_scan_incl(want, lane);
            int base = 0;
            if (lane == 63 && incl > 0) base = atomicAdd(&s_total, incl);
            base = __shfl(base, 63);
            if (k < ncell) s_off[k] = base + incl - want;
        }
        __syncthreads();
        staged = s_total <= TQ_POINTS;                  // then no range was cut short and every s_off[k] + s_len[k] <= TQ_POINTS
        if (staged) {
            for (int k = t; k < ncell; k += TQ_THREADS) {
                const int n = s_len[k], off = s_off[k];
                const float4* src = ix.sorted + s_lo[k];
                for (int j = 0; j < n; ++j) s_pts[off + j] = src[j];
            }
            __syncthreads();
        }
    }

    // ---- steps 1 to 3 over the 27 cells around the query's own
    uint64_t best = TQ_NO_KEY;
    if (ok) {
        if (!small) {
            best = tq_walk_global(ix, w[0], w[1], w[2]);
        } else {
            const int lx = c[0] - x0, ly = c[1] - y0, lz = c[2] - z0;                 // 1 <= lx <= nx - 2: the box has a rim of one cell
            for (int m = 0; m < 9; ++m) {
                const int row = ((lz + m / 3 - 1) * ny + (ly + m % 3 - 1)) * nx + lx - 1;
#pragma unroll
                for (int e = 0; e < 3; ++e) {
                    const int n = s_len[row + e];
                    if (n == 0) continue;
                    if (staged) tq_scan(&s_pts[s_off[row + e]], n, w[0], w[1], w[2], ix.r2, best);
                    else tq_scan(ix.sorted + s_lo[row + e], n, w[0], w[1], w[2], ix.r2, best);
                }
            }
        }
    }
    if (inside) tq_emit(o, ((int64_t)v * g.px.Hd + vi) * g.px.Wd + ui, best);
}

// map[n] = the i with masks[i, n] set and scores[i] >= thr of the largest score, ties to the lower i, -1 if none; `vec`: N % 4 == 0 and
// masks 4-byte aligned, so that the four bytes of a lane are one load
__global__ __launch_bounds__(256) void tq_instance_map_kernel(const uint8_t* __restrict__ masks, const float* __restrict__ scores, int I,
                                                              int64_t N, float thr, int vec, int32_t* __restrict__ map) {
    const int64_t n0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (n0 >= N) return;
    int best[4] = {-1, -1, -1, -1};
    float top[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    int i = 0;
    // 150 k points are 2 waves per CU: the loop, not the wave count, must keep loads in flight, so eight rows are read before any is used
    for (; vec && i + TQ_MAP_ROWS <= I; i += TQ_MAP_ROWS) {
        uint32_t bits[TQ_MAP_ROWS];
        float s[TQ_MAP_ROWS];
#pragma unroll
        for (int u = 0; u < TQ_MAP_ROWS; ++u) {
            s[u] = scores[i + u];                                                     // uniform
            bits[u] = s[u] >= thr ? *(const uint32_t*)(masks + (int64_t)(i + u) * N + n0) : 0u;   // a NaN score: the row is not read
        }
#pragma unroll
        for (int u = 0; u < TQ_MAP_ROWS; ++u)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (((bits[u] >> (8 * e)) & 0xFFu) != 0 && (best[e] < 0 || s[u] > top[e])) { best[e] = i + u; top[e] = s[u]; }
    }
    for (; i < I; ++i) {
        const float s = scores[i];                                                    // uniform
        if (!(s >= thr)) continue;                                                    // a NaN score stops here; the row is not read
        const uint8_t* row = masks + (int64_t)i * N + n0;
        uint32_t bits = 0;
        if (vec) {
            bits = *(const uint32_t*)row;
        } else {
            for (int e = 0; e < 4; ++e)
                if (n0 + e < N) bits |= (uint32_t)row[e] << (8 * e);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (((bits >> (8 * e)) & 0xFFu) != 0 && (best[e] < 0 || s > top[e])) { best[e] = i; top[e] = s; }
    }
    for (int e = 0; e < 4; ++e)
        if (n0 + e < N) map[n0 + e] = best[e];
}

// ---------------------------------------------------------------------------------------------- C entry points
static bool tq_size_ok(int64_t n) { return n >= 0 && n <= 0x7FFFFFFFll; }
static bool tq_radius_ok(float r) { return r > 0.0f && r <= 4.0f; }

extern "C" size_t sd3d_point_index_ws_bytes(int64_t n_points) { return tq_size_ok(n_points) ? knn_ws(nullptr, n_points).total_bytes : 0; }

static int tq_index(const char* who, const void* ws, size_t ws_bytes, int64_t N, float radius, TqIndex& ix) {
    char msg[160];                                      // sd3d_set_error copies it
    if (!tq_size_ok(N) || !tq_radius_ok(radius)) {
        snprintf(msg, sizeof msg, "%s: 0 <= n_points < 2^31, 0 < radius <= 4", who);
        return sd3d_set_error(SD3D_ERR_ARG, msg);
    }
    if (!ws || ((uintptr_t)ws & 255) != 0) {
        snprintf(msg, sizeof msg, "%s: ws is required and must be 256-byte aligned", who);
        return sd3d_set_error(SD3D_ERR_ARG, msg);
    }
    const KnnWs w = knn_ws(const_cast<void*>(ws), N);
    if (ws_bytes < w.total_bytes) {
        snprintf(msg, sizeof msg, "%s: workspace too small (sd3d_point_index_ws_bytes)", who);
        return sd3d_set_error(SD3D_ERR_WS, msg);
    }
    ix.sorted = w.sorted; ix.cell_lo = w.cell_lo; ix.cell_hi = w.cell_hi;
    ix.N = N; ix.H = knn_cell_units(radius); ix.bucket_bits = knn_bucket_bits(N);
    ix.r2 = radius * radius;
    return SD3D_OK;
}

static int tq_out(const char* who, int64_t M, int64_t N, const int32_t* labels, int n_labels, int fill, int32_t* idx_out, float* d2_out,
                  int32_t* labels_out, TqOut& o) {
    char msg[160];
    if (n_labels < 0 || n_labels > SD3D_NEAREST_MAX_LABELS) {
        snprintf(msg, sizeof msg, "%s: 0 <= n_labels <= 8", who);
        return sd3d_set_error(SD3D_ERR_ARG, msg);
    }
    if (n_labels > 0 && M > 0 && (!labels_out || (N > 0 && !labels))) {
        snprintf(msg, sizeof msg, "%s: labels and labels_out are required when n_labels > 0", who);
        return sd3d_set_error(SD3D_ERR_ARG, msg);
    }
    o.labels = labels; o.idx = idx_out; o.out = labels_out; o.d2 = d2_out;
    o.M = M; o.N = N; o.L = n_labels; o.fill = (int32_t)fill;
    return SD3D_OK;
}

extern "C" int sd3d_point_index_build(const float* points, int64_t n_points, float radius, void* ws, size_t ws_bytes, void* stream) {
    TqIndex ix;
    if (int rc = tq_index("point_index_build", ws, ws_bytes, n_points, radius, ix)) return rc;
    if (n_points > 0 && !points) return sd3d_set_error(SD3D_ERR_ARG, "point_index_build: NULL argument");
    const uint64_t* keys = nullptr;
    return knn_build_index(points, nullptr, 1, n_points, ix.H, ix.bucket_bits, knn_ws(ws, n_points), (hipStream_t)stream, &keys);
}

extern "C" int sd3d_nearest_points(const float* queries, int64_t n_queries, const void* index_ws, size_t ws_bytes, int64_t n_points,
                                   float radius, const int32_t* labels, int n_labels, int fill, int32_t* idx_out, float* d2_out,
                                   int32_t* labels_out, void* stream) {
    TqIndex ix;
    TqOut o;
    if (int rc = tq_index("nearest_points", index_ws, ws_bytes, n_points, radius, ix)) return rc;
    if (!tq_size_ok(n_queries)) return sd3d_set_error(SD3D_ERR_ARG, "nearest_points: 0 <= n_queries < 2^31");
    if (int rc = tq_out("nearest_points", n_queries, n_points, labels, n_labels, fill, idx_out, d2_out, labels_out, o)) return rc;
    if (n_queries == 0) return SD3D_OK;
    if (!queries) return sd3d_set_error(SD3D_ERR_ARG, "nearest_points: NULL argument");
    hipLaunchKernelGGL(tq_point_kernel, dim3((unsigned)cdiv(n_queries, TQ_THREADS)), dim3(TQ_THREADS), 0, (hipStream_t)stream, queries, ix, o);
    SD3D_CHECK_LAUNCH();
    return SD3D_OK;
}

extern "C" int sd3d_nearest_pixels(const void* depth, int depth_u16, float depth_scale, const float* intrinsics, const float* cam_to_world,
                                   int V, int Hd, int Wd, float near, float far, const void* index_ws, size_t ws_bytes, int64_t n_points,
                                   float radius, const int32_t* labels, int n_labels, int fill, int32_t* idx_out, float* d2_out,
                                   int32_t* labels_out, void* stream) {
    TqIndex ix;
    TqOut o;
    if (int rc = tq_index("nearest_pixels", index_ws, ws_bytes, n_points, radius, ix)) return rc;
    TqGeom g;
    if (int rc = sd3d_depth_rule("nearest_pixels", depth_u16, depth_scale, Hd, Wd, near, far, 0.0f, 0.0f, 0, g.px)) return rc;
    if (V < 0) return sd3d_set_error(SD3D_ERR_ARG, "nearest_pixels: V >= 0");
    g.tiles_x = (Wd + TQ_TILE_W - 1) / TQ_TILE_W;
    g.tiles_per_view = g.tiles_x * ((Hd + TQ_TILE_H - 1) / TQ_TILE_H);
    // V Hd Wd < 2^31 2^28 and L <= 8: the int64 indices of the outputs cannot overflow; the grid is what limits one call
    const int64_t blocks = (int64_t)V * g.tiles_per_view, M = (int64_t)V * Hd * Wd;
    if (blocks > 0x7FFFFFFFll) return sd3d_set_error(SD3D_ERR_ARG, "nearest_pixels: more than 2^31 - 1 tiles in one call; cut the views into several");
    if (int rc = tq_out("nearest_pixels", M, n_points, labels, n_labels, fill, idx_out, d2_out, labels_out, o)) return rc;
    if (V == 0) return SD3D_OK;
    if (!depth || !intrinsics || !cam_to_world) return sd3d_set_error(SD3D_ERR_ARG, "nearest_pixels: NULL argument");
    const dim3 grid((unsigned)blocks), block(TQ_THREADS);
    SD3D_LAUNCH_DEPTH(tq_pixel_kernel, grid, block, (hipStream_t)stream, depth_u16, depth, intrinsics, cam_to_world, g, ix, o);
    SD3D_CHECK_LAUNCH();
    return SD3D_OK;
}

extern "C" int sd3d_instance_map(const void* masks, const float* scores, int n_instances, int64_t n_points, float score_thr, int32_t* map,
                                 void* stream) {
    if (n_instances < 0 || !tq_size_ok(n_points) || score_thr != score_thr)
        return sd3d_set_error(SD3D_ERR_ARG, "instance_map: n_instances >= 0, 0 <= n_points < 2^31, score_thr not a NaN");
    if (n_points == 0) return SD3D_OK;
    if (!map || (n_instances > 0 && (!masks || !scores))) return sd3d_set_error(SD3D_ERR_ARG, "instance_map: NULL argument");
    const int vec = n_points % 4 == 0 && ((uintptr_t)masks & 3) == 0;
    hipLaunchKernelGGL(tq_instance_map_kernel, dim3((unsigned)cdiv(cdiv(n_points, 4), 256)), dim3(256), 0, (hipStream_t)stream,
                       (const uint8_t*)masks, scores, n_instances, n_points, score_thr, vec, map);
    SD3D_CHECK_LAUNCH();
    return SD3D_OK;
}
