// A triangle mesh rasterised into posed views: per pixel the depth of the nearest face, that face, and the face's corner nearest the
// pixel, plus label channels read through either (the rule: include/segdino3d_hip.h, "Mesh rasteriser"; segdino3d_amd/raster.py has it
// in full).  It is what turns a mesh and a pose back into the fp32 depth image a `lift2d.Views` takes, for frames that have no depth.
// The reference has no counterpart, so tests/raster_ref.py - a numpy restatement of the rule - is what these kernels are pinned
// against, bit for bit.
//
// Every coordinate is touched by the functions of raster_rule.h and by nothing else.  The image is a minimum over a SET of keys
// (bits of d << 32) | face, so it is a pure function of mesh, cameras and rule: nothing depends on the order of the faces in flight, on
// the cut of the views into calls or passes, or on the stream.  The only atomics on global memory are the 64-bit integer minimum of
// the keys and integer sums of the counters.
//
// One pass = at most `views_per_pass` views that share one key buffer uint64 [views, H, W]:
//   raster_setup_kernel       one lane per (view, face): steps 1 to 4 up to the bounding box, the class of the pair.  The classes are
//                             counted with one ballot per class and one atomic per wave and class.  A drawn pair becomes a record
//                             (view << 32 | face): one ballot and one atomic per wave and size class, small records from the front of
//                             the list, large ones from its back, so one list of views x F records serves both.
//   raster_draw_small_kernel  one lane per small record (clamped bounding box of at most SD3D_RASTER_SMALL_MAX_PIXELS pixels) walks
//                             its box and issues one atomicMin per covered, in-range sample.
//   raster_draw_large_kernel  one wave per large record, the lanes strided over the box: a wall-sized triangle does not serialise on
//                             one lane.  The same sample function, the same keys.
//   raster_resolve_kernel     one lane per pixel: key -> depth, face; the weights recomputed for the winning face -> vertex; labels.
// The draw kernels take their record counts from the device (grid-stride loops over a fixed grid): nothing here reads the device.
// A record holds no coordinate: the draw kernels run the setup function again, 3 vertex loads against a walk over the box.
// All values are written with plain vector stores.
#include "common.h"
// The kernels here must EQUAL the restatement, so nothing in this file may be contracted into a fused multiply-add (see
// fuse_views.hip).  The pragma covers raster_rule.h as it is compiled here.
#pragma clang fp contract(off)
#include "raster_rule.h"
#include "../../include/segdino3d_hip.h"
#include <stdio.h>

#define RS_THREADS 256
#define RS_NO_KEY 0xFFFFFFFFFFFFFFFFull
#define RS_SMALL_BLOCKS 8192                            // the fixed grids of the draw kernels (they loop over the records)
#define RS_LARGE_BLOCKS 4096
#define RS_INFO_PIXELS 5

struct RsMesh {
    const float* vertices;                              // [Nv, 3]
    const int32_t* faces;                               // [F, 3]
    const float *world_to_cam, *intrinsics;             // [V, 12], [V, 4]
    int64_t Nv, F;
    float near, far;
    int H, W;
};
struct RsOut {
    const int32_t *face_labels, *vertex_labels;         // [Lf, F], [Lv, Nv] or NULL
    float* depth;                                       // [V, H, W] or NULL
    int32_t *face, *vertex, *face_labels_out, *vertex_labels_out;       // [V, H, W] or NULL, [L, V, H, W] or NULL
    int64_t pitch;                                      // V H W: the pitch of a label channel
    int Lf, Lv;
    int32_t fill;
};
struct RsWs {
    uint64_t* keys;                                     // [views_per_pass, H, W]
    uint64_t* records;                                  // [views_per_pass * F]: small from the front, large from the back
    uint32_t* counts;                                   // n_small, n_large
    int64_t capacity;                                   // records
    size_t total_bytes;
};

static RsWs rs_ws(void* ws, int64_t F, int views, int H, int W) {
    RsWs w;
    char* p = (char*)ws;
    size_t off = 0;
    w.capacity = (int64_t)views * F;
    w.keys = (uint64_t*)(p + off); off += align_up((size_t)views * H * W * 8, 256);
    w.records = (uint64_t*)(p + off); off += align_up((size_t)(w.capacity > 0 ? w.capacity : 1) * 8, 256);
    w.counts = (uint32_t*)(p + off); off += 256;
    w.total_bytes = off;
    return w;
}

// the rank of this lane among the set bits of `bal`, and their number
__device__ __forceinline__ int rs_rank(unsigned long long bal, int lane) { return __popcll(bal & ((1ull << lane) - 1ull)); }

__global__ __launch_bounds__(RS_THREADS) void raster_setup_kernel(RsMesh m, int v0, int views, RsWs w, int64_t* __restrict__ info) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x, n = (int64_t)views * m.F;
    int cls = -1;
    bool small = false;
    uint64_t rec = 0;
    if (i < n) {
        const int vl = (int)(i / m.F);
        const int64_t f = i - (int64_t)vl * m.F;
        const RasterView c = raster_view(m.world_to_cam, m.intrinsics, v0 + vl);
        RasterTri t;
        cls = raster_setup(m.vertices, m.Nv, m.faces, f, c, m.near, m.H, m.W, t);
        if (cls == RASTER_DRAWN) small = raster_box_pixels(t) <= SD3D_RASTER_SMALL_MAX_PIXELS;
        rec = ((uint64_t)vl << 32) | (uint64_t)f;
    }
    // the counters: integer sums, one atomic per wave and class that occurs
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const unsigned long long bal = __ballot(cls == k);
        if (lane == 0 && bal) atomicAdd((unsigned long long*)&info[k], (unsigned long long)__popcll(bal));
    }
    // the records: one atomic per wave and size class
    const bool drawn = cls == RASTER_DRAWN;
    const unsigned long long bs = __ballot(drawn && small), bl = __ballot(drawn && !small);
    uint32_t base_s = 0, base_l = 0;
    if (lane == 0) {
        if (bs) base_s = atomicAdd(&w.counts[0], (uint32_t)__popcll(bs));
        if (bl) base_l = atomicAdd(&w.counts[1], (uint32_t)__popcll(bl));
    }
    base_s = __shfl(base_s, 0); base_l = __shfl(base_l, 0);
    // small + large <= views * F = capacity: the two ends cannot meet
    if (drawn && small) w.records[(int64_t)base_s + rs_rank(bs, lane)] = rec;
    if (drawn && !small) w.records[w.capacity - 1 - ((int64_t)base_l + rs_rank(bl, lane))] = rec;
}

// the record's triangle again, by the function that classified it
__device__ __forceinline__ bool rs_record(const RsMesh& m, int v0, uint64_t rec, RasterTri& t, int& vl, uint32_t& f) {
    vl = (int)(rec >> 32); f = (uint32_t)rec;
    const RasterView c = raster_view(m.world_to_cam, m.intrinsics, v0 + vl);
    return raster_setup(m.vertices, m.Nv, m.faces, (int64_t)f, c, m.near, m.H, m.W, t) == RASTER_DRAWN;
}

__global__ __launch_bounds__(RS_THREADS) void raster_draw_small_kernel(RsMesh m, int v0, RsWs w) {
    const int64_t n = (int64_t)w.counts[0], step = (int64_t)gridDim.x * RS_THREADS;
    const int64_t hw = (int64_t)m.H * m.W;
    for (int64_t i = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x; i < n; i += step) {
        RasterTri t;
        int vl;
        uint32_t f;
        if (!rs_record(m, v0, w.records[i], t, vl, f)) continue;
        uint64_t* img = w.keys + (int64_t)vl * hw;
        for (int vi = t.y0; vi <= t.y1; ++vi)
            for (int ui = t.x0; ui <= t.x1; ++ui) {
                uint64_t key;
                if (raster_sample(t, ui, vi, m.near, m.far, f, key)) atomicMin((unsigned long long*)&img[(int64_t)vi * m.W + ui], (unsigned long long)key);
            }
    }
}

__global__ __launch_bounds__(RS_THREADS) void raster_draw_large_kernel(RsMesh m, int v0, RsWs w) {
    const int lane = threadIdx.x & 63;
    const int64_t n = (int64_t)w.counts[1], step = (int64_t)gridDim.x * (RS_THREADS / 64);
    const int64_t hw = (int64_t)m.H * m.W;
    for (int64_t i = (int64_t)blockIdx.x * (RS_THREADS / 64) + (threadIdx.x >> 6); i < n; i += step) {
        RasterTri t;
        int vl;
        uint32_t f;
        if (!rs_record(m, v0, w.records[w.capacity - 1 - i], t, vl, f)) continue;       // wave-uniform
        uint64_t* img = w.keys + (int64_t)vl * hw;
        const int bw = t.x1 - t.x0 + 1;
        const int64_t area = raster_box_pixels(t);
        for (int64_t p = lane; p < area; p += 64) {
            const int row = (int)(p / bw), ui = t.x0 + (int)(p - (int64_t)row * bw), vi = t.y0 + row;
            uint64_t key;
            if (raster_sample(t, ui, vi, m.near, m.far, f, key)) atomicMin((unsigned long long*)&img[(int64_t)vi * m.W + ui], (unsigned long long)key);
        }
    }
}

__global__ __launch_bounds__(RS_THREADS) void raster_resolve_kernel(RsMesh m, int v0, int views, RsWs w, RsOut o, int64_t* __restrict__ info) {
    const int lane = threadIdx.x & 63;
    const int64_t hw = (int64_t)m.H * m.W, n = (int64_t)views * hw;
    const int64_t i = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x;
    bool hit = false;
    if (i < n) {
        const uint64_t key = w.keys[i];
        hit = key != RS_NO_KEY;
        const int vl = (int)(i / hw);
        const int64_t pix = i - (int64_t)vl * hw, at = (int64_t)(v0 + vl) * hw + pix;
        const int32_t face = hit ? (int32_t)(uint32_t)key : -1;
        if (o.depth) o.depth[at] = hit ? __uint_as_float((uint32_t)(key >> 32)) : 0.0f;
        if (o.face) o.face[at] = face;
        for (int l = 0; l < o.Lf; ++l) o.face_labels_out[(int64_t)l * o.pitch + at] = hit ? o.face_labels[(int64_t)l * m.F + face] : o.fill;
        if (o.vertex || o.Lv > 0) {
            int32_t vertex = -1;
            if (hit) {
                const int vi = (int)(pix / m.W), ui = (int)(pix - (int64_t)vi * m.W);
                const RasterView c = raster_view(m.world_to_cam, m.intrinsics, v0 + vl);
                RasterTri t;
                int64_t wt[3];
                raster_setup(m.vertices, m.Nv, m.faces, (int64_t)face, c, m.near, m.H, m.W, t);   // a face that won a pixel is a drawn one
                raster_weights(t, ui, vi, wt);
                const int k = raster_corner(wt);
                vertex = k == 0 ? t.idx[0] : k == 1 ? t.idx[1] : t.idx[2];             // no dynamic index: the triangle stays in registers
            }
            if (o.vertex) o.vertex[at] = vertex;
            for (int l = 0; l < o.Lv; ++l)
                o.vertex_labels_out[(int64_t)l * o.pitch + at] = hit ? o.vertex_labels[(int64_t)l * m.Nv + vertex] : o.fill;
        }
    }
    const unsigned long long bal = __ballot(hit);
    if (lane == 0 && bal) atomicAdd((unsigned long long*)&info[RS_INFO_PIXELS], (unsigned long long)__popcll(bal));
}

// ---------------------------------------------------------------------------------------------- C entry points
static bool rs_size_ok(int64_t n) { return n >= 0 && n <= 0x7FFFFFFFll; }
static bool rs_image_ok(int H, int W) { return H >= 1 && H <= 16384 && W >= 1 && W <= 16384; }
// one pass: its (view, face) pairs must fit the 32-bit record counts, its pixels the grid of the resolve kernel
static bool rs_pass_ok(int64_t F, int views, int H, int W) {
    return views >= 1 && (int64_t)views * F <= 0x7FFFFFFFll && cdiv((int64_t)views * H * W, RS_THREADS) <= 0x7FFFFFFFll;
}

extern "C" size_t sd3d_raster_ws_bytes(int64_t n_faces, int views_per_pass, int H, int W) {
    if (!rs_size_ok(n_faces) || !rs_image_ok(H, W) || !rs_pass_ok(n_faces, views_per_pass, H, W)) return 0;
    return rs_ws(nullptr, n_faces, views_per_pass, H, W).total_bytes;
}

extern "C" int sd3d_raster_views(const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, const float* world_to_cam,
                                 const float* intrinsics, int V, int H, int W, float near, float far, int views_per_pass,
                                 const int32_t* face_labels, int n_face_labels, const int32_t* vertex_labels, int n_vertex_labels, int fill,
                                 float* depth_out, int32_t* face_out, int32_t* vertex_out, int32_t* face_labels_out, int32_t* vertex_labels_out,
                                 int64_t* info, void* ws, size_t ws_bytes, void* stream) {
    if (!rs_size_ok(n_vertices) || !rs_size_ok(n_faces)) return sd3d_set_error(SD3D_ERR_ARG, "raster_views: 0 <= n_vertices, n_faces < 2^31");
    if (V < 0 || !rs_image_ok(H, W)) return sd3d_set_error(SD3D_ERR_ARG, "raster_views: V >= 0 and images of 1 .. 16384 a side");
    if (!(near > 0.0f) || !(far >= near)) return sd3d_set_error(SD3D_ERR_ARG, "raster_views: 0 < near <= far");
    if (views_per_pass < 1) return sd3d_set_error(SD3D_ERR_ARG, "raster_views: views_per_pass >= 1");
    if (n_face_labels < 0 || n_vertex_labels < 0 || n_face_labels + n_vertex_labels > SD3D_RASTER_MAX_LABELS)
        return sd3d_set_error(SD3D_ERR_ARG, "raster_views: n_face_labels, n_vertex_labels >= 0 and at most 8 label channels together");
    if (!info) return sd3d_set_error(SD3D_ERR_ARG, "raster_views: info is required");
    const hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(info, 0, SD3D_RASTER_INFO_WORDS * sizeof(int64_t), st) != hipSuccess)
        return sd3d_set_error(SD3D_ERR_LAUNCH, "raster_views: hipMemsetAsync failed");
    if (V == 0) return SD3D_OK;
    const int per_pass = views_per_pass < V ? views_per_pass : V;
    if (!rs_pass_ok(n_faces, per_pass, H, W))
        return sd3d_set_error(SD3D_ERR_ARG, "raster_views: views_per_pass * n_faces must stay below 2^31 (and the pixels of a pass below 2^39); lower views_per_pass");
    if (!ws || ((uintptr_t)ws & 255) != 0) return sd3d_set_error(SD3D_ERR_ARG, "raster_views: ws is required and must be 256-byte aligned");
    const RsWs w = rs_ws(ws, n_faces, per_pass, H, W);
    if (ws_bytes < w.total_bytes) return sd3d_set_error(SD3D_ERR_WS, "raster_views: workspace too small (sd3d_raster_ws_bytes)");
    if (!world_to_cam || !intrinsics || (n_faces > 0 && !faces) || (n_faces > 0 && n_vertices > 0 && !vertices))
        return sd3d_set_error(SD3D_ERR_ARG, "raster_views: NULL argument");
    if ((n_face_labels > 0 && (!face_labels_out || (n_faces > 0 && !face_labels))) ||
        (n_vertex_labels > 0 && (!vertex_labels_out || (n_vertices > 0 && !vertex_labels))))
        return sd3d_set_error(SD3D_ERR_ARG, "raster_views: labels and their output are required when their number is > 0");
    RsMesh m;
    m.vertices = vertices; m.faces = faces; m.world_to_cam = world_to_cam; m.intrinsics = intrinsics;
    m.Nv = n_vertices; m.F = n_faces; m.near = near; m.far = far; m.H = H; m.W = W;
    RsOut o;
    o.face_labels = face_labels; o.vertex_labels = vertex_labels; o.depth = depth_out; o.face = face_out; o.vertex = vertex_out;
    o.face_labels_out = face_labels_out; o.vertex_labels_out = vertex_labels_out;
    o.pitch = (int64_t)V * H * W; o.Lf = n_face_labels; o.Lv = n_vertex_labels; o.fill = (int32_t)fill;
    const int64_t hw = (int64_t)H * W;
    for (int v0 = 0; v0 < V; v0 += per_pass) {
        const int views = V - v0 < per_pass ? V - v0 : per_pass;
        const int64_t pairs = (int64_t)views * n_faces;
        if (hipMemsetAsync(w.keys, 0xFF, (size_t)views * hw * 8, st) != hipSuccess || hipMemsetAsync(w.counts, 0, 8, st) != hipSuccess)
            return sd3d_set_error(SD3D_ERR_LAUNCH, "raster_views: hipMemsetAsync failed");
        if (pairs > 0) {
            const int64_t small_blocks = cdiv(pairs, RS_THREADS), large_blocks = cdiv(pairs, RS_THREADS / 64);
            hipLaunchKernelGGL(raster_setup_kernel, dim3((unsigned)cdiv(pairs, RS_THREADS)), dim3(RS_THREADS), 0, st, m, v0, views, w, info);
            SD3D_CHECK_LAUNCH();
            hipLaunchKernelGGL(raster_draw_small_kernel, dim3((unsigned)(small_blocks < RS_SMALL_BLOCKS ? small_blocks : RS_SMALL_BLOCKS)),
                               dim3(RS_THREADS), 0, st, m, v0, w);
            SD3D_CHECK_LAUNCH();
            hipLaunchKernelGGL(raster_draw_large_kernel, dim3((unsigned)(large_blocks < RS_LARGE_BLOCKS ? large_blocks : RS_LARGE_BLOCKS)),
                               dim3(RS_THREADS), 0, st, m, v0, w);
            SD3D_CHECK_LAUNCH();
        }
        hipLaunchKernelGGL(raster_resolve_kernel, dim3((unsigned)cdiv((int64_t)views * hw, RS_THREADS)), dim3(RS_THREADS), 0, st, m, v0, views, w, o,
                           info);
        SD3D_CHECK_LAUNCH();
    }
    return SD3D_OK;
}
