// 3D box AP / AR of `instance_boxes` accumulated and scored on the device: the VOC-style indoor detection protocol for axis-aligned
// boxes (what mmdet3d's `indoor_eval` computes), stated in include/segdino3d_hip.h and restated in numpy by tests/box_ap_ref.py.
//
//   sd3d_gt_boxes      gtb_points_kernel  per point: the id rule of sd3d_ap_scene (ap_ids.h); a point of an instance column widens the
//                                         column's box.  fp32 min / max through integers: ord(x) is the order-preserving transform of the
//                                         float bits (-0 reads as +0), the maximum is kept as max ord(x), the minimum as max ~ord(x), so
//                                         zero means "nothing yet" for both, one memset clears the scene and the result does not depend
//                                         on the order of the points.  Partials per workgroup in LDS, flushed with integer atomics.
//                      gtb_cols_kernel    per column: class, consistency check, the corners decoded.
//   sd3d_box_ap_scene  box_gt_kernel      per ground truth: class / corner checks, npos.
//                      box_best_kernel    one wave per prediction: label / score / box checks, IoU (float64, uncontracted) against every
//                                         ground truth of its class, (jmax, iou_max) with the lowest column on equal IoU; then per
//                                         threshold t with iou_max > t an atomicMin of the prediction's 64-bit rank key
//                                         (~sortable(score) << 32 | row) into best[jmax, t].
//                      box_emit_kernel    per (threshold, prediction): true iff iou_max > t and best[jmax, t] is the prediction's own key -
//                                         the first prediction in (score descending, row ascending) order among those whose best ground
//                                         truth is jmax and that pass t, which is the one the sequential walk lets take it.  One entry or
//                                         the sentinel into the prediction's slot.
//   sd3d_box_ap_finish radix sort of the codes, then box_curve_kernel: one workgroup per (class, threshold) walks its segment in tiles of
//                      256 in ASCENDING code order - the reverse of the curve's order, so cumulative counts are suffix counts and the
//                      running maximum of precision "from the back" is a prefix maximum - and adds (r[i+1] - r[i]) * p[i+1] at every true
//                      entry, per thread in ascending index, then over the threads in a fixed tree.
// Slots are fixed per prediction and every float result is either order-independent (min / max) or summed in a fixed order: the same
// bits on every run.
#include "common.h"
#include "ap_curve.h"
#include "ap_ids.h"
#include "../../include/segdino3d_hip.h"

#define GTB_PER 4
#define GTB_PTS (256 * GTB_PER)                         // points per workgroup of gtb_points_kernel
#define BOX_MAX_POINTS 0x7F000000ll

__device__ static inline uint32_t box_ord(float x) {    // ascending in x; never 0 or 0xFFFFFFFF for a finite x
    if (x == 0.0f) x = 0.0f;
    const uint32_t u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ static inline float box_unord(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

__device__ static inline bool box_finite(float x) { return fabsf(x) <= 3.402823466e38f; }

// ---------------------------------------------------------------------------------------------- ground-truth boxes
// ws (uint32, all cleared per scene): kmax [AP_NI, 3] = max ord(x), kmin [AP_NI, 3] = max ~ord(x), cmax / cmin [AP_NI] as in
// ap_points_kernel (class + 1, C - class), nf [AP_NI] = a non-finite coordinate
struct GtbWs {
    uint32_t *kmax, *kmin, *cmax, *cmin, *nf;
    size_t total;
};

static GtbWs gtb_carve(void* ws) {
    GtbWs w;
    uint32_t* p = (uint32_t*)ws;
    w.kmax = p;
    w.kmin = p + 3 * AP_NI;
    w.cmax = p + 6 * AP_NI;
    w.cmin = p + 7 * AP_NI;
    w.nf = p + 8 * AP_NI;
    w.total = (size_t)9 * AP_NI * 4;
    return w;
}

__global__ __launch_bounds__(256) void gtb_points_kernel(const float* __restrict__ points, int64_t ld, const int64_t* __restrict__ gt_sem,
                                                         int64_t s_sem, const int64_t* __restrict__ gt_inst, int64_t s_inst, int64_t N,
                                                         const int64_t* __restrict__ id_map, int map_len, int num_stuff,
                                                         const int32_t* __restrict__ lut, int lut_len, int C, GtbWs w, unsigned long long* status) {
    __shared__ uint32_t acc[9 * AP_NI];                 // the layout of the workspace
    for (int c = threadIdx.x; c < 9 * AP_NI; c += 256) acc[c] = 0u;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * GTB_PTS;
    int bad = 0;
#pragma unroll
    for (int j = 0; j < GTB_PER; ++j) {
        const int64_t i = base + j * 256 + threadIdx.x;
        if (i >= N) continue;
        int cls;
        const int col = ap_point_column(gt_sem[i * s_sem], gt_inst[i * s_inst], id_map, map_len, num_stuff, lut, lut_len, C, &cls, &bad);
        if (col >= AP_NI) continue;
        atomicMax(&acc[6 * AP_NI + col], (uint32_t)(cls + 1));
        atomicMax(&acc[7 * AP_NI + col], (uint32_t)(C - cls));
        const float x = points[i * ld], y = points[i * ld + 1], z = points[i * ld + 2];
        if (!(box_finite(x) && box_finite(y) && box_finite(z))) {
            bad |= SD3D_BOX_BAD_COORD;
            atomicOr(&acc[8 * AP_NI + col], 1u);
            continue;
        }
        const uint32_t kx = box_ord(x), ky = box_ord(y), kz = box_ord(z);
        atomicMax(&acc[3 * col], kx);
        atomicMax(&acc[3 * col + 1], ky);
        atomicMax(&acc[3 * col + 2], kz);
        atomicMax(&acc[3 * AP_NI + 3 * col], ~kx);
        atomicMax(&acc[3 * AP_NI + 3 * col + 1], ~ky);
        atomicMax(&acc[3 * AP_NI + 3 * col + 2], ~kz);
    }
    ap_raise(status, bad);
    __syncthreads();
    for (int c = threadIdx.x; c < 9 * AP_NI; c += 256) {
        const uint32_t v = acc[c];
        if (v) atomicMax(&w.kmax[c], v);                // nf holds 0 / 1: its maximum is its OR
    }
}

__global__ __launch_bounds__(256) void gtb_cols_kernel(GtbWs w, int C, float* __restrict__ corners, int32_t* __restrict__ cls_out,
                                                       unsigned long long* status) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    int bad = 0;
    if (g < AP_NI) {
        int cls = -1;
        if (w.cmax[g] > 0) {
            cls = (int)w.cmax[g] - 1;
            if (cls != C - (int)w.cmin[g]) bad = SD3D_AP_MIXED_SEMANTIC;
            if (w.nf[g]) cls = -1;                                            // SD3D_BOX_BAD_COORD was raised at the point
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            corners[6 * g + a] = cls >= 0 ? box_unord(~w.kmin[3 * g + a]) : 0.0f;
            corners[6 * g + 3 + a] = cls >= 0 ? box_unord(w.kmax[3 * g + a]) : 0.0f;
        }
        cls_out[g] = cls;
    }
    ap_raise(status, bad);
}

// ---------------------------------------------------------------------------------------------- one scene of the matching
struct BoxWs {
    int32_t *gt_ok, *pred_cls, *jmax;
    double* iou;
    unsigned long long* best;
    size_t best_bytes, total;
};

static BoxWs box_carve(void* ws, int n, int n_gt, int T) {
    BoxWs w;
    char* p = (char*)ws;
    auto take = [&](size_t bytes) { char* q = p; p += align_up(bytes, 256); return q; };
    w.gt_ok = (int32_t*)take((size_t)(n_gt > 0 ? n_gt : 1) * 4);
    w.pred_cls = (int32_t*)take((size_t)(n > 0 ? n : 1) * 4);
    w.jmax = (int32_t*)take((size_t)(n > 0 ? n : 1) * 4);
    w.iou = (double*)take((size_t)(n > 0 ? n : 1) * 8);
    w.best_bytes = (size_t)(n_gt > 0 ? n_gt : 1) * T * 8;
    w.best = (unsigned long long*)take(w.best_bytes);
    w.total = (size_t)(p - (char*)ws);
    return w;
}

// IoU of two axis-aligned boxes given by their corners, in float64, every operation rounded on its own
__device__ static inline double box_iou(const double* alo, const double* ahi, const double* blo, const double* bhi) {
#pragma clang fp contract(off)
    const double va = ((ahi[0] - alo[0]) * (ahi[1] - alo[1])) * (ahi[2] - alo[2]);
    const double vb = ((bhi[0] - blo[0]) * (bhi[1] - blo[1])) * (bhi[2] - blo[2]);
    double o[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) o[a] = fmax(0.0, fmin(ahi[a], bhi[a]) - fmax(alo[a], blo[a]));
    const double inter = (o[0] * o[1]) * o[2];
    const double den = (va + vb) - inter;
    return den == 0.0 ? 0.0 : inter / den;
}

__global__ __launch_bounds__(256) void box_gt_kernel(const float* __restrict__ gt_corners, const int32_t* __restrict__ gt_cls, int n_gt, int C,
                                                     int32_t* __restrict__ gt_ok, unsigned long long* npos, unsigned long long* status) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    int bad = 0;
    if (g < n_gt) {
        int cls = gt_cls[g];
        if (cls < -1 || cls >= C) { bad |= SD3D_AP_BAD_LABEL; cls = -1; }
        if (cls >= 0) {
            bool ok = true;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const float lo = gt_corners[6 * g + a], hi = gt_corners[6 * g + 3 + a];
                ok = ok && box_finite(lo) && box_finite(hi) && hi >= lo;
            }
            if (!ok) { bad |= SD3D_BOX_BAD_COORD; cls = -1; }
        }
        if (cls >= 0) atomicAdd(&npos[cls], 1ull);
        gt_ok[g] = cls;
    }
    ap_raise(status, bad);
}

__device__ static inline unsigned long long box_rank_key(float score, int r) {         // ascending = (score descending, row ascending)
    return ((unsigned long long)(~ap_sortable(score)) << 32) | (unsigned long long)(uint32_t)r;
}

// four waves per workgroup, one wave per prediction row
__global__ __launch_bounds__(256) void box_best_kernel(const float* __restrict__ boxes, int n, const int64_t* __restrict__ labels,
                                                       const float* __restrict__ scores, const float* __restrict__ gt_corners,
                                                       const int32_t* __restrict__ gt_ok, int n_gt, int C, const double* __restrict__ th, int T,
                                                       BoxWs w, unsigned long long* has_pred, unsigned long long* status) {
#pragma clang fp contract(off)
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= n) return;                                                       // the whole wave
    const int64_t lab = labels[r];
    const float s = scores[r];
    float b[6];
#pragma unroll
    for (int a = 0; a < 6; ++a) b[a] = boxes[6 * (size_t)r + a];
    int bad = 0;
    if (lab < 0 || lab >= C) bad |= SD3D_AP_BAD_LABEL;
    if (!box_finite(s)) bad |= SD3D_AP_BAD_SCORE;
    bool box_ok = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) box_ok = box_ok && box_finite(b[a]) && box_finite(b[3 + a]) && b[3 + a] >= 0.0f;
    if (!box_ok) bad |= SD3D_BOX_BAD_BOX;
    const int cls = bad ? -1 : (int)lab;
    double plo[3], phi[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double half = (double)b[3 + a] / 2.0;
        plo[a] = (double)b[a] - half;
        phi[a] = (double)b[a] + half;
    }
    double best = -1.0;
    int bj = 0x7FFFFFFF;
    if (cls >= 0) {
        for (int g = lane; g < n_gt; g += 64) {
            if (gt_ok[g] != cls) continue;
            double glo[3], ghi[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) { glo[a] = (double)gt_corners[6 * g + a]; ghi[a] = (double)gt_corners[6 * g + 3 + a]; }
            const double v = box_iou(plo, phi, glo, ghi);
            if (v > best) { best = v; bj = g; }                               // ascending g: the lowest column keeps an equal IoU
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const double ov = __shfl_xor(best, d);
        const int oj = __shfl_xor(bj, d);
        if (ov > best || (ov == best && oj < bj)) { best = ov; bj = oj; }
    }
    const int j = bj == 0x7FFFFFFF ? -1 : bj;
    if (lane == 0) {
        w.pred_cls[r] = cls;
        w.jmax[r] = j;
        w.iou[r] = best;
        if (cls >= 0) atomicOr(&has_pred[cls], 1ull);
    }
    if (j >= 0 && lane < T && best > th[lane]) atomicMin(&w.best[(size_t)j * T + lane], box_rank_key(s, r));
    ap_raise(status, bad);
}

__global__ __launch_bounds__(256) void box_emit_kernel(int n, const float* __restrict__ scores, const double* __restrict__ th, int T, int C, BoxWs w,
                                                       int64_t* __restrict__ store, int64_t slot_begin, int64_t slot_cap,
                                                       unsigned long long* status) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int bad = 0;
    if (idx < (int64_t)n * T) {
        const int o = (int)(idx / n), r = (int)(idx % n);
        const int cls = w.pred_cls[r];
        int64_t code = (int64_t)((uint64_t)(C * T) << 33);                    // the sentinel
        if (cls >= 0) {
            const int j = w.jmax[r];
            const float s = scores[r];
            const bool truth = j >= 0 && w.iou[r] > th[o] && w.best[(size_t)j * T + o] == box_rank_key(s, r);
            code = ap_code(cls * T + o, s, truth ? 1 : 0);
        }
        if (idx < slot_cap) store[slot_begin + idx] = code;
        else bad = SD3D_AP_STORE_FULL;
    }
    ap_raise(status, bad);
}

// ---------------------------------------------------------------------------------------------- curves
// inclusive maximum scan of one non-negative double over the 256 threads of the workgroup
__device__ static inline double box_scan_max(double v, double* wmax, double& total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double x = __shfl_up(v, d);
        if (lane >= d) v = fmax(v, x);
    }
    __syncthreads();                                                          // the previous round's readers are done with wmax
    if (lane == 63) wmax[wv] = v;
    __syncthreads();
    total = 0.0;
    for (int k = 0; k < 4; ++k) {
        if (k < wv) v = fmax(v, wmax[k]);
        total = fmax(total, wmax[k]);
    }
    return v;
}

__global__ __launch_bounds__(256) void box_curve_kernel(const uint64_t* __restrict__ codes, int64_t n, int T, const int64_t* __restrict__ npos,
                                                        double* __restrict__ ap_out, double* __restrict__ ar_out) {
#pragma clang fp contract(off)
    __shared__ int wsum[2][4];
    __shared__ double wmax[4], part[256];
    const int g = blockIdx.x, c = g / T, t = threadIdx.x;
    const int64_t np = npos[c];
    if (np <= 0) {
        if (t == 0) ap_out[g] = ar_out[g] = __longlong_as_double(0x7FF8000000000000ll);
        return;
    }
    const int64_t lo = ap_lower_bound(codes, n, (uint64_t)g << 33), hi = ap_lower_bound(codes, n, (uint64_t)(g + 1) << 33);
    if (hi == lo) {
        if (t == 0) ap_out[g] = ar_out[g] = 0.0;
        return;
    }
    int64_t n_true = 0;
    {
        int cnt = 0, zero = 0, tot = 0, tot0 = 0;
        for (int64_t j = lo + t; j < hi; j += 256) cnt += (int)(codes[j] & 1ull);
        ap_scan2(cnt, zero, wsum, tot, tot0);
        n_true = tot;
    }
    // entry j: tp = true entries of [j, hi), tp + fp = hi - j; the running maximum of precision from the back of the curve = over [lo, j]
    const double dn = (double)np;
    int64_t carry_true = 0;
    double carry_max = 0.0, s = 0.0;
    for (int64_t b = lo; b < hi; b += 256) {
        const int64_t j = b + t;
        const bool valid = j < hi;
        const int tr = valid ? (int)(codes[j] & 1ull) : 0;
        int inc_t = tr, zero = 0, tot_t, tot0;
        ap_scan2(inc_t, zero, wsum, tot_t, tot0);
        const int64_t tp = n_true - (carry_true + inc_t - tr);
        const double prec = valid ? (double)tp / fmax((double)(hi - j), 2.220446049250313e-16) : 0.0;
        double tile_max;
        const double m = fmax(carry_max, box_scan_max(prec, wmax, tile_max));
        if (tr) s = s + ((double)tp / dn - (double)(tp - 1) / dn) * m;
        carry_true += tot_t;
        carry_max = fmax(carry_max, tile_max);
    }
    part[t] = s;
    __syncthreads();
    for (int d = 128; d >= 1; d >>= 1) {
        if (t < d) part[t] += part[t + d];
        __syncthreads();
    }
    if (t == 0) {
        ap_out[g] = part[0];
        ar_out[g] = (double)n_true / dn;
    }
}

// ---------------------------------------------------------------------------------------------- C entry points
extern "C" size_t sd3d_gt_boxes_ws_bytes(void) { return gtb_carve(nullptr).total; }

extern "C" int sd3d_gt_boxes(const float* points, int64_t ld, int64_t N, const int64_t* gt_sem, int64_t sem_stride, const int64_t* gt_inst,
                             int64_t inst_stride, const int64_t* id_map, int map_len, int num_stuff, const int32_t* class_lut, int lut_len,
                             int n_classes, float* corners, int32_t* cls, int64_t* status, void* ws, size_t ws_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (N < 0 || N > BOX_MAX_POINTS || ld < 3 || sem_stride < 0 || inst_stride < 0 || lut_len < 0 || map_len < 0 || n_classes < 1 ||
        n_classes > SD3D_AP_MAX_CLASSES)
        return sd3d_set_error(SD3D_ERR_ARG, "gt_boxes: 0 <= N <= 0x7F000000 points with a leading dimension >= 3, 1..1024 classes");
    if (!class_lut || !corners || !cls || !status || !ws || (N > 0 && (!points || !gt_sem || !gt_inst)) || (id_map && map_len < 1))
        return sd3d_set_error(SD3D_ERR_ARG, "gt_boxes: NULL argument");
    const GtbWs w = gtb_carve(ws);
    if (ws_bytes < w.total) return sd3d_set_error(SD3D_ERR_WS, "gt_boxes: workspace too small");
    unsigned long long* stat = (unsigned long long*)status;
    if (hipMemsetAsync(ws, 0, w.total, st) != hipSuccess) return sd3d_set_error(SD3D_ERR_LAUNCH, "gt_boxes: memset failed");
    if (N > 0)
        hipLaunchKernelGGL(gtb_points_kernel, dim3((unsigned)cdiv(N, GTB_PTS)), dim3(256), 0, st, points, ld, gt_sem, sem_stride, gt_inst, inst_stride,
                           N, id_map, map_len, num_stuff, class_lut, lut_len, n_classes, w, stat);
    hipLaunchKernelGGL(gtb_cols_kernel, dim3((unsigned)cdiv(AP_NI, 256)), dim3(256), 0, st, w, n_classes, corners, cls, stat);
    SD3D_CHECK_LAUNCH();
    return SD3D_OK;
}

extern "C" size_t sd3d_box_ap_scene_ws_bytes(int n, int n_gt, int n_overlaps) {
    if (n < 0 || n > SD3D_AP_MAX_PREDS || n_gt < 0 || n_gt > SD3D_AP_INSTANCE_COLS || n_overlaps < 1 || n_overlaps > SD3D_AP_MAX_OVERLAPS) return 0;
    return box_carve(nullptr, n, n_gt, n_overlaps).total;
}

extern "C" int sd3d_box_ap_scene(const float* boxes, int n, const int64_t* labels, const float* scores, const float* gt_corners,
                                 const int32_t* gt_cls, int n_gt, int n_classes, const double* thresholds, int n_overlaps, int64_t* store,
                                 int64_t slot_begin, int64_t slot_cap, int64_t* npos, int64_t* has_pred, int64_t* status, void* ws,
                                 size_t ws_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (n < 0 || n > SD3D_AP_MAX_PREDS || n_gt < 0 || n_gt > SD3D_AP_INSTANCE_COLS || n_classes < 1 || n_classes > SD3D_AP_MAX_CLASSES ||
        n_overlaps < 1 || n_overlaps > SD3D_AP_MAX_OVERLAPS || slot_begin < 0 || slot_cap < 0)
        return sd3d_set_error(SD3D_ERR_ARG, "box_ap_scene: 0..4096 predictions, 0..1000 ground truths, 1..1024 classes, 1..16 thresholds");
    if (!thresholds || !npos || !has_pred || !status || !ws || (n_gt > 0 && (!gt_corners || !gt_cls)) ||
        (n > 0 && (!boxes || !labels || !scores || !store)))
        return sd3d_set_error(SD3D_ERR_ARG, "box_ap_scene: NULL argument");
    const BoxWs w = box_carve(ws, n, n_gt, n_overlaps);
    if (ws_bytes < w.total) return sd3d_set_error(SD3D_ERR_WS, "box_ap_scene: workspace too small");
    unsigned long long* stat = (unsigned long long*)status;
    if (hipMemsetAsync(w.best, 0xFF, w.best_bytes, st) != hipSuccess) return sd3d_set_error(SD3D_ERR_LAUNCH, "box_ap_scene: memset failed");
    if (n_gt > 0)
        hipLaunchKernelGGL(box_gt_kernel, dim3((unsigned)cdiv(n_gt, 256)), dim3(256), 0, st, gt_corners, gt_cls, n_gt, n_classes, w.gt_ok,
                           (unsigned long long*)npos, stat);
    if (n > 0) {
        hipLaunchKernelGGL(box_best_kernel, dim3((unsigned)cdiv(n, 4)), dim3(256), 0, st, boxes, n, labels, scores, gt_corners, w.gt_ok, n_gt,
                           n_classes, thresholds, n_overlaps, w, (unsigned long long*)has_pred, stat);
        hipLaunchKernelGGL(box_emit_kernel, dim3((unsigned)cdiv((int64_t)n * n_overlaps, 256)), dim3(256), 0, st, n, scores, thresholds, n_overlaps,
                           n_classes, w, store, slot_begin, slot_cap, stat);
    }
    SD3D_CHECK_LAUNCH();
    return SD3D_OK;
}

struct BoxFinishWs {
    uint64_t* keys;
    uint32_t *vals, *scratch;
    void* sort_ws;
    size_t sort_bytes, total;
};

static BoxFinishWs box_finish_carve(void* ws, int64_t n) {
    BoxFinishWs w;
    char* p = (char*)ws;
    auto take = [&](size_t bytes) { char* q = p; p += align_up(bytes, 256); return q; };
    const size_t m = (size_t)(n > 0 ? n : 1);
    w.keys = (uint64_t*)take(m * 8);
    w.vals = (uint32_t*)take(m * 4);
    w.scratch = (uint32_t*)take(m * 4);
    w.sort_bytes = sort_ws_bytes((int64_t)m);
    w.sort_ws = take(w.sort_bytes);
    w.total = (size_t)(p - (char*)ws);
    return w;
}

extern "C" size_t sd3d_box_ap_finish_ws_bytes(int64_t n_slots) {
    if (n_slots < 0 || n_slots > BOX_MAX_POINTS) return 0;
    return box_finish_carve(nullptr, n_slots).total;
}

extern "C" int sd3d_box_ap_finish(int64_t* codes, int64_t n_slots, int n_classes, int n_overlaps, const int64_t* npos, double* ap, double* ar,
                                  void* ws, size_t ws_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (n_slots < 0 || n_slots > BOX_MAX_POINTS || n_classes < 1 || n_classes > SD3D_AP_MAX_CLASSES || n_overlaps < 1 ||
        n_overlaps > SD3D_AP_MAX_OVERLAPS)
        return sd3d_set_error(SD3D_ERR_ARG, "box_ap_finish: 0 <= n_slots <= 0x7F000000, 1..1024 classes, 1..16 thresholds");
    if (!npos || !ap || !ar || !ws || (n_slots > 0 && !codes)) return sd3d_set_error(SD3D_ERR_ARG, "box_ap_finish: NULL argument");
    const BoxFinishWs w = box_finish_carve(ws, n_slots);
    if (ws_bytes < w.total) return sd3d_set_error(SD3D_ERR_WS, "box_ap_finish: workspace too small");
    const int groups = n_classes * n_overlaps;
    int group_bits = 1;
    while ((1 << group_bits) < groups + 1) ++group_bits;
    const uint64_t* sorted = (const uint64_t*)codes;
    if (n_slots > 0) {
        int landed = 0;
        if (int rc = sort_pairs_u64((uint64_t*)codes, nullptr, w.keys, w.vals, n_slots, 0, 33 + group_bits, w.sort_ws, w.sort_bytes, st, w.scratch,
                                    &landed))
            return rc;
        if (!landed) sorted = w.keys;
    }
    hipLaunchKernelGGL(box_curve_kernel, dim3((unsigned)groups), dim3(256), 0, st, sorted, n_slots, n_overlaps, npos, ap, ar);
    SD3D_CHECK_LAUNCH();
    return SD3D_OK;
}
