// ScanNet instance AP accumulated and scored on the device: the reference's `evaluate_matches`
// (evaluation/utils_instance_seg_3d_eval.py:18-209) decomposed per scene.  The `visited` flags of the greedy matching never cross a
// (scene, class, overlap) triple - pairs only exist between a prediction and ground truth of its own label - so every triple is matched
// on its own and emits ENTRIES (class, overlap, score, true), a count of hard false negatives and the two flags has_gt / has_pred.
// The entries of all scenes, sorted by (class, overlap, score), give the precision / recall curve of every (class, overlap) group.
//
//   sd3d_ap_scene   ap_points_kernel   per point: map_inst_markup (optional), class of the semantic id, ground-truth column (instance
//                                      index, void, nowhere); per column the point count and the largest / smallest class index, kept in
//                                      LDS per workgroup and flushed with integer atomics;
//                   sd3d_mask_overlaps counts[row][column] over the SD3D_AP_COLS columns (csrc/post.hip);
//                   ap_cols_kernel     per column: its class, the consistency check, has_gt, the class is present in the scene;
//                   ap_rows_kernel     one wave per prediction: vert = sum of its counts row, label / score checks, has_pred, and the
//                                      sentinel in every slot of the prediction;
//                   ap_match_kernel    one wave per (class, overlap), classes absent from the scene leave at once: the ground truths
//                                      (ascending instance index) and predictions (ascending row) of the class, their block of the count
//                                      matrix staged in LDS, the greedy matching in the reference's order (64 predictions are tested
//                                      against a ground truth per step, the qualifying ones are then taken in order), then per
//                                      prediction the "some IoU > th" / ignore test.
//   sd3d_ap_finish  radix sort of the codes, then ap_curve_kernel: one workgroup per (class, overlap) finds its segment by binary search,
//                   walks it in tiles of 256 with a running prefix (first index of each distinct score, exclusive prefix of the true
//                   flags), writes precision / recall per distinct score, and reduces AP and the first maximum of f1 in a fixed order.
// A prediction owns fixed slots of the store, so there is no append counter and no float atomic: the same bits on every run.
#include "common.h"
#include "ap_curve.h"
#include "ap_ids.h"
#include "../../include/segdino3d_hip.h"

#define AP_PER 4
#define AP_PTS (256 * AP_PER)                           // points per workgroup of ap_points_kernel
#define AP_TILE 8192                                    // ints of the count matrix a matcher stages in LDS
#define AP_MAX_POINTS 0x7F000000ll

struct ApSpec {
    int C, O, n, min_region, zero_class;
    int k[SD3D_AP_MAX_OVERLAPS], koff[SD3D_AP_MAX_OVERLAPS];        // slots per prediction at overlap o; slots per prediction before o
    int64_t slot_begin, slot_cap;
};

struct ApWs {
    int32_t *gt_vert, *cmax, *cmin, *present;           // [AP_NI] x 3, [C]: cleared per scene
    int32_t *gt_cls, *pred_cls, *pred_vert, *gt_index, *counts;
    size_t zero_bytes, total;
};

static ApWs ap_carve(void* ws, int64_t N, int n) {
    ApWs w;
    char* p = (char*)ws;
    auto take = [&](size_t bytes) { char* q = p; p += align_up(bytes, 256); return q; };
    w.gt_vert = (int32_t*)take(AP_NI * 4);
    w.cmax = (int32_t*)take(AP_NI * 4);
    w.cmin = (int32_t*)take(AP_NI * 4);
    w.present = (int32_t*)take(SD3D_AP_MAX_CLASSES * 4);
    w.zero_bytes = (size_t)(p - (char*)ws);
    w.gt_cls = (int32_t*)take(AP_NI * 4);
    w.pred_cls = (int32_t*)take((size_t)(n > 0 ? n : 1) * 4);
    w.pred_vert = (int32_t*)take((size_t)(n > 0 ? n : 1) * 4);
    w.gt_index = (int32_t*)take((size_t)(N > 0 ? N : 1) * 4);
    w.counts = (int32_t*)take((size_t)(n > 0 ? n : 1) * SD3D_AP_COLS * 4);
    w.total = (size_t)(p - (char*)ws);
    return w;
}

// ---------------------------------------------------------------------------------------------- points -> columns
__global__ __launch_bounds__(256) void ap_points_kernel(const int64_t* __restrict__ gt_sem, int64_t s_sem, const int64_t* __restrict__ gt_inst,
                                                        int64_t s_inst, int64_t N, const int64_t* __restrict__ id_map, int map_len, int num_stuff,
                                                        const int32_t* __restrict__ lut, int lut_len, int C, int32_t* __restrict__ gt_index,
                                                        int32_t* gt_vert, int32_t* cmax, int32_t* cmin, unsigned long long* status) {
    __shared__ int vert[AP_NI], hi[AP_NI], lo[AP_NI];
    for (int c = threadIdx.x; c < AP_NI; c += 256) vert[c] = hi[c] = lo[c] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * AP_PTS;
    int64_t sem[AP_PER], inst[AP_PER];
#pragma unroll
    for (int j = 0; j < AP_PER; ++j) {
        const int64_t i = base + j * 256 + threadIdx.x;
        sem[j] = inst[j] = -1;
        if (i < N) { sem[j] = gt_sem[i * s_sem]; inst[j] = gt_inst[i * s_inst]; }
    }
    int bad = 0;
#pragma unroll
    for (int j = 0; j < AP_PER; ++j) {
        const int64_t i = base + j * 256 + threadIdx.x;
        if (i >= N) continue;
        int cls;
        const int col = ap_point_column(sem[j], inst[j], id_map, map_len, num_stuff, lut, lut_len, C, &cls, &bad);   // the id rule (ap_ids.h)
        gt_index[i] = col;
        if (col < AP_NI) {
            atomicAdd(&vert[col], 1);
            atomicMax(&hi[col], cls + 1);
            atomicMax(&lo[col], C - cls);
        }
    }
    ap_raise(status, bad);
    __syncthreads();
    for (int c = threadIdx.x; c < AP_NI; c += 256) {
        if (vert[c]) {
            atomicAdd(&gt_vert[c], vert[c]);
            atomicMax(&cmax[c], hi[c]);
            atomicMax(&cmin[c], lo[c]);
        }
    }
}

__global__ __launch_bounds__(256) void ap_cols_kernel(const int32_t* __restrict__ gt_vert, const int32_t* __restrict__ cmax,
                                                      const int32_t* __restrict__ cmin, int C, int min_region, int32_t* __restrict__ gt_cls,
                                                      int32_t* present, unsigned long long* has_gt, unsigned long long* status) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    int bad = 0;
    if (g < AP_NI) {
        int cls = -1;
        if (gt_vert[g] > 0) {
            cls = cmax[g] - 1;
            if (cls != C - cmin[g]) bad = SD3D_AP_MIXED_SEMANTIC;
            present[cls] = 1;
            if (gt_vert[g] >= min_region) atomicOr(&has_gt[cls], 1ull);
        }
        gt_cls[g] = cls;
    }
    ap_raise(status, bad);
}

// one wave per prediction row
__global__ __launch_bounds__(64) void ap_rows_kernel(const int32_t* __restrict__ counts, const int64_t* __restrict__ labels,
                                                     const float* __restrict__ scores, ApSpec spec, int32_t* __restrict__ pred_cls,
                                                     int32_t* __restrict__ pred_vert, int32_t* present, unsigned long long* has_pred,
                                                     int64_t* __restrict__ store, unsigned long long* status) {
    const int r = blockIdx.x, lane = threadIdx.x;
    int v = 0;
    for (int c = lane; c < SD3D_AP_COLS; c += 64) v += counts[(size_t)r * SD3D_AP_COLS + c];
    v = wave_sum(v);
    int bad = 0;
    if (lane == 0) {
        const int64_t lab = labels[r];
        const float s = scores[r];
        int cls = -1;
        if (lab < 0 || lab >= spec.C) bad |= SD3D_AP_BAD_LABEL;
        if (!(fabsf(s) <= 3.402823466e38f)) bad |= SD3D_AP_BAD_SCORE;
        if (!bad && v >= spec.min_region) {
            cls = (int)lab;
            present[cls] = 1;
            atomicOr(&has_pred[cls], 1ull);
        }
        pred_cls[r] = cls;
        pred_vert[r] = v;
    }
    const int64_t sentinel = (int64_t)((uint64_t)(spec.C * spec.O) << 33);
    for (int o = 0; o < spec.O; ++o) {
        for (int j = lane; j < spec.k[o]; j += 64) {
            const int64_t idx = (int64_t)spec.n * spec.koff[o] + (int64_t)r * spec.k[o] + j;
            if (idx < spec.slot_cap) store[spec.slot_begin + idx] = sentinel;
            else bad |= SD3D_AP_STORE_FULL;
        }
    }
    ap_raise(status, bad);
}

// ---------------------------------------------------------------------------------------------- greedy matching
// grid (C, O), one wave.  Lists of the class in LDS: ground-truth columns `cols` (ascending) with their sizes, prediction rows `rows`
// (ascending).  inter(pi, gi) comes from the staged block when ng * np <= AP_TILE, from the count matrix otherwise.
__global__ __launch_bounds__(64) void ap_match_kernel(ApSpec spec, const double* __restrict__ overlaps, const int32_t* __restrict__ present,
                                                      const int32_t* __restrict__ gt_cls, const int32_t* __restrict__ gt_vert,
                                                      const int32_t* __restrict__ pred_cls, const int32_t* __restrict__ pred_vert,
                                                      const float* __restrict__ scores, const int32_t* __restrict__ counts,
                                                      int64_t* __restrict__ store, unsigned long long* hard_fn, unsigned long long* status) {
#pragma clang fp contract(off)
    __shared__ uint16_t cols[AP_NI], rows[SD3D_AP_MAX_PREDS];
    __shared__ int gv[AP_NI];
    __shared__ uint8_t visited[SD3D_AP_MAX_PREDS], nslot[SD3D_AP_MAX_PREDS];
    __shared__ int tile[AP_TILE];
    const int c = blockIdx.x, o = blockIdx.y, lane = threadIdx.x;
    if (!present[c]) return;
    const double th = overlaps[o];
    const int k = spec.k[o], group = c * spec.O + o;
    const unsigned long long below = (1ull << lane) - 1ull;
    int ng = 0, np = 0;
    for (int b = 0; b < AP_NI; b += 64) {
        const int g = b + lane;
        const bool ok = g < AP_NI && gt_cls[g] == c;
        const unsigned long long m = __ballot(ok);
        if (ok) {
            const int at = ng + __popcll(m & below);
            cols[at] = (uint16_t)g;
            gv[at] = gt_vert[g];
        }
        ng += __popcll(m);
    }
    for (int b = 0; b < spec.n; b += 64) {
        const int r = b + lane;
        const bool ok = r < spec.n && pred_cls[r] == c;
        const unsigned long long m = __ballot(ok);
        if (ok) {
            const int at = np + __popcll(m & below);
            rows[at] = (uint16_t)r;
            visited[at] = 0;
            nslot[at] = 0;
        }
        np += __popcll(m);
    }
    __syncthreads();
    const bool staged = (int64_t)ng * np <= AP_TILE;
    if (staged)
        for (int i = lane; i < ng * np; i += 64) tile[i] = counts[(size_t)rows[i / ng] * SD3D_AP_COLS + cols[i % ng]];
    __syncthreads();
    auto inter = [&](int pi, int gi) -> int64_t {
        return staged ? tile[pi * ng + gi] : counts[(size_t)rows[pi] * SD3D_AP_COLS + cols[gi]];
    };
    auto iou_over = [&](int64_t it, int64_t g_size, int64_t p_size) -> bool { return (double)it / (double)(g_size + p_size - it) > th; };
    int bad = 0;
    // entry j of prediction pi: only lane 0 emits in the ground-truth loop, so nslot needs no atomics
    auto emit = [&](int pi, float score, int truth) {
        const int j = nslot[pi];
        const int64_t idx = (int64_t)spec.n * spec.koff[o] + (int64_t)rows[pi] * k + j;
        if (j < k && idx < spec.slot_cap) {
            store[spec.slot_begin + idx] = ap_code(group, score, truth);
            nslot[pi] = (uint8_t)(j + 1);
        } else {
            bad |= SD3D_AP_STORE_FULL;
        }
    };
    int hard = 0;
    for (int gi = 0; gi < ng; ++gi) {
        const int64_t g_size = gv[gi];
        if (g_size < spec.min_region) continue;
        bool cur_match = false;
        float cur_score = 0.f;
        int first_pi = -1;
        for (int pb = 0; pb < np; pb += 64) {
            const int pi = pb + lane;
            bool q = false;
            if (pi < np && !visited[pi]) q = iou_over(inter(pi, gi), g_size, pred_vert[rows[pi]]);
            unsigned long long m = __ballot(q);
            while (m) {                                                       // the qualifying predictions in ascending row, on every lane
                const int l = __ffsll((long long)m) - 1;
                m &= m - 1;
                const int qi = pb + l;
                const float conf = scores[rows[qi]];
                if (cur_match) {                                              // a second prediction on this ground truth: the weaker score is a false positive
                    const float lo = fminf(cur_score, conf);
                    cur_score = fmaxf(cur_score, conf);
                    if (lane == 0) emit(qi, lo, 0);
                } else {
                    cur_match = true;
                    cur_score = conf;
                    first_pi = qi;
                    if (lane == 0) visited[qi] = 1;
                }
            }
        }
        if (!cur_match) ++hard;
        else if (lane == 0) emit(first_pi, cur_score, 1);
        __syncthreads();                                                      // visited of this ground truth before the next one reads it
    }
    if (lane == 0 && hard) atomicAdd(&hard_fn[group], (unsigned long long)hard);
    // predictions that no ground truth of their label overlaps by more than th: false positives unless mostly void / small ground truth
    for (int pi = lane; pi < np; pi += 64) {
        const int r = rows[pi];
        const int64_t p_size = pred_vert[r];
        bool found = false;
        int64_t ignore = counts[(size_t)r * SD3D_AP_COLS + AP_VOID];
        for (int gi = 0; gi < ng; ++gi) {
            const int64_t it = inter(pi, gi), g_size = gv[gi];
            if (it == 0) continue;
            found |= iou_over(it, g_size, p_size);
            if (c == spec.zero_class) ignore += it;                           // the reference's `gt_id < 1000`
            if (g_size < spec.min_region) ignore += it;
        }
        if (!found && (double)ignore / (double)p_size <= th) {
            const int64_t idx = (int64_t)spec.n * spec.koff[o] + (int64_t)r * k;
            if (k > 0 && idx < spec.slot_cap) store[spec.slot_begin + idx] = ap_code(group, scores[r], 0);
            else bad |= SD3D_AP_STORE_FULL;
        }
    }
    ap_raise(status, bad);
}

// ---------------------------------------------------------------------------------------------- curves
// the curve body (ap_curve.h) is shared with the per-scene finish of csrc/apeval_scene.hip
__global__ __launch_bounds__(256) void ap_curve_kernel(const uint64_t* __restrict__ codes, int64_t n, int O, const int64_t* __restrict__ hard_fn,
                                                       const int64_t* __restrict__ has_gt, const int64_t* __restrict__ has_pred,
                                                       double* __restrict__ P, double* __restrict__ R, double* __restrict__ ap_out,
                                                       double* __restrict__ pr_out, double* __restrict__ rc_out) {
    const int g = blockIdx.x, c = g / O;
    const bool gt = has_gt[c] != 0, pred = has_pred[c] != 0;
    int64_t lo = 0, hi = 0, hf = 0;
    if (gt && pred) {
        lo = ap_lower_bound(codes, n, (uint64_t)g << 33);
        hi = ap_lower_bound(codes, n, (uint64_t)(g + 1) << 33);
        hf = hard_fn[g];
    }
    ap_curve_body(codes, lo, hi, hf, gt, pred, P, R, ap_out + g, pr_out + g, rc_out + g);
}

// ---------------------------------------------------------------------------------------------- C entry points
extern "C" size_t sd3d_ap_scene_ws_bytes(int64_t N, int n) {
    if (N < 0 || N > AP_MAX_POINTS || n < 0 || n > SD3D_AP_MAX_PREDS) return 0;
    return ap_carve(nullptr, N, n).total;
}

extern "C" int sd3d_ap_scene(const int64_t* gt_sem, int64_t sem_stride, const int64_t* gt_inst, int64_t inst_stride, int64_t N,
                             const int64_t* id_map, int map_len, int num_stuff, const uint8_t* masks, int64_t mask_stride, int n,
                             const int64_t* labels, const float* scores, const int32_t* class_lut, int lut_len, int zero_class, int n_classes,
                             const double* overlaps, const int32_t* slots_host, int n_overlaps, int min_region, int64_t* store,
                             int64_t slot_begin, int64_t slot_cap, int64_t* hard_fn, int64_t* has_gt, int64_t* has_pred, int64_t* status,
                             void* ws, size_t ws_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (N < 0 || N > AP_MAX_POINTS || n < 0 || n > SD3D_AP_MAX_PREDS || n_classes < 1 || n_classes > SD3D_AP_MAX_CLASSES || n_overlaps < 1 ||
        n_overlaps > SD3D_AP_MAX_OVERLAPS || sem_stride < 0 || inst_stride < 0 || lut_len < 0 || map_len < 0 || slot_begin < 0 || slot_cap < 0 ||
        zero_class >= n_classes || (n > 0 && mask_stride < N))
        return sd3d_set_error(SD3D_ERR_ARG, "ap_scene: 0 <= N <= 0x7F000000 points, 0..4096 predictions with a pitch >= N, 1..1024 classes, 1..16 overlaps");
    if (!class_lut || !overlaps || !slots_host || !hard_fn || !has_gt || !has_pred || !status || !ws || (N > 0 && (!gt_sem || !gt_inst)) ||
        (n > 0 && (!masks || !labels || !scores || !store)) || (id_map && map_len < 1))
        return sd3d_set_error(SD3D_ERR_ARG, "ap_scene: NULL argument");
    ApSpec spec;
    spec.C = n_classes;
    spec.O = n_overlaps;
    spec.n = n;
    spec.min_region = min_region;
    spec.zero_class = zero_class;
    spec.slot_begin = slot_begin;
    spec.slot_cap = slot_cap;
    int per_pred = 0;
    for (int o = 0; o < SD3D_AP_MAX_OVERLAPS; ++o) {
        spec.k[o] = o < n_overlaps ? slots_host[o] : 0;
        spec.koff[o] = per_pred;
        if (spec.k[o] < 0 || spec.k[o] > 255) return sd3d_set_error(SD3D_ERR_ARG, "ap_scene: 0..255 slots per prediction and overlap");
        per_pred += spec.k[o];
    }
    const ApWs w = ap_carve(ws, N, n);
    if (ws_bytes < w.total) return sd3d_set_error(SD3D_ERR_WS, "ap_scene: workspace too small");
    unsigned long long* stat = (unsigned long long*)status;

    if (hipMemsetAsync(w.gt_vert, 0, w.zero_bytes, st) != hipSuccess) return sd3d_set_error(SD3D_ERR_LAUNCH, "ap_scene: memset failed");
    if (N > 0)
        hipLaunchKernelGGL(ap_points_kernel, dim3((unsigned)cdiv(N, AP_PTS)), dim3(256), 0, st, gt_sem, sem_stride, gt_inst, inst_stride, N, id_map,
                           map_len, num_stuff, class_lut, lut_len, n_classes, w.gt_index, w.gt_vert, w.cmax, w.cmin, stat);
    SD3D_CHECK_LAUNCH();
    if (int rc = sd3d_mask_overlaps(masks, mask_stride, n, w.gt_index, N, SD3D_AP_COLS, w.counts, stream)) return rc;
    hipLaunchKernelGGL(ap_cols_kernel, dim3((unsigned)cdiv(AP_NI, 256)), dim3(256), 0, st, w.gt_vert, w.cmax, w.cmin, n_classes, min_region, w.gt_cls,
                       w.present, (unsigned long long*)has_gt, stat);
    if (n > 0)
        hipLaunchKernelGGL(ap_rows_kernel, dim3((unsigned)n), dim3(64), 0, st, w.counts, labels, scores, spec, w.pred_cls, w.pred_vert, w.present,
                           (unsigned long long*)has_pred, store, stat);
    hipLaunchKernelGGL(ap_match_kernel, dim3((unsigned)n_classes, (unsigned)n_overlaps), dim3(64), 0, st, spec, overlaps, w.present, w.gt_cls,
                       w.gt_vert, w.pred_cls, w.pred_vert, scores, w.counts, store, (unsigned long long*)hard_fn, stat);
    SD3D_CHECK_LAUNCH();
    return SD3D_OK;
}

struct ApFinishWs {
    uint64_t* keys;
    uint32_t *vals, *scratch;
    double *P, *R;
    void* sort_ws;
    size_t sort_bytes, total;
};

static ApFinishWs ap_finish_carve(void* ws, int64_t n) {
    ApFinishWs w;
    char* p = (char*)ws;
    auto take = [&](size_t bytes) { char* q = p; p += align_up(bytes, 256); return q; };
    const size_t m = (size_t)(n > 0 ? n : 1);
    w.keys = (uint64_t*)take(m * 8);
    w.vals = (uint32_t*)take(m * 4);
    w.scratch = (uint32_t*)take(m * 4);
    w.P = (double*)take(m * 8);
    w.R = (double*)take(m * 8);
    w.sort_bytes = sort_ws_bytes((int64_t)m);
    w.sort_ws = take(w.sort_bytes);
    w.total = (size_t)(p - (char*)ws);
    return w;
}

extern "C" size_t sd3d_ap_finish_ws_bytes(int64_t n_slots) {
    if (n_slots < 0 || n_slots > AP_MAX_POINTS) return 0;
    return ap_finish_carve(nullptr, n_slots).total;
}

extern "C" int sd3d_ap_finish(int64_t* codes, int64_t n_slots, int n_classes, int n_overlaps, const int64_t* hard_fn, const int64_t* has_gt,
                              const int64_t* has_pred, double* ap, double* pr_rc, void* ws, size_t ws_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (n_slots < 0 || n_slots > AP_MAX_POINTS || n_classes < 1 || n_classes > SD3D_AP_MAX_CLASSES || n_overlaps < 1 ||
        n_overlaps > SD3D_AP_MAX_OVERLAPS)
        return sd3d_set_error(SD3D_ERR_ARG, "ap_finish: 0 <= n_slots <= 0x7F000000, 1..1024 classes, 1..16 overlaps");
    if (!hard_fn || !has_gt || !has_pred || !ap || !pr_rc || !ws || (n_slots > 0 && !codes)) return sd3d_set_error(SD3D_ERR_ARG, "ap_finish: NULL argument");
    const ApFinishWs w = ap_finish_carve(ws, n_slots);
    if (ws_bytes < w.total) return sd3d_set_error(SD3D_ERR_WS, "ap_finish: workspace too small");
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
    hipLaunchKernelGGL(ap_curve_kernel, dim3((unsigned)groups), dim3(256), 0, st, sorted, n_slots, n_overlaps, hard_fn, has_gt, has_pred, w.P, w.R, ap,
                       pr_rc, pr_rc + groups);
    SD3D_CHECK_LAUNCH();
    return SD3D_OK;
}
