// ScanNet instance AP per scene on the device: the reference's `compute_each_sample_metrics` (evaluation/evaluator_3d.py:227-321), which
// runs `instance_seg_eval` on one scene at a time.  sd3d_ap_scene (csrc/apeval.hip) already matches every (scene, class, overlap) triple
// on its own and a scene owns a contiguous slot range of the store; what is added here is a finish step segmented by scene, over counters
// that are kept per scene (row s of [S, C O + 2 C]: hard_fn, has_gt, has_pred) instead of summed.
//
//   sd3d_ap_finish_scenes  ap_scene_keys_kernel     per slot: its scene by binary search in the slot offsets, the composite key
//                                                   (scene * (C O + 1) + group) << 33 | low 33 bits of the code.  The store's codes are
//                                                   only read: the scene prefix exists in the workspace alone;
//                          sort_pairs_u64           over 33 + ceil(log2(S (C O + 1))) bits: afterwards scene s again occupies
//                                                   [off[s], off[s + 1]), ordered by (group, score, true);
//                          ap_scene_curve_kernel    one workgroup per (scene, class, overlap): the segment by binary search inside the
//                                                   scene's range, then the curve body of ap_curve.h - the one sd3d_ap_finish runs;
//                          ap_scene_summary_kernel  one wave per scene: the five NaN-skipping means of `compute_averages`.
//   sd3d_ap_reduce_counters  [S, n] -> [n] in integers (hard_fn added, the flags OR-ed): what an ApAccumulator fed the same scenes holds.
// No float atomics and no append counters: the same bits on every run.
#include "common.h"
#include "ap_curve.h"
#include "../../include/segdino3d_hip.h"

#define APS_MAX_SLOTS 0x7F000000ll
#define APS_MAX_GRID (1 << 20)                          // workgroups per launch; the kernels stride over what lies beyond
#define APS_KEY_LIMIT (1ll << 30)                       // S (C O + 1) below this: prefix and the 33 low bits fit a 63-bit key

__global__ __launch_bounds__(256) void ap_scene_keys_kernel(const int64_t* __restrict__ codes, int64_t n, const int64_t* __restrict__ off, int S,
                                                            int G, uint64_t* __restrict__ keys) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int lo = 0, hi = S - 1;                             // the last scene whose first slot is <= i (empty scenes share a first slot)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= i) lo = mid;
        else hi = mid - 1;
    }
    const uint64_t code = (uint64_t)codes[i];
    uint64_t g = code >> 33;
    if (g > (uint64_t)G) g = (uint64_t)G;               // whatever is no group is the sentinel
    keys[i] = (((uint64_t)lo * (uint64_t)(G + 1) + g) << 33) | (code & 0x1FFFFFFFFull);
}

__global__ __launch_bounds__(256) void ap_scene_curve_kernel(const uint64_t* __restrict__ keys, int64_t n, const int64_t* __restrict__ off, int S,
                                                             int C, int O, const int64_t* __restrict__ counters, double* __restrict__ P,
                                                             double* __restrict__ R, double* __restrict__ ap_out, double* __restrict__ pr_out,
                                                             double* __restrict__ rc_out) {
    const int G = C * O;
    const int64_t total = (int64_t)S * G;
    for (int64_t idx = blockIdx.x; idx < total; idx += gridDim.x) {
        const int s = (int)(idx / G), g = (int)(idx - (int64_t)s * G), c = g / O;
        const int64_t* row = counters + (int64_t)s * (G + 2 * C);
        const bool gt = row[G + c] != 0, pred = row[G + C + c] != 0;
        int64_t lo = 0, hi = 0, hf = 0;
        if (gt && pred) {
            int64_t b = off[s], e = off[s + 1];         // the scene's range, kept inside the buffers whatever the offsets say
            b = b < 0 ? 0 : (b > n ? n : b);
            e = e < b ? b : (e > n ? n : e);
            const uint64_t key = ((uint64_t)s * (uint64_t)(G + 1) + (uint64_t)g) << 33;
            lo = b + ap_lower_bound(keys + b, e - b, key);
            hi = b + ap_lower_bound(keys + b, e - b, key + (1ull << 33));
            hf = row[g];
        }
        ap_curve_body(keys, lo, hi, hf, gt, pred, P, R, ap_out + idx, pr_out + idx, rc_out + idx);
        __syncthreads();                                // the body's LDS before the next group of this workgroup
    }
}

// columns: all_ap (overlaps outside the 0.25 set), all_ap_50%, all_ap_25%, all_prec_50%, all_rec_50%
__global__ __launch_bounds__(64) void ap_scene_summary_kernel(const double* __restrict__ ap, const double* __restrict__ pr, const double* __restrict__ rc,
                                                              int S, int G, int O, unsigned mask50, unsigned mask25, double* __restrict__ summary) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x;
    for (int64_t s = blockIdx.x; s < S; s += gridDim.x) {
        double sum[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        int cnt[5] = {0, 0, 0, 0, 0};
        auto acc = [&](int k, double v) {
            if (v == v) { sum[k] = sum[k] + v; ++cnt[k]; }
        };
        for (int i = lane; i < G; i += 64) {            // class-major, a fixed order per lane
            const unsigned bit = 1u << (i % O);
            const double a = ap[s * G + i];
            if (!(bit & mask25)) acc(0, a);
            if (bit & mask50) { acc(1, a); acc(3, pr[s * G + i]); acc(4, rc[s * G + i]); }
            if (bit & mask25) acc(2, a);
        }
#pragma unroll
        for (int k = 0; k < 5; ++k) {
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {         // a + b on both lanes of a pair: every lane ends with the same bits
                sum[k] = sum[k] + __shfl_xor(sum[k], d);
                cnt[k] += __shfl_xor(cnt[k], d);
            }
        }
        if (lane < 5) {
            double v = __longlong_as_double(0x7FF8000000000000ll);
#pragma unroll
            for (int k = 0; k < 5; ++k)
                if (k == lane && cnt[k] > 0) v = sum[k] / (double)cnt[k];
            summary[s * 5 + lane] = v;
        }
    }
}

__global__ __launch_bounds__(256) void ap_reduce_counters_kernel(const int64_t* __restrict__ in, int S, int n, int n_add, int64_t* __restrict__ out) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    int64_t acc = 0;
    if (j < n_add)
        for (int s = 0; s < S; ++s) acc += in[(int64_t)s * n + j];
    else
        for (int s = 0; s < S; ++s) acc |= (int64_t)(in[(int64_t)s * n + j] != 0);
    out[j] = acc;
}

// ---------------------------------------------------------------------------------------------- C entry points
struct ApScenesWs {
    uint64_t *keys_a, *keys_b;
    uint32_t *vals, *scratch;
    double *P, *R;
    void* sort_ws;
    size_t sort_bytes, total;
};

static ApScenesWs ap_scenes_carve(void* ws, int64_t n) {
    ApScenesWs w;
    char* p = (char*)ws;
    auto take = [&](size_t bytes) { char* q = p; p += align_up(bytes, 256); return q; };
    const size_t m = (size_t)(n > 0 ? n : 1);
    w.keys_a = (uint64_t*)take(m * 8);
    w.keys_b = (uint64_t*)take(m * 8);
    w.vals = (uint32_t*)take(m * 4);
    w.scratch = (uint32_t*)take(m * 4);
    w.P = (double*)take(m * 8);
    w.R = (double*)take(m * 8);
    w.sort_bytes = sort_ws_bytes((int64_t)m);
    w.sort_ws = take(w.sort_bytes);
    w.total = (size_t)(p - (char*)ws);
    return w;
}

extern "C" size_t sd3d_ap_finish_scenes_ws_bytes(int64_t n_slots) {
    if (n_slots < 0 || n_slots > APS_MAX_SLOTS) return 0;
    return ap_scenes_carve(nullptr, n_slots).total;
}

extern "C" int sd3d_ap_finish_scenes(const int64_t* codes, int64_t n_slots, const int64_t* slot_offsets, int n_scenes, int n_classes, int n_overlaps,
                                     const int64_t* counters, int mask50, int mask25, double* ap, double* pr_rc, double* summary, void* ws,
                                     size_t ws_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (n_slots < 0 || n_slots > APS_MAX_SLOTS || n_scenes < 1 || n_classes < 1 || n_classes > SD3D_AP_MAX_CLASSES || n_overlaps < 1 ||
        n_overlaps > SD3D_AP_MAX_OVERLAPS || mask50 < 0 || mask25 < 0 || mask50 >= (1 << n_overlaps) || mask25 >= (1 << n_overlaps))
        return sd3d_set_error(SD3D_ERR_ARG, "ap_finish_scenes: 0 <= n_slots <= 0x7F000000, >= 1 scene, 1..1024 classes, 1..16 overlaps, masks over the overlaps");
    const int groups = n_classes * n_overlaps;
    const int64_t prefixes = (int64_t)n_scenes * (groups + 1);
    if (prefixes >= APS_KEY_LIMIT) return sd3d_set_error(SD3D_ERR_ARG, "ap_finish_scenes: scenes * (classes * overlaps + 1) must stay below 2^30");
    if (!slot_offsets || !counters || !ap || !pr_rc || !summary || !ws || (n_slots > 0 && !codes))
        return sd3d_set_error(SD3D_ERR_ARG, "ap_finish_scenes: NULL argument");
    const ApScenesWs w = ap_scenes_carve(ws, n_slots);
    if (ws_bytes < w.total) return sd3d_set_error(SD3D_ERR_WS, "ap_finish_scenes: workspace too small");
    int prefix_bits = 1;
    while ((1ll << prefix_bits) < prefixes) ++prefix_bits;
    const uint64_t* sorted = w.keys_a;
    if (n_slots > 0) {
        hipLaunchKernelGGL(ap_scene_keys_kernel, dim3((unsigned)cdiv(n_slots, 256)), dim3(256), 0, st, codes, n_slots, slot_offsets, n_scenes, groups,
                           w.keys_a);
        int landed = 0;
        if (int rc = sort_pairs_u64(w.keys_a, nullptr, w.keys_b, w.vals, n_slots, 0, 33 + prefix_bits, w.sort_ws, w.sort_bytes, st, w.scratch, &landed))
            return rc;
        if (!landed) sorted = w.keys_b;
    }
    const int64_t total = (int64_t)n_scenes * groups;
    double* pr = pr_rc;
    double* rc_out = pr_rc + total;
    hipLaunchKernelGGL(ap_scene_curve_kernel, dim3((unsigned)(total < APS_MAX_GRID ? total : APS_MAX_GRID)), dim3(256), 0, st, sorted, n_slots,
                       slot_offsets, n_scenes, n_classes, n_overlaps, counters, w.P, w.R, ap, pr, rc_out);
    hipLaunchKernelGGL(ap_scene_summary_kernel, dim3((unsigned)(n_scenes < APS_MAX_GRID ? n_scenes : APS_MAX_GRID)), dim3(64), 0, st, ap, pr, rc_out,
                       n_scenes, groups, n_overlaps, (unsigned)mask50, (unsigned)mask25, summary);
    SD3D_CHECK_LAUNCH();
    return SD3D_OK;
}

extern "C" int sd3d_ap_reduce_counters(const int64_t* counters, int n_scenes, int n_classes, int n_overlaps, int64_t* out, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (n_scenes < 0 || n_classes < 1 || n_classes > SD3D_AP_MAX_CLASSES || n_overlaps < 1 || n_overlaps > SD3D_AP_MAX_OVERLAPS)
        return sd3d_set_error(SD3D_ERR_ARG, "ap_reduce_counters: >= 0 scenes, 1..1024 classes, 1..16 overlaps");
    if (!out || (n_scenes > 0 && !counters)) return sd3d_set_error(SD3D_ERR_ARG, "ap_reduce_counters: NULL argument");
    const int groups = n_classes * n_overlaps, n = groups + 2 * n_classes;
    hipLaunchKernelGGL(ap_reduce_counters_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, st, counters, n_scenes, n, groups, out);
    SD3D_CHECK_LAUNCH();
    return SD3D_OK;
}
