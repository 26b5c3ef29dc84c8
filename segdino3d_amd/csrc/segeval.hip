// Semantic and panoptic evaluation on the device: the per-scene counting of mmdet3d's `seg_eval` (fast_hist) and `panoptic_seg_eval`
// (EvalPanoptic.add_batch_panoptic), added into accumulators that stay on the device from the first scene to the read-back of the
// metrics (the reference collects the inputs, evaluation/evaluator_3d.py:128-163, and leaves the scoring commented out, :184-196).
//
//   sd3d_semantic_confusion   se_confusion_kernel   one pass: key = gt * C + pred; equal keys of a wave are combined and merged with the wave's
//                                                   previous group when the key repeats (se_wave_groups), one lane adds the count of a key;
//                                                   a workgroup keeps the table in LDS when C * C <= SE_LDS_BINS and flushes one atomic per
//                                                   non-zero bin, otherwise the waves add into the int64 table in global memory.
//   sd3d_panoptic_accumulate  pq_mark_kernel        per point: drop ignored ground truth, shift ids, segment keys (class << 16 | id) of both
//                                                   sides, a presence BIT per key (C * 2^16 bits a side), range status;
//                             pq_rank_kernel        one workgroup per (side, class): prefix popcount over the class's 2048 words;
//                             pq_offsets_kernel     one workgroup: exclusive scan of the class counts = first rank of every class.  The rank of
//                                                   a segment = class offset + word prefix + popcount below its bit: segments of a class are
//                                                   consecutive rows in ascending id;
//                             pq_count_kernel       per point: area of its two segments, and for a ground-truth segment 16 counters, one per bit
//                                                   of the shifted id of the same-class prediction at the point;
//                             pq_cand_kernel        per ground-truth segment: candidate id = the bits that MORE THAN HALF of the segment's points
//                                                   carry.  A pair with iou > 0.5 has inter > area_gt / 2, so its prediction id is that candidate;
//                             pq_inter_kernel       per point: intersection of every ground-truth segment with its candidate - an exact count;
//                             pq_finish_kernel      one workgroup per class: 2 * inter > union decides on integers, iou = inter / union in
//                                                   float64, summed per thread in ascending segment order and across threads in a fixed tree;
//                                                   then the unmatched segments of area >= min_num_points.  One writer per class: plain adds.
// No sort, no hash table and no [gt, pred] table: every buffer is indexed by point, by key bit or by segment rank, and the only capacity is
// SD3D_SEG_EVAL_MAX_SEGMENTS rows a side.  Atomics are integer adds / ORs (order-free); there is no float atomic anywhere.
#include "common.h"
#include "../../include/segdino3d_hip.h"
#include <stdio.h>

#define SE_PER 4                                        // points per thread of the per-point kernels: loaded together, then grouped
#define SE_PTS (256 * SE_PER)                           // points per workgroup (point j of thread t: base + j * 256 + t, coalesced)
#define SE_LDS_BINS 16384                               // confusion bins (int32) a workgroup keeps in LDS: C <= 128
#define SE_ID_BITS 16
#define SE_ID_WORDS (1 << (SE_ID_BITS - 5))             // presence words per class and side
#define SE_MAX_POINTS 0x7F000000ll

// Groups the wave's valid lanes by key: one round per distinct key (1 - 3 for superpoint-coherent labels, 64 at the worst), every lane of
// the wave must arrive (the ballots are wave-wide).  The group's (key, count) is the same value on every lane; it is merged into the pending
// pair (pk, pc) when the key repeats - the usual case from one point of a thread to the next - and flush(key, count) is called BY ALL
// LANES for a pair that ends, so the lanes can share its atomics.  The caller flushes the last pending pair (pc != 0) itself.
template <class K, class F>
__device__ static inline void se_wave_groups(K key, bool valid, K& pk, int& pc, F&& flush) {
    unsigned long long todo = __ballot(valid);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const K k = __shfl(key, leader);
        const unsigned long long same = __ballot(valid && key == k);
        const int c = __popcll(same);
        if (pc && k == pk) pc += c;
        else {
            if (pc) flush(pk, pc);
            pk = k;
            pc = c;
        }
        todo &= ~same;
    }
}

__device__ static inline void se_raise(unsigned long long* status, int bits) {
    const unsigned long long any = __ballot(bits != 0);
    if (!any) return;
    bits = wave_or(bits);
    if ((threadIdx.x & 63) == 0) atomicOr(status, (unsigned long long)bits);
}

// ---------------------------------------------------------------------------------------------- semantic confusion
template <bool LDS>
__global__ __launch_bounds__(256) void se_confusion_kernel(const int64_t* __restrict__ pred, int64_t pred_stride, const int64_t* __restrict__ gt,
                                                           int64_t gt_stride, int64_t n, int C, int64_t ignore, unsigned long long* conf,
                                                           unsigned long long* status) {
    __shared__ int tab[LDS ? SE_LDS_BINS : 1];
    const int bins = C * C;
    if (LDS) {
        for (int b = threadIdx.x; b < bins; b += 256) tab[b] = 0;
        __syncthreads();
    }
    const int64_t base = (int64_t)blockIdx.x * SE_PTS;
    const int lane = threadIdx.x & 63;
    int bad = 0, keys[SE_PER];
#pragma unroll
    for (int j = 0; j < SE_PER; ++j) {                                        // all loads first: they overlap
        const int64_t i = base + j * 256 + threadIdx.x;
        int64_t g = -1, p = 0;
        if (i < n) { g = gt[i * gt_stride]; p = pred[i * pred_stride]; }
        keys[j] = -1;
        if (g != ignore && g >= 0 && g < C) {
            if (p < 0 || p >= C) bad = SD3D_SEG_EVAL_BAD_PRED_CLASS;
            else keys[j] = (int)g * C + (int)p;
        }
    }
    auto flush = [&](int k, int c) {
        if (lane != 0) return;
        if (LDS) atomicAdd(&tab[k], c);
        else atomicAdd(&conf[k], (unsigned long long)c);
    };
    int pk = 0, pc = 0;
#pragma unroll
    for (int j = 0; j < SE_PER; ++j) se_wave_groups(keys[j], keys[j] >= 0, pk, pc, flush);
    if (pc) flush(pk, pc);
    se_raise(status, bad);
    if (LDS) {
        __syncthreads();
        for (int b = threadIdx.x; b < bins; b += 256)
            if (tab[b]) atomicAdd(&conf[b], (unsigned long long)tab[b]);
    }
}

// ---------------------------------------------------------------------------------------------- panoptic
struct PqSpec {
    int C, n_ignore, min_pts, cap;                      // cap: segment rows a side the workspace holds
    int64_t ignore[SD3D_SEG_EVAL_MAX_IGNORE];
};

struct PqWs {
    int32_t* header;                                    // [0] G, [1] P (segments of the scene, not read back)
    uint32_t* bits;                                     // [2][C * SE_ID_WORDS] presence of (class, id): ground truth, then prediction
    int32_t *area_g, *inter, *vote, *area_p, *matched_p;
    int32_t *prefix, *class_cnt, *class_off, *cand;
    int32_t *gkey, *pkey, *grank;
    size_t zero_bytes, total;                           // [bits, bits + zero_bytes) is cleared per scene
};

static PqWs pq_carve(void* ws, int64_t n, int C) {
    PqWs w;
    char* p = (char*)ws;
    auto take = [&](size_t bytes) { char* q = p; p += align_up(bytes, 256); return q; };
    const size_t words = (size_t)C * SE_ID_WORDS, cap = (size_t)(n < SD3D_SEG_EVAL_MAX_SEGMENTS ? n : SD3D_SEG_EVAL_MAX_SEGMENTS);
    w.header = (int32_t*)take(8 * 4);
    w.bits = (uint32_t*)take(2 * words * 4);
    w.area_g = (int32_t*)take(cap * 4);
    w.inter = (int32_t*)take(cap * 4);
    w.vote = (int32_t*)take(cap * SE_ID_BITS * 4);
    w.area_p = (int32_t*)take(cap * 4);
    w.matched_p = (int32_t*)take(cap * 4);
    w.zero_bytes = (size_t)(p - (char*)w.bits);
    w.prefix = (int32_t*)take(2 * words * 4);
    w.class_cnt = (int32_t*)take(2 * (size_t)C * 4);
    w.class_off = (int32_t*)take(2 * (size_t)C * 4);
    w.cand = (int32_t*)take(cap * 4);
    w.gkey = (int32_t*)take((size_t)n * 4);
    w.pkey = (int32_t*)take((size_t)n * 4);
    w.grank = (int32_t*)take((size_t)n * 4);
    w.total = (size_t)(p - (char*)ws);
    return w;
}

__device__ static inline bool pq_ignored(const PqSpec& s, int64_t cls) {
    bool ig = false;
#pragma unroll
    for (int k = 0; k < SD3D_SEG_EVAL_MAX_IGNORE; ++k) ig |= (k < s.n_ignore && cls == s.ignore[k]);
    return ig;
}

__device__ static inline int pq_word(int key) { return (key >> SE_ID_BITS) * SE_ID_WORDS + ((key & 0xFFFF) >> 5); }

// rank of a PRESENT key among the keys of its side
__device__ static inline int pq_rank(const uint32_t* __restrict__ bits, const int32_t* __restrict__ prefix, const int32_t* __restrict__ class_off,
                                     int key) {
    const int w = pq_word(key);
    return class_off[key >> SE_ID_BITS] + prefix[w] + __popc(bits[w] & ((1u << (key & 31)) - 1u));
}

__global__ __launch_bounds__(256) void pq_mark_kernel(const int64_t* __restrict__ pred_sem, int64_t s_ps, const int64_t* __restrict__ pred_inst,
                                                      int64_t s_pi, const int64_t* __restrict__ gt_sem, int64_t s_gs,
                                                      const int64_t* __restrict__ gt_inst, int64_t s_gi, int64_t n, PqSpec spec,
                                                      int32_t* __restrict__ gkey, int32_t* __restrict__ pkey, uint32_t* bits,
                                                      unsigned long long* status) {
    uint32_t* bits_g = bits;
    uint32_t* bits_p = bits + (size_t)spec.C * SE_ID_WORDS;
    const int64_t base = (int64_t)blockIdx.x * SE_PTS;
    const int lane = threadIdx.x & 63;
    int bad = 0, gks[SE_PER], pks[SE_PER];
    int64_t gs[SE_PER], gi[SE_PER], ps[SE_PER], pi[SE_PER];
#pragma unroll
    for (int j = 0; j < SE_PER; ++j) {
        const int64_t i = base + j * 256 + threadIdx.x;
        gs[j] = gi[j] = ps[j] = pi[j] = -1;
        if (i < n) { gs[j] = gt_sem[i * s_gs]; gi[j] = gt_inst[i * s_gi]; ps[j] = pred_sem[i * s_ps]; pi[j] = pred_inst[i * s_pi]; }
    }
#pragma unroll
    for (int j = 0; j < SE_PER; ++j) {
        const int64_t i = base + j * 256 + threadIdx.x;
        gks[j] = pks[j] = -1;
        if (i < n) {
            if (!pq_ignored(spec, gs[j])) {
                int64_t g1 = gi[j] + 1, p1 = pi[j] + 1;
                if (g1 < 0 || g1 >= (1 << SE_ID_BITS)) { bad = SD3D_SEG_EVAL_BAD_INSTANCE_ID; g1 = 0; }
                if (p1 < 0 || p1 >= (1 << SE_ID_BITS)) { bad = SD3D_SEG_EVAL_BAD_INSTANCE_ID; p1 = 0; }
                if (gs[j] >= 0 && gs[j] < spec.C && g1 > 0) gks[j] = ((int)gs[j] << SE_ID_BITS) | (int)g1;
                if (ps[j] >= 0 && ps[j] < spec.C && p1 > 0 && !pq_ignored(spec, ps[j])) pks[j] = ((int)ps[j] << SE_ID_BITS) | (int)p1;
            }
            gkey[i] = gks[j];
            pkey[i] = pks[j];
        }
    }
    auto set_g = [&](int k, int) { if (lane == 0) atomicOr(&bits_g[pq_word(k)], 1u << (k & 31)); };
    auto set_p = [&](int k, int) { if (lane == 0) atomicOr(&bits_p[pq_word(k)], 1u << (k & 31)); };
    int gk = 0, gc = 0, pk = 0, pc = 0;
#pragma unroll
    for (int j = 0; j < SE_PER; ++j) {
        se_wave_groups(gks[j], gks[j] >= 0, gk, gc, set_g);
        se_wave_groups(pks[j], pks[j] >= 0, pk, pc, set_p);
    }
    if (gc) set_g(gk, gc);
    if (pc) set_p(pk, pc);
    se_raise(status, bad);
}

// grid (C, 2): prefix[w] = keys of this class and side below word w; class_cnt = their number.  Thread t takes 8 consecutive words.
__global__ __launch_bounds__(256) void pq_rank_kernel(const uint32_t* __restrict__ bits, int32_t* __restrict__ prefix, int32_t* __restrict__ class_cnt,
                                                      int C) {
    __shared__ int wave_sum[4];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const size_t w0 = ((size_t)blockIdx.y * C + blockIdx.x) * SE_ID_WORDS + (size_t)t * (SE_ID_WORDS / 256);
    int pc[SE_ID_WORDS / 256], s = 0;
#pragma unroll
    for (int k = 0; k < SE_ID_WORDS / 256; ++k) { pc[k] = __popc(bits[w0 + k]); s += pc[k]; }
    int inc = wave_scan_incl(s, lane);
    if (lane == 63) wave_sum[wv] = inc;
    __syncthreads();
    int run = inc - s, total = 0;
    for (int k = 0; k < 4; ++k) {
        if (k < wv) run += wave_sum[k];
        total += wave_sum[k];
    }
#pragma unroll
    for (int k = 0; k < SE_ID_WORDS / 256; ++k) { prefix[w0 + k] = run; run += pc[k]; }
    if (t == 0) class_cnt[blockIdx.y * C + blockIdx.x] = total;
}

// one workgroup of 1024: class_off[side][c] = segments of the classes below c; header = {G, P}; more than cap on a side raises the status
__global__ __launch_bounds__(1024) void pq_offsets_kernel(const int32_t* __restrict__ class_cnt, int32_t* __restrict__ class_off, int C, int cap,
                                                          int32_t* header, unsigned long long* status) {
    __shared__ int wave_sum[2][16];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int v0 = t < C ? class_cnt[t] : 0, v1 = t < C ? class_cnt[C + t] : 0;
    int i0 = v0, i1 = v1;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int a = __shfl_up(i0, d), b = __shfl_up(i1, d);
        if (lane >= d) { i0 += a; i1 += b; }
    }
    if (lane == 63) { wave_sum[0][wv] = i0; wave_sum[1][wv] = i1; }
    __syncthreads();
    int r0 = i0 - v0, r1 = i1 - v1, t0 = 0, t1 = 0;
    for (int k = 0; k < 16; ++k) {
        if (k < wv) { r0 += wave_sum[0][k]; r1 += wave_sum[1][k]; }
        t0 += wave_sum[0][k];
        t1 += wave_sum[1][k];
    }
    if (t < C) { class_off[t] = r0; class_off[C + t] = r1; }
    if (t == 0) {
        header[0] = t0;
        header[1] = t1;
        if (t0 > cap || t1 > cap) atomicOr(status, (unsigned long long)SD3D_SEG_EVAL_TOO_MANY_SEGMENTS);
    }
}

__global__ __launch_bounds__(256) void pq_count_kernel(const int32_t* __restrict__ gkey, const int32_t* __restrict__ pkey, int64_t n, PqSpec spec,
                                                       const uint32_t* __restrict__ bits, const int32_t* __restrict__ prefix,
                                                       const int32_t* __restrict__ class_off, int32_t* __restrict__ grank, int32_t* area_g,
                                                       int32_t* area_p, int32_t* vote) {
    const size_t words = (size_t)spec.C * SE_ID_WORDS;
    const int64_t base = (int64_t)blockIdx.x * SE_PTS;
    const int lane = threadIdx.x & 63;
    int gks[SE_PER], pks[SE_PER];
    long long keys[SE_PER];
#pragma unroll
    for (int j = 0; j < SE_PER; ++j) {
        const int64_t i = base + j * 256 + threadIdx.x;
        gks[j] = pks[j] = -1;
        if (i < n) { gks[j] = gkey[i]; pks[j] = pkey[i]; }
    }
#pragma unroll
    for (int j = 0; j < SE_PER; ++j) {
        const int64_t i = base + j * 256 + threadIdx.x;
        const int gk = gks[j], pk = pks[j];
        int g = -1, p = -1;
        if (gk >= 0) g = pq_rank(bits, prefix, class_off, gk);
        if (pk >= 0) p = pq_rank(bits + words, prefix + words, class_off + spec.C, pk);
        if (g >= spec.cap) g = -1;                                           // past the capacity: left out (the status says so)
        if (p >= spec.cap) p = -1;
        if (i < n) grank[i] = g;
        // the id bits vote only where the prediction has the segment's class
        const int pid = (g >= 0 && pk >= 0 && (gk >> SE_ID_BITS) == (pk >> SE_ID_BITS)) ? (pk & 0xFFFF) : 0;
        keys[j] = ((long long)(g + 1) << 40) | ((long long)(p + 1) << 16) | pid;   // g + 1, p + 1 <= 2^16: 17 bits each; 0: nothing to count
    }
    // lanes 0..15 add the 16 vote counters of the segment (64 contiguous bytes), lanes 16 / 17 the two areas
    auto flush = [&](long long k, int c) {
        const int g = (int)(k >> 40) - 1, p = (int)((k >> 16) & 0x1FFFF) - 1, pid = (int)(k & 0xFFFF);
        if (lane < SE_ID_BITS) {
            if (g >= 0 && ((pid >> lane) & 1)) atomicAdd(&vote[(size_t)g * SE_ID_BITS + lane], c);
        } else if (lane == SE_ID_BITS) {
            if (g >= 0) atomicAdd(&area_g[g], c);
        } else if (lane == SE_ID_BITS + 1) {
            if (p >= 0) atomicAdd(&area_p[p], c);
        }
    };
    long long pk = 0;
    int pc = 0;
#pragma unroll
    for (int j = 0; j < SE_PER; ++j) se_wave_groups(keys[j], (keys[j] >> 16) != 0, pk, pc, flush);
    if (pc) flush(pk, pc);
}

__global__ __launch_bounds__(256) void pq_cand_kernel(const int32_t* __restrict__ header, int cap, const int32_t* __restrict__ area_g,
                                                      const int32_t* __restrict__ vote, int32_t* __restrict__ cand) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= cap || g >= header[0]) return;
    const int64_t a = area_g[g];
    int pid = 0;
#pragma unroll
    for (int b = 0; b < SE_ID_BITS; ++b)
        if (2 * (int64_t)vote[(size_t)g * SE_ID_BITS + b] > a) pid |= 1 << b;
    cand[g] = pid;
}

__global__ __launch_bounds__(256) void pq_inter_kernel(const int32_t* __restrict__ gkey, const int32_t* __restrict__ pkey,
                                                       const int32_t* __restrict__ grank, int64_t n, const int32_t* __restrict__ cand,
                                                       int32_t* inter) {
    const int64_t base = (int64_t)blockIdx.x * SE_PTS;
    const int lane = threadIdx.x & 63;
    int gs[SE_PER];
#pragma unroll
    for (int j = 0; j < SE_PER; ++j) {
        const int64_t i = base + j * 256 + threadIdx.x;
        gs[j] = -1;
        if (i < n) {
            const int r = grank[i], gk = gkey[i], pk = pkey[i];
            if (r >= 0 && pk >= 0 && (gk >> SE_ID_BITS) == (pk >> SE_ID_BITS) && (pk & 0xFFFF) == cand[r]) gs[j] = r;
        }
    }
    auto flush = [&](int k, int c) { if (lane == 0) atomicAdd(&inter[k], c); };
    int pk = 0, pc = 0;
#pragma unroll
    for (int j = 0; j < SE_PER; ++j) se_wave_groups(gs[j], gs[j] >= 0, pk, pc, flush);
    if (pc) flush(pk, pc);
}

// One workgroup per class.  Ground-truth segments of the class are rows g0 .. g0 + ng in ascending id, prediction segments p0 .. p0 + np.
__global__ __launch_bounds__(256) void pq_finish_kernel(PqSpec spec, const uint32_t* __restrict__ bits, const int32_t* __restrict__ prefix,
                                                        const int32_t* __restrict__ class_cnt, const int32_t* __restrict__ class_off,
                                                        const int32_t* __restrict__ area_g, const int32_t* __restrict__ area_p,
                                                        const int32_t* __restrict__ inter, const int32_t* __restrict__ cand, int32_t* matched_p,
                                                        int64_t* tp, int64_t* fp, int64_t* fn, double* iou_sum) {
    __shared__ double part[256];
    __shared__ int cnt[3];
    const int cl = blockIdx.x, t = threadIdx.x;
    const size_t words = (size_t)spec.C * SE_ID_WORDS;
    const uint32_t* bits_p = bits + words;
    if (t < 3) cnt[t] = 0;
    __syncthreads();
    const int g0 = class_off[cl], ng = class_cnt[cl], p0 = class_off[spec.C + cl], np = class_cnt[spec.C + cl];
    int n_tp = 0, n_fn = 0, n_fp = 0;
    double s = 0.0;
    for (int j = t; j < ng; j += 256) {
        const int g = g0 + j;
        if (g >= spec.cap) break;
        const int64_t a = area_g[g];
        const int pid = cand[g];
        bool matched = false;
        if (pid > 0) {
            const int key = (cl << SE_ID_BITS) | pid;
            if ((bits_p[pq_word(key)] >> (pid & 31)) & 1u) {
                const int p = pq_rank(bits_p, prefix + words, class_off + spec.C, key);
                if (p < spec.cap) {
                    const int64_t it = inter[g], uni = a + (int64_t)area_p[p] - it;
                    if (2 * it > uni) {                                       // iou > 0.5, strictly, on integers: unique per segment on both sides
                        matched = true;
                        ++n_tp;
                        s += (double)it / (double)uni;
                        matched_p[p] = 1;
                    }
                }
            }
        }
        if (!matched && a >= spec.min_pts) ++n_fn;
    }
    part[t] = s;
    __syncthreads();                                                          // also orders the matched_p stores before the reads below
    for (int d = 128; d >= 1; d >>= 1) {
        if (t < d) part[t] += part[t + d];
        __syncthreads();
    }
    for (int j = t; j < np; j += 256) {
        const int p = p0 + j;
        if (p >= spec.cap) break;
        if (!matched_p[p] && area_p[p] >= spec.min_pts) ++n_fp;
    }
    if (n_tp) atomicAdd(&cnt[0], n_tp);
    if (n_fp) atomicAdd(&cnt[1], n_fp);
    if (n_fn) atomicAdd(&cnt[2], n_fn);
    __syncthreads();
    if (t == 0) {
        if (cnt[0]) { tp[cl] += cnt[0]; iou_sum[cl] += part[0]; }
        if (cnt[1]) fp[cl] += cnt[1];
        if (cnt[2]) fn[cl] += cnt[2];
    }
}

// ---------------------------------------------------------------------------------------------- C entry points
extern "C" size_t sd3d_seg_eval_ws_bytes(int64_t n, int n_classes) {
    if (n < 1) n = 1;
    if (n > SE_MAX_POINTS || n_classes < 1 || n_classes > SD3D_SEG_EVAL_MAX_CLASSES) return 0;
    return pq_carve(nullptr, n, n_classes).total;
}

extern "C" int sd3d_semantic_confusion(const int64_t* pred_sem, int64_t pred_stride, const int64_t* gt_sem, int64_t gt_stride, int64_t n,
                                       int n_classes, int64_t ignore_index, int64_t* confusion, int64_t* status, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (n < 0 || n > SE_MAX_POINTS || n_classes < 1 || n_classes > SD3D_SEG_EVAL_MAX_CLASSES || pred_stride < 0 || gt_stride < 0)
        return sd3d_set_error(SD3D_ERR_ARG, "semantic_confusion: 0 <= n <= 0x7F000000 points, 1..1024 classes, strides >= 0");
    if (!confusion || !status || (n > 0 && (!pred_sem || !gt_sem))) return sd3d_set_error(SD3D_ERR_ARG, "semantic_confusion: NULL argument");
    if (n == 0) return SD3D_OK;
    const dim3 grid((unsigned)cdiv(n, SE_PTS));
    if (n_classes * n_classes <= SE_LDS_BINS)
        hipLaunchKernelGGL(se_confusion_kernel<true>, grid, dim3(256), 0, st, pred_sem, pred_stride, gt_sem, gt_stride, n, n_classes, ignore_index,
                           (unsigned long long*)confusion, (unsigned long long*)status);
    else
        hipLaunchKernelGGL(se_confusion_kernel<false>, grid, dim3(256), 0, st, pred_sem, pred_stride, gt_sem, gt_stride, n, n_classes, ignore_index,
                           (unsigned long long*)confusion, (unsigned long long*)status);
    SD3D_CHECK_LAUNCH();
    return SD3D_OK;
}

extern "C" int sd3d_panoptic_accumulate(const int64_t* pred_sem, int64_t pred_sem_stride, const int64_t* pred_inst, int64_t pred_inst_stride,
                                        const int64_t* gt_sem, int64_t gt_sem_stride, const int64_t* gt_inst, int64_t gt_inst_stride, int64_t n,
                                        int n_classes, const int32_t* ignore_ids_host, int n_ignore, int min_num_points, int64_t* tp, int64_t* fp,
                                        int64_t* fn, double* iou_sum, int64_t* status, void* ws, size_t ws_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (n < 0 || n > SE_MAX_POINTS || n_classes < 1 || n_classes > SD3D_SEG_EVAL_MAX_CLASSES || n_ignore < 0 || n_ignore > SD3D_SEG_EVAL_MAX_IGNORE ||
        (n_ignore > 0 && !ignore_ids_host) || pred_sem_stride < 0 || pred_inst_stride < 0 || gt_sem_stride < 0 || gt_inst_stride < 0)
        return sd3d_set_error(SD3D_ERR_ARG, "panoptic_accumulate: 0 <= n <= 0x7F000000 points, 1..1024 classes, 0..8 ignored classes, strides >= 0");
    if (!tp || !fp || !fn || !iou_sum || !status || (n > 0 && (!pred_sem || !pred_inst || !gt_sem || !gt_inst || !ws)))
        return sd3d_set_error(SD3D_ERR_ARG, "panoptic_accumulate: NULL argument");
    if (n == 0) return SD3D_OK;
    const PqWs w = pq_carve(ws, n, n_classes);
    if (ws_bytes < w.total) return sd3d_set_error(SD3D_ERR_WS, "panoptic_accumulate: workspace too small");
    PqSpec spec;
    spec.C = n_classes;
    spec.n_ignore = n_ignore;
    spec.min_pts = min_num_points;
    spec.cap = (int)(n < SD3D_SEG_EVAL_MAX_SEGMENTS ? n : SD3D_SEG_EVAL_MAX_SEGMENTS);
    for (int k = 0; k < SD3D_SEG_EVAL_MAX_IGNORE; ++k) spec.ignore[k] = k < n_ignore ? (int64_t)ignore_ids_host[k] : 0;
    unsigned long long* stat = (unsigned long long*)status;

    if (hipMemsetAsync(w.bits, 0, w.zero_bytes, st) != hipSuccess) return sd3d_set_error(SD3D_ERR_LAUNCH, "panoptic_accumulate: memset failed");
    const dim3 pgrid((unsigned)cdiv(n, SE_PTS));
    hipLaunchKernelGGL(pq_mark_kernel, pgrid, dim3(256), 0, st, pred_sem, pred_sem_stride, pred_inst, pred_inst_stride, gt_sem, gt_sem_stride, gt_inst,
                       gt_inst_stride, n, spec, w.gkey, w.pkey, w.bits, stat);
    hipLaunchKernelGGL(pq_rank_kernel, dim3((unsigned)n_classes, 2), dim3(256), 0, st, w.bits, w.prefix, w.class_cnt, n_classes);
    hipLaunchKernelGGL(pq_offsets_kernel, dim3(1), dim3(1024), 0, st, w.class_cnt, w.class_off, n_classes, spec.cap, w.header, stat);
    SD3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(pq_count_kernel, pgrid, dim3(256), 0, st, w.gkey, w.pkey, n, spec, w.bits, w.prefix, w.class_off, w.grank, w.area_g, w.area_p,
                       w.vote);
    hipLaunchKernelGGL(pq_cand_kernel, dim3((unsigned)cdiv(spec.cap, 256)), dim3(256), 0, st, w.header, spec.cap, w.area_g, w.vote, w.cand);
    hipLaunchKernelGGL(pq_inter_kernel, pgrid, dim3(256), 0, st, w.gkey, w.pkey, w.grank, n, w.cand, w.inter);
    hipLaunchKernelGGL(pq_finish_kernel, dim3((unsigned)n_classes), dim3(256), 0, st, spec, w.bits, w.prefix, w.class_cnt, w.class_off, w.area_g,
                       w.area_p, w.inter, w.cand, w.matched_p, tp, fp, fn, iou_sum);
    SD3D_CHECK_LAUNCH();
    return SD3D_OK;
}
