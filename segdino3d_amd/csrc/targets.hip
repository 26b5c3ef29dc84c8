// Dataset targets on the device: raw per-point labels -> instance masks, labels, areas and superpoint votes
// (the label side of the reference's `Dataset.__getitem__`, scannet200.py:155-193, 243-253, 291-326 + instance_seg_3d_preparer.py).
//
// Two C calls per scene with ONE 16-byte read-back between them (the sizes of the outputs are data):
//   sd3d_targets_scan   tg_labels_kernel  one pass over the points: swap 2 <-> 3, lookup table, stuff / background masking, a presence BIT per
//                                         masked raw instance id (2^20 + 1 bits), largest superpoint id, present stuff classes, range status;
//                       tg_rank_kernel    one workgroup: prefix popcount over the presence words in use = the rank of every id, and the header
//                                         {status, G', S, stuff-present bits};
//   sd3d_targets_build  tg_relabel_kernel second pass: new id = rank - 1 (the rule that reproduces `exclude_stuffs_`, quirk included), the
//                                         mask row of every point for the requested view, area and first point index per row;
//                       sort + starts     points grouped by superpoint with the library's radix sort and segment starts;
//                       tg_votes_kernel   one wave per superpoint: Boyer-Moore majority candidate across lanes, then a counting pass
//                                         that confirms 2 k > n - for the instance id and the class at once, no [S, G] histogram;
//                       tg_expand_kernel  store-only expansion of `masks` [G, N] and `sp_inst_sem_masks` [G' + C + 1, S] bytes;
//                       tg_finish_kernel  labels / area as int64.
// Everything is integer and a pure function of the input: the atomics are OR of presence bits, integer counts and the minimum of a point
// index, whose results do not depend on arrival order.  No floating point anywhere (the reference's fp32 `scatter_mean(...) > 0.5`
// equals 2 k > n for every superpoint of fewer than 2^22 points).
// Atomics (guide, Guideline 12): status / stuff bits / largest ids are reduced per workgroup first, one atomic per workgroup and only
// when it would change what a plain load already sees; presence bits are collected in an LDS bitmap per workgroup and flushed once per
// non-zero word; area and first index are accumulated in LDS per workgroup (rows <= TG_LDS_ROWS) and flushed once per touched row.
#include "common.h"
#include "../../include/segdino3d_hip.h"
#include <stdio.h>

#define TG_STATUS 0
#define TG_G 1
#define TG_S 2
#define TG_STUFF 3
#define TG_EMAX 4                                       // largest id + 1 seen (not read back)

#define TG_MAX_INST (1 << 20)                           // raw instance ids lie in [-1, 2^20)
#define TG_WORDS ((TG_MAX_INST + 1 + 31) / 32)          // presence bits of id + 1 in [0, 2^20]
#define TG_RANK_THREADS 1024
#define TG_LDS_WORDS 1024                               // presence words a workgroup of pass 1 keeps in LDS
#define TG_LABEL_PTS 1024                               // points per workgroup of pass 1 (512 .. 4096 measured alike)
#define TG_MAX_STUFF 8
#define TG_LDS_ROWS 2048                                // rows whose area / first index fit the workgroup's LDS tables
#define TG_RELABEL_PTS 1024                             // points per workgroup of the second pass
#define TG_EXPAND_BYTES 4096                            // output bytes per workgroup of the expansion
#define TG_MAX_POINTS 0x7F000000ll                      // point indices stay below the 0x7F7F7F7F "no point yet" fill, columns in 32 bits

struct TgSpec {
    int C, n_stuff, swap23;
    int stuff[TG_MAX_STUFF];
};

struct TgWs {
    int32_t* header;
    uint32_t* bits;
    int32_t* prefix;
    int32_t *sem, *inst, *vote, *row, *cnt, *first;
    uint64_t *keys_a, *keys_b;
    uint32_t *vals_a, *vals_b;
    void* sort_ws;
    size_t sort_ws_bytes, total;
};

static TgWs tg_carve(void* ws, int64_t n) {
    TgWs w;
    char* p = (char*)ws;
    auto take = [&](size_t bytes) { char* q = p; p += align_up(bytes, 256); return q; };
    w.header = (int32_t*)take(8 * sizeof(int32_t));
    w.bits = (uint32_t*)take((size_t)TG_WORDS * 4);
    w.prefix = (int32_t*)take((size_t)TG_WORDS * 4);
    w.sem = (int32_t*)take((size_t)n * 4);
    w.inst = (int32_t*)take((size_t)n * 4);
    w.vote = (int32_t*)take((size_t)n * 4);
    w.row = (int32_t*)take((size_t)n * 4);
    w.cnt = (int32_t*)take((size_t)(n + TG_MAX_STUFF) * 4);
    w.first = (int32_t*)take((size_t)(n + TG_MAX_STUFF) * 4);
    w.keys_a = (uint64_t*)take((size_t)n * 8);
    w.keys_b = (uint64_t*)take((size_t)n * 8);
    w.vals_a = (uint32_t*)take((size_t)n * 4);
    w.vals_b = (uint32_t*)take((size_t)n * 4);
    w.sort_ws_bytes = sort_ws_bytes(n);
    w.sort_ws = take(w.sort_ws_bytes);
    w.total = (size_t)(p - (char*)ws);
    return w;
}

static int tg_spec(TgSpec& s, int n_classes, const int32_t* stuff_ids, int n_stuff, int swap_2_3, const char* who) {
    char msg[160];
    if (n_classes < 1 || n_stuff < 0 || n_stuff > TG_MAX_STUFF || (n_stuff > 0 && !stuff_ids)) {
        snprintf(msg, sizeof(msg), "%s: n_classes >= 1 and 0..%d stuff ids", who, TG_MAX_STUFF);
        return sd3d_set_error(SD3D_ERR_ARG, msg);
    }
    s.C = n_classes;
    s.n_stuff = n_stuff;
    s.swap23 = swap_2_3 ? 1 : 0;
    for (int k = 0; k < TG_MAX_STUFF; ++k) s.stuff[k] = -1;
    for (int k = 0; k < n_stuff; ++k) {
        if (stuff_ids[k] < 0 || stuff_ids[k] >= n_classes || (k > 0 && stuff_ids[k] <= stuff_ids[k - 1])) {
            snprintf(msg, sizeof(msg), "%s: stuff ids must be ascending class ids below n_classes", who);
            return sd3d_set_error(SD3D_ERR_ARG, msg);
        }
        s.stuff[k] = stuff_ids[k];
    }
    return SD3D_OK;
}

// ---------------------------------------------------------------------------------------------- pass 1
// TG_LABEL_PTS points per workgroup.  Presence bits of the ids below 32 * TG_LDS_WORDS - 1 (every id of a usual scene) are OR-ed into
// an LDS bitmap and flushed with one global atomic per non-zero word: device-scope atomics on one address are served one after the
// other (150 k of them on the dozen words a scene touches took 0.55 ms; a test-before-set does not help, the test reads the XCD's own
// L2).  Larger ids set their global bit directly.
__global__ __launch_bounds__(256) void tg_labels_kernel(const int64_t* __restrict__ inst_raw, const int64_t* __restrict__ sem_raw,
                                                        const int64_t* __restrict__ sp, const int64_t* __restrict__ lut, int64_t lut_len,
                                                        int64_t n, TgSpec spec, int32_t* __restrict__ sem_out, int32_t* __restrict__ inst_out,
                                                        uint64_t* __restrict__ keys, uint32_t* bits, int32_t* header) {
    __shared__ uint32_t lbits[TG_LDS_WORDS];
    for (int w = threadIdx.x; w < TG_LDS_WORDS; w += 256) lbits[w] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * TG_LABEL_PTS;
    int status = 0, stuffm = 0, spm = 0, emax = 0;
#pragma unroll
    for (int j = 0; j < TG_LABEL_PTS / 256; ++j) {
        const int64_t i = base + j * 256 + threadIdx.x;
        if (i >= n) continue;
        int64_t r = sem_raw[i];
        if (spec.swap23) r = (r == 2) ? 3 : ((r == 3) ? 2 : r);
        int sem = spec.C;
        if (r < 0 || r >= lut_len) status |= SD3D_TARGETS_BAD_SEMANTIC;
        else sem = (int)lut[r];
        const int64_t g = inst_raw[i];
        int id = -1;
        if (g < -1 || g >= TG_MAX_INST) status |= SD3D_TARGETS_BAD_INSTANCE;
        else id = (int)g;
        bool bg = (sem == spec.C);
#pragma unroll
        for (int k = 0; k < TG_MAX_STUFF; ++k)
            if (k < spec.n_stuff && sem == spec.stuff[k]) { bg = true; stuffm |= 1 << k; }
        if (bg) id = -1;
        const int64_t s = sp[i];
        uint64_t key = 0;
        if (s < 0 || s > 0x7FFFFFFEll) status |= SD3D_TARGETS_BAD_SUPERPOINT;
        else { key = (uint64_t)s; spm = max(spm, (int)s); }
        keys[i] = key;
        sem_out[i] = sem;
        inst_out[i] = id;
        const int e = id + 1;
        emax = max(emax, e);
        if ((e >> 5) < TG_LDS_WORDS) atomicOr(&lbits[e >> 5], 1u << (e & 31));
        else atomicOr(&bits[e >> 5], 1u << (e & 31));
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        status |= __shfl_xor(status, d);
        stuffm |= __shfl_xor(stuffm, d);
        spm = max(spm, __shfl_xor(spm, d));
        emax = max(emax, __shfl_xor(emax, d));
    }
    __shared__ int red[4][4];
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = status;
        red[1][threadIdx.x >> 6] = stuffm;
        red[2][threadIdx.x >> 6] = spm;
        red[3][threadIdx.x >> 6] = emax;
    }
    __syncthreads();
    for (int w = threadIdx.x; w < TG_LDS_WORDS; w += 256)
        if (lbits[w]) atomicOr(&bits[w], lbits[w]);
    if (threadIdx.x == 0) {
        status = red[0][0] | red[0][1] | red[0][2] | red[0][3];
        stuffm = red[1][0] | red[1][1] | red[1][2] | red[1][3];
        spm = max(max(red[2][0], red[2][1]), max(red[2][2], red[2][3]));
        emax = max(max(red[3][0], red[3][1]), max(red[3][2], red[3][3]));
        // (a stale read costs a redundant atomic at worst: these words only grow inside the launch)
        if (status & ~__builtin_nontemporal_load(&header[TG_STATUS])) atomicOr(&header[TG_STATUS], status);
        if (stuffm & ~__builtin_nontemporal_load(&header[TG_STUFF])) atomicOr(&header[TG_STUFF], stuffm);
        if (spm > __builtin_nontemporal_load(&header[TG_S])) atomicMax(&header[TG_S], spm);
        if (emax > __builtin_nontemporal_load(&header[TG_EMAX])) atomicMax(&header[TG_EMAX], emax);
    }
}

// prefix[w] = number of distinct ids (id + 1) below word w, for the words up to the largest id seen (later words are never read);
// header: G' = distinct ids - 1, S = largest superpoint id + 1.  Thread t takes `per` consecutive words: one for a scene whose ids stay
// below 32 767 (coalesced), up to 33 for ids near 2^20.
__global__ __launch_bounds__(TG_RANK_THREADS) void tg_rank_kernel(const uint32_t* __restrict__ bits, int32_t* __restrict__ prefix, int32_t* header) {
    __shared__ int wave_sum[TG_RANK_THREADS / 64];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int words = (header[TG_EMAX] >> 5) + 1;
    const int per = (words + TG_RANK_THREADS - 1) / TG_RANK_THREADS;
    int s = 0;
    for (int k = 0; k < per; ++k) {
        const int w = t * per + k;
        if (w < words) s += __popc(bits[w]);
    }
    int inc = wave_scan_incl(s, lane);
    if (lane == 63) wave_sum[wv] = inc;
    __syncthreads();
    int run = inc - s, total = 0;
    for (int k = 0; k < TG_RANK_THREADS / 64; ++k) {
        if (k < wv) run += wave_sum[k];
        total += wave_sum[k];
    }
    for (int k = 0; k < per; ++k) {
        const int w = t * per + k;
        if (w < words) { prefix[w] = run; run += __popc(bits[w]); }
    }
    if (t == 0) {
        header[TG_G] = total > 0 ? total - 1 : 0;
        header[TG_S] = header[TG_S] + 1;
    }
}

// ---------------------------------------------------------------------------------------------- pass 2
struct TgView {
    int rows, inst_row0;                 // mask rows of the view; row of new id 0
    int stuff_row[TG_MAX_STUFF];         // val view: row of stuff class k when it is present, else -1
};

template <bool LDS>
__global__ __launch_bounds__(256) void tg_relabel_kernel(const int32_t* __restrict__ sem, const int32_t* __restrict__ inst,
                                                         const uint32_t* __restrict__ bits, const int32_t* __restrict__ prefix, int64_t n,
                                                         TgSpec spec, TgView view, int32_t* __restrict__ vote, int32_t* __restrict__ row_out,
                                                         int32_t* cnt, int32_t* first) {
    __shared__ int lc[LDS ? TG_LDS_ROWS : 1], lf[LDS ? TG_LDS_ROWS : 1];
    if (LDS) {
        for (int r = threadIdx.x; r < view.rows; r += 256) { lc[r] = 0; lf[r] = 0x7FFFFFFF; }
        __syncthreads();
    }
    const int64_t base = (int64_t)blockIdx.x * TG_RELABEL_PTS;
    for (int j = 0; j < TG_RELABEL_PTS / 256; ++j) {
        const int64_t i = base + j * 256 + threadIdx.x;
        if (i >= n) break;
        const uint32_t e = (uint32_t)(inst[i] + 1);
        const int id = prefix[e >> 5] + __popc(bits[e >> 5] & ((1u << (e & 31)) - 1u)) - 1;
        int row = id >= 0 ? id + view.inst_row0 : -1;
        const int s = sem[i];
#pragma unroll
        for (int k = 0; k < TG_MAX_STUFF; ++k)
            if (k < spec.n_stuff && s == spec.stuff[k] && view.stuff_row[k] >= 0) row = view.stuff_row[k];
        vote[i] = id;
        row_out[i] = row;
        if (row >= 0 && row < view.rows) {
            if (LDS) { atomicAdd(&lc[row], 1); atomicMin(&lf[row], (int)i); }
            else { atomicAdd(&cnt[row], 1); atomicMin(&first[row], (int)i); }
        }
    }
    if (LDS) {
        __syncthreads();
        for (int r = threadIdx.x; r < view.rows; r += 256)
            if (lc[r]) { atomicAdd(&cnt[r], lc[r]); atomicMin(&first[r], lf[r]); }
    }
}

__device__ static inline void tg_bm_add(int& c, int& w, int x) {
    if (w == 0) { c = x; w = 1; }
    else if (c == x) ++w;
    else --w;
}
// (candidate, weight) of two disjoint groups: equal candidates add their weights, otherwise the heavier keeps the difference
__device__ static inline void tg_bm_merge(int& c, int& w, int d) {
    const int oc = __shfl_xor(c, d), ow = __shfl_xor(w, d);
    if (oc == c) w += ow;
    else if (ow > w) { c = oc; w = ow - w; }
    else w -= ow;
}

// One wave per superpoint, four per workgroup.  A strict majority, if there is one, survives every Boyer-Moore merge; the counting pass decides.
__global__ __launch_bounds__(256) void tg_votes_kernel(const uint32_t* __restrict__ sidx, const int32_t* __restrict__ start, int64_t S,
                                                       const int32_t* __restrict__ vote, const int32_t* __restrict__ sem, int C,
                                                       int32_t* __restrict__ sp_inst, int32_t* __restrict__ sp_sem) {
    const int lane = threadIdx.x & 63;
    const int64_t s = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= S) return;
    const int j0 = start[s], j1 = start[s + 1];
    int ci = -2, wi = 0, cs = -2, ws = 0;                    // -2: no candidate (ids are >= -1, classes >= 0)
    for (int j = j0 + lane; j < j1; j += 64) {
        const uint32_t p = sidx[j];
        tg_bm_add(ci, wi, vote[p]);
        tg_bm_add(cs, ws, sem[p]);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { tg_bm_merge(ci, wi, d); tg_bm_merge(cs, ws, d); }
    ci = __shfl(ci, 0);
    cs = __shfl(cs, 0);
    int ki = 0, ks = 0;
    for (int j = j0 + lane; j < j1; j += 64) {
        const uint32_t p = sidx[j];
        ki += vote[p] == ci;
        ks += sem[p] == cs;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { ki += __shfl_xor(ki, d); ks += __shfl_xor(ks, d); }
    if (lane == 0) {
        const int64_t cnt = (int64_t)j1 - j0;
        sp_inst[s] = (ci >= 0 && 2 * (int64_t)ki > cnt) ? ci : -1;
        sp_sem[s] = (cs >= 0 && cs <= C && 2 * (int64_t)ks > cnt) ? cs : C;
    }
}

// out[r, c] = (a[c] == r) for r < split, (b[c] == r - split) below: flat over the bytes so that every lane issues one aligned 16-byte
// store whatever the row length is.  A workgroup stages its 4096 flags in LDS with coalesced loads of a / b, then stores.
__global__ __launch_bounds__(256) void tg_expand_kernel(const int32_t* __restrict__ a, const int32_t* __restrict__ b, uint32_t ncol,
                                                        int64_t total, int64_t split, uint8_t* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) uint8_t flag[TG_EXPAND_BYTES];
    const int64_t base = (int64_t)blockIdx.x * TG_EXPAND_BYTES;
    const int64_t r0 = base / ncol;
    const uint32_t c0 = (uint32_t)(base - r0 * ncol);
#pragma unroll 4
    for (int j = 0; j < TG_EXPAND_BYTES / 256; ++j) {
        const uint32_t k = j * 256 + threadIdx.x;
        uint8_t f = 0;
        if (base + k < total) {
            const uint32_t off = c0 + k;                                           // off < ncol + 4096 < 2^32
            const uint32_t q = ncol >= TG_EXPAND_BYTES ? (uint32_t)(off >= ncol) : off / ncol, c = off - q * ncol;
            const int64_t r = r0 + q;
            f = r < split ? (a[c] == r) : (b[c] == r - split);
        }
        flag[k] = f;
    }
    __syncthreads();
    const int64_t o = base + (int64_t)threadIdx.x * 16;
    if (o + 16 <= total) {
        *(uint4*)(out + o) = *(const uint4*)(flag + threadIdx.x * 16);
    } else {
        for (int k = 0; k < 16 && o + k < total; ++k) out[o + k] = flag[threadIdx.x * 16 + k];
    }
}

__global__ __launch_bounds__(256) void tg_finish_kernel(const int32_t* __restrict__ cnt, const int32_t* __restrict__ first,
                                                        const int32_t* __restrict__ sem, int64_t n, int rows, int shift, int C,
                                                        int64_t* __restrict__ labels, int64_t* __restrict__ area) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    const int f = first[r];
    labels[r] = (f >= 0 && f < n) ? (int64_t)sem[f] - shift : (int64_t)C;
    area[r] = cnt[r];
}

// ---------------------------------------------------------------------------------------------- C entry points
extern "C" size_t sd3d_targets_ws_bytes(int64_t n) { return tg_carve(nullptr, n > 0 ? n : 1).total; }

extern "C" int sd3d_targets_scan(const int64_t* instance_mask, const int64_t* semantic_mask, const int64_t* super_points, int64_t n,
                                 const int64_t* lut, int64_t lut_len, int n_classes, const int32_t* stuff_ids, int n_stuff, int swap_2_3,
                                 void* ws, size_t ws_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!instance_mask || !semantic_mask || !super_points || !lut || !ws) return sd3d_set_error(SD3D_ERR_ARG, "targets_scan: NULL argument");
    if (n < 1 || n > TG_MAX_POINTS || lut_len < 1) return sd3d_set_error(SD3D_ERR_ARG, "targets_scan: 1 <= n <= 0x7F000000 points, a non-empty table");
    TgSpec spec;
    if (int rc = tg_spec(spec, n_classes, stuff_ids, n_stuff, swap_2_3, "targets_scan")) return rc;
    const TgWs w = tg_carve(ws, n);
    if (ws_bytes < w.total) return sd3d_set_error(SD3D_ERR_WS, "targets_scan: workspace too small");
    // header and presence bits are adjacent: one fill
    if (hipMemsetAsync(w.header, 0, (size_t)((char*)w.prefix - (char*)w.header), st) != hipSuccess)
        return sd3d_set_error(SD3D_ERR_LAUNCH, "targets_scan: memset failed");
    hipLaunchKernelGGL(tg_labels_kernel, dim3((unsigned)cdiv(n, TG_LABEL_PTS)), dim3(256), 0, st, instance_mask, semantic_mask, super_points, lut, lut_len,
                       n, spec, w.sem, w.inst, w.keys_a, w.bits, w.header);
    hipLaunchKernelGGL(tg_rank_kernel, dim3(1), dim3(TG_RANK_THREADS), 0, st, w.bits, w.prefix, w.header);
    SD3D_CHECK_LAUNCH();
    return SD3D_OK;
}

extern "C" int sd3d_targets_rows(const int32_t* header, int n_stuff, int val_view) {
    if (!header || n_stuff < 0 || n_stuff > TG_MAX_STUFF) return sd3d_set_error(SD3D_ERR_ARG, "targets_rows: header and 0..8 stuff ids");
    int rows = header[TG_G];
    if (val_view)
        for (int k = 0; k < n_stuff; ++k) rows += (header[TG_STUFF] >> k) & 1;
    return rows;
}

extern "C" int sd3d_targets_build(int64_t n, const int32_t* header, int n_classes, const int32_t* stuff_ids, int n_stuff, int val_view,
                                  uint8_t* masks, int64_t* labels, int64_t* area, int32_t* seg_start, int32_t* sp_inst, int32_t* sp_sem,
                                  uint8_t* sp_masks, void* ws, size_t ws_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!header || !ws) return sd3d_set_error(SD3D_ERR_ARG, "targets_build: NULL argument");
    if (n < 1 || n > TG_MAX_POINTS) return sd3d_set_error(SD3D_ERR_ARG, "targets_build: 1 <= n <= 0x7F000000 points");
    if (header[TG_STATUS] != 0) {
        char msg[256];
        const int s = header[TG_STATUS];
        snprintf(msg, sizeof(msg), "targets: status %d:%s%s%s", s,
                 (s & SD3D_TARGETS_BAD_SEMANTIC) ? " a raw semantic id lies outside the lookup table;" : "",
                 (s & SD3D_TARGETS_BAD_INSTANCE) ? " a raw instance id lies outside [-1, 2^20);" : "",
                 (s & SD3D_TARGETS_BAD_SUPERPOINT) ? " a superpoint id lies outside [0, 2^31 - 2];" : "");
        return sd3d_set_error(SD3D_ERR_RANGE, msg);
    }
    TgSpec spec;
    if (int rc = tg_spec(spec, n_classes, stuff_ids, n_stuff, 0, "targets_build")) return rc;
    const int G1 = header[TG_G];
    const int64_t S = header[TG_S];
    if (G1 < 0 || G1 > n || G1 > TG_MAX_INST || S < 1 || S > 0x7FFFFFFFll) return sd3d_set_error(SD3D_ERR_ARG, "targets_build: header is not one sd3d_targets_scan wrote");
    TgView view;
    view.inst_row0 = 0;
    for (int k = 0; k < TG_MAX_STUFF; ++k) view.stuff_row[k] = -1;
    if (val_view)
        for (int k = 0; k < n_stuff; ++k)
            if ((header[TG_STUFF] >> k) & 1) view.stuff_row[k] = view.inst_row0++;
    view.rows = view.inst_row0 + G1;
    const int G = view.rows;
    if (!seg_start || !sp_inst || !sp_sem || !sp_masks || (G > 0 && (!masks || !labels || !area)))
        return sd3d_set_error(SD3D_ERR_ARG, "targets_build: NULL output");
    const TgWs w = tg_carve(ws, n);
    if (ws_bytes < w.total) return sd3d_set_error(SD3D_ERR_WS, "targets_build: workspace too small");
    const int64_t sp_total = ((int64_t)G1 + spec.C + 1) * S;
    if (cdiv(sp_total, TG_EXPAND_BYTES) > 0x7FFFFFFFll || cdiv((int64_t)G * n, TG_EXPAND_BYTES) > 0x7FFFFFFFll)
        return sd3d_set_error(SD3D_ERR_ARG, "targets_build: an output exceeds 2^43 bytes");

    if (G > 0) {
        if (hipMemsetAsync(w.cnt, 0, (size_t)G * 4, st) != hipSuccess || hipMemsetAsync(w.first, 0x7F, (size_t)G * 4, st) != hipSuccess)
            return sd3d_set_error(SD3D_ERR_LAUNCH, "targets_build: memset failed");
    }
    const dim3 rgrid((unsigned)cdiv(n, TG_RELABEL_PTS));
    if (G <= TG_LDS_ROWS)
        hipLaunchKernelGGL(tg_relabel_kernel<true>, rgrid, dim3(256), 0, st, w.sem, w.inst, w.bits, w.prefix, n, spec, view, w.vote, w.row, w.cnt, w.first);
    else
        hipLaunchKernelGGL(tg_relabel_kernel<false>, rgrid, dim3(256), 0, st, w.sem, w.inst, w.bits, w.prefix, n, spec, view, w.vote, w.row, w.cnt, w.first);
    SD3D_CHECK_LAUNCH();

    // points grouped by superpoint: the library's sort over the bits S needs, then segment starts
    int bits = 1;
    while (bits < 32 && ((int64_t)1 << bits) < S) ++bits;
    int landed = 0;
    if (int rc = sd3d_sort_pairs_u64_ex(w.keys_a, nullptr, w.keys_b, w.vals_b, w.vals_a, n, 0, bits, w.sort_ws, w.sort_ws_bytes, &landed, stream)) return rc;
    const uint64_t* sorted = landed ? w.keys_a : w.keys_b;
    const uint32_t* sidx = landed ? w.vals_a : w.vals_b;
    const int32_t id_off = 0;                                   // one scene: the sorted keys are plain ids (at most 32 bits, above)
    if (int rc = sd3d_segment_starts_batch(sorted, n, S, &id_off, 1, seg_start, stream)) return rc;
    hipLaunchKernelGGL(tg_votes_kernel, dim3((unsigned)cdiv(S, 4)), dim3(256), 0, st, sidx, seg_start, S, w.vote, w.sem, spec.C, sp_inst, sp_sem);
    SD3D_CHECK_LAUNCH();

    if (G > 0) {
        const int64_t total = (int64_t)G * n;
        hipLaunchKernelGGL(tg_expand_kernel, dim3((unsigned)cdiv(total, TG_EXPAND_BYTES)), dim3(256), 0, st, w.row, w.row, (uint32_t)n, total, (int64_t)G,
                           masks);
        hipLaunchKernelGGL(tg_finish_kernel, dim3((unsigned)cdiv(G, 256)), dim3(256), 0, st, w.cnt, w.first, w.sem, n, G, val_view ? 0 : n_stuff,
                           spec.C, labels, area);
    }
    hipLaunchKernelGGL(tg_expand_kernel, dim3((unsigned)cdiv(sp_total, TG_EXPAND_BYTES)), dim3(256), 0, st, sp_inst, sp_sem, (uint32_t)S, sp_total, (int64_t)G1,
                       sp_masks);
    SD3D_CHECK_LAUNCH();
    return SD3D_OK;
}
