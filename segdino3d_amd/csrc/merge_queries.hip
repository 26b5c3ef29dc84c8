// Merging of lifted 2D queries across views into one query per object (the stage between csrc/lift_queries.hip and the decoder's
// `query2d_feats` / `query2d_pos`).  The reference has no counterpart (it loads a per-scene dump); tests/merge_queries_ref.py restates
// the rule of include/segdino3d_hip.h, and these kernels are pinned against that restatement.  Every decision is an integer one.
//
//   sd3d_merge_queries_adjacency  mq_valid_kernel (a non-finite or out-of-world centre zeroes the row's count), sd3d_lift_query_select
//                                 with the cap SD3D_MERGE_MAX_ROWS (step 1), sd3d_keys_from_f32(descending) + a stable sort over 33
//                                 bits (step 2), mq_code_kernel (one wave per rank: the int8 code row padded with zeros to a multiple
//                                 of 64 channels, nrm and the fixed-point centre, steps 3 and 4), mq_gram_kernel (step 5).
//                 mq_gram_kernel  one workgroup of four waves per 64 x 64 tile pair on or above the diagonal; a wave owns 16 ranks `a`
//                                 and 64 ranks `b`: four accumulators of __builtin_amdgcn_mfma_i32_16x16x64_i8 over the code rows.
//                                 Both operands are rows of the same matrix and every lane loads the same 16 bytes of the k step for
//                                 A and for B (row = lane & 15, bytes 16 (lane >> 4) ..), so whatever k the hardware assigns to a slot,
//                                 the two agree and the dot product is the one of the rows.  The epilogue applies the distance and
//                                 the cosine test in int64 and packs the verdicts with ballots: the 16-bit group g of a ballot over
//                                 register i is rank a = 4 g + i against 16 ranks b.  Word [a][b / 64] holds bit b % 64; words below
//                                 the diagonal are never written and never read.
//   sd3d_merge_queries_sweep      mq_sweep_kernel: one workgroup.  Per block of 64 ranks, wave 0 settles the block from the diagonal
//                                 64 x 64 bits (fetched one block ahead) in scalar registers: an unlabelled rank is a seed and labels
//                                 the later unlabelled ranks of its row.  Then each thread owns one later word of the bitmap (LDS),
//                                 loads the seeds' words for it in batches of eight, labels the newly covered ranks and ORs.
//   sd3d_merge_queries_reduce     keys (seed rank, row) sorted, mq_bounds_kernel (segment bounds), mq_cluster_kernel (one wave per cluster: the int64
//                                 sums, the distinct views of the ascending rows), then sd3d_lift_query_select over the seeds' rows
//                                 with `views` as the count: min_views, max_queries, ascending seed row (step 8) -> *k_dev.
//   sd3d_merge_queries_emit       mq_emit_kernel: one workgroup per emitted cluster, one lane per channel walks the members in
//                                 ascending row order with two rounded operations per member (never contracted).
// All values are written with plain vector stores.
#include "common.h"
#include "../../include/segdino3d_hip.h"
#include <hip/hip_fp16.h>
#include <cstdio>

// The feature mean is two rounded operations per member.  Written with the operators: the header's __fmul_rn / __fadd_rn are inline
// functions compiled under the default contraction mode, and the two may fuse once inlined.
#pragma clang fp contract(off)

#define MQ_MAX_N 0x7F000000ll
#define MQ_MAX_C 1024
#define MQ_W_MAX (1 << 20)                              // the cap on a member's weight

typedef int mq_v4i __attribute__((ext_vector_type(4)));

struct MqWs {
    int32_t *cnt2, *row_rank, *cl_views, *out_rows;     // [n]
    int32_t *rows, *rank_row, *label, *start, *m_dev;   // [Mp]; start [Mp][2] = begin, end of a seed rank's members
    float *sel_scores, *cl_pos;
    int64_t* cl_wsum;
    uint64_t *keys_a, *keys_b, *sorted, *adj;
    uint32_t *vals_a, *vals_b;
    int8_t* codes;
    int4* p4;                                           // x, y, z fixed point, nrm
    void *sel_ws, *sort_ws;
    size_t sel_bytes, sort_bytes, total;
    int64_t Mc, Mp, W;
    int Cp;
};
static MqWs mq_ws(void* ws, int64_t n, int C) {
    MqWs w;
    char* p = (char*)ws;
    size_t o = 0;
    auto take = [&](size_t bytes) { char* q = p + o; o += align_up(bytes, 256); return (void*)q; };
    const size_t nn = (size_t)(n > 0 ? n : 1);
    w.Mc = n < SD3D_MERGE_MAX_ROWS ? (n > 0 ? n : 1) : SD3D_MERGE_MAX_ROWS;
    w.Mp = (w.Mc + 63) / 64 * 64;
    w.W = w.Mp / 64;
    w.Cp = (C + 63) / 64 * 64;
    const size_t mp = (size_t)w.Mp;
    w.cnt2 = (int32_t*)take(nn * 4); w.row_rank = (int32_t*)take(nn * 4); w.cl_views = (int32_t*)take(nn * 4);
    w.out_rows = (int32_t*)take(nn * 4);
    w.rows = (int32_t*)take(mp * 4); w.rank_row = (int32_t*)take(mp * 4); w.label = (int32_t*)take(mp * 4);
    w.start = (int32_t*)take(mp * 2 * 4); w.m_dev = (int32_t*)take(4);
    w.sel_scores = (float*)take(mp * 4); w.cl_pos = (float*)take(mp * 3 * 4);
    w.cl_wsum = (int64_t*)take(mp * 8);
    w.keys_a = (uint64_t*)take(mp * 8); w.keys_b = (uint64_t*)take(mp * 8); w.sorted = (uint64_t*)take(mp * 8);
    w.vals_a = (uint32_t*)take(mp * 4); w.vals_b = (uint32_t*)take(mp * 4);
    w.p4 = (int4*)take(mp * 16);
    w.codes = (int8_t*)take(mp * (size_t)w.Cp);
    w.adj = (uint64_t*)take(mp * (size_t)w.W * 8);
    w.sel_bytes = sd3d_lift_query_select_ws_bytes(n); w.sel_ws = take(w.sel_bytes);
    w.sort_bytes = sort_ws_bytes(w.Mp); w.sort_ws = take(w.sort_bytes);
    w.total = o;
    return w;
}

// ---------------------------------------------------------------------------------------------- steps 1 and 2
__global__ __launch_bounds__(256) void mq_valid_kernel(const float* __restrict__ centre, const int32_t* __restrict__ count, int64_t n,
                                                       int32_t* __restrict__ cnt2, int32_t* __restrict__ row_rank,
                                                       int32_t* __restrict__ cl_views) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float lim = (float)(1 << SD3D_LIFTQ_WORLD_BITS);
    const bool ok = fabsf(centre[i * 3]) < lim && fabsf(centre[i * 3 + 1]) < lim && fabsf(centre[i * 3 + 2]) < lim;       // NaN fails
    cnt2[i] = ok ? count[i] : 0;
    row_rank[i] = -1;
    cl_views[i] = 0;
}

__global__ __launch_bounds__(256) void mq_sel_scores_kernel(const int32_t* __restrict__ rows, const int32_t* __restrict__ m_dev,
                                                            const float* __restrict__ scores, int64_t Mc, float* __restrict__ sel) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j < Mc) sel[j] = j < *m_dev ? scores[rows[j]] : 0.0f;
}
// the keys of sd3d_keys_from_f32 use 32 bits: bit 32 puts the unused tail behind every entering row
__global__ __launch_bounds__(256) void mq_key_tail_kernel(uint64_t* __restrict__ keys, const int32_t* __restrict__ m_dev, int64_t Mc) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j < Mc && j >= *m_dev) keys[j] |= 1ull << 32;
}

// ---------------------------------------------------------------------------------------------- steps 3 and 4
__device__ __forceinline__ float mq_load(const __half* p) { return __half2float(*p); }
__device__ __forceinline__ float mq_load(const float* p) { return *p; }

// one wave per rank of [0, Mp): ranks at or beyond *m_dev get a zero code, nrm = 0, rank_row = -1
template <typename T>
__global__ __launch_bounds__(256) void mq_code_kernel(const T* __restrict__ feats, const float* __restrict__ centre,
                                                      const int32_t* __restrict__ rows, const uint32_t* __restrict__ order,
                                                      const int32_t* __restrict__ m_dev, int64_t n, int64_t Mc, int64_t Mp, int C, int Cp,
                                                      int8_t* __restrict__ codes, int4* __restrict__ p4, int32_t* __restrict__ rank_row,
                                                      int32_t* __restrict__ row_rank, int32_t* __restrict__ label) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= Mp) return;
    const int M = *m_dev;
    int64_t row = -1;
    if (r < M && r < Mc) {
        const uint32_t j = order[r];
        if (j < (uint32_t)Mc) row = rows[j];
        if (row < 0 || row >= n) row = -1;                                            // never from the select kernels
    }
    int8_t* out = codes + r * Cp;
    if (row < 0) {
        for (int c = lane; c < Cp; c += 64) out[c] = 0;
        if (lane == 0) { p4[r] = make_int4(0, 0, 0, 0); rank_row[r] = -1; label[r] = -1; }
        return;
    }
    const T* f = feats + row * C;
    float s = 0.0f;
    int bad = 0;
    for (int c = lane; c < C; c += 64) {
        const float a = fabsf(mq_load(f + c));
        if (!(a <= 3.4028234663852886e38f)) bad = 1;                                  // NaN or infinite
        else s = fmaxf(s, a);
    }
    s = wave_max(s);
    bad = wave_or(bad);
    const bool zero = bad || !(s >= 7.888609052210118e-31f);                          // 2^-100
    int e = 0;
    (void)frexpf(s, &e);                                                              // s = m 2^e, 1/2 <= m < 1
    const float scale = zero ? 0.0f : ldexpf(1.0f, 7 - e);                            // 2^-121 .. 2^107: a normal float
    int nrm = 0;
    for (int c = lane; c < Cp; c += 64) {
        int q = 0;
        if (!zero && c < C) {
            const float x = rintf(__fmul_rn(mq_load(f + c), scale));                  // |x| <= 128
            q = (int)fminf(fmaxf(x, -127.0f), 127.0f);
        }
        out[c] = (int8_t)q;
        nrm += q * q;
    }
    nrm = wave_sum(nrm);
    if (lane == 0) {
        const float* ce = centre + row * 3;
        p4[r] = make_int4((int)rintf(__fmul_rn(ce[0], 1024.0f)), (int)rintf(__fmul_rn(ce[1], 1024.0f)), (int)rintf(__fmul_rn(ce[2], 1024.0f)), nrm);
        rank_row[r] = (int32_t)row;
        row_rank[row] = (int32_t)r;
        label[r] = -1;
    }
}

// ---------------------------------------------------------------------------------------------- step 5
__global__ __launch_bounds__(256) void mq_gram_kernel(const int8_t* __restrict__ codes, const int4* __restrict__ p4,
                                                      const int32_t* __restrict__ m_dev, int Cp, int W, long long rq2, long long s72,
                                                      uint64_t* __restrict__ adj) {
    const int tb = blockIdx.x, ta = blockIdx.y;
    const int M = *m_dev;
    if (tb < ta || tb * 64 >= M) return;                                              // below the diagonal, or no rank there (ta <= tb)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int a0 = ta * 64 + wv * 16, b0 = tb * 64;                                   // rows below Mp = 64 W: the codes hold them all
    const int8_t* arow = codes + (size_t)(a0 + (lane & 15)) * Cp + 16 * (lane >> 4);
    const int8_t* brow = codes + (size_t)(b0 + (lane & 15)) * Cp + 16 * (lane >> 4);
    const size_t bstep = (size_t)16 * Cp;
    mq_v4i acc[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) acc[nt] = (mq_v4i){0, 0, 0, 0};
    for (int k = 0; k < Cp; k += 64) {
        const mq_v4i a = *(const mq_v4i*)(arow + k);
        mq_v4i b[4];
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) b[nt] = *(const mq_v4i*)(brow + nt * bstep + k);
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) acc[nt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b[nt], acc[nt], 0, 0, 0);
    }
    // register i of lane l: a = a0 + 4 (l >> 4) + i, b = b0 + 16 nt + (l & 15)
    int4 pa[4], pb[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) pa[i] = p4[a0 + 4 * (lane >> 4) + i];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) pb[nt] = p4[b0 + 16 * nt + (lane & 15)];
    unsigned long long bal[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int a = a0 + 4 * (lane >> 4) + i;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            const int b = b0 + 16 * nt + (lane & 15);
            const int dx = pa[i].x - pb[nt].x, dy = pa[i].y - pb[nt].y, dz = pa[i].z - pb[nt].z;     // |p| <= 2^24: the differences fit
            bool ok = a < b && b < M && pa[i].w > 0 && pb[nt].w > 0 &&
                      (long long)dx * dx + (long long)dy * dy + (long long)dz * dz <= rq2;
            unsigned long long near = __ballot(ok);
            if (s72 > 0 && near) {                                                    // uniform: most 64-lane groups hold no near pair
                const int d = acc[nt][i];
                ok = ok && d > 0 && (long long)d * d * 16384ll >= s72 * (long long)pa[i].w * (long long)pb[nt].w;
                near = __ballot(ok);
            }
            bal[i][nt] = near;
        }
    }
    if (lane < 16) {
        const int i = lane & 3, g = lane >> 2;
        unsigned long long word = 0;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            const unsigned long long v = i == 0 ? bal[0][nt] : i == 1 ? bal[1][nt] : i == 2 ? bal[2][nt] : bal[3][nt];
            word |= ((v >> (16 * g)) & 0xFFFFull) << (16 * nt);
        }
        adj[(size_t)(a0 + lane) * W + tb] = word;
    }
}

// a copy of the ranks and of the bit matrix with the words below the diagonal (never written) as zero: for tests and tools
__global__ __launch_bounds__(256) void mq_adj_copy_kernel(const uint64_t* __restrict__ adj, const int32_t* __restrict__ m_dev, int64_t Mp, int W,
                                                          uint64_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= Mp * W) return;
    const int64_t a = i / W, w = i - a * W;
    const int M = *m_dev;
    out[i] = (a < M && w >= a / 64 && w * 64 < M) ? adj[i] : 0ull;
}

// ---------------------------------------------------------------------------------------------- step 6
__device__ __forceinline__ unsigned long long mq_uniform(unsigned long long v) {
    const uint32_t lo = __builtin_amdgcn_readfirstlane((int)(uint32_t)v), hi = __builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
    return ((unsigned long long)hi << 32) | lo;
}

__global__ __launch_bounds__(256) void mq_sweep_kernel(const uint64_t* __restrict__ adj, const int32_t* __restrict__ m_dev, int W,
                                                       int32_t* __restrict__ label) {
    __shared__ unsigned long long bm[SD3D_MERGE_MAX_ROWS / 64];                      // bit = the rank is labelled
    __shared__ unsigned long long s_seeds;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int M = *m_dev;
    const int Wm = (M + 63) / 64;                                                     // <= W <= 256
    bm[t] = 0ull;
    __syncthreads();
    unsigned long long dnext = 0ull;
    if (wv == 0 && Wm > 0) dnext = adj[(size_t)lane * W];
    for (int k = 0; k < Wm; ++k) {
        if (wv == 0) {
            const unsigned long long dcur = dnext;
            if (k + 1 < Wm) dnext = adj[(size_t)((k + 1) * 64 + lane) * W + (k + 1)]; // does not depend on the walk: in flight meanwhile
            const int live = M - 64 * k;                                              // >= 1
            unsigned long long L = mq_uniform(bm[k]) | (live >= 64 ? 0ull : ~0ull << live), seeds = 0ull;
            int mine = -1;
#pragma unroll
            for (int i = 0; i < 64; ++i) {
                const uint32_t lo = __builtin_amdgcn_readlane((int)(uint32_t)dcur, i), hi = __builtin_amdgcn_readlane((int)(uint32_t)(dcur >> 32), i);
                if (!((L >> i) & 1ull)) {                                             // uniform: rank 64 k + i is a seed
                    const unsigned long long row = (((unsigned long long)hi << 32) | lo) | (1ull << i);
                    if (((row & ~L) >> lane) & 1ull) mine = 64 * k + i;
                    L |= row;
                    seeds |= 1ull << i;
                }
            }
            if (mine >= 0) label[64 * k + lane] = mine;
            if (lane == 0) s_seeds = seeds;
        }
        __syncthreads();
        const unsigned long long seeds = s_seeds;
        const int w = k + 1 + t;                                                      // W <= 256 threads: one later word each
        if (w < Wm) {
            unsigned long long cur = bm[w], s = seeds;
            while (s) {                                                               // uniform over the workgroup
                int idx[8];
                unsigned long long r[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    idx[j] = s ? __builtin_ctzll(s) : -1;
                    if (s) s &= s - 1;
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) r[j] = idx[j] >= 0 ? adj[(size_t)(64 * k + idx[j]) * W + w] : 0ull;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    unsigned long long fresh = r[j] & ~cur;
                    while (fresh) {
                        label[64 * w + __builtin_ctzll(fresh)] = 64 * k + idx[j];     // bits at or beyond M are never set
                        fresh &= fresh - 1;
                    }
                    cur |= r[j];
                }
            }
            bm[w] = cur;
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------- steps 7 and 8
// key of rank r: (seed rank << 32) | row; the unused tail sorts behind with the segment id Mc
__global__ __launch_bounds__(256) void mq_member_keys_kernel(const int32_t* __restrict__ label, const int32_t* __restrict__ rank_row,
                                                             const int32_t* __restrict__ m_dev, int64_t Mc, uint64_t* __restrict__ keys) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= Mc) return;
    const bool live = r < *m_dev && label[r] >= 0 && label[r] < Mc && rank_row[r] >= 0;
    keys[r] = live ? ((uint64_t)(uint32_t)label[r] << 32) | (uint32_t)rank_row[r] : ((uint64_t)Mc << 32) | (uint32_t)r;
}
// seg[2 s], seg[2 s + 1] = where the members of seed rank s begin and end in the sorted keys (zeroed before: no members).  One thread per
// sorted position.  (sd3d_segment_starts_batch fills the starts of absent ids in a serial loop per gap: the seeds are a few hundred of 16384
// ranks, most of them early, and the one thread behind the last seed took 0.19 ms.)
__global__ __launch_bounds__(256) void mq_bounds_kernel(const uint64_t* __restrict__ sorted, int64_t Mc, int32_t* __restrict__ seg) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= Mc) return;
    const uint64_t id = sorted[j] >> 32;
    if (id >= (uint64_t)Mc) return;                                                   // the unused tail
    if (j == 0 || (sorted[j - 1] >> 32) != id) seg[2 * id] = (int32_t)j;
    if (j == Mc - 1 || (sorted[j + 1] >> 32) != id) seg[2 * id + 1] = (int32_t)(j + 1);
}

// one wave per seed rank
__global__ __launch_bounds__(256) void mq_cluster_kernel(const uint64_t* __restrict__ sorted, const int32_t* __restrict__ start,
                                                         const int32_t* __restrict__ m_dev, const int32_t* __restrict__ count,
                                                         const int32_t* __restrict__ row_rank, const int32_t* __restrict__ rank_row,
                                                         const int4* __restrict__ p4, int64_t n, int64_t Mc, int Q,
                                                         float* __restrict__ cl_pos, int64_t* __restrict__ cl_wsum,
                                                         int32_t* __restrict__ cl_views) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= Mc || r >= *m_dev) return;
    const int s0 = start[2 * r], s1 = start[2 * r + 1];
    if (s0 >= s1 || s1 > Mc) return;                                                  // not a seed
    long long sx = 0, sy = 0, sz = 0, sw = 0;
    int views = 0;
    for (int j = s0 + lane; j < s1; j += 64) {
        const int64_t row = (int64_t)(sorted[j] & 0xFFFFFFFFull);
        if (row >= n) continue;
        const int rk = row_rank[row];
        if (rk < 0 || rk >= Mc) continue;
        const int4 p = p4[rk];
        const long long w = min(count[row], MQ_W_MAX);
        sx += w * p.x; sy += w * p.y; sz += w * p.z; sw += w;
        const int64_t prev = j > s0 ? (int64_t)(sorted[j - 1] & 0xFFFFFFFFull) / Q : -1;  // ascending rows: equal views are neighbours
        views += row / Q != prev;
    }
    sx = wave_sum(sx); sy = wave_sum(sy); sz = wave_sum(sz); sw = wave_sum(sw); views = wave_sum(views);
    if (lane == 0 && sw > 0) {
        cl_pos[r * 3] = (float)((double)sx / (double)sw / 1024.0);
        cl_pos[r * 3 + 1] = (float)((double)sy / (double)sw / 1024.0);
        cl_pos[r * 3 + 2] = (float)((double)sz / (double)sw / 1024.0);
        cl_wsum[r] = sw;
        const int seed_row = rank_row[r];
        if (seed_row >= 0 && seed_row < n) cl_views[seed_row] = views;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void mq_emit_kernel(const T* __restrict__ feats, const float* __restrict__ scores,
                                                      const int32_t* __restrict__ count, const int32_t* __restrict__ out_rows,
                                                      const int32_t* __restrict__ row_rank, const uint64_t* __restrict__ sorted,
                                                      const int32_t* __restrict__ start, const float* __restrict__ cl_pos,
                                                      const int64_t* __restrict__ cl_wsum, const int32_t* __restrict__ cl_views, int64_t n,
                                                      int64_t Mc, int C, int best, float* __restrict__ out_feats, float* __restrict__ out_pos,
                                                      float* __restrict__ out_scores, int32_t* __restrict__ out_views,
                                                      int32_t* __restrict__ labels) {
    const int k = blockIdx.x, t = threadIdx.x;
    const int64_t seed_row = out_rows[k];
    if (seed_row < 0 || seed_row >= n) return;
    const int r = row_rank[seed_row];
    if (r < 0 || r >= Mc) return;
    const int s0 = start[2 * r], s1 = start[2 * r + 1];
    if (s0 >= s1 || s1 > Mc) return;
    if (t < 3) out_pos[(int64_t)k * 3 + t] = cl_pos[(int64_t)r * 3 + t];
    if (t == 3) out_scores[k] = scores[seed_row];
    if (t == 4) out_views[k] = cl_views[seed_row];
    for (int j = s0 + t; j < s1; j += 256) {
        const int64_t row = (int64_t)(sorted[j] & 0xFFFFFFFFull);
        if (row < n) labels[row] = k;
    }
    const float wsum = (float)cl_wsum[r];
    for (int c = t; c < C; c += 256) {
        float v;
        if (best) {
            v = mq_load(feats + seed_row * C + c);
        } else {
            float acc = 0.0f;
            for (int j = s0; j < s1; ++j) {
                const int64_t row = (int64_t)(sorted[j] & 0xFFFFFFFFull);
                if (row >= n) continue;
                const float w = (float)min(count[row], MQ_W_MAX);
                const float prod = w * mq_load(feats + row * C + c);                  // contraction is off in this file: two rounded
                acc = acc + prod;                                                     // operations, never one fused
            }
            v = __fdiv_rn(acc, wsum);
        }
        out_feats[(int64_t)k * C + c] = v;
    }
}

// ---------------------------------------------------------------------------------------------- C entry points
static int mq_check(const char* who, int64_t n, int C, const void* ws, size_t ws_bytes, MqWs* w) {
    if (n < 0 || n > MQ_MAX_N || C < 1 || C > MQ_MAX_C) {
        char msg[160];
        snprintf(msg, sizeof msg, "%s: 0 <= n <= 0x7F000000 rows, 1 <= C <= 1024 channels (the int64 cosine test is exact up to there)", who);
        return sd3d_set_error(SD3D_ERR_ARG, msg);
    }
    if (n == 0) return SD3D_OK;
    if (!ws || ((uintptr_t)ws & 255) != 0) return sd3d_set_error(SD3D_ERR_ARG, "merge_queries: ws must be given and 256-byte aligned");
    *w = mq_ws((void*)ws, n, C);
    if (ws_bytes < w->total) return sd3d_set_error(SD3D_ERR_WS, "merge_queries: workspace too small");
    return SD3D_OK;
}

extern "C" size_t sd3d_merge_queries_ws_bytes(int64_t n, int C) {
    if (n < 0 || n > MQ_MAX_N || C < 1 || C > MQ_MAX_C) return 0;
    return mq_ws(nullptr, n, C).total;
}

extern "C" int sd3d_merge_queries_adjacency(const void* feats, int feats_f16, const float* centre, const float* scores, const int32_t* count,
                                            int64_t n, int C, float score_thr, int min_pixels, int radius_q, int sim_q, void* ws,
                                            size_t ws_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    MqWs w;
    if (int rc = mq_check("merge_queries_adjacency", n, C, ws, ws_bytes, &w)) return rc;
    if (min_pixels < 1 || radius_q < 1 || radius_q > (1 << 20) || sim_q < 0 || sim_q > 128)
        return sd3d_set_error(SD3D_ERR_ARG, "merge_queries_adjacency: min_pixels >= 1, 1 <= radius_q <= 2^20, 0 (no test) <= sim_q <= 128");
    if (n == 0) return SD3D_OK;
    if (!feats || !centre || !scores || !count) return sd3d_set_error(SD3D_ERR_ARG, "merge_queries_adjacency: NULL argument");
    hipLaunchKernelGGL(mq_valid_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, st, centre, count, n, w.cnt2, w.row_rank, w.cl_views);
    if (int rc = sd3d_lift_query_select(scores, w.cnt2, n, score_thr, min_pixels, SD3D_MERGE_MAX_ROWS, w.rows, w.Mc, w.m_dev, w.sel_ws,
                                        w.sel_bytes, stream))
        return rc;
    const dim3 gm((unsigned)cdiv(w.Mc, 256)), b256(256);
    hipLaunchKernelGGL(mq_sel_scores_kernel, gm, b256, 0, st, w.rows, w.m_dev, scores, w.Mc, w.sel_scores);
    if (int rc = sd3d_keys_from_f32(w.sel_scores, w.Mc, 1, w.keys_a, stream)) return rc;
    hipLaunchKernelGGL(mq_key_tail_kernel, gm, b256, 0, st, w.keys_a, w.m_dev, w.Mc);
    int landed = 0;
    if (int rc = sd3d_sort_pairs_u64_ex(w.keys_a, nullptr, w.keys_b, w.vals_b, w.vals_a, w.Mc, 0, 33, w.sort_ws, w.sort_bytes, &landed, stream)) return rc;
    const uint32_t* order = landed ? w.vals_a : w.vals_b;
    const dim3 gw((unsigned)cdiv(w.Mp, 4));
    if (feats_f16)
        hipLaunchKernelGGL(mq_code_kernel<__half>, gw, b256, 0, st, (const __half*)feats, centre, w.rows, order, w.m_dev, n, w.Mc, w.Mp, C, w.Cp,
                           w.codes, w.p4, w.rank_row, w.row_rank, w.label);
    else
        hipLaunchKernelGGL(mq_code_kernel<float>, gw, b256, 0, st, (const float*)feats, centre, w.rows, order, w.m_dev, n, w.Mc, w.Mp, C, w.Cp,
                           w.codes, w.p4, w.rank_row, w.row_rank, w.label);
    hipLaunchKernelGGL(mq_gram_kernel, dim3((unsigned)w.W, (unsigned)w.W), b256, 0, st, w.codes, w.p4, w.m_dev, w.Cp, (int)w.W,
                       (long long)radius_q * radius_q, (long long)sim_q * sim_q, w.adj);
    SD3D_CHECK_LAUNCH();
    return SD3D_OK;
}

extern "C" int sd3d_merge_queries_adjacency_read(int64_t n, int C, const void* ws, size_t ws_bytes, int32_t* rank_row, void* adj, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    MqWs w;
    if (int rc = mq_check("merge_queries_adjacency_read", n, C, ws, ws_bytes, &w)) return rc;
    if (n == 0) return SD3D_OK;
    if (!rank_row || !adj) return sd3d_set_error(SD3D_ERR_ARG, "merge_queries_adjacency_read: NULL argument");
    if (hipMemcpyAsync(rank_row, w.rank_row, (size_t)w.Mp * 4, hipMemcpyDeviceToDevice, st) != hipSuccess)
        return sd3d_set_error(SD3D_ERR_LAUNCH, "merge_queries_adjacency_read: copy");
    hipLaunchKernelGGL(mq_adj_copy_kernel, dim3((unsigned)cdiv(w.Mp * w.W, 256)), dim3(256), 0, st, w.adj, w.m_dev, w.Mp, (int)w.W, (uint64_t*)adj);
    SD3D_CHECK_LAUNCH();
    return SD3D_OK;
}

extern "C" int sd3d_merge_queries_sweep(int64_t n, int C, void* ws, size_t ws_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    MqWs w;
    if (int rc = mq_check("merge_queries_sweep", n, C, ws, ws_bytes, &w)) return rc;
    if (n == 0) return SD3D_OK;
    hipLaunchKernelGGL(mq_sweep_kernel, dim3(1), dim3(256), 0, st, w.adj, w.m_dev, (int)w.W, w.label);
    SD3D_CHECK_LAUNCH();
    return SD3D_OK;
}

extern "C" int sd3d_merge_queries_reduce(const float* scores, const int32_t* count, int64_t n, int C, int queries_per_view, float score_thr,
                                         int min_views, int64_t max_queries, int32_t* k_dev, void* ws, size_t ws_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    MqWs w;
    if (int rc = mq_check("merge_queries_reduce", n, C, ws, ws_bytes, &w)) return rc;
    if (queries_per_view < 1 || min_views < 1 || !k_dev)
        return sd3d_set_error(SD3D_ERR_ARG, "merge_queries_reduce: queries_per_view >= 1, min_views >= 1, k_dev required");
    if (n == 0) {
        if (hipMemsetAsync(k_dev, 0, sizeof(int32_t), st) != hipSuccess) return sd3d_set_error(SD3D_ERR_LAUNCH, "merge_queries_reduce: memset");
        return SD3D_OK;
    }
    if (!scores || !count) return sd3d_set_error(SD3D_ERR_ARG, "merge_queries_reduce: NULL argument");
    const dim3 gm((unsigned)cdiv(w.Mc, 256)), b256(256);
    hipLaunchKernelGGL(mq_member_keys_kernel, gm, b256, 0, st, w.label, w.rank_row, w.m_dev, w.Mc, w.keys_a);
    int landed = 0;
    if (int rc = sd3d_sort_pairs_u64_ex(w.keys_a, nullptr, w.keys_b, w.vals_b, w.vals_a, w.Mc, 0, 48, w.sort_ws, w.sort_bytes, &landed, stream)) return rc;
    const uint64_t* sorted = landed ? w.keys_a : w.keys_b;
    if (hipMemcpyAsync(w.sorted, sorted, (size_t)w.Mc * 8, hipMemcpyDeviceToDevice, st) != hipSuccess)
        return sd3d_set_error(SD3D_ERR_LAUNCH, "merge_queries_reduce: copy");
    if (hipMemsetAsync(w.start, 0, (size_t)w.Mp * 2 * 4, st) != hipSuccess) return sd3d_set_error(SD3D_ERR_LAUNCH, "merge_queries_reduce: memset");
    hipLaunchKernelGGL(mq_bounds_kernel, gm, b256, 0, st, w.sorted, w.Mc, w.start);
    hipLaunchKernelGGL(mq_cluster_kernel, dim3((unsigned)cdiv(w.Mc, 4)), b256, 0, st, w.sorted, w.start, w.m_dev, count, w.row_rank, w.rank_row,
                       w.p4, n, w.Mc, queries_per_view, w.cl_pos, w.cl_wsum, w.cl_views);
    // step 8 on the seeds' rows: `views` takes the place of the pixel count, every other row has views = 0
    if (int rc = sd3d_lift_query_select(scores, w.cl_views, n, score_thr, min_views, max_queries, w.out_rows, n, k_dev, w.sel_ws, w.sel_bytes, stream))
        return rc;
    SD3D_CHECK_LAUNCH();
    return SD3D_OK;
}

extern "C" int sd3d_merge_queries_emit(const void* feats, int feats_f16, const float* scores, const int32_t* count, int64_t n, int C, int64_t K,
                                       int reduce_best, float* out_feats, float* out_pos, float* out_scores, int32_t* out_views,
                                       int32_t* labels, const void* ws, size_t ws_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    MqWs w;
    if (int rc = mq_check("merge_queries_emit", n, C, ws, ws_bytes, &w)) return rc;
    if (K < 0 || K > n || K > SD3D_MERGE_MAX_ROWS) return sd3d_set_error(SD3D_ERR_ARG, "merge_queries_emit: 0 <= K <= min(n, SD3D_MERGE_MAX_ROWS)");
    if (n == 0) return SD3D_OK;
    if (!labels) return sd3d_set_error(SD3D_ERR_ARG, "merge_queries_emit: labels required");
    if (hipMemsetAsync(labels, 0xFF, (size_t)n * 4, st) != hipSuccess) return sd3d_set_error(SD3D_ERR_LAUNCH, "merge_queries_emit: memset");
    if (K == 0) return SD3D_OK;
    if (!feats || !scores || !count || !out_feats || !out_pos || !out_scores || !out_views)
        return sd3d_set_error(SD3D_ERR_ARG, "merge_queries_emit: NULL argument");
#define MQ_EMIT(T) \
    hipLaunchKernelGGL(mq_emit_kernel<T>, dim3((unsigned)K), dim3(256), 0, st, (const T*)feats, scores, count, w.out_rows, w.row_rank, w.sorted, \
                       w.start, w.cl_pos, w.cl_wsum, w.cl_views, n, w.Mc, C, reduce_best ? 1 : 0, out_feats, out_pos, out_scores, out_views, labels)
    if (feats_f16) MQ_EMIT(__half); else MQ_EMIT(float);
#undef MQ_EMIT
    SD3D_CHECK_LAUNCH();
    return SD3D_OK;
}
