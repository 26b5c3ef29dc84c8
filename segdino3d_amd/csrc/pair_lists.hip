// Rulebook lists of the pair-major sparse convolution (pair_gemm.hip): for every neighbour table the pairs (in = nbr[k][r], out = r),
// offset-major and padded to 128-pair tiles (in_idx, tile_k), plus what pass 2 reads - the position table pos, the per-row lists, the
// output row of every entry (out_idx) - and the chained form, where mirror offsets and the centre share one partial product.
#include "pair_conv.h"

#define PL_ROWS 2048            // rows per workgroup of the list-building kernels

__device__ static inline int block_excl_scan_256p(int v, int* total, int* smem4) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int inc = v;                                         // (the loop stays written out: through wave_scan_incl the compiler schedules this kernel differently)
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        int t = __shfl_up(inc, d);
        if (lane >= d) inc += t;
    }
    if (lane == 63) smem4[w] = inc;
    __syncthreads();
    int base = 0;
    for (int i = 0; i < w; ++i) base += smem4[i];
    *total = smem4[0] + smem4[1] + smem4[2] + smem4[3];
    __syncthreads();
    return base + inc - v;
}

// ---- list building: count, scan, fill for SEVERAL tables in one launch set ----------------------------------------------------
// A U-Net forward needs the lists of ~14 tables (one 5^3, five 3^3, four down, four up); built one by one that was 14 x (2
// memsets + count + scan + fill) = 70 launches of a few microseconds each on the critical path of every scene.  Here a launch
// covers all tables: a workgroup finds its (table, offset, row block) from the tables' cumulative block counts, and the fill
// kernel writes the -1 padding itself (segment tails, the unused end of in_idx / tile_k) instead of two memsets per table.
#define PL_MAX_TABLES 16
#define RL_ROWS 256             // rows per workgroup of the row-list kernel
struct PLTable {
    const int32_t* nbr; int32_t* pos; int32_t* in_idx; int32_t* tile_k; int32_t* blk_cnt; int32_t* totals;
    int32_t* rlist;                // [M][rl_stride]: per output row {count, list positions of its pairs in offset order} (NULL: not built)
    int32_t* out_idx;              // [p_cap]: output row of every list entry, -1 on padding (NULL: not built)
    int64_t M, p_cap;
    int K, nblk, wg0, k0;          // wg0: first workgroup of this table in the (K * nblk)-flattened grid; k0: first of the K-flattened grid
    int rl_stride, rb0, meta;      // rb0: first workgroup of the table in the row-list grid; meta: tile_k carries two reserved (zero) slots behind the tile count
};
struct PLBatch { int n; PLTable t[PL_MAX_TABLES]; };

__device__ __forceinline__ int pl_find_table(const PLBatch& b, int wg, int by) {           // by: 0 = wg0, 1 = k0, 2 = rb0
    int ti = 0;
    for (int i = 1; i < b.n; ++i) if (wg >= (by == 1 ? b.t[i].k0 : (by == 2 ? b.t[i].rb0 : b.t[i].wg0))) ti = i;
    return ti;
}

__global__ __launch_bounds__(256) void pair_count_batch_kernel(const PLBatch b) {
    __shared__ int sm[4];
    const int ti = pl_find_table(b, blockIdx.x, 0);
    const PLTable& T = b.t[ti];
    const int local = blockIdx.x - T.wg0, k = local / T.nblk, blk = local - k * T.nblk, tid = threadIdx.x;
    int c = 0;
#pragma unroll
    for (int i = 0; i < PL_ROWS / 256; ++i) {
        const int64_t row = (int64_t)blk * PL_ROWS + i * 256 + tid;
        const bool v = row < T.M && T.nbr[(int64_t)k * T.M + row] >= 0;
        c += __popcll(__ballot(v));
    }
    if ((tid & 63) == 0) sm[tid >> 6] = c;
    __syncthreads();
    if (tid == 0) T.blk_cnt[(int64_t)k * T.nblk + blk] = sm[0] + sm[1] + sm[2] + sm[3];
}

__device__ __forceinline__ void pair_scan_batch_body(const PLBatch& b, const int bx) {
    __shared__ int sm[4];
    const int ti = pl_find_table(b, bx, 1);
    const PLTable& T = b.t[ti];
    const int k = bx - T.k0, tid = threadIdx.x;
    int running = 0;
    for (int base = 0; base < T.nblk; base += 256) {
        const int i = base + tid;
        const int v = i < T.nblk ? T.blk_cnt[(int64_t)k * T.nblk + i] : 0;
        int total;
        const int ex = block_excl_scan_256p(v, &total, sm);
        if (i < T.nblk) T.blk_cnt[(int64_t)k * T.nblk + i] = running + ex;
        running += total;
    }
    if (tid == 0) T.totals[k] = running;
}
__global__ __launch_bounds__(256) void pair_scan_batch_kernel(const PLBatch b) { pair_scan_batch_body(b, (int)blockIdx.x); }

__global__ __launch_bounds__(256) void pair_fill_batch_kernel(const PLBatch b) {
    __shared__ int sm[4];
    __shared__ int wcnt[4];
    const int ti = pl_find_table(b, blockIdx.x, 0);
    const PLTable& T = b.t[ti];
    const int local = blockIdx.x - T.wg0, k = local / T.nblk, blk = local - k * T.nblk;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int s = 0;
    for (int kk = tid; kk < k; kk += 256) s += (T.totals[kk] + PT - 1) / PT * PT;
    int seg;
    block_excl_scan_256p(s, &seg, sm);
    const int tot_k = T.totals[k];
    const int seg_len = (tot_k + PT - 1) / PT * PT;
    if (blk == 0) {
        for (int t = tid; t < seg_len / PT; t += 256)
            if ((int64_t)(seg / PT + t) * PT < T.p_cap) T.tile_k[seg / PT + t] = k;
        for (int e = tot_k + tid; e < seg_len; e += 256)       // the segment's padding
            if ((int64_t)seg + e < T.p_cap) {
                T.in_idx[seg + e] = -1;
                if (T.out_idx) T.out_idx[seg + e] = -1;
            }
        if (k == T.K - 1 && tid == 0) {                        // number of real tiles, after the last slot
            const int64_t end = (int64_t)seg + seg_len < T.p_cap ? (int64_t)seg + seg_len : T.p_cap;
            T.tile_k[T.p_cap / PT] = (int)(end / PT);
            if (T.meta & 1) { T.tile_k[T.p_cap / PT + 1] = 0; T.tile_k[T.p_cap / PT + 2] = 0; }
        }
    }
    if (k == T.K - 1 && !(T.meta & 2)) {
        // past the last segment: unused capacity reads as "no pair".  Every row block of the last offset fills its slice
        // (with worst-case sized lists, SD3D_EXACT_PAIRS=0, the tail is tens of MB: one workgroup would sit on the critical path;
        //  meta & 2: the caller's consumers walk tile_k[p_cap / 128] tiles and nothing else - the tail stays unwritten)
        const int64_t end = (int64_t)seg + seg_len < T.p_cap ? (int64_t)seg + seg_len : T.p_cap;
        for (int64_t e = end + (int64_t)blk * 256 + tid; e < T.p_cap; e += (int64_t)T.nblk * 256) {
            T.in_idx[e] = -1;
            if (T.out_idx) T.out_idx[e] = -1;
        }
        for (int64_t t = end / PT + (int64_t)blk * 256 + tid; t < T.p_cap / PT; t += (int64_t)T.nblk * 256) T.tile_k[t] = -1;
    }
    // Round 5: a wave owns 512 consecutive rows of the block and requests all eight of its 64-row slices at once; the waves meet ONCE
    // (their totals through LDS).  Before: eight rounds of {load, ballot, two barriers} per workgroup - 84 us for the stem's 5^3 table,
    // whose 12.5 M slots it walks at 1.2 TB/s.  Same positions (rows ascending within an offset).
    int base = seg + T.blk_cnt[(int64_t)k * T.nblk + blk];
    const uint64_t lt = (1ull << lane) - 1ull;
    constexpr int NS = PL_ROWS / 256;
    const int64_t row0 = (int64_t)blk * PL_ROWS + (int64_t)wv * (PL_ROWS / 4) + lane;
    int id[NS];
    uint64_t bal[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const int64_t row = row0 + i * 64;
        id[i] = T.nbr[(int64_t)k * T.M + (row < T.M ? row : 0)];
        if (row >= T.M) id[i] = -1;
    }
    int wtot = 0;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        bal[i] = __ballot(id[i] >= 0);
        wtot += __popcll(bal[i]);
    }
    if (lane == 0) wcnt[wv] = wtot;
    __syncthreads();
    for (int w = 0; w < wv; ++w) base += wcnt[w];
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const int64_t row = row0 + i * 64;
        const int p = base + __popcll(bal[i] & lt);
        if (T.pos && row < T.M) T.pos[(int64_t)k * T.M + row] = (id[i] >= 0 && p < T.p_cap) ? p : -1;
        if (id[i] >= 0 && p < T.p_cap) {
            T.in_idx[p] = id[i];
            if (T.out_idx) T.out_idx[p] = (int32_t)row;
        }
        base += __popcll(bal[i]);
    }
}

// Per output row: how many partial products pass 2 has to add up and where they are - {count, positions in offset order} in
// rl_stride ints per row (the count and the first three positions arrive with ONE 16-byte load; a level-0 row has ~2 partners, so
// walking all K slots of pos[k][r] was 27 loads for 3 hits).  One thread per row; pos is read offset-major (coalesced over rows).
__global__ __launch_bounds__(RL_ROWS) void pair_rowlist_batch_kernel(const PLBatch b) {
    const int ti = pl_find_table(b, blockIdx.x, 2);
    const PLTable& T = b.t[ti];
    if (!T.rlist) return;
    const int64_t row = (int64_t)(blockIdx.x - T.rb0) * RL_ROWS + threadIdx.x;
    if (row >= T.M) return;
    int32_t* rl = T.rlist + row * T.rl_stride;
    int cnt = 0;
    for (int k0 = 0; k0 < T.K; k0 += 16) {                    // sixteen columns requested together (the stem's table has 125)
        int v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            v[u] = T.pos[(int64_t)(k0 + u < T.K ? k0 + u : T.K - 1) * T.M + row];
            if (k0 + u >= T.K) v[u] = -1;
        }
#pragma unroll
        for (int u = 0; u < 16; ++u)
            if (v[u] >= 0) rl[1 + cnt++] = v[u];
    }
    rl[0] = cnt;
}

// ---- plain lists without a position table (round 5) -------------------------------------------------------------------------------
// An evaluation forward never reads pos [K, M]: pass 2 walks the per-row lists.  For the stem's 5^3 table pos is 69 MB written by the
// fill launch and read back by the row-list launch (and the lists' unused capacity, sized for the worst case when one scene is in
// flight, another 55 MB of -1).  When the caller asks for row lists but no pos (pos == NULL), the builder takes the row-block form
// of the chained builder: a workgroup owns 256 rows and walks all K offsets of them, the fill launch writes the rows' lists itself.
// Same in_idx / tile_k / rlist as the (offset, row block) form, entry for entry.
#define PR_MAX_K 128
template <class F>
__device__ __forceinline__ void pr_walk(const PLTable& T, int64_t row, bool live, F&& f) {
    const int64_t rc = live ? row : 0;
    for (int k0 = 0; k0 < T.K; k0 += 8) {
        int id[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) id[u] = T.nbr[(int64_t)(k0 + u < T.K ? k0 + u : T.K - 1) * T.M + rc];
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (k0 + u < T.K) f(k0 + u, live ? id[u] : -1);
    }
}
__device__ __forceinline__ void pair_count_rows_body(const PLBatch& b, const int bx) {
    __shared__ int wc[4][PR_MAX_K];
    const int ti = pl_find_table(b, bx, 0);
    const PLTable& T = b.t[ti];
    const int blk = bx - T.wg0, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t row = (int64_t)blk * 256 + tid;
    pr_walk(T, row, row < T.M, [&](int k, int id) {
        const int c = __popcll(__ballot(id >= 0));
        if (lane == 0) wc[wv][k] = c;
    });
    __syncthreads();
    if (tid < T.K) T.blk_cnt[(int64_t)tid * T.nblk + blk] = wc[0][tid] + wc[1][tid] + wc[2][tid] + wc[3][tid];
}
__global__ __launch_bounds__(256) void pair_count_rows_kernel(const PLBatch b) { pair_count_rows_body(b, (int)blockIdx.x); }
__device__ __forceinline__ void pair_fill_rows_body(const PLBatch& b, const int bx) {
    __shared__ int sm[4];
    __shared__ int wb[4][PR_MAX_K];
    __shared__ int seg[PR_MAX_K + 1], tot[PR_MAX_K];
    const int ti = pl_find_table(b, bx, 0);
    const PLTable& T = b.t[ti];
    const int blk = bx - T.wg0, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t row = (int64_t)blk * 256 + tid;
    const bool live = row < T.M;
    {   // first list position of every offset's segment = the padded totals before it
        const int t = tid < T.K ? T.totals[tid] : 0;
        int end;
        const int ex = block_excl_scan_256p((t + PT - 1) / PT * PT, &end, sm);
        if (tid < T.K) { seg[tid] = ex; tot[tid] = t; }
        if (tid == 0) seg[T.K] = end;
    }
    pr_walk(T, row, live, [&](int k, int id) {
        const int c = __popcll(__ballot(id >= 0));
        if (lane == 0) wb[wv][k] = c;
    });
    __syncthreads();
    if (tid < T.K) {
        int run = T.blk_cnt[(int64_t)tid * T.nblk + blk];
#pragma unroll
        for (int w = 0; w < 4; ++w) { const int c = wb[w][tid]; wb[w][tid] = run; run += c; }
    }
    __syncthreads();
    for (int k = blk; k < T.K; k += T.nblk) {                      // tile headers and the -1 padding of the segments, dealt out to the row blocks
        const int seg_len = (tot[k] + PT - 1) / PT * PT;
        for (int t = tid; t < seg_len / PT; t += 256)
            if ((int64_t)(seg[k] / PT + t) * PT < T.p_cap) T.tile_k[seg[k] / PT + t] = k;
        for (int e = tot[k] + tid; e < seg_len; e += 256)
            if ((int64_t)seg[k] + e < T.p_cap) {
                T.in_idx[seg[k] + e] = -1;
                if (T.out_idx) T.out_idx[seg[k] + e] = -1;
            }
    }
    {
        const int64_t end = (int64_t)seg[T.K] < T.p_cap ? (int64_t)seg[T.K] : T.p_cap;
        if (blk == 0 && tid == 0) {
            T.tile_k[T.p_cap / PT] = (int)(end / PT);
            if (T.meta & 1) { T.tile_k[T.p_cap / PT + 1] = 0; T.tile_k[T.p_cap / PT + 2] = 0; }
        }
        if (!(T.meta & 2)) {
            for (int64_t e = end + (int64_t)blk * 256 + tid; e < T.p_cap; e += (int64_t)T.nblk * 256) {
                T.in_idx[e] = -1;
                if (T.out_idx) T.out_idx[e] = -1;
            }
            for (int64_t t = end / PT + (int64_t)blk * 256 + tid; t < T.p_cap / PT; t += (int64_t)T.nblk * 256) T.tile_k[t] = -1;
        }
    }
    const uint64_t lt = (1ull << lane) - 1ull;
    int32_t* rl = T.rlist ? T.rlist + (live ? row : 0) * T.rl_stride : nullptr;
    int cnt = 0;
    pr_walk(T, row, live, [&](int k, int id) {
        const uint64_t bal = __ballot(id >= 0);
        if (id >= 0) {
            const int p = seg[k] + wb[wv][k] + __popcll(bal & lt);
            if (p < T.p_cap) {
                T.in_idx[p] = id;
                if (T.out_idx) T.out_idx[p] = (int32_t)row;
                if (rl) rl[1 + cnt] = p;
            }
            ++cnt;
        }
    });
    if (live && rl) rl[0] = cnt;
}
__global__ __launch_bounds__(256) void pair_fill_rows_kernel(const PLBatch b) { pair_fill_rows_body(b, (int)blockIdx.x); }

// ---- chained lists: mirror offsets and the centre share ONE partial product ----------------------------------------------------
// A stride-1 table of a voxel set onto itself with an odd kernel (3^3) enumerates its offsets symmetrically: off[K-1-k] == -off[k],
// centre = K / 2.  On a surface a row that has a neighbour at +d mostly has one at -d too (measured on the benchmark scene: 48 % /
// 76 % / 75 % of the non-centre entries of levels 1 / 2 / 3 come in such mirror pairs, tools/mirror_pairs.py), and EVERY row has
// its centre.  The pair-major convolution pays 2 x 4 x Cout bytes of HBM traffic per list entry for the partial product (written
// by pass 1, read by pass 2).  Here the entries of one output row that belong to the same mirror group g = {k = g, K-1-g}, plus
// the centre in the row's first non-empty group, share ONE partial product: pass 1 keeps accumulating across up to three
// consecutive "sub-tiles" (same 128 rows, sources centre -> +d -> -d, each with its own gather indices and its own W[k]) and
// stores once (tile_k carries PG_CHAIN on all but the last sub-tile).  Rows are sorted into SEGMENTS by (group, pattern) so that
// every sub-tile row is a real product: no MFMA row is wasted, the flops are exactly the rulebook's.  Partial rows at 150 k points:
// level 0 -27 %, level 1 -35 %, levels 2-4 -40...-44 %.  Pass 2 is unchanged (per-row lists of partial positions, ascending).
//   pattern: 0 {a} 1 {b} 2 {a,b} 3 {c,a} 4 {c,b} 5 {c,a,b}   (a = nbr[g][r], b = nbr[K-1-g][r], c = the centre: idx r)
//   segment g * 6 + pattern for g < G = K / 2;  segment 6 G = rows without any neighbour (centre alone)
//   entry i of a segment with n sources: sub-tile (i / 128) * n + s of the segment, slot i % 128
#define CH_NPAT 6
#define CH_ROWS 256              // rows per workgroup of the chained builder (one row per thread)
#define CH_GB 7                  // mirror groups whose two columns are requested together
#define CH_MAX_G 62              // K <= 125
#define CH_MAX_SEG (CH_MAX_G * CH_NPAT + 1)
// Round 5 form of the builder: a workgroup owns 256 ROWS and walks all mirror groups of them (before: one workgroup per (group, 2048
// rows), five launches - first group per row, count, scan, fill, per-row lists - with the group positions [G + 1][M] and the first
// groups [M] going through memory in between: 0.49 ms of kernel time per scene).  A row's first non-empty group is known on the fly
// when the groups are walked in ascending order, so the count launch needs no first-group pass, and the fill launch knows ALL partial
// positions of its rows: it writes the per-row lists itself.  Three launches (count, scan, fill); the table is read twice instead of
// ~4.5 times and nothing but the per-(segment, row block) counters sits between them.  The lists are the same, entry for entry.
struct CHTable {
    const int32_t* nbr; int32_t* in_idx; int32_t* tile_k; int32_t* blk_cnt; int32_t* totals; int32_t* rlist;
    int64_t M, p_cap;
    int K, G, nblk, rl_stride;
    int wg0, sg0;                  // first workgroup of the table in the row-block grid / the segment grid
    int lean;                      // 1: the unused capacity behind the last segment stays unwritten (sd3d_pair_table_desc.meta & 2)
};
struct CHBatch { int n; CHTable t[PL_MAX_TABLES]; };
__device__ __forceinline__ int ch_find(const CHBatch& b, int wg, int by) {
    int ti = 0;
    for (int i = 1; i < b.n; ++i) if (wg >= (by == 0 ? b.t[i].wg0 : b.t[i].sg0)) ti = i;
    return ti;
}
__device__ __forceinline__ int ch_nsrc(int pat) { return pat < 2 ? 1 : (pat < 5 ? 2 : 3); }

// The mirror groups of one row in ascending order: f(g, pattern, ia, ib) for EVERY group (pattern -1: no neighbour in it; the calls are
// wave-uniform, f may ballot).  Returns whether the row has any neighbour at all.  The two columns of CH_GB groups are requested
// together (coalesced over the rows, independent).
template <class F>
__device__ __forceinline__ bool ch_walk(const CHTable& T, int64_t row, bool live, F&& f) {
    bool seen = false;
    const int64_t rc = live ? row : 0;
    for (int g0 = 0; g0 < T.G; g0 += CH_GB) {
        int a[CH_GB], b[CH_GB];
#pragma unroll
        for (int u = 0; u < CH_GB; ++u) {
            const int g = g0 + u < T.G ? g0 + u : T.G - 1;
            a[u] = T.nbr[(int64_t)g * T.M + rc];
            b[u] = T.nbr[(int64_t)(T.K - 1 - g) * T.M + rc];
        }
#pragma unroll
        for (int u = 0; u < CH_GB; ++u) {
            if (g0 + u < T.G) {
                const int ia = live ? a[u] : -1, ib = live ? b[u] : -1;
                int pat = -1;
                if (ia >= 0 || ib >= 0) {
                    pat = (ia >= 0 ? (ib >= 0 ? 2 : 0) : 1) + (seen ? 0 : 3);     // the centre rides in the row's first non-empty group
                    seen = true;
                }
                f(g0 + u, pat, ia, ib);
            }
        }
    }
    return seen;
}

__device__ __forceinline__ void chain_count_body(const CHBatch& b, const int bx) {
    __shared__ int wc[4][CH_MAX_SEG];
    const int ti = ch_find(b, bx, 0);
    const CHTable& T = b.t[ti];
    const int blk = bx - T.wg0, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t row = (int64_t)blk * CH_ROWS + tid;
    const bool live = row < T.M;
    const bool seen = ch_walk(T, row, live, [&](int g, int pat, int, int) {
#pragma unroll
        for (int q = 0; q < CH_NPAT; ++q) {
            const int c = __popcll(__ballot(pat == q));
            if (lane == 0) wc[wv][g * CH_NPAT + q] = c;
        }
    });
    {
        const int c = __popcll(__ballot(live && !seen));        // the centre-only segment
        if (lane == 0) wc[wv][T.G * CH_NPAT] = c;
    }
    __syncthreads();
    const int nseg = T.G * CH_NPAT + 1;
    for (int sg = tid; sg < nseg; sg += 256) T.blk_cnt[(int64_t)sg * T.nblk + blk] = wc[0][sg] + wc[1][sg] + wc[2][sg] + wc[3][sg];
}
__global__ __launch_bounds__(256) void chain_count_kernel(const CHBatch b) { chain_count_body(b, (int)blockIdx.x); }
__device__ __forceinline__ void chain_scan_body(const CHBatch& b, const int bx) {
    __shared__ int sm[4];
    const int ti = ch_find(b, bx, 1);
    const CHTable& T = b.t[ti];
    const int seg = bx - T.sg0, tid = threadIdx.x;
    int running = 0;
    for (int base = 0; base < T.nblk; base += 256) {
        const int i = base + tid;
        const int v = i < T.nblk ? T.blk_cnt[(int64_t)seg * T.nblk + i] : 0;
        int total;
        const int ex = block_excl_scan_256p(v, &total, sm);
        if (i < T.nblk) T.blk_cnt[(int64_t)seg * T.nblk + i] = running + ex;
        running += total;
    }
    if (tid == 0) T.totals[seg] = running;
}
__global__ __launch_bounds__(256) void chain_scan_kernel(const CHBatch b) { chain_scan_body(b, (int)blockIdx.x); }
__device__ __forceinline__ void chain_fill_body(const CHBatch& b, const int bx) {
    __shared__ int sm[4];
    __shared__ int wb[4][CH_MAX_SEG];          // per wave: entries of the segment in this wave, then its first position in the segment
    __shared__ int seg_tile[CH_MAX_SEG], seg_tot[CH_MAX_SEG];
    const int ti = ch_find(b, bx, 0);
    const CHTable& T = b.t[ti];
    const int blk = bx - T.wg0, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int nseg = T.G * CH_NPAT + 1, centre = T.K / 2;
    const int64_t row = (int64_t)blk * CH_ROWS + tid;
    const bool live = row < T.M;
    // first tile of every segment = sum over the segments before it of ceil(total / 128) * sources
    int end_tile = 0;
    for (int base = 0; base < nseg; base += 256) {
        const int sg = base + tid;
        const int tot = sg < nseg ? T.totals[sg] : 0;
        const int v = (tot + PT - 1) / PT * (sg == nseg - 1 ? 1 : ch_nsrc(sg % CH_NPAT));
        int total;
        const int ex = block_excl_scan_256p(v, &total, sm);
        if (sg < nseg) { seg_tile[sg] = end_tile + ex; seg_tot[sg] = tot; }
        end_tile += total;
    }
    // this wave's entries per segment, then their first position: the block's start in the segment + the waves before this one
    const bool any = ch_walk(T, row, live, [&](int g, int pat, int, int) {
#pragma unroll
        for (int q = 0; q < CH_NPAT; ++q) {
            const int c = __popcll(__ballot(pat == q));
            if (lane == 0) wb[wv][g * CH_NPAT + q] = c;
        }
    });
    {
        const int c = __popcll(__ballot(live && !any));
        if (lane == 0) wb[wv][T.G * CH_NPAT] = c;
    }
    __syncthreads();
    for (int sg = tid; sg < nseg; sg += 256) {
        int run = T.blk_cnt[(int64_t)sg * T.nblk + blk];
#pragma unroll
        for (int w = 0; w < 4; ++w) { const int c = wb[w][sg]; wb[w][sg] = run; run += c; }
    }
    __syncthreads();
    // tile headers and the -1 padding of the segments, dealt out to the row blocks
    for (int sg = blk; sg < nseg; sg += T.nblk) {
        const int g = sg / CH_NPAT, q = sg - g * CH_NPAT;
        const int ns = g == T.G ? 1 : ch_nsrc(q), nt = (seg_tot[sg] + PT - 1) / PT;
        for (int e = tid; e < nt * ns; e += 256) {
            const int sub = e % ns;
            int k;                                      // source order: centre, +d (k = g), -d (k = K - 1 - g)
            if (g == T.G) k = centre;
            else if (q == 0) k = g;
            else if (q == 1) k = T.K - 1 - g;
            else if (q == 2) k = sub == 0 ? g : T.K - 1 - g;
            else if (q == 3) k = sub == 0 ? centre : g;
            else if (q == 4) k = sub == 0 ? centre : T.K - 1 - g;
            else k = sub == 0 ? centre : (sub == 1 ? g : T.K - 1 - g);
            if ((int64_t)(seg_tile[sg] + e) * PT < T.p_cap) T.tile_k[seg_tile[sg] + e] = k | (sub < ns - 1 ? PG_CHAIN : 0);
        }
        if (nt > 0) {
            const int fill0 = seg_tot[sg] - (nt - 1) * PT;       // real entries of the last tile row-block
            for (int e = tid; e < (PT - fill0) * ns; e += 256) {
                const int sub = e / (PT - fill0), off = fill0 + e % (PT - fill0);
                const int64_t pp = (int64_t)(seg_tile[sg] + (nt - 1) * ns + sub) * PT + off;
                if (pp < T.p_cap) T.in_idx[pp] = -1;
            }
        }
    }
    {
        // past the last segment: unused capacity reads as "no pair"; the number of real tiles after the last slot
        const int64_t cap_tiles = T.p_cap / PT;
        if (blk == 0 && tid == 0) { T.tile_k[cap_tiles] = (int)(end_tile < cap_tiles ? end_tile : cap_tiles); T.tile_k[cap_tiles + 1] = 0; T.tile_k[cap_tiles + 2] = 0; }
        if (!T.lean) {
            for (int64_t e = (int64_t)end_tile * PT + (int64_t)blk * 256 + tid; e < T.p_cap; e += (int64_t)T.nblk * 256) T.in_idx[e] = -1;
            for (int64_t tt = end_tile + (int64_t)blk * 256 + tid; tt < cap_tiles; tt += (int64_t)T.nblk * 256) T.tile_k[tt] = -1;
        }
    }
    // the entries of this row, group by group, and its list of partial positions (the last sub-tile of each of its chains, ascending)
    const uint64_t lt = (1ull << lane) - 1ull;
    int32_t* rl = T.rlist + (live ? row : 0) * T.rl_stride;
    int cnt = 0;
    ch_walk(T, row, live, [&](int g, int pat, int ia, int ib) {
        uint64_t mine = 0;
#pragma unroll
        for (int q = 0; q < CH_NPAT; ++q) {
            const uint64_t bal = __ballot(pat == q);
            if (pat == q) mine = bal;
        }
        if (pat >= 0) {
            const int sg = g * CH_NPAT + pat, ns = ch_nsrc(pat);
            const int my = wb[wv][sg] + __popcll(mine & lt);
            const int64_t tile = seg_tile[sg] + (int64_t)(my >> 7) * ns;
            const int off = my & (PT - 1);
            if ((tile + ns) * PT <= T.p_cap) {
                int64_t pp = tile * PT + off;
                if (pat >= 3) { T.in_idx[pp] = (int)row; pp += PT; }      // the centre: in = out = r
                if (ia >= 0) { T.in_idx[pp] = ia; pp += PT; }
                if (ib >= 0) { T.in_idx[pp] = ib; pp += PT; }
                rl[1 + cnt++] = (int32_t)(pp - PT);
            }
        }
    });
    {
        const bool lone = live && !any;
        const uint64_t bal = __ballot(lone);
        if (lone) {
            const int sg = T.G * CH_NPAT;
            const int my = wb[wv][sg] + __popcll(bal & lt);
            const int64_t pp = (int64_t)(seg_tile[sg] + (my >> 7)) * PT + (my & (PT - 1));
            if (pp < T.p_cap) { T.in_idx[pp] = (int)row; rl[1 + cnt++] = (int32_t)pp; }
        }
    }
    if (live) rl[0] = cnt;
}
__global__ __launch_bounds__(256) void chain_fill_kernel(const CHBatch b) { chain_fill_body(b, (int)blockIdx.x); }
// The chained tables and the position-free plain tables of a scene in the SAME three launches (count, scan, fill): two independent
// chains of three dependent launches on one stream were six launch latencies in front of the first convolution.  A workgroup below
// `n_chain` runs the chained builder's body, the others the row-block builder's - the same code on the same data.
__global__ __launch_bounds__(256) void lists_count_kernel(const CHBatch cb, const PLBatch rb, const int n_chain) {
    if ((int)blockIdx.x < n_chain) chain_count_body(cb, (int)blockIdx.x);
    else pair_count_rows_body(rb, (int)blockIdx.x - n_chain);
}
__global__ __launch_bounds__(256) void lists_scan_kernel(const CHBatch cb, const PLBatch rb, const int n_chain) {
    if ((int)blockIdx.x < n_chain) chain_scan_body(cb, (int)blockIdx.x);
    else pair_scan_batch_body(rb, (int)blockIdx.x - n_chain);
}
__global__ __launch_bounds__(256) void lists_fill_kernel(const CHBatch cb, const PLBatch rb, const int n_chain) {
    if ((int)blockIdx.x < n_chain) chain_fill_body(cb, (int)blockIdx.x);
    else pair_fill_rows_body(rb, (int)blockIdx.x - n_chain);
}
static size_t chain_lists_ws_bytes(int K, int64_t M) {
    const int64_t nblk = cdiv(M, CH_ROWS);
    const int64_t nseg = (int64_t)(K / 2) * CH_NPAT + 1;
    return (size_t)(nseg * nblk + nseg) * sizeof(int32_t) + 256;
}

// ---- launchers --------------------------------------------------------------------------------
extern "C" size_t sd3d_pair_lists_ws_bytes(int K, int64_t M) {
    const int64_t nblk = cdiv(M, PL_ROWS);
    const size_t plain = (size_t)((int64_t)K * nblk + K) * sizeof(int32_t) + 256;
    const size_t chained = (K & 1) ? chain_lists_ws_bytes(K, M) : 0;      // (a table may be built either way: size for all)
    const size_t rows = (size_t)((int64_t)K * cdiv(M, 256) + K) * sizeof(int32_t) + 256;
    const size_t m = plain > chained ? plain : chained;
    return m > rows ? m : rows;
}

// n tables at once (n <= PL_MAX_TABLES); the tables' scratch sits back to back in ws (sd3d_pair_lists_ws_bytes(K_i, M_i) bytes each,
// rounded up to 256).  p_cap: capacity of in_idx in pairs (multiple of 128, >= pairs + K * 127); tile_k has p_cap / 128 + 1 entries
// (the last one receives the number of real tiles).  rlist / out_idx / the two centre slots of tile_k are optional products (see sd3d_pair_table_desc).
// blk_counts: NULL, or per table NULL or device int32 [K, cdiv(M, 256)]: the entry counts per (offset, 256-row block) that the count
// pass of the row-block form would produce (sd3d_kernel_maps_hier leaves them while it writes the table).  Such a table has no
// workgroups in the count launch; scan and fill run as ever, the scan in place over the given counts (they are consumed).  Only a
// table that takes the row-block form (no pos, K <= 128, not chained) may bring counts.
extern "C" int sd3d_pair_lists_desc(int n, const sd3d_pair_table_desc* d, int32_t* const* blk_counts, void* ws, size_t ws_bytes, void* stream) {
    if (n > 0 && !d) return sd3d_set_error(SD3D_ERR_ARG, "pair_lists_desc: tables is NULL");
    hipStream_t st = (hipStream_t)stream;
    if (n <= 0) return SD3D_OK;
    if (n > PL_MAX_TABLES) return sd3d_set_error(SD3D_ERR_ARG, "pair_lists_batch: at most 16 tables per call");
    PLBatch b, rbt, rbc;                                       // (offset, row block) form / row-block form (no pos table) / those of rbt that must count
    b.n = 0;
    rbt.n = 0;
    rbc.n = 0;
    int rwg = 0, rkk = 0, rcwg = 0;
    CHBatch cb;
    cb.n = 0;
    size_t off = 0;
    int wg = 0, kk = 0, rb = 0;
    int cwg = 0, csg = 0;
    for (int i = 0; i < n; ++i) {
        const int K = d[i].K;
        const int64_t M = d[i].M, p_cap = d[i].p_cap;
        int32_t* const given = blk_counts ? blk_counts[i] : nullptr;
        if (given && (d[i].center == SD3D_PAIR_CHAINED || d[i].pos || K > PR_MAX_K))
            return sd3d_set_error(SD3D_ERR_ARG, "pair_lists_desc: only a row-block table (no pos, K <= 128, not chained) takes block counts");
        if (d[i].center == SD3D_PAIR_CHAINED && K > 0 && M > 0) {
            // chained lists (mirror groups + centre share a partial product): their own builder
            if (!(K & 1) || K < 3) return sd3d_set_error(SD3D_ERR_ARG, "pair_lists_batch: chained lists need an odd kernel (symmetric offsets)");
            if (K / 2 > CH_MAX_G) return sd3d_set_error(SD3D_ERR_ARG, "pair_lists_batch: chained lists take kernels up to 5^3");
            if (p_cap <= 0 || (p_cap % PT) || !d[i].rlist || d[i].rl_stride < K / 2 + 2 || (d[i].rl_stride & 3))
                return sd3d_set_error(SD3D_ERR_ARG, "pair_lists_batch: chained lists need rlist and rl_stride >= K / 2 + 2");
            CHTable& T = cb.t[cb.n++];
            T.nbr = d[i].nbr; T.in_idx = d[i].in_idx; T.tile_k = d[i].tile_k; T.rlist = d[i].rlist; T.M = M; T.p_cap = p_cap;
            T.K = K; T.G = K / 2; T.nblk = (int)cdiv(M, CH_ROWS); T.rl_stride = d[i].rl_stride;
            const int nseg = T.G * CH_NPAT + 1;
            T.blk_cnt = (int32_t*)((char*)ws + off);
            T.totals = T.blk_cnt + (int64_t)nseg * T.nblk;
            off += align_up(chain_lists_ws_bytes(K, M), 256);
            T.wg0 = cwg; T.sg0 = csg; T.lean = (d[i].meta & 2) ? 1 : 0;
            cwg += T.nblk; csg += nseg;
            continue;
        }
        if (K <= 0 || M <= 0) {                                // no rows: a later pair_conv on this table must see "0 real tiles"
            if (d[i].tile_k && p_cap > 0 && hipMemsetAsync(d[i].tile_k + p_cap / PT, 0, ((d[i].meta & 1) ? 3 : 1) * sizeof(int32_t), st) != hipSuccess)
                return sd3d_set_error(SD3D_ERR_LAUNCH, "pair_lists_batch: memset failed");
            continue;
        }
        if (p_cap <= 0 || (p_cap % PT)) return sd3d_set_error(SD3D_ERR_ARG, "pair_lists_batch: p_cap must be a positive multiple of 128");
        if (d[i].rlist && (d[i].rl_stride < K + 4 || (d[i].rl_stride & 3))) return sd3d_set_error(SD3D_ERR_ARG, "pair_lists_batch: rl_stride must be a multiple of 4, >= K + 4");
        if (d[i].center >= 0) return sd3d_set_error(SD3D_ERR_ARG, "pair_lists_batch: center must be -1 or SD3D_PAIR_CHAINED");
        if (!d[i].pos && !d[i].rlist && !d[i].out_idx)
            return sd3d_set_error(SD3D_ERR_ARG, "pair_lists_batch: a table without pos needs rlist or out_idx (nothing could run pass 2 on it)");
        if (!d[i].pos && K <= PR_MAX_K) {                      // no position table wanted: the row-block form (three launches, the rows' lists from the fill)
            PLTable& T = rbt.t[rbt.n++];
            T.nbr = d[i].nbr; T.pos = nullptr; T.in_idx = d[i].in_idx; T.tile_k = d[i].tile_k; T.M = M; T.p_cap = p_cap; T.K = K;
            T.rlist = d[i].rlist; T.out_idx = d[i].out_idx; T.rl_stride = d[i].rl_stride; T.meta = d[i].meta;
            T.nblk = (int)cdiv(M, 256);
            T.blk_cnt = (int32_t*)((char*)ws + off);
            T.totals = T.blk_cnt + (int64_t)T.K * T.nblk;
            if (given) T.blk_cnt = given;
            off += align_up(sd3d_pair_lists_ws_bytes(K, M), 256);
            T.wg0 = rwg; T.k0 = rkk; T.rb0 = 0;
            rwg += T.nblk; rkk += T.K;
            if (!given) {                                      // the count launch numbers its workgroups over the tables that count
                PLTable& C = rbc.t[rbc.n++];
                C = T;
                C.wg0 = rcwg;
                rcwg += T.nblk;
            }
            continue;
        }
        if (!d[i].pos && d[i].rlist) return sd3d_set_error(SD3D_ERR_ARG, "pair_lists_batch: row lists without pos take kernels up to 128 offsets");
        PLTable& T = b.t[b.n++];
        T.nbr = d[i].nbr; T.pos = d[i].pos; T.in_idx = d[i].in_idx; T.tile_k = d[i].tile_k; T.M = M; T.p_cap = p_cap; T.K = K;
        T.rlist = d[i].rlist; T.out_idx = d[i].out_idx; T.rl_stride = d[i].rl_stride; T.meta = d[i].meta;
        T.nblk = (int)cdiv(M, PL_ROWS);
        T.blk_cnt = (int32_t*)((char*)ws + off);
        T.totals = T.blk_cnt + (int64_t)T.K * T.nblk;
        off += align_up(sd3d_pair_lists_ws_bytes(K, M), 256);
        T.wg0 = wg; T.k0 = kk; T.rb0 = rb;
        wg += T.K * T.nblk; kk += T.K;
        rb += T.rlist ? (int)cdiv(M, RL_ROWS) : 0;
    }
    if (off > ws_bytes) return sd3d_set_error(SD3D_ERR_ARG, "pair_lists_batch: workspace too small");
    if (cb.n > 0 && rbt.n > 0) {
        hipLaunchKernelGGL(lists_count_kernel, dim3(cwg + rcwg), dim3(256), 0, st, cb, rbc, cwg);
        hipLaunchKernelGGL(lists_scan_kernel, dim3(csg + rkk), dim3(256), 0, st, cb, rbt, csg);
        hipLaunchKernelGGL(lists_fill_kernel, dim3(cwg + rwg), dim3(256), 0, st, cb, rbt, cwg);
        SD3D_CHECK_LAUNCH();
    } else if (cb.n > 0) {
        hipLaunchKernelGGL(chain_count_kernel, dim3(cwg), dim3(256), 0, st, cb);
        hipLaunchKernelGGL(chain_scan_kernel, dim3(csg), dim3(256), 0, st, cb);
        hipLaunchKernelGGL(chain_fill_kernel, dim3(cwg), dim3(256), 0, st, cb);
        SD3D_CHECK_LAUNCH();
    } else if (rbt.n > 0) {
        if (rcwg > 0) hipLaunchKernelGGL(pair_count_rows_kernel, dim3(rcwg), dim3(256), 0, st, rbc);
        hipLaunchKernelGGL(pair_scan_batch_kernel, dim3(rkk), dim3(256), 0, st, rbt);
        hipLaunchKernelGGL(pair_fill_rows_kernel, dim3(rwg), dim3(256), 0, st, rbt);
        SD3D_CHECK_LAUNCH();
    }
    if (b.n == 0) return SD3D_OK;
    hipLaunchKernelGGL(pair_count_batch_kernel, dim3(wg), dim3(256), 0, st, b);
    hipLaunchKernelGGL(pair_scan_batch_kernel, dim3(kk), dim3(256), 0, st, b);
    hipLaunchKernelGGL(pair_fill_batch_kernel, dim3(wg), dim3(256), 0, st, b);
    if (rb > 0) hipLaunchKernelGGL(pair_rowlist_batch_kernel, dim3(rb), dim3(RL_ROWS), 0, st, b);
    SD3D_CHECK_LAUNCH();
    return SD3D_OK;
}
