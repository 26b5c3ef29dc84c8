// Connected components of a mesh, an edge list or a neighbour table, and the clean that drops the small ones (the rule:
// include/segdino3d_hip.h, "Connected components"; segdino3d_amd/components.py has it in full).  It is the stage between
// TsdfVolume.mesh() and simplify_mesh - and between fuse_views and point_superpoints - that throws away what is not the scene: the
// floating shells and specks a TSDF fused from real depth leaves behind.  The reference has no counterpart (its meshes were cleaned
// offline), so tests/components_ref.py - a numpy restatement of the rule - is what these kernels are pinned against, bit for bit.
//
// Components are order-free: the answer is a function of the SET of links.  Every decision here is an integer one and every statistic
// a sum or a minimum over a set, so nothing depends on the order of the atomics, on the cut into waves, or on the stream.
//
//   cc_init_kernel      one lane per 8 nodes: step 1 (all channels |c| < 2^14), parent[i] = i.
//   cc_hook_kernel      one lane per 8 links, templated on the link source: step 2, then a lock-free union of the link's ends that always
//                       hooks the larger root under the smaller.  parent[x] <= x holds at all times, so every find walks a strictly
//                       decreasing chain and the final root of a class IS its smallest node.  The 8 XCDs have private L2s and a plain load
//                       may be stale for the whole launch: EVERY access to parent in this launch is an agent-scope relaxed atomic
//                       (cc_load, cc_find, cc_union).  A stale value is then still an ancestor and costs a retry, not correctness; a
//                       failed compare-and-swap continues from the value it returned.  Nothing spins on a word another workgroup must
//                       write: every retry is caused by someone else's SUCCESSFUL compare-and-swap, so the launch cannot wait on itself.
//   cc_flatten_kernel   a new launch, so everything is visible: root[i] by walking with plain loads, the root flags, the isolated nodes.
//                       scan_exclusive_i32 over the flags numbers the components in ascending order of their smallest node.
//   cc_label_kernel     labels, and the sort key (label, node).  sort_pairs_u64: a component's nodes become one run.
//   cc_node_stats_kernel  a wave walks 512 sorted positions in 8 steps of 64: a segmented scan over the 64 entries of a step (a run is
//                       contiguous), the run open at lane 63 carried into the next step, one atomic per (wave, run): the count by
//                       atomicAdd, the box by 32-bit atomicMin / atomicMax on the integer key of the coordinate's bits.  A component of
//                       all n nodes costs n / 512 atomics per word, not n.
//   cc_verify_kernel    one lane per 8 links: a good link whose ends have different roots adds to `unsettled` (a coherence mistake becomes
//                       an error instead of a wrong mesh), and the sort key of the link: the label of its first end.
//   cc_link_stats_kernel  the same segmented count over the sorted links.
//   cc_finish_kernel    one lane per component: box, extent (three fp32 subtractions, the only float arithmetic here), step 5's three
//                       thresholds, and with keep_largest the 62-bit rank key (n_links descending, label ascending) for sort_pairs_u64.
//   cc_rank_kernel      keep_largest: the first m sorted passing components stay.
//   cc_node_keep_kernel, cc_link_keep_kernel   the flags of the kept nodes and links; three scans (components, nodes, links).
//   cc_write_nodes_kernel, cc_write_links_kernel   step 6: rows, maps, renumbered links, the cleaned table.
//   cc_info_kernel      the eight counters.
// The kernels that count give a workgroup 2048 elements and one atomic per counter (same-address atomics serialise at the L2:
// profiles/raster.md).  All values are written with plain vector stores.
#include "common.h"
// The kernels here must EQUAL the restatement, so nothing in this file may be contracted into a fused multiply-add.
#pragma clang fp contract(off)
#include "../../include/segdino3d_hip.h"

#define CC_THREADS 256
#define CC_WAVES (CC_THREADS / 64)
#define CC_ITEMS 8                                      // elements per lane in the kernels that count
#define CC_LIMIT 16384.0f                               // |c| < 2^14
#define CC_NONE 0xFFFFFFFFull                           // the sort key of a bad node and of a link that is not good: sorts last
// the device counters: int32 components, kept, nodes, links | int64 bad_nodes, bad_links, isolated, unsettled
enum { CC_K = 0, CC_KEPT = 1, CC_NODES = 2, CC_LINKS = 3 };
enum { CC_BAD_N = 0, CC_BAD_L = 1, CC_ISOLATED = 2, CC_UNSETTLED = 3 };

struct CcWs {
    uint64_t *keys_a, *keys_b;                          // [max(n, L)]: the node sort, the link sort, the rank sort
    uint32_t *idx_a, *idx_b;
    uint8_t* good;                                      // [n]
    int32_t *parent, *root, *touched;                   // [n]
    int32_t *flag, *excl;                               // [n]: root flags and their exclusive scan
    uint32_t *box_lo, *box_hi;                          // [n][3]: per component the integer keys of the box
    int32_t *ckeep, *cexcl;                             // [n]: per component kept, the exclusive scan
    int32_t *nkeep, *nexcl;                             // [n]: per node kept, the exclusive scan
    int32_t *lkeep, *lexcl;                             // [L]: per link kept, the exclusive scan
    int32_t* ints;                                      // CC_K ..
    int64_t* counts;                                    // CC_BAD_N ..
    void *sort_ws, *scan_ws;
    size_t sort_bytes, scan_bytes, total;
};
static CcWs cc_ws(void* ws, int64_t n, int64_t L) {
    CcWs w;
    char* p = (char*)ws;
    size_t o = 0;
    const size_t v = (size_t)(n > 0 ? n : 1), f = (size_t)(L > 0 ? L : 1), m = v > f ? v : f;
    auto take = [&](size_t bytes) { char* q = p + o; o += align_up(bytes, 256); return (void*)q; };
    w.keys_a = (uint64_t*)take(m * 8); w.keys_b = (uint64_t*)take(m * 8);
    w.idx_a = (uint32_t*)take(m * 4); w.idx_b = (uint32_t*)take(m * 4);
    w.good = (uint8_t*)take(v);
    w.parent = (int32_t*)take(v * 4); w.root = (int32_t*)take(v * 4); w.touched = (int32_t*)take(v * 4);
    w.flag = (int32_t*)take(v * 4); w.excl = (int32_t*)take(v * 4);
    w.box_lo = (uint32_t*)take(v * 12); w.box_hi = (uint32_t*)take(v * 12);
    w.ckeep = (int32_t*)take(v * 4); w.cexcl = (int32_t*)take(v * 4);
    w.nkeep = (int32_t*)take(v * 4); w.nexcl = (int32_t*)take(v * 4);
    w.lkeep = (int32_t*)take(f * 4); w.lexcl = (int32_t*)take(f * 4);
    w.ints = (int32_t*)take(16);
    w.counts = (int64_t*)take(32);
    w.sort_bytes = sort_ws_bytes((int64_t)m); w.sort_ws = take(w.sort_bytes);
    w.scan_bytes = scan_ws_bytes((int64_t)m); w.scan_ws = take(w.scan_bytes);
    w.total = o;
    return w;
}

// One integer sum per class and workgroup (the shape of simplify.hip's counters): a lane counts its own CC_ITEMS elements, wave_sum,
// the waves through LDS, then one atomic where the class occurs.
template <int K>
__device__ __forceinline__ void cc_count(const int (&mine)[K], int64_t* __restrict__ counts, const int (&slot)[K]) {
    __shared__ int part[CC_WAVES][K];
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
            for (int i = 0; i < CC_WAVES; ++i) s += part[i][k];
            if (s) atomicAdd((unsigned long long*)&counts[slot[k]], (unsigned long long)s);
        }
}
// element `it` of this lane in a counting kernel: a workgroup covers CC_THREADS * CC_ITEMS consecutive elements, a wave 64 adjacent ones at a time
__device__ __forceinline__ int64_t cc_item(int it) { return ((int64_t)blockIdx.x * CC_ITEMS + it) * CC_THREADS + threadIdx.x; }
static inline unsigned cc_item_blocks(int64_t n) { return (unsigned)cdiv(n > 0 ? n : 1, (int64_t)CC_THREADS * CC_ITEMS); }
static inline unsigned cc_blocks(int64_t n) { return (unsigned)cdiv(n > 0 ? n : 1, (int64_t)CC_THREADS); }

// The runs of one wave: `run` is this lane's run (the lanes of a run are adjacent).  start = the first lane of this lane's run within
// the wave, last = whether this lane is the run's last in the wave.
__device__ __forceinline__ void cc_segments(int run, int lane, int& start, bool& last) {
    const int prev = __shfl_up(run, 1);
    const unsigned long long heads = __ballot(lane == 0 || prev != run);               // bit 0 is always set
    start = 63 - __clzll(heads & (~0ull >> (63 - lane)));
    last = lane == 63 || (((heads >> lane) >> 1) & 1ull);
}
// inclusive segmented scans over the wave: lane l ends with the sum / minimum / maximum over the lanes start .. l of its run
__device__ __forceinline__ int cc_seg_sum(int v, int lane, int start) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(v, d);
        if (lane - d >= start) v += t;
    }
    return v;
}
__device__ __forceinline__ uint32_t cc_seg_min(uint32_t v, int lane, int start) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(v, d);
        if (lane - d >= start && t < v) v = t;
    }
    return v;
}
__device__ __forceinline__ uint32_t cc_seg_max(uint32_t v, int lane, int start) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(v, d);
        if (lane - d >= start && t > v) v = t;
    }
    return v;
}

// the integer key of a float's bits: the order of the keys is the order of the floats, with -0 below +0
__device__ __forceinline__ uint32_t cc_float_key(float x) {
    const uint32_t b = __float_as_uint(x);
    return (b & 0x80000000u) ? ~b : (b ^ 0x80000000u);
}
__device__ __forceinline__ float cc_key_float(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

// ---------------------------------------------------------------------------------------------- the link sources
// The ends of link l as a triple (a source of two ends repeats the second) -> 0: an empty slot of the table, skipped; 1: good;
// 2: bad (an index outside [0, n) or a bad end).  In the table form link l is entry l % width of row l / width.
template <int S>
__device__ __forceinline__ int cc_link(const int32_t* __restrict__ links, int64_t l, int width, int64_t n, const uint8_t* __restrict__ good,
                                       int (&e)[3]) {
    if (S == SD3D_COMPONENTS_FACES) {
        e[0] = links[3 * l]; e[1] = links[3 * l + 1]; e[2] = links[3 * l + 2];
    } else if (S == SD3D_COMPONENTS_EDGES) {
        e[0] = links[2 * l]; e[1] = links[2 * l + 1]; e[2] = e[1];
    } else {
        e[0] = (int)(l / width); e[1] = links[l]; e[2] = e[1];
        if (e[1] == -1) return 0;
    }
#pragma unroll
    for (int j = 0; j < 3; ++j)
        if (e[j] < 0 || e[j] >= n || !good[e[j]]) return 2;
    return 1;
}

// ---------------------------------------------------------------------------------------------- hooking
__device__ __forceinline__ int cc_load(int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// The root of x as this lane can see it, halving the path on the way.  Every value read is an ancestor of x or was one (parent only
// ever decreases, inside the class), the chain decreases strictly, so the walk ends at a node that was a root when it was read.
__device__ __forceinline__ int cc_find(int32_t* parent, int x) {
    int p = cc_load(&parent[x]);
    while (p != x) {
        const int g = cc_load(&parent[p]);
        if (g != p) __hip_atomic_fetch_min(&parent[x], g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = p;
        p = g;
    }
    return x;
}
// Joins the classes of a and b: the larger root goes under the smaller node by one compare-and-swap on the root's own word.  A failure
// means somebody else hooked that root (their success): go on from the parent they wrote.  max(ra, rb) falls with every failure.
__device__ __forceinline__ void cc_union(int32_t* parent, int a, int b) {
    if (a == b) return;
    int ra = cc_find(parent, a), rb = cc_find(parent, b);
    while (ra != rb) {
        const int hi = ra > rb ? ra : rb, lo = ra > rb ? rb : ra;
        int seen = hi;
        if (__hip_atomic_compare_exchange_strong(&parent[hi], &seen, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
        ra = cc_find(parent, seen);
        rb = lo;
    }
}

__global__ __launch_bounds__(CC_THREADS) void cc_init_kernel(const float* __restrict__ coords, int64_t n, int C, uint8_t* __restrict__ good,
                                                             int32_t* __restrict__ parent, int64_t* __restrict__ counts) {
    int bad[1] = {0};
#pragma unroll 2
    for (int it = 0; it < CC_ITEMS; ++it) {
        const int64_t i = cc_item(it);
        if (i >= n) break;
        bool ok = true;
        if (coords) {
            const float* row = coords + i * C;
            for (int j = 0; j < C; ++j) ok = ok && fabsf(row[j]) < CC_LIMIT;            // a NaN fails
        }
        good[i] = ok;
        parent[i] = (int32_t)i;
        bad[0] += !ok;
    }
    const int slot[1] = {CC_BAD_N};
    cc_count<1>(bad, counts, slot);
}

template <int S>
__global__ __launch_bounds__(CC_THREADS) void cc_hook_kernel(const int32_t* __restrict__ links, int64_t L, int width, int64_t n,
                                                             const uint8_t* __restrict__ good, int32_t* parent, int32_t* __restrict__ touched,
                                                             int64_t* __restrict__ counts) {
    // 8 links per lane, not one: the roots of a large component are what every union meets, and with eight times as many lanes in
    // flight the same compare-and-swaps and loads queue on the same words for longer (measured: profiles/mesh_components.md)
    int bad[1] = {0};
    for (int it = 0; it < CC_ITEMS; ++it) {
        const int64_t l = cc_item(it);
        if (l >= L) break;
        int e[3];
        const int s = cc_link<S>(links, l, width, n, good, e);
        bad[0] += s == 2;
        if (s != 1) continue;
        touched[e[0]] = 1; touched[e[1]] = 1; touched[e[2]] = 1;                        // racing stores of the same value
        cc_union(parent, e[0], e[1]);
        cc_union(parent, e[1], e[2]);
    }
    const int slot[1] = {CC_BAD_L};
    cc_count<1>(bad, counts, slot);
}

// ---------------------------------------------------------------------------------------------- flatten, number, verify
__global__ __launch_bounds__(CC_THREADS) void cc_flatten_kernel(int64_t n, const uint8_t* __restrict__ good, const int32_t* __restrict__ parent,
                                                                const int32_t* __restrict__ touched, int32_t* __restrict__ root,
                                                                int32_t* __restrict__ flag, int64_t* __restrict__ counts) {
    int iso[1] = {0};
    for (int it = 0; it < CC_ITEMS; ++it) {
        const int64_t i = cc_item(it);
        if (i >= n) break;
        int r = -1;
        if (good[i]) {
            r = (int)i;
            for (int p = parent[r]; p != r; p = parent[r]) r = p;
            iso[0] += !touched[i];
        }
        root[i] = r;
        flag[i] = r == (int)i;
    }
    const int slot[1] = {CC_ISOLATED};
    cc_count<1>(iso, counts, slot);
}

__global__ __launch_bounds__(CC_THREADS) void cc_label_kernel(int64_t n, const int32_t* __restrict__ root, const int32_t* __restrict__ excl,
                                                              int32_t* __restrict__ labels, uint64_t* __restrict__ keys) {
    const int64_t i = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    if (i >= n) return;
    const int r = root[i];
    const int lab = r >= 0 ? excl[r] : -1;
    labels[i] = lab;
    keys[i] = (uint64_t)(uint32_t)lab;                                                   // -1 is CC_NONE
}

// A wave of the two statistics kernels walks CC_ITEMS * 64 consecutive sorted positions in steps of 64.  The run that is still open at
// lane 63 is not emitted: its partial result is carried (wave-uniform) into the next step, where lane 0 takes it over if its label is
// the same and emits it otherwise.  Only the last step emits at lane 63.
#define CC_STEP_SPAN (64 * CC_ITEMS)

__global__ __launch_bounds__(CC_THREADS) void cc_node_stats_kernel(const float* __restrict__ coords, int64_t n, int C,
                                                                   const uint64_t* __restrict__ keys, const uint32_t* __restrict__ idx,
                                                                   int32_t* __restrict__ comp_nodes, uint32_t* __restrict__ box_lo,
                                                                   uint32_t* __restrict__ box_hi) {
    const int lane = threadIdx.x & 63;
    const int64_t base = ((int64_t)blockIdx.x * CC_WAVES + (threadIdx.x >> 6)) * CC_STEP_SPAN;
    int c_lab = -1, c_cnt = 0;                                                          // the carried run
    uint32_t c_lo[3] = {~0u, ~0u, ~0u}, c_hi[3] = {0u, 0u, 0u};
    for (int s = 0; s < CC_ITEMS; ++s) {
        const int64_t first = base + (int64_t)s * 64, p = first + lane;
        if (first >= n) break;                                                          // uniform over the wave
        const bool final = s == CC_ITEMS - 1 || first + 64 >= n;
        int lab = -1;
        int64_t v = 0;
        if (p < n) {
            lab = (int)(uint32_t)keys[p];
            v = (int64_t)idx[p];
        }
        int start;
        bool last;
        cc_segments(lab, lane, start, last);
        const bool take = lane == 0 && c_lab >= 0 && lab == c_lab, flush = lane == 0 && c_lab >= 0 && lab != c_lab;
        const bool emit = last && lab >= 0 && (final || lane != 63);
        if (flush) atomicAdd(&comp_nodes[c_lab], c_cnt);
        const int cnt = cc_seg_sum((lab >= 0 ? 1 : 0) + (take ? c_cnt : 0), lane, start);
        if (emit) atomicAdd(&comp_nodes[lab], cnt);
        c_cnt = __shfl(cnt, 63);
        if (coords) {                                                                   // uniform
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const uint32_t k = cc_float_key(coords[v * C + a]);
                uint32_t lo = lab >= 0 ? k : ~0u, hi = lab >= 0 ? k : 0u;
                if (take) { lo = lo < c_lo[a] ? lo : c_lo[a]; hi = hi > c_hi[a] ? hi : c_hi[a]; }
                if (flush) {
                    atomicMin(&box_lo[(int64_t)c_lab * 3 + a], c_lo[a]);
                    atomicMax(&box_hi[(int64_t)c_lab * 3 + a], c_hi[a]);
                }
                lo = cc_seg_min(lo, lane, start);
                hi = cc_seg_max(hi, lane, start);
                if (emit) {
                    atomicMin(&box_lo[(int64_t)lab * 3 + a], lo);
                    atomicMax(&box_hi[(int64_t)lab * 3 + a], hi);
                }
                c_lo[a] = __shfl(lo, 63);
                c_hi[a] = __shfl(hi, 63);
            }
        }
        c_lab = final ? -1 : __shfl(lab, 63);
    }
}

template <int S>
__global__ __launch_bounds__(CC_THREADS) void cc_verify_kernel(const int32_t* __restrict__ links, int64_t L, int width, int64_t n,
                                                               const uint8_t* __restrict__ good, const int32_t* __restrict__ root,
                                                               const int32_t* __restrict__ labels, uint64_t* __restrict__ keys,
                                                               int64_t* __restrict__ counts) {
    int uns[1] = {0};
#pragma unroll 2
    for (int it = 0; it < CC_ITEMS; ++it) {
        const int64_t l = cc_item(it);
        if (l >= L) break;
        int e[3];
        uint64_t key = CC_NONE;
        if (cc_link<S>(links, l, width, n, good, e) == 1) {
            key = (uint64_t)(uint32_t)labels[e[0]];
            const int r = root[e[0]];
            uns[0] += root[e[1]] != r || root[e[2]] != r;
        }
        keys[l] = key;
    }
    const int slot[1] = {CC_UNSETTLED};
    cc_count<1>(uns, counts, slot);
}

__global__ __launch_bounds__(CC_THREADS) void cc_link_stats_kernel(int64_t L, const uint64_t* __restrict__ keys, int32_t* __restrict__ comp_links) {
    const int lane = threadIdx.x & 63;
    const int64_t base = ((int64_t)blockIdx.x * CC_WAVES + (threadIdx.x >> 6)) * CC_STEP_SPAN;
    int c_lab = -1, c_cnt = 0;                                                          // the carried run
    for (int s = 0; s < CC_ITEMS; ++s) {
        const int64_t first = base + (int64_t)s * 64, p = first + lane;
        if (first >= L) break;                                                          // uniform over the wave
        const bool final = s == CC_ITEMS - 1 || first + 64 >= L;
        const int lab = p < L ? (int)(uint32_t)keys[p] : -1;
        int start;
        bool last;
        cc_segments(lab, lane, start, last);
        const bool take = lane == 0 && c_lab >= 0 && lab == c_lab, flush = lane == 0 && c_lab >= 0 && lab != c_lab;
        if (flush) atomicAdd(&comp_links[c_lab], c_cnt);
        const int cnt = cc_seg_sum((lab >= 0 ? 1 : 0) + (take ? c_cnt : 0), lane, start);
        if (last && lab >= 0 && (final || lane != 63)) atomicAdd(&comp_links[lab], cnt);
        c_cnt = __shfl(cnt, 63);
        c_lab = final ? -1 : __shfl(lab, 63);
    }
}

// ---------------------------------------------------------------------------------------------- keep, rank, compact
__global__ __launch_bounds__(CC_THREADS) void cc_finish_kernel(int64_t n, int has_coords, const int32_t* __restrict__ ints,
                                                               const int32_t* __restrict__ comp_nodes, const int32_t* __restrict__ comp_links,
                                                               const uint32_t* __restrict__ box_lo, const uint32_t* __restrict__ box_hi,
                                                               int min_nodes, int min_links, float min_extent, int keep_largest,
                                                               float* __restrict__ box, int32_t* __restrict__ ckeep, uint8_t* __restrict__ keep,
                                                               uint64_t* __restrict__ keys) {
    const int64_t c = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    if (c >= n) return;
    if (c >= ints[CC_K]) {
        ckeep[c] = 0;
        if (keep_largest > 0) keys[c] = SD3D_EMPTY_KEY;
        return;
    }
    float extent = 0.0f;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float lo = has_coords ? cc_key_float(box_lo[c * 3 + a]) : 0.0f, hi = has_coords ? cc_key_float(box_hi[c * 3 + a]) : 0.0f;
        if (box) { box[c * 6 + 2 * a] = lo; box[c * 6 + 2 * a + 1] = hi; }
        const float d = hi - lo;
        extent = a == 0 ? d : fmaxf(extent, d);
    }
    const int nl = comp_links[c];
    const bool pass = comp_nodes[c] >= min_nodes && nl >= min_links && extent >= min_extent;
    if (keep_largest > 0) {
        // (n_links descending, label ascending) in 62 bits; the rank kernel decides
        keys[c] = pass ? ((uint64_t)(uint32_t)(0x7FFFFFFF - nl) << 31) | (uint64_t)c : SD3D_EMPTY_KEY;
        ckeep[c] = 0;
        if (keep) keep[c] = 0;
    } else {
        ckeep[c] = pass;
        if (keep) keep[c] = pass;
    }
}

__global__ __launch_bounds__(CC_THREADS) void cc_rank_kernel(int64_t n, int keep_largest, const uint64_t* __restrict__ keys,
                                                             int32_t* __restrict__ ckeep, uint8_t* __restrict__ keep) {
    const int64_t p = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    if (p >= n || p >= keep_largest) return;
    const uint64_t k = keys[p];
    if (k == SD3D_EMPTY_KEY) return;
    const int64_t c = (int64_t)(k & 0x7FFFFFFFull);
    ckeep[c] = 1;
    if (keep) keep[c] = 1;
}

__global__ __launch_bounds__(CC_THREADS) void cc_node_keep_kernel(int64_t n, const int32_t* __restrict__ labels, const int32_t* __restrict__ ckeep,
                                                                  int32_t* __restrict__ nkeep) {
    const int64_t i = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    if (i >= n) return;
    const int lab = labels[i];
    nkeep[i] = lab >= 0 && ckeep[lab];
}

template <int S>
__global__ __launch_bounds__(CC_THREADS) void cc_link_keep_kernel(const int32_t* __restrict__ links, int64_t L, int width, int64_t n,
                                                                  const uint8_t* __restrict__ good, const int32_t* __restrict__ nkeep,
                                                                  int32_t* __restrict__ lkeep) {
    const int64_t l = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    if (l >= L) return;
    int e[3];
    lkeep[l] = cc_link<S>(links, l, width, n, good, e) == 1 && nkeep[e[0]];
}

__global__ __launch_bounds__(CC_THREADS) void cc_write_nodes_kernel(const float* __restrict__ coords, int64_t n, int C,
                                                                    const int32_t* __restrict__ labels, const int32_t* __restrict__ nkeep,
                                                                    const int32_t* __restrict__ nexcl, const int32_t* __restrict__ cexcl,
                                                                    float* __restrict__ nodes_out, int32_t* __restrict__ node_map,
                                                                    int32_t* __restrict__ labels_out) {
    const int64_t i = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    if (i >= n) return;
    if (!nkeep[i]) {
        if (node_map) node_map[i] = -1;
        return;
    }
    const int64_t o = (int64_t)nexcl[i];
    if (node_map) node_map[i] = (int32_t)o;
    if (labels_out) labels_out[o] = cexcl[labels[i]];
    if (coords && nodes_out) {
        const uint32_t* row = (const uint32_t*)coords + i * C;                         // the row, bit for bit
        uint32_t* out = (uint32_t*)nodes_out + o * C;
        for (int j = 0; j < C; ++j) out[j] = row[j];
    }
}

template <int S>
__global__ __launch_bounds__(CC_THREADS) void cc_write_links_kernel(const int32_t* __restrict__ links, int64_t L, int width, int64_t n,
                                                                    const uint8_t* __restrict__ good, const int32_t* __restrict__ nkeep,
                                                                    const int32_t* __restrict__ nexcl, const int32_t* __restrict__ lkeep,
                                                                    const int32_t* __restrict__ lexcl, int32_t* __restrict__ links_out,
                                                                    int32_t* __restrict__ link_source) {
    const int64_t l = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    if (l >= L) return;
    if (S == SD3D_COMPONENTS_TABLE) {
        // the cleaned table keeps its k: row l / width moves to its node's new number, a dangling or empty entry is -1, in place
        const int64_t i = l / width;
        if (!nkeep[i] || !links_out) return;
        links_out[(int64_t)nexcl[i] * width + (l - i * width)] = lkeep[l] ? nexcl[links[l]] : -1;
        return;
    }
    if (!lkeep[l]) return;
    constexpr int W = S == SD3D_COMPONENTS_FACES ? 3 : 2;
    const int64_t o = (int64_t)lexcl[l];
    if (links_out)
#pragma unroll
        for (int j = 0; j < W; ++j) links_out[o * W + j] = nexcl[links[l * W + j]];
    if (link_source) link_source[o] = (int32_t)l;
}

__global__ void cc_info_kernel(const int32_t* __restrict__ ints, const int64_t* __restrict__ counts, int64_t* __restrict__ info) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    info[0] = ints[CC_K]; info[1] = ints[CC_KEPT]; info[2] = ints[CC_NODES]; info[3] = ints[CC_LINKS];
    info[4] = counts[CC_BAD_N]; info[5] = counts[CC_BAD_L]; info[6] = counts[CC_ISOLATED]; info[7] = counts[CC_UNSETTLED];
}

// ---------------------------------------------------------------------------------------------- C entry points
static bool cc_size_ok(int64_t n) { return n >= 0 && n <= 0x7FFFFFFFll; }
static bool cc_width_ok(int source, int width) {
    return source == SD3D_COMPONENTS_FACES ? width == 3 : source == SD3D_COMPONENTS_EDGES ? width == 2 : source == SD3D_COMPONENTS_TABLE && width >= 1;
}
static bool cc_channels_ok(int C) { return C == 0 || (C >= 3 && C <= SD3D_COMPONENTS_MAX_CHANNELS); }

// n_links counts LINKS: the rows of faces and edges, the entries of a table (rows times k)
extern "C" size_t sd3d_components_ws_bytes(int64_t n_nodes, int64_t n_links, int link_width, int n_channels) {
    if (!cc_size_ok(n_nodes) || !cc_size_ok(n_links) || link_width < 1 || !cc_channels_ok(n_channels)) return 0;
    return cc_ws(nullptr, n_nodes, n_links).total;
}

template <int S>
static int cc_run(const int32_t* links, int64_t L, int width, const float* coords, int64_t n, int C, int min_nodes, int min_links, float min_extent,
                  int keep_largest, int32_t* labels, int32_t* comp_nodes, int32_t* comp_links, float* box, uint8_t* keep, float* nodes_out,
                  int32_t* node_map, int32_t* links_out, int32_t* link_source, int32_t* labels_out, int64_t* info, const CcWs& w, hipStream_t st) {
    bool ok = hipMemsetAsync(w.ints, 0, 16, st) == hipSuccess && hipMemsetAsync(w.counts, 0, 32, st) == hipSuccess;
    if (n > 0) {
        ok = ok && hipMemsetAsync(w.touched, 0, (size_t)n * 4, st) == hipSuccess && hipMemsetAsync(comp_nodes, 0, (size_t)n * 4, st) == hipSuccess &&
             hipMemsetAsync(comp_links, 0, (size_t)n * 4, st) == hipSuccess && hipMemsetAsync(w.box_lo, 0xFF, (size_t)n * 12, st) == hipSuccess &&
             hipMemsetAsync(w.box_hi, 0, (size_t)n * 12, st) == hipSuccess;
    }
    if (!ok) return sd3d_set_error(SD3D_ERR_LAUNCH, "components: hipMemsetAsync failed");
    const dim3 block(CC_THREADS), ngrid(cc_blocks(n)), lgrid(cc_blocks(L)), nitems(cc_item_blocks(n)), litems(cc_item_blocks(L));
    if (n > 0) hipLaunchKernelGGL(cc_init_kernel, nitems, block, 0, st, coords, n, C, w.good, w.parent, w.counts);
    if (L > 0) hipLaunchKernelGGL(cc_hook_kernel<S>, litems, block, 0, st, links, L, width, n, w.good, w.parent, w.touched, w.counts);
    SD3D_CHECK_LAUNCH();
    if (n > 0) {
        hipLaunchKernelGGL(cc_flatten_kernel, nitems, block, 0, st, n, w.good, w.parent, w.touched, w.root, w.flag, w.counts);
        if (int rc = scan_exclusive_i32(w.flag, w.excl, n, nullptr, &w.ints[CC_K], w.scan_ws, w.scan_bytes, st)) return rc;
        hipLaunchKernelGGL(cc_label_kernel, ngrid, block, 0, st, n, w.root, w.excl, labels, w.keys_a);
        int landed = 0;
        if (int rc = sort_pairs_u64(w.keys_a, nullptr, w.keys_b, w.idx_b, n, 0, 32, w.sort_ws, w.sort_bytes, st, w.idx_a, &landed)) return rc;
        hipLaunchKernelGGL(cc_node_stats_kernel, nitems, block, 0, st, coords, n, C, landed ? w.keys_a : w.keys_b, landed ? w.idx_a : w.idx_b, comp_nodes,
                           w.box_lo, w.box_hi);
        SD3D_CHECK_LAUNCH();
    }
    if (L > 0) {
        hipLaunchKernelGGL(cc_verify_kernel<S>, litems, block, 0, st, links, L, width, n, w.good, w.root, labels, w.keys_a, w.counts);
        if (n > 0) {                                                                    // (with no node every link is bad)
            int landed = 0;
            if (int rc = sort_pairs_u64(w.keys_a, nullptr, w.keys_b, w.idx_b, L, 0, 32, w.sort_ws, w.sort_bytes, st, w.idx_a, &landed)) return rc;
            hipLaunchKernelGGL(cc_link_stats_kernel, litems, block, 0, st, L, landed ? w.keys_a : w.keys_b, comp_links);
        }
        SD3D_CHECK_LAUNCH();
    }
    if (n > 0) {
        hipLaunchKernelGGL(cc_finish_kernel, ngrid, block, 0, st, n, coords != nullptr, w.ints, comp_nodes, comp_links, w.box_lo, w.box_hi, min_nodes,
                           min_links, min_extent, keep_largest, box, w.ckeep, keep, w.keys_a);
        if (keep_largest > 0) {
            int landed = 0;
            if (int rc = sort_pairs_u64(w.keys_a, nullptr, w.keys_b, w.idx_b, n, 0, 62, w.sort_ws, w.sort_bytes, st, w.idx_a, &landed)) return rc;
            hipLaunchKernelGGL(cc_rank_kernel, ngrid, block, 0, st, n, keep_largest, landed ? w.keys_a : w.keys_b, w.ckeep, keep);
        }
        if (int rc = scan_exclusive_i32(w.ckeep, w.cexcl, n, nullptr, &w.ints[CC_KEPT], w.scan_ws, w.scan_bytes, st)) return rc;
        hipLaunchKernelGGL(cc_node_keep_kernel, ngrid, block, 0, st, n, labels, w.ckeep, w.nkeep);
        if (int rc = scan_exclusive_i32(w.nkeep, w.nexcl, n, nullptr, &w.ints[CC_NODES], w.scan_ws, w.scan_bytes, st)) return rc;
        if (L > 0) {
            hipLaunchKernelGGL(cc_link_keep_kernel<S>, lgrid, block, 0, st, links, L, width, n, w.good, w.nkeep, w.lkeep);
            if (int rc = scan_exclusive_i32(w.lkeep, w.lexcl, L, nullptr, &w.ints[CC_LINKS], w.scan_ws, w.scan_bytes, st)) return rc;
        }
        if (nodes_out || node_map || labels_out)
            hipLaunchKernelGGL(cc_write_nodes_kernel, ngrid, block, 0, st, coords, n, C, labels, w.nkeep, w.nexcl, w.cexcl, nodes_out, node_map, labels_out);
        if (L > 0 && (links_out || link_source))
            hipLaunchKernelGGL(cc_write_links_kernel<S>, lgrid, block, 0, st, links, L, width, n, w.good, w.nkeep, w.nexcl, w.lkeep, w.lexcl, links_out,
                               link_source);
    }
    hipLaunchKernelGGL(cc_info_kernel, dim3(1), dim3(64), 0, st, w.ints, w.counts, info);
    SD3D_CHECK_LAUNCH();
    return SD3D_OK;
}

extern "C" int sd3d_components(int source, const int32_t* links, int64_t n_links, int link_width, const float* coords, int64_t n_nodes, int n_channels,
                               int min_nodes, int min_links, float min_extent, int keep_largest, int32_t* labels, int32_t* comp_nodes,
                               int32_t* comp_links, float* box, uint8_t* keep, float* nodes_out, int32_t* node_map, int32_t* links_out,
                               int32_t* link_source, int32_t* labels_out, int64_t* info, void* ws, size_t ws_bytes, void* stream) {
    const int64_t n = n_nodes;
    if (!cc_width_ok(source, link_width)) return sd3d_set_error(SD3D_ERR_ARG, "components: source 0 (faces) has width 3, 1 (edges) width 2, 2 (table) width >= 1");
    if (!cc_size_ok(n) || !cc_size_ok(n_links)) return sd3d_set_error(SD3D_ERR_ARG, "components: 0 <= n_nodes, n_links < 2^31");
    const int64_t L = n_links;
    if (source == SD3D_COMPONENTS_TABLE && L != n * link_width)
        return sd3d_set_error(SD3D_ERR_ARG, "components: a table has one row of link_width entries per node (n_links = n_nodes * link_width < 2^31)");
    if (!cc_channels_ok(n_channels) || (coords != nullptr) != (n_channels != 0))
        return sd3d_set_error(SD3D_ERR_ARG, "components: 3 <= n_channels <= 11 with coordinates, 0 without");
    if (min_nodes < 0 || min_links < 0 || keep_largest < 0 || !(min_extent >= 0.0f) || !(min_extent < __builtin_inff()))
        return sd3d_set_error(SD3D_ERR_ARG, "components: min_nodes, min_links, keep_largest >= 0 and min_extent finite and >= 0");
    if (!info) return sd3d_set_error(SD3D_ERR_ARG, "components: info is required");
    if (!ws || ((uintptr_t)ws & 255) != 0) return sd3d_set_error(SD3D_ERR_ARG, "components: ws is required and must be 256-byte aligned");
    const CcWs w = cc_ws(ws, n, L);
    if (ws_bytes < w.total) return sd3d_set_error(SD3D_ERR_WS, "components: workspace too small (sd3d_components_ws_bytes)");
    if ((n > 0 && (!labels || !comp_nodes || !comp_links)) || (L > 0 && !links) || (nodes_out && !coords))
        return sd3d_set_error(SD3D_ERR_ARG, "components: NULL argument");
    const hipStream_t st = (hipStream_t)stream;
#define CC_RUN(S)                                                                                                                           \
    cc_run<S>(links, L, link_width, coords, n, n_channels, min_nodes, min_links, min_extent, keep_largest, labels, comp_nodes, comp_links, box, \
              keep, nodes_out, node_map, links_out, link_source, labels_out, info, w, st)
    if (source == SD3D_COMPONENTS_FACES) return CC_RUN(SD3D_COMPONENTS_FACES);
    if (source == SD3D_COMPONENTS_EDGES) return CC_RUN(SD3D_COMPONENTS_EDGES);
    return CC_RUN(SD3D_COMPONENTS_TABLE);
#undef CC_RUN
}
