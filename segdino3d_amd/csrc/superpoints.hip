// Superpoints from a triangle mesh: the graph segmentation ScanNet's segmentator applies to a scan (the reference loads its result from
// a dump; it has no counterpart here).  tests/superpoints_ref.py restates the rule of include/segdino3d_hip.h and these kernels EQUAL that
// restatement label for label: every arithmetic step is one correctly rounded fp32 operation (contraction is off in this file) or an
// exact integer one.  A batch of scenes is concatenated; vertex_offsets / face_offsets [n_scenes + 1] int64 say where each scene lies.
//
//   sp_init_kernel      parent = self, size = 1, thr = k_thresh, minv = INT_MAX per vertex.
//   sp_face_kernel      one thread per face: the unit normal as rint(n 2^24), added to the int64 sums of its three vertices with integer
//                       atomics (order-free); a face with an index outside its scene only counts in bad[scene].
//   sp_vnormal_kernel   one thread per vertex: (float)(double)sum, normalised.
//   sp_edge_kernel      one thread per edge 3 f + k: the weight's bits and the sort key (scene << 32) | bits.  sort_pairs_u64 with
//                       "value = original index" then orders every scene's edges by (bits, edge index), scenes staying contiguous.
//   sp_sweep_kernel     one workgroup of SP_BATCH lanes per scene, one launch per pass.  Per batch of SP_BATCH edges: every lane finds the roots of
//                       its edge's ends in the forest as it stands at the start of the batch (read-only, all finds in flight together);
//                       edges inside one component are dropped by ballot; the surviving edges' start-roots (at most 2 SP_BATCH distinct)
//                       enter an LDS hash table with their size and thr; wave 0 settles the survivors in order on a miniature union-find
//                       over the table's slots (every join inside a batch joins two start-roots, so this is the sequential rule), 64 at
//                       a time: an edge that is the lowest pending one at both of its components decides independently; the
//                       table is written back: a slot that is no longer a root links its vertex under its slot-root's vertex, a root
//                       stores size and thr.  Only roots are ever linked, under roots, and an end is only ever re-pointed at its root: the
//                       forest has no cycle.  Union by size keeps every path at log2 N links at most.  Every loop has a trip count the
//                       input cannot stretch: ceil(E / SP_BATCH) batches, N hops per find, SP_TABLE probes per insert.
//   sp_cand_kernel      between the passes, one thread per edge of the order: pass 2 can only ever join across an edge whose ends lie in
//                       different components, one of them below min_verts, when pass 2 begins - components only merge and sizes only
//                       grow.  Those candidates (few: 0.4 % of a scan's edges reach the table in pass 2) are flagged, scan_exclusive_i32 and sp_compact_kernel
//                       keep them in order, and pass 2 sweeps that list alone.
//   sp_min_kernel .. sp_info_kernel   the root of every vertex, the smallest vertex of every component (integer atomicMin), a flag at
//                       that vertex, scan_exclusive_i32 over the flags = the component's number, labels int64 and {S, bad_faces} per scene.
// All values are written with plain vector stores.
#include "common.h"
#include "../../include/segdino3d_hip.h"
#include <cstdio>

// Written with the operators: the header's __fmul_rn / __fadd_rn may fuse once inlined under the default contraction mode.
#pragma clang fp contract(off)

#define SP_BATCH 512                                    // edges per sweep batch = lanes of the sweep workgroup
#define SP_TABLE 2048                                   // hash slots: at most 2 SP_BATCH distinct start-roots, load <= 1 / 2
#define SP_MAX_SCENES (1 << 16)
#define SP_MAX_VERTICES 0x7FFFFFFFll

struct SpWs {
    long long* sums;                                    // [N][3]
    float* vnorm;                                       // [N][3]
    int32_t *parent, *size, *minv, *root, *flag, *excl; // [N]
    float* thr;                                         // [N]
    uint32_t *wbits, *vals_a, *vals_b;                  // [E]
    uint64_t *keys_a, *keys_b;                          // [E]
    int32_t *bad, *total, *cand_total;                  // [S], [1], [1]
    long long* stats;                                   // [S][2]
    void *sort_ws, *scan_ws;
    size_t sort_bytes, scan_bytes, total_bytes;
};
static SpWs sp_ws(void* ws, int64_t N, int64_t F, int S) {
    SpWs w;
    char* p = (char*)ws;
    size_t o = 0;
    auto take = [&](size_t bytes) { char* q = p + o; o += align_up(bytes, 256); return (void*)q; };
    const size_t n = (size_t)(N > 0 ? N : 1), e = (size_t)(F > 0 ? 3 * F : 1), s = (size_t)(S > 0 ? S : 1);
    w.sums = (long long*)take(n * 3 * 8);
    w.vnorm = (float*)take(n * 3 * 4);
    w.parent = (int32_t*)take(n * 4); w.size = (int32_t*)take(n * 4); w.minv = (int32_t*)take(n * 4);
    w.root = (int32_t*)take(n * 4); w.flag = (int32_t*)take(n * 4); w.excl = (int32_t*)take(n * 4);
    w.thr = (float*)take(n * 4);
    w.wbits = (uint32_t*)take(e * 4); w.vals_a = (uint32_t*)take(e * 4); w.vals_b = (uint32_t*)take(e * 4);
    w.keys_a = (uint64_t*)take(e * 8); w.keys_b = (uint64_t*)take(e * 8);
    w.bad = (int32_t*)take(s * 4); w.total = (int32_t*)take(4); w.cand_total = (int32_t*)take(4);
    w.stats = (long long*)take(s * 2 * 8);
    w.sort_bytes = sort_ws_bytes((int64_t)e); w.sort_ws = take(w.sort_bytes);
    w.scan_bytes = scan_ws_bytes((int64_t)(n > e ? n : e)); w.scan_ws = take(w.scan_bytes);
    w.total_bytes = o;
    return w;
}

// ---------------------------------------------------------------------------------------------- scenes, faces
// the scene of element i < off[S]: the last s with off[s] <= i (off ascends from 0; empty scenes repeat a value)
__device__ __forceinline__ int sp_scene_of(const int64_t* __restrict__ off, int S, int64_t i) {
    int lo = 0, hi = S - 1;                                                           // at most 17 rounds
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= i) lo = mid; else hi = mid - 1;
    }
    return lo;
}
__device__ __forceinline__ int64_t sp_clamp(int64_t x, int64_t lo, int64_t hi) { return x < lo ? lo : (x > hi ? hi : x); }

// the global vertex indices of face f -> whether all three lie in the face's scene (offsets that do not fit the arrays are clamped)
template <typename I>
__device__ __forceinline__ bool sp_face(const I* __restrict__ faces, int64_t f, int s, const int64_t* __restrict__ voff, int64_t N, int64_t v[3]) {
    const int64_t v0 = sp_clamp(voff[s], 0, N), v1 = sp_clamp(voff[s + 1], v0, N);
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int64_t i = (int64_t)faces[f * 3 + k];
        ok = ok && i >= 0 && i < v1 - v0;
        v[k] = v0 + i;
    }
    return ok;
}
__device__ __forceinline__ bool sp_normalise(float& x, float& y, float& z) {
    const float l = sqrtf((x * x + y * y) + z * z);            // correctly rounded (the header's __fsqrt_rn is the 1 ulp native one)
    const bool ok = l > 0.0f && l < __builtin_inff();                                 // NaN fails
    if (ok) { x = __fdiv_rn(x, l); y = __fdiv_rn(y, l); z = __fdiv_rn(z, l); }
    return ok;
}

__global__ __launch_bounds__(256) void sp_init_kernel(int64_t N, float k_thresh, int32_t* __restrict__ parent, int32_t* __restrict__ size,
                                                      float* __restrict__ thr, int32_t* __restrict__ minv) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= N) return;
    parent[v] = (int32_t)v;
    size[v] = 1;
    thr[v] = k_thresh;
    minv[v] = 0x7FFFFFFF;
}

template <typename I>
__global__ __launch_bounds__(256) void sp_face_kernel(const float* __restrict__ vert, const I* __restrict__ faces,
                                                      const int64_t* __restrict__ voff, const int64_t* __restrict__ foff, int S, int64_t N,
                                                      int64_t F, long long* __restrict__ sums, int32_t* __restrict__ bad) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    const int s = sp_scene_of(foff, S, f);
    int64_t v[3];
    if (!sp_face(faces, f, s, voff, N, v)) { atomicAdd(&bad[s], 1); return; }
    float p[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c) p[k][c] = vert[v[k] * 3 + c];
    const float ax = p[1][0] - p[0][0], ay = p[1][1] - p[0][1], az = p[1][2] - p[0][2];
    const float bx = p[2][0] - p[0][0], by = p[2][1] - p[0][1], bz = p[2][2] - p[0][2];
    float nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
    if (!sp_normalise(nx, ny, nz)) return;
    const long long q[3] = {(long long)rintf(nx * 16777216.0f), (long long)rintf(ny * 16777216.0f), (long long)rintf(nz * 16777216.0f)};
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c) atomicAdd((unsigned long long*)&sums[v[k] * 3 + c], (unsigned long long)q[c]);
}

__global__ __launch_bounds__(256) void sp_vnormal_kernel(const long long* __restrict__ sums, int64_t N, float* __restrict__ vnorm,
                                                         float* __restrict__ normals_out) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= N) return;
    float x = (float)(double)sums[v * 3], y = (float)(double)sums[v * 3 + 1], z = (float)(double)sums[v * 3 + 2];
    if (!sp_normalise(x, y, z)) x = y = z = 0.0f;
    vnorm[v * 3] = x; vnorm[v * 3 + 1] = y; vnorm[v * 3 + 2] = z;
    if (normals_out) { normals_out[v * 3] = x; normals_out[v * 3 + 1] = y; normals_out[v * 3 + 2] = z; }
}

// the ends of edge 3 f + k: (i, j), (i, k), (k, j)
__device__ __forceinline__ void sp_ends(const int64_t v[3], int k, int64_t& a, int64_t& b) {
    a = k == 2 ? v[2] : v[0];
    b = k == 1 ? v[2] : v[1];
}

template <typename I>
__global__ __launch_bounds__(256) void sp_edge_kernel(const float* __restrict__ vert, const I* __restrict__ faces,
                                                      const int64_t* __restrict__ voff, const int64_t* __restrict__ foff, int S, int64_t N,
                                                      int64_t F, const float* __restrict__ vnorm, uint32_t* __restrict__ wbits,
                                                      uint64_t* __restrict__ keys, uint32_t* __restrict__ weights_out) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= 3 * F) return;
    const int64_t f = g / 3;
    const int k = (int)(g - 3 * f);
    const int s = sp_scene_of(foff, S, f);
    int64_t v[3];
    uint32_t bits = 0u;                                                               // the edges of an ignored face: never looked at
    if (sp_face(faces, f, s, voff, N, v)) {
        int64_t a, b;
        sp_ends(v, k, a, b);
        const float max_ = vnorm[a * 3], may = vnorm[a * 3 + 1], maz = vnorm[a * 3 + 2];
        const float mbx = vnorm[b * 3], mby = vnorm[b * 3 + 1], mbz = vnorm[b * 3 + 2];
        const float dot = (max_ * mbx + may * mby) + maz * mbz;
        const float t = 1.0f - dot;
        float w = t > 0.0f ? t : 0.0f;
        const float dx = vert[b * 3] - vert[a * 3], dy = vert[b * 3 + 1] - vert[a * 3 + 1], dz = vert[b * 3 + 2] - vert[a * 3 + 2];
        const float sd = (mbx * dx + mby * dy) + mbz * dz;
        if (sd > 0.0f) w = w * w;                                                     // a NaN is not > 0
        bits = __float_as_uint(w);
    }
    wbits[g] = bits;
    keys[g] = ((uint64_t)(uint32_t)s << 32) | bits;
    if (weights_out) weights_out[g] = bits;
}

// ---------------------------------------------------------------------------------------------- the sweep
__device__ __forceinline__ int sp_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void sp_store(int32_t* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// the root of x; `hops` = links followed.  At most max_hops of them: a forest of n vertices has no longer path.
__device__ __forceinline__ int sp_find(const int32_t* parent, int x, int64_t max_hops, int& hops) {
    hops = 0;
    for (int64_t h = 0; h < max_hops; ++h) {
        const int p = sp_load(parent + x);
        if (p == x) break;
        x = p;
        ++hops;
    }
    return x;
}
// the slot of `key` in the table, inserted if absent (*fresh: this lane inserted it).  The table never fills: -1 only if it did.
__device__ __forceinline__ int sp_insert(int* t_key, int key, bool* fresh) {
    int h = (int)(hash_u64((uint64_t)(uint32_t)key) & (SP_TABLE - 1));
    *fresh = false;
    for (int probe = 0; probe < SP_TABLE; ++probe) {
        const int old = atomicCAS(&t_key[h], -1, key);
        if (old == -1) { *fresh = true; return h; }
        if (old == key) return h;
        h = (h + 1) & (SP_TABLE - 1);
    }
    return -1;
}
__device__ __forceinline__ int sp_find_slot(const unsigned short* t_par, int x) {
    for (int h = 0; h < SP_TABLE; ++h) {
        const int p = t_par[x];
        if (p == x) break;
        x = p;
    }
    return x;
}

// the lanes of one wave exchange values through LDS: its LDS operations complete in issue order, the compiler must not move them
__device__ __forceinline__ void sp_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

template <typename I>
__global__ __launch_bounds__(SP_BATCH) void sp_sweep_kernel(const I* __restrict__ faces, const int64_t* __restrict__ voff,
                                                            const int64_t* __restrict__ foff, int64_t N, int64_t F,
                                                            const uint32_t* __restrict__ order, const uint32_t* __restrict__ wbits,
                                                            float k_thresh, int min_verts, int pass, const int32_t* __restrict__ cand_excl,
                                                            const int32_t* __restrict__ cand_total, int32_t* parent, int32_t* size,
                                                            float* thr, long long* __restrict__ stats) {
    __shared__ int t_key[SP_TABLE];
    __shared__ int t_size[SP_TABLE];
    __shared__ float t_thr[SP_TABLE];
    __shared__ unsigned short t_par[SP_TABLE];
    __shared__ int t_claim[SP_TABLE];                                                 // the lowest pending lane at a slot, 64 = none
    __shared__ unsigned short s_a[SP_BATCH], s_b[SP_BATCH];
    __shared__ float s_w[SP_BATCH];
    __shared__ int s_cnt[SP_BATCH / 64];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int s = blockIdx.x;
    int64_t e0 = 3 * sp_clamp(foff[s], 0, F), e1 = 3 * sp_clamp(foff[s + 1], e0 / 3, F);
    if (pass == 1) {                                                                  // `order` holds the candidates only: the scene's share of them
        e0 = e0 < 3 * F ? cand_excl[e0] : *cand_total;
        e1 = e1 < 3 * F ? cand_excl[e1] : *cand_total;
    }
    const int64_t v0 = sp_clamp(voff[s], 0, N), n_s = sp_clamp(voff[s + 1], v0, N) - v0;
    {
        long long settled = 0;
        for (int64_t base = e0; base < e1; base += SP_BATCH) {
            for (int i = t; i < SP_TABLE; i += SP_BATCH) { t_key[i] = -1; t_claim[i] = 64; }
            const int64_t e = base + t;
            int a = -1, b = -1, ra = -1, rb = -1, ha = 0, hb = 0;
            float w = 0.0f;
            bool surv = false;
            if (e < e1) {
                const int64_t g = (int64_t)order[e];
                if (g < 3 * F) {
                    const int64_t f = g / 3;
                    int64_t v[3], va, vb;
                    if (sp_face(faces, f, s, voff, N, v)) {
                        sp_ends(v, (int)(g - 3 * f), va, vb);
                        a = (int)va; b = (int)vb;
                        w = __uint_as_float(wbits[g]);
                        ra = sp_find(parent, a, n_s, ha);
                        rb = sp_find(parent, b, n_s, hb);
                        surv = ra != rb;
                        if (surv && pass == 1) surv = size[ra] < min_verts || size[rb] < min_verts;    // sizes only grow
                    }
                }
            }
            const unsigned long long bal = __ballot(surv);
            if (lane == 0) s_cnt[wv] = __popcll(bal);
            __syncthreads();                                                          // every find is done, the table is clear
            if (ha > 1) sp_store(parent + a, ra);                                     // an end is re-pointed at its root, an ancestor
            if (hb > 1) sp_store(parent + b, rb);
            int pos = __popcll(bal & ((1ull << lane) - 1ull)), n_surv = 0;
#pragma unroll
            for (int i = 0; i < SP_BATCH / 64; ++i) { const int c = s_cnt[i]; if (i < wv) pos += c; n_surv += c; }
            if (surv) {
                bool fa, fb;
                const int sa = sp_insert(t_key, ra, &fa), sb = sp_insert(t_key, rb, &fb);
                if (fa && sa >= 0) { t_size[sa] = size[ra]; t_thr[sa] = thr[ra]; t_par[sa] = (unsigned short)sa; }
                if (fb && sb >= 0) { t_size[sb] = size[rb]; t_thr[sb] = thr[rb]; t_par[sb] = (unsigned short)sb; }
                s_a[pos] = (unsigned short)(sa >= 0 ? sa : 0);
                s_b[pos] = (unsigned short)(sa >= 0 && sb >= 0 ? sb : (sa >= 0 ? sa : 0));     // a full table (never): the edge joins nothing
                s_w[pos] = w;
            }
            __syncthreads();
            if (t == 0) settled += n_surv;
            if (wv == 0) {
                // Wave 0 settles the survivors in order, 64 at a time, one lane per edge.  A lane whose edge is the lowest pending one
                // at both of its components (an LDS atomicMin of the lane number per component) decides now: no earlier pending edge
                // can reach either component before its turn - the first to do so would have to touch it as it stands, and would hold
                // the claim - so their state is what the sequential walk would show it, and two lanes deciding together touch
                // disjoint components.  The lowest pending lane always decides: at most 64 rounds.
                for (int g0 = 0; g0 < n_surv; g0 += 64) {
                    const int i = g0 + lane;
                    bool pending = i < n_surv;
                    int x = pending ? s_a[i] : 0, y = pending ? s_b[i] : 0;
                    const float we = pending ? s_w[i] : 0.0f;
                    for (int round = 0; round < 64; ++round) {
                        if (pending) {
                            x = sp_find_slot(t_par, x);
                            y = sp_find_slot(t_par, y);
                            pending = x != y;                                         // joined meanwhile: nothing to decide
                        }
                        if (__ballot(pending) == 0ull) break;
                        if (pending) { atomicMin(&t_claim[x], lane); atomicMin(&t_claim[y], lane); }
                        sp_wave_sync();
                        const bool mine = pending && t_claim[x] == lane && t_claim[y] == lane;
                        sp_wave_sync();
                        if (pending) { t_claim[x] = 64; t_claim[y] = 64; }
                        if (mine) {
                            const int sx = t_size[x], sy = t_size[y];
                            const bool join = pass == 0 ? (we <= t_thr[x] && we <= t_thr[y]) : (sx < min_verts || sy < min_verts);
                            if (join) {
                                if (sx < sy || (sx == sy && t_key[y] < t_key[x])) { const int z = x; x = y; y = z; }      // x stays the root
                                const int sz = sx + sy;
                                t_par[y] = (unsigned short)x;
                                t_size[x] = sz;
                                t_thr[x] = we + __fdiv_rn(k_thresh, (float)sz);
                            }
                            pending = false;                                          // joined or refused: never looked at again
                        }
                        sp_wave_sync();
                    }
                }
            }
            __syncthreads();
            for (int i = t; i < SP_TABLE; i += SP_BATCH) {
                const int key = t_key[i];
                if (key < 0) continue;
                const int r = sp_find_slot(t_par, i);
                if (r != i) sp_store(parent + key, t_key[r]);                         // a root goes under a root
                else { size[key] = t_size[i]; thr[key] = t_thr[i]; }
            }
            __syncthreads();
        }
        if (t == 0 && stats) stats[2 * s + pass] = settled;
    }
}

// ---------------------------------------------------------------------------------------------- the candidates of pass 2
template <typename I>
__global__ __launch_bounds__(256) void sp_cand_kernel(const I* __restrict__ faces, const int64_t* __restrict__ voff,
                                                      const int64_t* __restrict__ foff, int S, int64_t N, int64_t F,
                                                      const uint32_t* __restrict__ order, const int32_t* __restrict__ parent,
                                                      const int32_t* __restrict__ size, int min_verts, int32_t* __restrict__ flag) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= 3 * F) return;
    const int64_t g = (int64_t)order[e];
    int keep = 0;
    if (g < 3 * F) {
        const int64_t f = g / 3;
        int64_t v[3], va, vb;
        if (sp_face(faces, f, sp_scene_of(foff, S, f), voff, N, v)) {
            sp_ends(v, (int)(g - 3 * f), va, vb);
            int ra = (int)va, rb = (int)vb;
            for (int64_t h = 0; h < N; ++h) { const int p = parent[ra]; if (p == ra) break; ra = p; }
            for (int64_t h = 0; h < N; ++h) { const int p = parent[rb]; if (p == rb) break; rb = p; }
            keep = ra != rb && (size[ra] < min_verts || size[rb] < min_verts);
        }
    }
    flag[e] = keep;
}
__global__ __launch_bounds__(256) void sp_compact_kernel(const uint32_t* __restrict__ order, const int32_t* __restrict__ flag,
                                                         const int32_t* __restrict__ excl, int64_t E, uint32_t* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < E && flag[e]) out[excl[e]] = order[e];                                    // excl[e] < the number of flags <= E
}

// ---------------------------------------------------------------------------------------------- labels
__global__ __launch_bounds__(256) void sp_min_kernel(const int32_t* __restrict__ parent, int64_t N, int32_t* __restrict__ root,
                                                     int32_t* __restrict__ minv) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= N) return;
    int x = (int)v;
    for (int64_t h = 0; h < N; ++h) {
        const int p = parent[x];
        if (p == x) break;
        x = p;
    }
    root[v] = x;
    if (__hip_atomic_load(&minv[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > (int)v) atomicMin(&minv[x], (int)v);   // it only ever falls
}
__global__ __launch_bounds__(256) void sp_flag_kernel(const int32_t* __restrict__ root, const int32_t* __restrict__ minv, int64_t N,
                                                      int32_t* __restrict__ flag) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v < N) flag[v] = minv[root[v]] == (int)v;
}
__global__ __launch_bounds__(256) void sp_label_kernel(const int32_t* __restrict__ root, const int32_t* __restrict__ minv,
                                                       const int32_t* __restrict__ excl, const int64_t* __restrict__ voff, int S, int64_t N,
                                                       int64_t* __restrict__ labels) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= N) return;
    const int s = sp_scene_of(voff, S, v);
    const int64_t v0 = sp_clamp(voff[s], 0, N - 1);
    labels[v] = (int64_t)excl[minv[root[v]]] - (int64_t)excl[v0];
}
__global__ __launch_bounds__(256) void sp_info_kernel(const int32_t* __restrict__ excl, const int32_t* __restrict__ total,
                                                      const int32_t* __restrict__ bad, const int64_t* __restrict__ voff, int S, int64_t N,
                                                      const long long* __restrict__ stats, int32_t* __restrict__ info,
                                                      long long* __restrict__ stats_out) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= S) return;
    const int64_t v0 = sp_clamp(voff[s], 0, N), v1 = sp_clamp(voff[s + 1], v0, N);
    const int c0 = v0 < N ? excl[v0] : *total, c1 = v1 < N ? excl[v1] : *total;
    info[2 * s] = N > 0 ? c1 - c0 : 0;
    info[2 * s + 1] = bad[s];
    if (stats_out) { stats_out[2 * s] = stats[2 * s]; stats_out[2 * s + 1] = stats[2 * s + 1]; }
}

// ---------------------------------------------------------------------------------------------- C entry points
static bool sp_sizes_ok(int64_t N, int64_t F, int S) {
    return N >= 0 && N <= SP_MAX_VERTICES && F >= 0 && 3 * F <= 0x7FFFFFFFll && S >= 1 && S <= SP_MAX_SCENES;
}

extern "C" size_t sd3d_superpoints_ws_bytes(int64_t n_vertices, int64_t n_faces, int n_scenes) {
    if (!sp_sizes_ok(n_vertices, n_faces, n_scenes)) return 0;
    return sp_ws(nullptr, n_vertices, n_faces, n_scenes).total_bytes;
}

extern "C" int sd3d_mesh_superpoints(const float* vertices, const void* faces, int faces_i64, const int64_t* vertex_offsets,
                                     const int64_t* face_offsets, int64_t n_vertices, int64_t n_faces, int n_scenes, float k_thresh,
                                     int min_verts, int64_t* labels, int32_t* info, float* normals_out, void* weights_out,
                                     int64_t* sweep_stats_out, void* ws, size_t ws_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const int64_t N = n_vertices, F = n_faces;
    const int S = n_scenes;
    if (!sp_sizes_ok(N, F, S))
        return sd3d_set_error(SD3D_ERR_ARG, "mesh_superpoints: 0 <= n_vertices < 2^31, 0 <= 3 n_faces < 2^31, 1 <= n_scenes <= 65536");
    if (!(k_thresh >= 0.0f && k_thresh < __builtin_inff()) || min_verts < 1)
        return sd3d_set_error(SD3D_ERR_ARG, "mesh_superpoints: k_thresh must be finite and >= 0, min_verts >= 1");
    if (!vertex_offsets || !face_offsets || !info || (N > 0 && (!vertices || !labels)) || (F > 0 && !faces))
        return sd3d_set_error(SD3D_ERR_ARG, "mesh_superpoints: NULL argument");
    if (!ws || ((uintptr_t)ws & 255) != 0) return sd3d_set_error(SD3D_ERR_ARG, "mesh_superpoints: ws must be given and 256-byte aligned");
    const SpWs w = sp_ws(ws, N, F, S);
    if (ws_bytes < w.total_bytes) return sd3d_set_error(SD3D_ERR_WS, "mesh_superpoints: workspace too small");
    const dim3 b256(256), gv((unsigned)cdiv(N > 0 ? N : 1, 256)), gf((unsigned)cdiv(F > 0 ? F : 1, 256)), ge((unsigned)cdiv(F > 0 ? 3 * F : 1, 256));
    if (hipMemsetAsync(w.bad, 0, (size_t)S * 4, st) != hipSuccess || hipMemsetAsync(w.stats, 0, (size_t)S * 16, st) != hipSuccess ||
        hipMemsetAsync(w.total, 0, 4, st) != hipSuccess || (N > 0 && hipMemsetAsync(w.sums, 0, (size_t)N * 24, st) != hipSuccess))
        return sd3d_set_error(SD3D_ERR_LAUNCH, "mesh_superpoints: memset");
    if (N > 0) hipLaunchKernelGGL(sp_init_kernel, gv, b256, 0, st, N, k_thresh, w.parent, w.size, w.thr, w.minv);
    if (F > 0) {
        if (faces_i64)
            hipLaunchKernelGGL(sp_face_kernel<int64_t>, gf, b256, 0, st, vertices, (const int64_t*)faces, vertex_offsets, face_offsets, S, N, F, w.sums, w.bad);
        else
            hipLaunchKernelGGL(sp_face_kernel<int32_t>, gf, b256, 0, st, vertices, (const int32_t*)faces, vertex_offsets, face_offsets, S, N, F, w.sums, w.bad);
    }
    if (N > 0) hipLaunchKernelGGL(sp_vnormal_kernel, gv, b256, 0, st, w.sums, N, w.vnorm, normals_out);
    if (F > 0 && N > 0) {
        const int64_t E = 3 * F;
        if (faces_i64)
            hipLaunchKernelGGL(sp_edge_kernel<int64_t>, ge, b256, 0, st, vertices, (const int64_t*)faces, vertex_offsets, face_offsets, S, N, F, w.vnorm,
                               w.wbits, w.keys_a, (uint32_t*)weights_out);
        else
            hipLaunchKernelGGL(sp_edge_kernel<int32_t>, ge, b256, 0, st, vertices, (const int32_t*)faces, vertex_offsets, face_offsets, S, N, F, w.vnorm,
                               w.wbits, w.keys_a, (uint32_t*)weights_out);
        int scene_bits = 0;
        while ((1 << scene_bits) < S) ++scene_bits;
        int landed = 0;
        if (int rc = sort_pairs_u64(w.keys_a, nullptr, w.keys_b, w.vals_b, E, 0, 32 + scene_bits, w.sort_ws, w.sort_bytes, st, w.vals_a, &landed))
            return rc;
        const uint32_t* order = landed ? w.vals_a : w.vals_b;
        uint32_t* order2 = landed ? w.vals_b : w.vals_a;                              // the candidates of pass 2
        int32_t *cflag = (int32_t*)w.keys_a, *cexcl = (int32_t*)w.keys_b;             // the sorted keys are done with
        const dim3 gs((unsigned)S), bs(SP_BATCH);
#define SP_SWEEP(T, pass, ord) \
    hipLaunchKernelGGL(sp_sweep_kernel<T>, gs, bs, 0, st, (const T*)faces, vertex_offsets, face_offsets, N, F, ord, w.wbits, k_thresh, min_verts, \
                       pass, cexcl, w.cand_total, w.parent, w.size, w.thr, w.stats)
        if (faces_i64) SP_SWEEP(int64_t, 0, order); else SP_SWEEP(int32_t, 0, order);
        if (min_verts > 1) {                                                          // (no component is below one vertex)
            if (faces_i64)
                hipLaunchKernelGGL(sp_cand_kernel<int64_t>, ge, b256, 0, st, (const int64_t*)faces, vertex_offsets, face_offsets, S, N, F, order,
                                   w.parent, w.size, min_verts, cflag);
            else
                hipLaunchKernelGGL(sp_cand_kernel<int32_t>, ge, b256, 0, st, (const int32_t*)faces, vertex_offsets, face_offsets, S, N, F, order,
                                   w.parent, w.size, min_verts, cflag);
            if (int rc = scan_exclusive_i32(cflag, cexcl, E, nullptr, w.cand_total, w.scan_ws, w.scan_bytes, st)) return rc;
            hipLaunchKernelGGL(sp_compact_kernel, ge, b256, 0, st, order, cflag, cexcl, E, order2);
            if (faces_i64) SP_SWEEP(int64_t, 1, order2); else SP_SWEEP(int32_t, 1, order2);
        }
#undef SP_SWEEP
    } else if (F > 0 && weights_out) {
        if (hipMemsetAsync(weights_out, 0, (size_t)F * 12, st) != hipSuccess) return sd3d_set_error(SD3D_ERR_LAUNCH, "mesh_superpoints: memset");
    }
    if (N > 0) {
        hipLaunchKernelGGL(sp_min_kernel, gv, b256, 0, st, w.parent, N, w.root, w.minv);
        hipLaunchKernelGGL(sp_flag_kernel, gv, b256, 0, st, w.root, w.minv, N, w.flag);
        if (int rc = scan_exclusive_i32(w.flag, w.excl, N, nullptr, w.total, w.scan_ws, w.scan_bytes, st)) return rc;
        hipLaunchKernelGGL(sp_label_kernel, gv, b256, 0, st, w.root, w.minv, w.excl, vertex_offsets, S, N, labels);
    }
    hipLaunchKernelGGL(sp_info_kernel, dim3((unsigned)cdiv(S, 256)), b256, 0, st, w.excl, w.total, w.bad, vertex_offsets, S, N, w.stats, info,
                       (long long*)sweep_stats_out);
    SD3D_CHECK_LAUNCH();
    return SD3D_OK;
}
