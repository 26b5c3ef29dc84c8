// Linear sum assignment on the device: the HungarianMatcher of the training criterion (loss_3d.py:274-312, which calls
// scipy.optimize.linear_sum_assignment on the host).  Rectangular minimum-cost assignment by shortest augmenting paths, the
// Jonker-Volgenant form of Crouse (2016) that scipy implements: the result is THE optimum, not an approximation.
//
// One problem = one [Q, G] fp32 cost matrix (row-major, as sd3d_match_costs writes it).  The smaller side holds the n = min(Q, G)
// "agents", each assigned exactly once; the larger side holds the m = max(Q, G) columns that every search step scans in parallel.
// One workgroup solves one problem: no workgroup waits for another, nothing spins on global memory, there are no atomics; a
// batch of problems is one launch with grid = number of problems.
//
//   pre-pass  (hm_stage_kernel, one 32x32 tile per workgroup): zeroes match, flags NaN / -inf entries in the problem's status
//             word and, when G < Q (the agents are the COLUMNS of the caller's matrix), writes the agent-major copy ct[G][Q]
//             into the workspace, so that every search step reads one contiguous row of m values.
//   solver    (hm_solve_kernel): per-column state - tentative distance, column dual, predecessor, visited flag, owning agent -
//             and the agents' duals live in LDS while m <= HM_LDS_MAX_M, in the workspace beyond.  All arithmetic is fp64
//             in scipy's order of operations: fp32 costs convert exactly, and the outcome is integer decisions.
//
// One search step: every thread relaxes its unvisited columns against the current agent's row, then a block-wide arg-min
// (wave shuffles, then LDS across waves) picks the column, lexicographic on (distance, column index): deterministic and
// independent of the thread count.  A column belongs to one thread (j mod HM_THREADS) for the whole solve, so the step needs
// ONE barrier (the cross-wave slots alternate between two sets).
//
// Termination is structural: every step marks one more column visited and at most (agents assigned so far) visited columns are
// owned, so an augmentation ends within m steps and a problem within n * m, whatever the values; the loops are bounded by
// counters as well.  NaN never enters a distance (r < d is false for NaN: NaN compares as +inf).  When the smallest distance is
// +inf the lowest-index unvisited column is taken, hung below the current agent, and the status word is set (scipy raises
// "infeasible" there), so the result is still a one-to-one match.  NaN or -inf anywhere in the matrix sets the status word too
// (scipy raises ValueError); +inf entries and the 1e8 of masked costs are ordinary values.
//
// Ties: where the optimum is not unique, this returns AN optimal assignment (lowest column index among equal distances), which
// need not be the one scipy returns (scipy prefers unassigned columns among equal distances).  Where the optimum is unique the
// two agree.
#include "common.h"
#include "../../include/segdino3d_hip.h"
#include <math.h>

#define HM_THREADS 512
#define HM_WAVES (HM_THREADS / 64)
#define HM_LDS_MAX_M 4096            // columns whose solver state fits LDS (37 B per column at n = m: 148 KB)
#define HM_TILE 32

struct HmProblem {
    const float* cost;               // [Q, G] the caller's matrix
    const float* rows;               // agent-major [n, m]: cost itself when Q <= G, else the staged transpose
    float* ct;                       // where the pre-pass writes the transpose (null when Q <= G)
    uint8_t* match;                  // [Q, G]
    char* state;                     // solver state in the workspace (null: LDS)
    int32_t* status_ws;              // this problem's word in the workspace (zeroed before the pre-pass)
    int32_t* status;                 // the caller's word or null
    int Q, G;
};
struct HmBatch { int n; int tiles_g[SD3D_MAX_BATCH]; HmProblem p[SD3D_MAX_BATCH]; };

// bytes of solver state for n agents and m columns: dist[m], v[m], u[n] doubles; pred[m], owner[m], col_of[n] ints; visited[m]
__host__ __device__ static inline size_t hm_state_bytes(int n, int m) {
    return ((size_t)8 * (2 * (size_t)m + n) + (size_t)4 * (2 * (size_t)m + n) + (size_t)m + 15) / 16 * 16;
}

// ------------------------------------------------------------------ pre-pass
__global__ __launch_bounds__(256) void hm_stage_kernel(const HmBatch b) {
    __shared__ float tile[HM_TILE][HM_TILE + 1];
    const HmProblem& p = b.p[blockIdx.y];
    const int tg = b.tiles_g[blockIdx.y];
    if (p.Q <= 0 || p.G <= 0) return;
    const int64_t tiles = (int64_t)tg * ((p.Q + HM_TILE - 1) / HM_TILE);
    if ((int64_t)blockIdx.x >= tiles) return;
    const int q0 = (int)(blockIdx.x / tg) * HM_TILE, g0 = (int)(blockIdx.x % tg) * HM_TILE;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    bool bad = false;
    for (int r = ty; r < HM_TILE; r += 8) {
        const int q = q0 + r, g = g0 + tx;
        if (q < p.Q && g < p.G) {
            const float c = p.cost[(int64_t)q * p.G + g];
            bad |= (c != c) || c == -INFINITY;
            tile[r][tx] = c;
            p.match[(int64_t)q * p.G + g] = 0;
        }
    }
    if (bad) *p.status_ws = 1;                                 // every writer stores the same value
    if (!p.ct) return;                                         // (uniform per workgroup)
    __syncthreads();
    for (int r = ty; r < HM_TILE; r += 8) {
        const int g = g0 + r, q = q0 + tx;
        if (q < p.Q && g < p.G) p.ct[(int64_t)g * p.Q + q] = tile[tx][r];
    }
}

// ------------------------------------------------------------------ solver
// (value, index) minimum, lexicographic; the `(value, index)` pattern of loss_sparse_match_kernel in fp64
__device__ __forceinline__ void hm_min(double& bv, int& bi, double ov, int oi) {
    if (ov < bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
}

template <bool kLds>
__global__ __launch_bounds__(HM_THREADS) void hm_solve_kernel(const HmBatch b) {
    extern __shared__ __attribute__((aligned(16))) char hm_smem[];
    __shared__ double red_v[2][HM_WAVES];
    __shared__ int red_i[2][HM_WAVES];
    const HmProblem& p = b.p[blockIdx.x];
    const int Q = p.Q, G = p.G;
    if (Q <= 0 || G <= 0) return;
    const bool agents_are_cols = G < Q;
    const int n = agents_are_cols ? G : Q, m = agents_are_cols ? Q : G;
    if (kLds != (p.state == nullptr)) return;                  // the other instantiation's launch solves this problem
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;

    char* s = kLds ? hm_smem : p.state;
    double* dist = (double*)s;             s += (size_t)8 * m;
    double* v = (double*)s;                s += (size_t)8 * m;
    double* u = (double*)s;                s += (size_t)8 * n;
    int* pred = (int*)s;                   s += (size_t)4 * m;
    int* owner = (int*)s;                  s += (size_t)4 * m;
    int* col_of = (int*)s;                 s += (size_t)4 * n;
    uint8_t* visited = (uint8_t*)s;

    for (int j = tid; j < m; j += HM_THREADS) { v[j] = 0.0; owner[j] = -1; pred[j] = -1; }
    for (int a = tid; a < n; a += HM_THREADS) { u[a] = 0.0; col_of[a] = -1; }
    bool infeasible = false;
    int slot = 0;

    for (int cur = 0; cur < n; ++cur) {
        for (int j = tid; j < m; j += HM_THREADS) { dist[j] = INFINITY; visited[j] = 0; }
        __syncthreads();                                       // duals, owners of the previous augmentation; the initial state
        int i = cur, sink = -1;
        double min_val = 0.0;
        for (int step = 0; step < m && sink < 0; ++step) {
            const float* row = p.rows + (int64_t)i * m;
            const double ui = u[i];
            double bv = INFINITY; int bi = 0x7fffffff;
            for (int j = tid; j < m; j += HM_THREADS) {
                const double c = (double)row[j];
                if (!visited[j]) {
                    const double r = min_val + c - ui - v[j];  // scipy's order of operations
                    double d = dist[j];
                    if (r < d) { d = r; dist[j] = r; pred[j] = i; }
                    if (d < bv || bi == 0x7fffffff) { bv = d; bi = j; }   // j ascends: the first of equal distances stays, +inf included
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const double ov = __shfl_xor(bv, o, 64); const int oi = __shfl_xor(bi, o, 64);
                hm_min(bv, bi, ov, oi);
            }
            if (lane == 0) { red_v[slot][wv] = bv; red_i[slot][wv] = bi; }
            __syncthreads();
            bv = red_v[slot][0]; bi = red_i[slot][0];
#pragma unroll
            for (int w = 1; w < HM_WAVES; ++w) hm_min(bv, bi, red_v[slot][w], red_i[slot][w]);
            slot ^= 1;
            if (bi < 0 || bi >= m) break;                      // cannot happen while step < m: an unvisited column exists
            const int j = bi;
            if (bv == INFINITY) infeasible = true;
            if ((j % HM_THREADS) == tid) {                     // the column's own thread: nobody else reads these before a barrier
                visited[j] = 1;
                if (bv == INFINITY) pred[j] = i;               // never reached: hang it below the current agent
            }
            min_val = bv;
            const int o = owner[j];
            if (o < 0) sink = j; else i = o;
        }
        if (sink < 0) { infeasible = true; continue; }         // only after the defensive break above; uniform
        // duals (scipy: u[cur] += minVal; u[i] += minVal - dist[col4row[i]] for visited rows; v[j] -= minVal - dist[j])
        if (tid == 0) u[cur] += min_val;
        for (int j = tid; j < m; j += HM_THREADS) {
            if (visited[j]) {
                const double delta = min_val - dist[j];
                const int o = owner[j];
                if (o >= 0) u[o] += delta;                     // an agent owns one column: no two threads write one u
                v[j] -= delta;
            }
        }
        __syncthreads();                                       // predecessors and owners before the path is flipped
        if (tid == 0) {
            int j = sink;
            for (int hop = 0; hop <= n; ++hop) {
                const int a = pred[j];
                if (a < 0 || a >= n) break;                    // (defensive; a visited column always has a predecessor)
                owner[j] = a;
                const int prev = col_of[a]; col_of[a] = j; j = prev;
                if (a == cur || j < 0) break;
            }
        }
    }
    __syncthreads();
    for (int a = tid; a < n; a += HM_THREADS) {
        const int j = col_of[a];
        if (j >= 0 && j < m && owner[j] == a) {
            if (agents_are_cols) p.match[(int64_t)j * G + a] = 1; else p.match[(int64_t)a * G + j] = 1;
        }
    }
    if (tid == 0) {
        const int st = (infeasible || *p.status_ws) ? 1 : 0;
        *p.status_ws = st;
        if (p.status) *p.status = st;
    }
}

// ------------------------------------------------------------------ C ABI
static inline size_t hm_problem_ws(int Q, int G) {
    if (Q <= 0 || G <= 0) return 0;
    const int n = Q < G ? Q : G, m = Q < G ? G : Q;
    size_t b = 0;
    if (G < Q) b += align_up((size_t)Q * G * sizeof(float), 256);
    if (m > HM_LDS_MAX_M) b += align_up(hm_state_bytes(n, m), 256);
    return b;
}

extern "C" size_t sd3d_hungarian_match_ws_bytes(int n, const int* Q, const int* G) {
    if (n <= 0 || !Q || !G) return 0;
    size_t b = align_up((size_t)n * sizeof(int32_t), 256);
    for (int i = 0; i < n; ++i) b += hm_problem_ws(Q[i], G[i]);
    return b;
}

extern "C" int sd3d_hungarian_match_batch(int n, const float* const* cost, const int* Q, const int* G, uint8_t* const* match,
                                          int32_t* status, void* ws, size_t ws_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (n <= 0) return SD3D_OK;
    if (!cost || !Q || !G || !match) return sd3d_set_error(SD3D_ERR_ARG, "hungarian_match: null argument array");
    for (int i = 0; i < n; ++i) {
        if (Q[i] < 0 || G[i] < 0) return sd3d_set_error(SD3D_ERR_ARG, "hungarian_match: negative shape");
        if (Q[i] > 0 && G[i] > 0 && (!cost[i] || !match[i])) return sd3d_set_error(SD3D_ERR_ARG, "hungarian_match: null cost / match matrix");
    }
    if (!ws || ws_bytes < sd3d_hungarian_match_ws_bytes(n, Q, G)) return sd3d_set_error(SD3D_ERR_WS, "hungarian_match: workspace too small");
    static Sd3dLdsRaised raised;
    const size_t lds_max = hm_state_bytes(HM_LDS_MAX_M, HM_LDS_MAX_M);
    if (int rc = sd3d_raise_lds_limit(raised, {{(const void*)hm_solve_kernel<true>, (int)lds_max}})) return rc;
    int32_t* status_ws = (int32_t*)ws;
    char* w = (char*)ws + align_up((size_t)n * sizeof(int32_t), 256);
    if (hipMemsetAsync(status_ws, 0, (size_t)n * sizeof(int32_t), st) != hipSuccess) return sd3d_set_error(SD3D_ERR_LAUNCH, "hungarian_match: memset failed");
    for (int i0 = 0; i0 < n; i0 += SD3D_MAX_BATCH) {           // one launch (of each kind) per 16 problems
        HmBatch b;
        b.n = n - i0 < SD3D_MAX_BATCH ? n - i0 : SD3D_MAX_BATCH;
        int64_t max_tiles = 0;
        size_t lds = 0;
        bool any_lds = false, any_ws = false;
        for (int k = 0; k < b.n; ++k) {
            const int i = i0 + k, q = Q[i], g = G[i];
            HmProblem& p = b.p[k];
            p.cost = cost[i]; p.match = match[i]; p.Q = q; p.G = g;
            p.rows = cost[i]; p.ct = nullptr; p.state = nullptr;
            p.status_ws = status_ws + i; p.status = status ? status + i : nullptr;
            b.tiles_g[k] = (int)cdiv(g, HM_TILE);
            if (q <= 0 || g <= 0) { b.tiles_g[k] = 1; continue; }
            const int na = q < g ? q : g, m = q < g ? g : q;
            if (g < q) { p.ct = (float*)w; p.rows = p.ct; w += align_up((size_t)q * g * sizeof(float), 256); }
            if (m > HM_LDS_MAX_M) { p.state = w; w += align_up(hm_state_bytes(na, m), 256); any_ws = true; }
            else { any_lds = true; const size_t need = hm_state_bytes(na, m); lds = need > lds ? need : lds; }
            const int64_t tiles = cdiv(q, HM_TILE) * cdiv(g, HM_TILE);
            max_tiles = tiles > max_tiles ? tiles : max_tiles;
        }
        if (max_tiles == 0) continue;                          // empty problems only: their status words are zero already
        if (max_tiles > 0x7fffffff) return sd3d_set_error(SD3D_ERR_ARG, "hungarian_match: matrix too large");
        hipLaunchKernelGGL(hm_stage_kernel, dim3((unsigned)max_tiles, (unsigned)b.n), dim3(256), 0, st, b);
        if (any_lds) hipLaunchKernelGGL(hm_solve_kernel<true>, dim3((unsigned)b.n), dim3(HM_THREADS), lds, st, b);
        if (any_ws) hipLaunchKernelGGL(hm_solve_kernel<false>, dim3((unsigned)b.n), dim3(HM_THREADS), 0, st, b);
        SD3D_CHECK_LAUNCH();
    }
    if (status) {                                              // empty problems are never visited by a workgroup
        for (int i = 0; i < n; ++i)
            if (Q[i] <= 0 || G[i] <= 0)
                if (hipMemsetAsync(status + i, 0, sizeof(int32_t), st) != hipSuccess) return sd3d_set_error(SD3D_ERR_LAUNCH, "hungarian_match: memset failed");
    }
    return SD3D_OK;
}
