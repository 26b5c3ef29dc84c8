// Shared declarations of the gather-GEMM translation units.
#pragma once
#include "common.h"

struct GGParams {
    const float* in0; int ld0; int C0;        // input features, first C0 channels
    const float* in1; int ld1;                // optional second source for channels C0..Cin-1 (skip concat)
    const int32_t* nbr;                       // [K][M] gather indices (-1 = no neighbour) or NULL (identity, K == 1)
    const float* wt;                          // [K][Cout][Cin]
    int K, Cin, Cout;
    int64_t M;                                // output rows
    const float* scale; const float* shift;   // per-column, optional
    const float* res; int ld_res;             // optional residual
    float* out; int ld_out;
    int act;                                  // 0 none, 1 relu, 2 gelu(erf), 3 sigmoid
    int col_groups;                           // ceil(Cout / (32*NT))
    int ksplit;                               // lock-step kernel only: gridDim.z offset slices (partials -> ws)
    float* ws;                                // [ksplit][M][Cout] partial sums when ksplit > 1
};

// The fields a caller sets; col_groups, ksplit and ws are the launcher's to choose.
static inline GGParams gg_params(const float* in0, int ld0, int C0, const float* in1, int ld1, const int32_t* nbr, const float* wt, int K,
                                 int Cin, int Cout, int64_t M, const float* scale, const float* shift, const float* res, int ld_res,
                                 float* out, int ld_out, int act) {
    GGParams p;
    p.in0 = in0; p.ld0 = ld0; p.C0 = C0; p.in1 = in1; p.ld1 = ld1; p.nbr = nbr; p.wt = wt; p.K = K; p.Cin = Cin; p.Cout = Cout;
    p.M = M; p.scale = scale; p.shift = shift; p.res = res; p.ld_res = ld_res; p.out = out; p.ld_out = ld_out; p.act = act;
    p.col_groups = 1;
    p.ksplit = 1;
    p.ws = nullptr;
    return p;
}

// gather_gemm.hip; called from gather_gemm_split.hip and executor.hip as well
int launch_gather_gemm(const GGParams& p_in, int nt, void* ws, size_t ws_bytes, hipStream_t st);
void launch_splitk_epilogue(const GGParams& p, hipStream_t st);

// The tail of every gather-GEMM epilogue: out[rr][n] = act(acc * scale[n] + shift[n] + res[rr][n]).
// (sc, sh: column n's scale and shift, which a caller that finishes several rows of the column loads once)
__device__ __forceinline__ float gg_scale(const GGParams& p, int n) { return p.scale ? p.scale[n] : 1.f; }
__device__ __forceinline__ float gg_shift(const GGParams& p, int n) { return p.shift ? p.shift[n] : 0.f; }
__device__ __forceinline__ void gg_finish(const GGParams& p, float acc, int64_t rr, int n, float sc, float sh) {
    float y = acc * sc + sh;
    if (p.res) y += p.res[rr * p.ld_res + n];
    p.out[rr * p.ld_out + n] = sd3d_act(y, p.act);
}
__device__ __forceinline__ void gg_finish(const GGParams& p, float acc, int64_t rr, int n) { gg_finish(p, acc, rr, n, gg_scale(p, n), gg_shift(p, n)); }

__device__ __forceinline__ int next_active(uint64_t m0, uint64_t m1, int after) {
    // smallest set bit index > after in the 128-bit mask (m1:m0), or -1
    int s = after + 1;
    if (s < 64) {
        const uint64_t r = m0 >> s;
        if (r) return s + __builtin_ctzll(r);
        s = 64;
    }
    if (s < 128) {
        const uint64_t r = m1 >> (s - 64);
        if (r) return s + __builtin_ctzll(r);
    }
    return -1;
}

