// Internal interface of the pair-major sparse convolution: what the rulebook lists (pair_lists.hip) and pass 1 / pass 2 (pair_gemm.hip) share.
// Every translation unit that calls one of these launchers includes this header instead of declaring them itself.
#pragma once
#include "common.h"
#include "../../include/segdino3d_hip.h"

#define PT 128                  // pairs per tile / segment padding
#define PG_CHAIN 0x40000000     // tile_k flag of chained lists: this tile's products add onto the next tile's (pair_lists.hip)
#define PG_KMASK 0x3FFFFFFF

struct GGParams;

// pass 1 + pass 2 (pair_gemm.hip)
int launch_pair_conv(const float* in0, int ld0, int C0, const float* in1, int ld1, const int32_t* in_idx, const int32_t* tile_k,
                     int64_t p_cap, const int32_t* pos, const int32_t* rlist, int rl_stride, int center, const int32_t* out_idx,
                     const float* wt, int K, int Cin, int Cout, int64_t M, const float* scale,
                     const float* shift, const float* res, int ld_res, float* out, int ld_out, int act, float* part,
                     size_t part_bytes, hipStream_t st);
int launch_pair_dense(const GGParams& q, hipStream_t st);
