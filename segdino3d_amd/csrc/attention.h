// What the fused attention's forward (attention.hip) and backward (attention_bwd.hip) share: the constants of their common
// register layout and softmax, and the keep mask of attention dropout.
#pragma once
#include <stdint.h>

// Softmax in the log2 domain: a probability is one v_exp_f32 of (score - max or lse) * log2(e).  (The row chain's attention op
// pre-scales its queries by the same constant.)
#define SD3D_LOG2E 1.4426950408889634f
// Index of 32-channel block w in a register array with one entry per block (W blocks per head).  With one block it is the constant 0
// already when the template is instantiated, so the array is promoted to registers before the w loops unroll, as a single tile written
// without a loop would be: the W = 1 kernels are then the instruction streams of a 32-channel-only body (profiles/attention_heads.md).
#define ATTN_BLK(w) (W == 1 ? 0 : (w))

// Keep mask of attention dropout (nn.MultiheadAttention(dropout=p): dropout on the softmax probabilities, attention.py:383):
// ONE definition for the fused forward, the two backward kernels and the mask kernel.
//
// Element (head, q, k) of attention number `call` is a pure function of (key, call, head, q, k): Philox4x32-10 (the counter-based
// generator of Random123, torch and rocRAND) with the two key words read from device memory and the counter (k >> 2, q, head, call);
// the element takes output word k & 3 and is KEPT iff that word >= thr, thr = floor(p 2^32).  Nothing about the asking kernel enters -
// waves per workgroup, key split, tile order and head width cannot change a bit, and the backward regenerates what the forward drew.
// Four consecutive keys share one call; in the forward and the q kernel a lane holds four such runs per key tile.

struct AttnDrop {
    const uint32_t* key;                      // two words (device memory)
    uint32_t call;                            // which attention of the step
    uint32_t thr;                             // floor(p 2^32): a word below it drops its element
    float c;                                  // 1 / (1 - p), applied to kept probabilities in fp32
};

// p in [0, 1) -> threshold; the drop probability realised is thr / 2^32 (p itself for every fp32 p >= 2^-8)
static inline uint32_t attn_drop_threshold(float p) { return (uint32_t)((double)p * 4294967296.0); }

#if defined(__HIPCC__)
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t (&out)[4]) {
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// bit c = 1: element (head, q, 4 kblk + c) of attention `call` is kept
__device__ __forceinline__ uint32_t attn_keep4(uint32_t key0, uint32_t key1, uint32_t call, int head, int q, int kblk, uint32_t thr) {
    uint32_t w[4];
    philox4x32_10((uint32_t)kblk, (uint32_t)q, (uint32_t)head, call, key0, key1, w);
    return (w[0] >= thr ? 1u : 0u) | (w[1] >= thr ? 2u : 0u) | (w[2] >= thr ? 4u : 0u) | (w[3] >= thr ? 8u : 0u);
}
#endif
