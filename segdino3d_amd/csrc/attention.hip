// ---------------------------------------------------------------------------------------------
// Fused multi-head attention, head slices of D = 32 W channels (W = 1 or 2), NSRC concatenated sources per head.
// (The width shows in two places only: the score contraction walks W 32-channel blocks per source, and the output is W 32-channel
//  O^T accumulator tiles; everything between - mask, online softmax, tile skip - is per (query, key) and does not see the width.)
//   score(q, key) = scale * sum_src  q_src[q, head*D : +D] . k_src[key, head*D : +D]
//   (NSRC = 2 is the reference's per-head [content | positional] concatenation, decoder :681-687,
//    without ever building the 512-wide tensors)
//   out[q, head*D : +D] = softmax_keys(score masked by bits) @ v[key, head*D : +D]
// One workgroup = (32-query tile, head); its NW waves split the key tiles and are merged through
// LDS in a fixed order.  Per wave and 32-key tile:
//   S^T  = K_tile . Q_tile^T        16*W*NSRC MFMA 32x32x2 : lane (col = query) holds 16 keys of ITS query
//   online softmax is therefore lane-local (+1 cross-half shuffle for the max)
//   O^T += V_tile^T . P^T           16*W MFMA             : P registers feed the B operand unchanged
// mask bits: word [q][tile], bit b = 1 -> key tile*32+b is blocked.
// Never materialises the [H, Q, S] score tensor (reference: segdino3d/models/module/attention.py:186-395).
// The backward pass is attention_bwd.hip.
// ---------------------------------------------------------------------------------------------
#include "common.h"
#include "attention.h"
#include "../../include/segdino3d_hip.h"

struct AttnParams {
    const float* q[2]; int ldq[2];
    const float* k[2]; int ldk[2];
    const float* v; int ldv;
    const uint32_t* bits; int nwords;
    float* out; int ldo;
    int Lq, Lk, H;
    float scale;
    int ksplit;                               // key tiles are dealt to gridDim.z workgroups; partials -> part
    float* part;                              // [qtile][head][ksplit][64 + 1024 W]: m[32], l[32], O[32 W dv][32 q]
    int bf16;                                 // 1: Q, K, P, V rounded to bf16 for the two contractions (fp32 accumulate, fp32 softmax)
    float* lse;                               // optional [H][Lq]: log-sum-exp of every score row (kept for the backward pass)
};

typedef __bf16 abf16x8 __attribute__((ext_vector_type(8)));

// BF16 = the "bf16 decoder" of BASELINE config #3: both contractions run on v_mfma_f32_32x32x16_bf16 (8 contraction
// indices per lane instead of 1: 2 * NSRC + 2 MFMAs per key tile instead of 16 * NSRC + 16); scores, softmax and the
// accumulators stay fp32.  The (lane half, register) -> (channel | key) assignment is the fp32 kernel's, which both
// operands of each product share, so only the grouping of the contraction changes.
// Softmax in the log2 domain: the queries are pre-scaled by scale * log2(e), so a probability is ONE v_exp_f32
// (`__builtin_amdgcn_exp2f`) of score - max instead of a library expf (~10 VALU instructions x 16 scores per lane and key tile:
// the VALU, not the matrix pipe, bounded the kernel at one query per superpoint - 42 % pipe busy).  M / lse leave the kernel
// converted back to natural units.  The next tile's keys and mask word are requested while the current tile multiplies, and a
// key tile whose 32 x 32 mask block is all "blocked" is skipped before its keys are touched (wave-uniform).
#define SD3D_LN2 0.6931471805599453f
// DROP: dropout on the probabilities (attention.h). The keep mask multiplies the tile's probabilities AFTER they are summed into
// l, so m, l, the partial states of a key split, the merge pass and lse are those of the attention without dropout (the reference
// normalises before it drops, attention.py:381-383) and only the O^T contraction sees c K o P.  A lane is a query and holds four runs of
// four consecutive keys of the tile: four Philox calls per lane and key tile.
template <int W, int NSRC, bool BF16, bool DROP = false>
__device__ __forceinline__ void attention_body(const AttnParams& p, const int bx, float* smem, const AttnDrop& dr = AttnDrop{}) {
    constexpr int D = 32 * W;                                   // channels per head: W blocks of 32
    constexpr int PART = 64 + 1024 * W;                         // floats of one partial softmax state
    if ((int)blockIdx.z >= p.ksplit) return;                   // (a batched launch: this scene splits its keys fewer ways than the widest)
    const int nw = blockDim.x >> 6;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int i = lane & 31, h = lane >> 5;
    const int head = blockIdx.y;
    const int q0 = bx * 32;
    const int qi = min(q0 + i, p.Lq - 1);
    const int hc = head * D + h * 16;                            // channel block w of the head starts at hc + 32 w

    float qreg[NSRC][16 * W];
#pragma unroll
    for (int s = 0; s < NSRC; ++s) {
        const float* src = p.q[s] + (int64_t)qi * p.ldq[s] + hc;
#pragma unroll
        for (int e = 0; e < 4 * W; ++e) {
            const f32x4 t = *(const f32x4*)(src + (e >> 2) * 32 + (e & 3) * 4);
#pragma unroll
            for (int c = 0; c < 4; ++c) qreg[s][e * 4 + c] = t[c] * (p.scale * SD3D_LOG2E);
        }
    }
    abf16x8 qb[NSRC][2 * W];
    if (BF16) {
#pragma unroll
        for (int s = 0; s < NSRC; ++s)
#pragma unroll
            for (int g = 0; g < 2 * W; ++g)
#pragma unroll
                for (int c = 0; c < 8; ++c) qb[s][g][c] = (__bf16)qreg[s][g * 8 + c];
    }
    f32x16 O[W];
#pragma unroll
    for (int w = 0; w < W; ++w)
#pragma unroll
        for (int r = 0; r < 16; ++r) O[ATTN_BLK(w)][r] = 0.f;
    float m = -INFINITY, l = 0.f;                       // running max (log2 units) and sum
    uint32_t dkey0 = 0u, dkey1 = 0u;
    if (DROP) { dkey0 = dr.key[0]; dkey1 = dr.key[1]; }

    const int ntiles = (p.Lk + 31) >> 5;
    const int tstep = nw * p.ksplit;
    const uint32_t tail = (p.Lk & 31) ? ~0u << (p.Lk & 31) : 0u;          // key slots of the last tile that lie past Lk
    // bit (slot + 4 * h) of the word belongs to this lane's register r with slot = mfma32_row(r, 0): shift once per tile
    auto load_word = [&](int t) -> uint32_t {
        uint32_t w = (p.bits && t < ntiles) ? p.bits[(int64_t)qi * p.nwords + t] : 0u;
        if (t == ntiles - 1) w |= tail;
        return w;
    };
    auto load_k = [&](f32x4 (&kk)[NSRC][4 * W], int t) {
        const int kr = min(t * 32 + i, p.Lk - 1);      // A-operand row = key (tiles past the end reload the last key: harmless)
#pragma unroll
        for (int s = 0; s < NSRC; ++s) {
            const float* src = p.k[s] + (int64_t)kr * p.ldk[s] + hc;
#pragma unroll
            for (int e = 0; e < 4 * W; ++e) kk[s][e] = *(const f32x4*)(src + (e >> 2) * 32 + (e & 3) * 4);
        }
    };
    constexpr bool KPF = !BF16 && W == 1;               // next tile's keys in flight while this one multiplies: fp32 187 vs 198 us at Q = S = 3000;
                                                        // the bf16 kernel is better off with the registers (4 waves per SIMD: 91 vs 105 us)
    // no key prefetch at W = 2: with two sources the fp32 kernel already holds 64 query + 64 key + 32 value registers and two O^T tiles;
    // another 64 for the next tile's keys would pass 256 and leave one wave per SIMD
    int t = blockIdx.z * nw + wave;
    uint32_t word = load_word(t);
    f32x4 kcur[NSRC][4 * W], knxt[NSRC][4 * W];
    if (KPF && t < ntiles) load_k(kcur, t);
    for (; t < ntiles; t += tstep) {
        const int kt0 = t * 32;
        const uint32_t word_nxt = load_word(t + tstep);
        if (KPF) load_k(knxt, t + tstep);
        if (__ballot(word != ~0u) != 0ull) {                              // some query of the tile sees some key of it
        if (!KPF) load_k(kcur, t);
        // the value rows of this tile are requested before the score MFMAs: their latency hides behind QK^T + softmax
        float vreg[W][16];
        {
            const float* vsrc = p.v + head * D + i;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = min(kt0 + mfma32_row(r, h), p.Lk - 1);
#pragma unroll
                for (int w = 0; w < W; ++w) vreg[ATTN_BLK(w)][r] = vsrc[(int64_t)key * p.ldv + 32 * w];
            }
        }
        f32x16 S;
#pragma unroll
        for (int r = 0; r < 16; ++r) S[r] = 0.f;
#pragma unroll
        for (int s = 0; s < NSRC; ++s) {
            if (BF16) {
#pragma unroll
                for (int g = 0; g < 2 * W; ++g) {
                    abf16x8 kb;
#pragma unroll
                    for (int c = 0; c < 8; ++c) kb[c] = (__bf16)kcur[s][2 * g + (c >> 2)][c & 3];
                    S = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kb, qb[s][g], S, 0, 0, 0);
                }
            } else {
#pragma unroll
                for (int e = 0; e < 4 * W; ++e)
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        S = __builtin_amdgcn_mfma_f32_32x32x2f32(kcur[s][e][c], qreg[s][e * 4 + c], S, 0, 0, 0);
            }
        }
        // S[r] = log2-score(key = kt0 + (r&3) + 8*(r>>2) + 4*h, query = q0 + i)
        const uint32_t wh = word >> (4 * h);
        float tmax = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            S[r] = ((wh >> mfma32_row(r, 0)) & 1u) ? -INFINITY : S[r];
            tmax = fmaxf(tmax, S[r]);
        }
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
        const float mn = fmaxf(m, tmax);
        float alpha = 1.f;
        float pr[16];
        if (mn == -INFINITY) {
#pragma unroll
            for (int r = 0; r < 16; ++r) pr[r] = 0.f;
        } else {
            alpha = __builtin_amdgcn_exp2f(m - mn);     // m = -inf -> 0
            float ls = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) { pr[r] = __builtin_amdgcn_exp2f(S[r] - mn); ls += pr[r]; }
            l = l * alpha + ls;
            m = mn;
        }
        if (DROP) {                                     // pr[4 g + c] belongs to key kt0 + 8 g + 4 h + c: keys 4 kblk .. 4 kblk + 3
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const uint32_t keep = attn_keep4(dkey0, dkey1, dr.call, head, q0 + i, (kt0 >> 2) + 2 * g + h, dr.thr);
#pragma unroll
                for (int c = 0; c < 4; ++c) pr[4 * g + c] = ((keep >> c) & 1u) ? pr[4 * g + c] * dr.c : 0.f;
            }
        }
        if (__ballot(alpha != 1.f) != 0ull) {           // the running maxima settle after a few tiles: no rescale, no dependency on O
#pragma unroll
            for (int w = 0; w < W; ++w)
#pragma unroll
                for (int r = 0; r < 16; ++r) O[ATTN_BLK(w)][r] *= alpha;
        }
        // O^T[dv][query] += sum_key V[key][dv] * P[query][key];  A = V^T (row = dv = i), B = P^T
#pragma unroll
        for (int w = 0; w < W; ++w) {
        if (BF16) {
#pragma unroll
            for (int g = 0; g < 2; ++g) {
                abf16x8 vb, pb;
#pragma unroll
                for (int c = 0; c < 8; ++c) { vb[c] = (__bf16)vreg[ATTN_BLK(w)][g * 8 + c]; pb[c] = (__bf16)pr[g * 8 + c]; }
                O[ATTN_BLK(w)] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vb, pb, O[ATTN_BLK(w)], 0, 0, 0);
            }
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) O[ATTN_BLK(w)] = __builtin_amdgcn_mfma_f32_32x32x2f32(vreg[ATTN_BLK(w)][r], pr[r], O[ATTN_BLK(w)], 0, 0, 0);
        }
        }
        }
        word = word_nxt;
        if (KPF) {
#pragma unroll
            for (int s = 0; s < NSRC; ++s)
#pragma unroll
                for (int e = 0; e < 4 * W; ++e) kcur[s][e] = knxt[s][e];
        }
    }
    l += __shfl_xor(l, 32);

    // ---- merge the NW partial results: smem layout per wave: m[32], l[32], O[32 W dv][32 q]
    float* wm = smem + wave * PART;
    float* wl = wm + 32;
    float* wo = wl + 32;
    if (h == 0) { wm[i] = m; wl[i] = l; }
#pragma unroll
    for (int w = 0; w < W; ++w)
#pragma unroll
        for (int r = 0; r < 16; ++r) wo[(32 * w + mfma32_row(r, h)) * 32 + i] = O[ATTN_BLK(w)][r];
    __syncthreads();
    for (int e = threadIdx.x; e < 1024 * W; e += blockDim.x) {
        const int qq = e >> (4 + W), dv = e & (D - 1);  // consecutive threads -> consecutive dv (coalesced store)
        float M = -INFINITY;
        for (int w = 0; w < nw; ++w) M = fmaxf(M, smem[w * PART + qq]);
        float L = 0.f, acc = 0.f;
        for (int w = 0; w < nw; ++w) {
            const float* base = smem + w * PART;
            const float mw = base[qq];
            const float f = (mw == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f(mw - M);
            L += base[32 + qq] * f;
            acc += base[64 + dv * 32 + qq] * f;
        }
        if (p.ksplit > 1) {                             // this workgroup's share of the keys: leave (M, L, sum) for the merge pass
            float* dst = p.part + (((int64_t)bx * p.H + head) * p.ksplit + blockIdx.z) * PART;
            if (dv == 0) { dst[qq] = M; dst[32 + qq] = L; }
            dst[64 + dv * 32 + qq] = acc;
        } else if (q0 + qq < p.Lq) {
            p.out[(int64_t)(q0 + qq) * p.ldo + head * D + dv] = acc / L;
            if (p.lse && dv == 0) p.lse[(int64_t)head * p.Lq + q0 + qq] = M * SD3D_LN2 + logf(L);      // back to natural units
        }
    }
}

// W = 1: up to eight waves per workgroup (launch bounds 512, 128 registers a wave).  W = 2: at most four (attention_config), so a wave may
// hold up to 512 registers - the fp32 kernel with two sources keeps 64 query and 64 key registers beside two O^T tiles - and four partial
// states (4 x 2112 floats) fit the default 64 KiB of LDS.
template <int W, int NSRC, bool BF16>
__global__ __launch_bounds__(W == 1 ? 512 : 256) void attention_kernel(const AttnParams p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    attention_body<W, NSRC, BF16>(p, blockIdx.x, smem);
}

// the same workgroups with dropout on the probabilities (training, one scene per launch)
template <int W, int NSRC, bool BF16>
__global__ __launch_bounds__(W == 1 ? 512 : 256) void attention_dropout_kernel(const AttnParams p, const AttnDrop dr) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    attention_body<W, NSRC, BF16, true>(p, blockIdx.x, smem, dr);
}

// Several scenes' attentions in ONE launch (the decoder of a batched evaluation forward): blockIdx.x runs over the query tiles of all
// scenes, a workgroup finds its scene from the tiles' prefix sums and then IS that scene's workgroup - same code, same waves per
// workgroup, same key split, so every scene's rows are the bits of its own launch.
struct AttnBatch { int n; int tile0[SD3D_MAX_BATCH + 1]; AttnParams s[SD3D_MAX_BATCH]; };
template <int W, int NSRC, bool BF16>
__global__ __launch_bounds__(W == 1 ? 512 : 256) void attention_batch_kernel(const AttnBatch b) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    int si = 0;
    for (int k = 1; k < b.n; ++k) if ((int)blockIdx.x >= b.tile0[k]) si = k;
    attention_body<W, NSRC, BF16>(b.s[si], blockIdx.x - b.tile0[si], smem);
}

// second pass of the key-split attention: combine the ksplit partial softmax states (64 + 1024 W floats each) of one (query tile, head)
template <int W>
__device__ __forceinline__ void attention_merge_body(const AttnParams& p, const int bx) {
    constexpr int D = 32 * W, PART = 64 + 1024 * W;
    if (p.ksplit <= 1) return;
    const int head = blockIdx.y, q0 = bx * 32;
    const float* base = p.part + ((int64_t)bx * p.H + head) * p.ksplit * PART;
    for (int e = threadIdx.x; e < 1024 * W; e += 256) {
        const int qq = e >> (4 + W), dv = e & (D - 1);
        float M = -INFINITY, L = 0.f, acc = 0.f;
        if (p.ksplit <= 8) {
            // every split's three values requested before the first is used (splits past the end re-read the last one and contribute
            // an exact zero): the two dependent loops below ran at two memory latencies per split - 11 us for a 56-workgroup launch
            float mz[8], lz[8], oz[8];
#pragma unroll
            for (int z = 0; z < 8; ++z) {
                const float* b = base + (z < p.ksplit ? z : p.ksplit - 1) * PART;
                mz[z] = b[qq]; lz[z] = b[32 + qq]; oz[z] = b[64 + dv * 32 + qq];
            }
#pragma unroll
            for (int z = 0; z < 8; ++z) M = fmaxf(M, mz[z]);
#pragma unroll
            for (int z = 0; z < 8; ++z) {
                const float f = (z >= p.ksplit || mz[z] == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f(mz[z] - M);
                if (z < p.ksplit) { L = __builtin_fmaf(lz[z], f, L); acc = __builtin_fmaf(oz[z], f, acc); }
            }
        } else {
        for (int z = 0; z < p.ksplit; ++z) M = fmaxf(M, base[z * PART + qq]);
        for (int z = 0; z < p.ksplit; ++z) {
            const float* b = base + z * PART;
            const float mz = b[qq];
            const float f = (mz == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f(mz - M);
            L = __builtin_fmaf(b[32 + qq], f, L);
            acc = __builtin_fmaf(b[64 + dv * 32 + qq], f, acc);
        }
        }
        if (q0 + qq < p.Lq) {
            p.out[(int64_t)(q0 + qq) * p.ldo + head * D + dv] = acc / L;
            if (p.lse && dv == 0) p.lse[(int64_t)head * p.Lq + q0 + qq] = M * SD3D_LN2 + logf(L);
        }
    }
}
template <int W>
__global__ __launch_bounds__(256) void attention_merge_kernel(const AttnParams p) { attention_merge_body<W>(p, blockIdx.x); }
template <int W>
__global__ __launch_bounds__(256) void attention_merge_batch_kernel(const AttnBatch b) {
    int si = 0;
    for (int k = 1; k < b.n; ++k) if ((int)blockIdx.x >= b.tile0[k]) si = k;
    attention_merge_body<W>(b.s[si], blockIdx.x - b.tile0[si]);
}

// W = head width / 32 of a supported head width (32 or 64 channels), else 0
static int attention_width(int head_dim) { return head_dim == 32 ? 1 : (head_dim == 64 ? 2 : 0); }
// floats of one partial softmax state: m[32], l[32], O[32 W][32]
static size_t attention_part_floats(int W) { return 64 + 1024 * (size_t)W; }
static size_t attention_ws_bytes(int Lq, int H, int W) { return (size_t)cdiv(Lq, 32) * H * 8 * attention_part_floats(W) * sizeof(float); }
extern "C" size_t sd3d_attention_ws_bytes(int Lq, int H, int head_dim) {
    const int W = attention_width(head_dim);
    return W ? attention_ws_bytes(Lq, H, W) : 0;
}

// waves per workgroup and key split of one attention (Lq queries, Lk keys, H heads) given `ws_bytes` of split workspace
// W = 2 (64-channel heads): the same rule with at most four waves per workgroup (the kernel's launch bounds).
static void attention_config(int Lq, int Lk, int H, int W, bool have_ws, size_t ws_bytes, int* nw_out, int* ks_out) {
    const int ntiles = (Lk + 31) / 32;
    // 4 - 7 key tiles (the 200-key self-attention, the 301-key 2D-query attention): four waves of one or two tiles each instead of two waves
    // of up to four (every tile is a dependent load -> MFMA round trip): decoder 1.863 -> 1.840 ms against round 3's two waves.
    int nw = ntiles >= 32 ? 8 : (ntiles >= 4 ? 4 : (ntiles >= 2 ? 2 : 1));
    if (W == 2 && nw > 4) nw = 4;
    // few query tiles x heads (200 queries: 56 workgroups on 256 CUs) and many key tiles: deal the key tiles to several
    // workgroups and merge their softmax states in a second, tiny pass (each wave walks its tiles serially, so the
    // single-pass kernel is bound by ~12 dependent load -> MFMA round trips per wave)
    const int64_t wgs = cdiv(Lq, 32) * H;
    int ks = 1;
    if (have_ws && wgs < 128 && ntiles >= 4 * nw) {
        nw = nw > 4 ? 4 : nw;                                  // 4 waves x more key splits: 200 queries x 3000 keys 44.4 -> 37.7 us (8 waves merge through LDS longer than they multiply)
        ks = (int)(512 / wgs);
        const int most = ntiles / (2 * nw);
        ks = ks > most ? most : ks;
        ks = ks > 8 ? 8 : ks;
        if (ks < 2 || ws_bytes < (size_t)wgs * ks * attention_part_floats(W) * sizeof(float)) ks = 1;
    }
    *nw_out = nw; *ks_out = ks;
}

// the instantiations by [W - 1][nsrc - 1][bf16]
#define ATTN_TABLE(K) {{{K<1, 1, false>, K<1, 1, true>}, {K<1, 2, false>, K<1, 2, true>}}, {{K<2, 1, false>, K<2, 1, true>}, {K<2, 2, false>, K<2, 2, true>}}}
static void (*const attn_scene_kernels[2][2][2])(const AttnParams) = ATTN_TABLE(attention_kernel);
static void (*const attn_batch_kernels[2][2][2])(const AttnBatch) = ATTN_TABLE(attention_batch_kernel);
static void (*const attn_dropout_kernels[2][2][2])(const AttnParams, const AttnDrop) = ATTN_TABLE(attention_dropout_kernel);
#undef ATTN_TABLE

// dr: dropout on the probabilities (same grid, waves and key split; the merge pass is the plain one), nullptr = none
static int launch_attention(const AttnParams& p_in, int nsrc, int W, void* ws, size_t ws_bytes, hipStream_t st, bool merge = true,
                            const AttnDrop* dr = nullptr) {
    AttnParams p = p_in;
    if (W != 1 && W != 2) return sd3d_set_error(SD3D_ERR_ARG, "attention: heads must be 32 or 64 channels wide");
    if (nsrc != 1 && nsrc != 2) return sd3d_set_error(SD3D_ERR_ARG, "attention: nsrc must be 1 or 2");
    if (p.Lq <= 0 || p.Lk <= 0) return sd3d_set_error(SD3D_ERR_ARG, "attention: empty query or key set");
    for (int s = 0; s < nsrc; ++s)
        if ((p.ldq[s] & 3) || (p.ldk[s] & 3)) return sd3d_set_error(SD3D_ERR_ARG, "attention: q/k strides must be multiples of 4");
    int nw, ks;
    attention_config(p.Lq, p.Lk, p.H, W, ws != nullptr, ws_bytes, &nw, &ks);
    p.ksplit = ks;
    p.part = (float*)ws;
    const dim3 grid((unsigned)cdiv(p.Lq, 32), (unsigned)p.H, (unsigned)ks), block(64 * nw);
    const size_t sm = (size_t)nw * attention_part_floats(W) * sizeof(float);
    if (dr) hipLaunchKernelGGL(attn_dropout_kernels[W - 1][nsrc - 1][p.bf16 ? 1 : 0], grid, block, sm, st, p, *dr);
    else hipLaunchKernelGGL(attn_scene_kernels[W - 1][nsrc - 1][p.bf16 ? 1 : 0], grid, block, sm, st, p);
    if (ks > 1 && merge)
        hipLaunchKernelGGL(W == 1 ? attention_merge_kernel<1> : attention_merge_kernel<2>, dim3((unsigned)cdiv(p.Lq, 32), (unsigned)p.H), dim3(256), 0, st, p);
    SD3D_CHECK_LAUNCH();
    return SD3D_OK;
}

// n <= SD3D_MAX_BATCH independent attentions (same heads, scale, sources, arithmetic type) in one launch - when every scene's own launch
// would use the same number of waves per workgroup; otherwise one launch per scene.  Scene i's split workspace is
// sd3d_attention_ws_bytes(Lq_i, H, head_dim) bytes, back to back in ws.
// ksplit_out / part_off_out (host arrays of n entries, optional): the launch then STOPS after the key-split pass - scene i's rows are
// final in its `out` where ksplit_out[i] == 1 and otherwise wait as partial softmax states at ws + part_off_out[i] floats for the
// consumer that combines them (rowchain.hip MERGE: the expression of attention_merge_body).
static int launch_attention_batch(int n, const AttnParams* jobs, int nsrc, int W, void* ws, size_t ws_bytes, hipStream_t st,
                                  int32_t* ksplit_out = nullptr, int64_t* part_off_out = nullptr) {
    if (n <= 0) return SD3D_OK;
    if (W != 1 && W != 2) return sd3d_set_error(SD3D_ERR_ARG, "attention_batch: heads must be 32 or 64 channels wide");
    if (nsrc != 1 && nsrc != 2) return sd3d_set_error(SD3D_ERR_ARG, "attention_batch: nsrc must be 1 or 2");
    const bool merge = ksplit_out == nullptr;
    if (n > SD3D_MAX_BATCH) return sd3d_set_error(SD3D_ERR_ARG, "attention_batch: at most 16 scenes per call");
    AttnBatch b;
    b.n = n;
    int nw0 = 0, ks_max = 1, tiles = 0;
    bool same = true;
    size_t off = 0;
    for (int i = 0; i < n; ++i) {
        AttnParams p = jobs[i];
        if (p.Lq <= 0 || p.Lk <= 0) return sd3d_set_error(SD3D_ERR_ARG, "attention_batch: empty query or key set");
        for (int s = 0; s < nsrc; ++s)
            if ((p.ldq[s] & 3) || (p.ldk[s] & 3)) return sd3d_set_error(SD3D_ERR_ARG, "attention_batch: q/k strides must be multiples of 4");
        const size_t need = attention_ws_bytes(p.Lq, p.H, W);
        const bool have = ws != nullptr && off + need <= ws_bytes;
        int nw, ks;
        attention_config(p.Lq, p.Lk, p.H, W, have, need, &nw, &ks);
        p.ksplit = ks;
        p.part = have ? (float*)((char*)ws + off) : nullptr;
        off += need;
        if (i == 0) nw0 = nw;
        same = same && nw == nw0;
        ks_max = ks > ks_max ? ks : ks_max;
        b.tile0[i] = tiles;
        tiles += (int)cdiv(p.Lq, 32);
        b.s[i] = p;
        if (!merge) {
            ksplit_out[i] = ks;
            if (part_off_out) part_off_out[i] = have ? (int64_t)((off - need) / sizeof(float)) : 0;
        }
    }
    b.tile0[n] = tiles;
    if (!same) {                                               // different workgroup shapes: each scene its own launch (same results)
        for (int i = 0; i < n; ++i) {
            const int rc = launch_attention(jobs[i], nsrc, W, b.s[i].part, b.s[i].part ? attention_ws_bytes(jobs[i].Lq, jobs[i].H, W) : 0, st, merge);
            if (rc != SD3D_OK) return rc;
        }
        return SD3D_OK;
    }
    const dim3 grid((unsigned)tiles, (unsigned)b.s[0].H, (unsigned)ks_max), block(64 * nw0);
    const size_t sm = (size_t)nw0 * attention_part_floats(W) * sizeof(float);
    hipLaunchKernelGGL(attn_batch_kernels[W - 1][nsrc - 1][b.s[0].bf16 ? 1 : 0], grid, block, sm, st, b);
    if (ks_max > 1 && merge)
        hipLaunchKernelGGL(W == 1 ? attention_merge_batch_kernel<1> : attention_merge_batch_kernel<2>, dim3((unsigned)tiles, (unsigned)b.s[0].H), dim3(256), 0, st, b);
    SD3D_CHECK_LAUNCH();
    return SD3D_OK;
}

// The caller's part of AttnParams; ksplit and part are the launcher's to choose.
static AttnParams attn_params(const float* q0, int ldq0, const float* q1, int ldq1, const float* k0, int ldk0, const float* k1, int ldk1,
                              const float* v, int ldv, const uint32_t* mask_bits, int Lq, int Lk, int H, float scale, float* out, int ldo,
                              int bf16, float* lse) {
    AttnParams p;
    p.q[0] = q0; p.ldq[0] = ldq0; p.q[1] = q1; p.ldq[1] = ldq1;
    p.k[0] = k0; p.ldk[0] = ldk0; p.k[1] = k1; p.ldk[1] = ldk1;
    p.v = v; p.ldv = ldv; p.bits = mask_bits; p.nwords = (Lk + 31) / 32; p.out = out; p.ldo = ldo;
    p.Lq = Lq; p.Lk = Lk; p.H = H; p.scale = scale; p.ksplit = 1; p.part = nullptr; p.bf16 = bf16 ? 1 : 0; p.lse = lse;
    return p;
}
// Heads of 32 or 64 channels, dropout rate p in [0, 1) on the probabilities (p > 0: training, needs the key; p == 0: the kernels without
// dropout, key ignored); anything else -> SD3D_ERR_ARG before anything is launched.
extern "C" int sd3d_attention(const float* q0, int ldq0, const float* q1, int ldq1, const float* k0, int ldk0, const float* k1, int ldk1,
                              const float* v, int ldv, const uint32_t* mask_bits, int Lq, int Lk, int H, int head_dim, float scale,
                              float* out, int ldo, float* lse, int bf16, void* ws, size_t ws_bytes, const uint32_t* key, int call, float p,
                              void* stream) {
    if (!(p >= 0.f && p < 1.f)) return sd3d_set_error(SD3D_ERR_ARG, "attention: p must lie in [0, 1)");
    if (p > 0.f && !key) return sd3d_set_error(SD3D_ERR_ARG, "attention: dropout needs a key");
    const int W = attention_width(head_dim);
    if (!W) return sd3d_set_error(SD3D_ERR_ARG, "attention: heads must be 32 or 64 channels wide");
    if ((q1 == nullptr) != (k1 == nullptr)) return sd3d_set_error(SD3D_ERR_ARG, "attention: q1 and k1 must be given together");
    const AttnParams ap = attn_params(q0, ldq0, q1, ldq1, k0, ldk0, k1, ldk1, v, ldv, mask_bits, Lq, Lk, H, scale, out, ldo, bf16, lse);
    const AttnDrop dr = {key, (uint32_t)call, attn_drop_threshold(p), 1.f / (1.f - p)};
    return launch_attention(ap, q1 ? 2 : 1, W, ws, ws_bytes, (hipStream_t)stream, true, p > 0.f ? &dr : nullptr);
}

// the keep mask alone, keep[H, Lq, Lk] bytes (1 = kept): one thread per (head, query, four consecutive keys)
__global__ __launch_bounds__(256) void attention_dropout_keep_kernel(const AttnDrop dr, int H, int Lq, int Lk, uint8_t* __restrict__ keep) {
    const int nblk = (Lk + 3) >> 2;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)H * Lq * nblk) return;
    const int kblk = (int)(e % nblk), q = (int)((e / nblk) % Lq), head = (int)(e / ((int64_t)nblk * Lq));
    const uint32_t bits = attn_keep4(dr.key[0], dr.key[1], dr.call, head, q, kblk, dr.thr);
    uint8_t* dst = keep + ((int64_t)head * Lq + q) * Lk;
    for (int c = 0; c < 4; ++c)
        if (4 * kblk + c < Lk) dst[4 * kblk + c] = (uint8_t)((bits >> c) & 1u);
}
extern "C" int sd3d_attention_dropout_keep(const uint32_t* key, int call, int H, int Lq, int Lk, float p, uint8_t* keep, void* stream) {
    if (!(p >= 0.f && p < 1.f)) return sd3d_set_error(SD3D_ERR_ARG, "attention_dropout_keep: p must lie in [0, 1)");
    if (!key || !keep || H <= 0 || Lq <= 0 || Lk <= 0) return sd3d_set_error(SD3D_ERR_ARG, "attention_dropout_keep: key, output and positive sizes needed");
    const AttnDrop dr = {key, (uint32_t)call, attn_drop_threshold(p), 1.f / (1.f - p)};
    const int64_t n = (int64_t)H * Lq * ((Lk + 3) / 4);
    hipLaunchKernelGGL(attention_dropout_keep_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, dr, H, Lq, Lk, keep);
    SD3D_CHECK_LAUNCH();
    return SD3D_OK;
}

static int attention_batch_impl(int n, const sd3d_attn_job* jobs, int H, int W, float scale, int bf16, void* ws, size_t ws_bytes, void* stream,
                                int32_t* ksplit_out, int64_t* part_off_out) {
    if (n <= 0) return SD3D_OK;
    if (n > SD3D_MAX_BATCH || !jobs) return sd3d_set_error(SD3D_ERR_ARG, "attention_batch: 1..16 jobs");
    AttnParams p[SD3D_MAX_BATCH];
    const bool two = jobs[0].q1 != nullptr;
    for (int i = 0; i < n; ++i) {
        const sd3d_attn_job& j = jobs[i];
        if ((j.q1 == nullptr) != (j.k1 == nullptr) || (j.q1 != nullptr) != two) return sd3d_set_error(SD3D_ERR_ARG, "attention_batch: all jobs need the same sources");
        p[i] = attn_params(j.q0, j.ldq0, j.q1, j.ldq1, j.k0, j.ldk0, j.k1, j.ldk1, j.v, j.ldv, j.mask_bits, j.Lq, j.Lk, H, scale, j.out, j.ldo, bf16, nullptr);
    }
    return launch_attention_batch(n, p, two ? 2 : 1, W, ws, ws_bytes, (hipStream_t)stream, ksplit_out, part_off_out);
}
extern "C" int sd3d_attention_batch(int n, const sd3d_attn_job* jobs, int H, int head_dim, float scale, int bf16, void* ws, size_t ws_bytes,
                                    void* stream) {
    const int W = attention_width(head_dim);
    if (!W) return sd3d_set_error(SD3D_ERR_ARG, "attention_batch: heads must be 32 or 64 channels wide");
    return attention_batch_impl(n, jobs, H, W, scale, bf16, ws, ws_bytes, stream, nullptr, nullptr);
}
extern "C" int sd3d_attention_config(int Lq, int Lk, int H, int head_dim, size_t ws_bytes, int* waves_out, int* ksplit_out) {
    const int W = attention_width(head_dim);
    if (!W || Lq <= 0 || Lk <= 0 || H <= 0 || !waves_out || !ksplit_out)
        return sd3d_set_error(SD3D_ERR_ARG, "attention_config: heads must be 32 or 64 channels wide, sizes positive, outputs given");
    attention_config(Lq, Lk, H, W, ws_bytes > 0, ws_bytes, waves_out, ksplit_out);
    return SD3D_OK;
}
// 32-channel heads only: the row chain that combines the partial states is built for that width
extern "C" int sd3d_attention_batch_parts(int n, const sd3d_attn_job* jobs, int H, float scale, int bf16, void* ws, size_t ws_bytes,
                                          int32_t* ksplit_out_host, int64_t* part_off_out_host, void* stream) {
    if (!ksplit_out_host || !part_off_out_host) return sd3d_set_error(SD3D_ERR_ARG, "attention_batch_parts: output arrays missing");
    return attention_batch_impl(n, jobs, H, 1, scale, bf16, ws, ws_bytes, stream, ksplit_out_host, part_off_out_host);
}
