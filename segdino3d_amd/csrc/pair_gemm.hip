// Pair-major sparse convolution (exact fp32 MFMA).
//
// The output-stationary kernels of gather_gemm.hip walk all K offsets for every 32-row output tile, so
// at rulebook density d they spend 1/d of their MFMA time on zeros (d = 0.06 .. 0.6 on a ScanNet
// scene), and the pair-compacted variants there are limited by LDS capacity (small row tiles -> the
// 32-pair MFMA chunks are half empty and every small tile re-reads all K weight matrices).
//
// Here the rulebook is laid out pair-major ONCE per neighbour table (it is shared by every
// convolution of a U-Net level):
//     for k in 0..K-1:  the pairs (in = nbr[k][r], out = r) with in >= 0, in row order,
//     each k segment padded to a multiple of 128 pairs (pad entries have in = -1)
// so that a 128-pair tile has ONE weight matrix W[k] and every MFMA row is a real pair:
//     pass 1  part[p][:] = X[in_idx[p]][:] . W[k(p)]^T        dense 128 x Cout x Cin tiles, lock-step
//                                                              LDS-shared weights, fp32 MFMA
//     pass 2  out[r][:]  = act(scale * sum_k part[pos[k][r]][:] + shift + res[r][:])   k ascending
// pos[k][r] = position of pair (k, r) in the list or -1.  Pass 2 is pure streaming (HBM-bound);
// the partial products cost 2 x 4 x P x Cout bytes of extra traffic, cheap next to the 157 TFLOP/s
// fp32 matrix rate (>= 16 flop per byte moved at Cin = 96).  The sum order is fixed (full Cin dot
// product per pair, then k ascending) so results are deterministic.
// The rulebook lists are built in pair_lists.hip.
#include "gg_common.h"
#include "pair_conv.h"
#include <stdlib.h>
#include <vector>

static std::atomic<int> g_scenes_in_flight{1};
extern "C" int sd3d_set_scenes_in_flight(int n) { return g_scenes_in_flight.exchange(n < 1 ? 1 : n); }

// Partial products are written once by pass 1 and read once by pass 2, hundreds of megabytes per convolution.  Measured (same box,
// tools/ab_lib.sh; conv ms per scene in the instrumented replay / single-scene latency): non-temporal READS in pass 2 7.49 -> 7.34 ms /
// 12.10 -> 12.00 ms (they stop displacing the activation rows the next pass 1 gathers); non-temporal STORES in pass 1 7.49 -> 7.68 ms /
// 12.1 -> 12.7 ms (one scene in flight: 7.92 -> 8.43 ms) - the plain stores are combined in L2 and part of them is still on chip when
// pass 2 asks.  So: plain stores, non-temporal loads.
// (with SEVERAL scenes in flight the trade flips: non-temporal stores 114.5 -> 116.8 scenes/s - the other scenes' kernels, not this
// convolution's pass 2, are what the written-back lines would displace - so pass 1 takes the store flavour from `p.nt_part`,
// set by the launcher from the scenes-in-flight hint.)
#define PART_STORE4(PTR, V) do { if (p.nt_part) __builtin_nontemporal_store((V), (f32x4*)(PTR)); else *(f32x4*)(PTR) = (V); } while (0)
#define PART_LOAD4(PTR) __builtin_nontemporal_load((const f32x4*)(PTR))
#define PBS_LD 36

// ---- pass 1: dense tiles over the pair list --------------------------------------------------
struct PGParams {
    const float* in0; int ld0; int C0;
    const float* in1; int ld1;
    const int32_t* in_idx;                    // [n_tiles * 128]
    const int32_t* tile_k;                    // [n_tiles], -1 = past the end
    const float* wt;                          // [K][Cout][Cin]
    int Cin, Cout;
    float* part;                              // [n_tiles * 128][Cout]
    int n_tiles;                              // capacity; the real count is tile_k[n_tiles]
    // direct epilogue (out_idx != NULL): every output row has exactly ONE pair (transposed k2s2 convolution), so the tile's
    // products ARE the output rows: out[out_idx[p]] = act(scale * acc + shift + res) straight from pass 1, no partial products
    const int32_t* out_idx;
    const float* scale; const float* shift; const float* res; int ld_res;
    float* out; int ld_out; int act;
    int nt_part;                              // 1: non-temporal partial-product stores (several scenes in flight; see PART_STORE4)
    int chained;                              // 1: tile_k carries PG_CHAIN flags (chained lists: a tile's products add onto the next tile's)
    int64_t dense_rows;                       // > 0: no lists at all - pair p is (in = out = row p) of a dense [rows, Cin] x W[0]^T product (direct epilogue)
    unsigned long long* pool_ctr;             // lock-step kernel: one {epoch, next unit} word per column group of this launch's slot, or NULL (static partition only)
    unsigned int pool_epoch;                  // this launch's epoch (never 0)
    int k_flip;                               // >= 0: the weight matrix of offset k is W[k_flip - k] (mirrored offset order: SD3D_PAIR_MIRROR_W), -1: W[k]
};
// The shared tail of a lock-step launch.  A static partition gives every workgroup the same number of tiles, not the same time: a chained
// table's ranges are snapped to chain boundaries (+-2 tiles of the 6 - 10 a workgroup has at levels 0 - 2), the workgroups of a CU are
// served oldest first, the tiles' gathers hit or miss L2 - the counters of profiles/r05_pmc_pair_gemm.md put the MEAN wave lifetime at
// 68 - 80 % of a launch while the pipe is 73 - 82 % busy during a wave's lifetime: a fifth of every launch is waiting for the last
// workgroups.  So only the first 13/16 of the tile list is dealt out statically; the rest is a pool of small units (>= 6 steps each) that
// the workgroups draw from a counter as they run dry.  Which workgroup multiplies a tile never changes what is stored for it: the
// results are the same bits.
// Round 6: the counters carry the EPOCH of the launch that owns them.  A counter is one 64-bit word {epoch : 32 | next unit : 32} per
// (launch slot, column group); the host hands every pooled launch a ticket t -> slot t % PG_POOL_SLOTS, epoch t / PG_POOL_SLOTS + 1 (never
// 0: zero-initialised memory is "no launch yet").  The launch's first claim (below) replaces whatever an OLDER epoch left in the word, so a
// launch that died half-way (device fault, a killed debugger, hipDeviceReset in a long-lived server) cannot make a later launch skip units,
// no launch has to leave the slot clean, and no "workgroups done" counter is needed (round 5's form zeroed the slot from the launch's last
// workgroup and trusted it to be zero on entry: VERDICT r5 "the shared tail has no in-suite guard").  A word with a NEWER epoch is caught at
// the draw: the launch splits its pool statically (same bits) and sd3d_pair_pool_check() reports it.  What is NOT tolerated: a foreign write
// that carries the launch's OWN epoch and a non-zero count - the claim keeps it and the draws start behind the units it counts, which are
// skipped.  So the ring is assumed to be written by these launches only, and to be long enough that the previous user of a slot (16384
// pooled launches ago, ~150 forwards) has finished; sd3d_pair_pool_check() looks for words no sequence of finished launches can leave.
// A launch that is being captured into a HIP graph gets NO pool (a replay would meet its own exhausted epoch): static partition.
#define PG_POOL_SLOTS 16384
#define PG_POOL_WORDS 4                                         // per slot: one {epoch, next} word per column group (<= 4)
__device__ unsigned long long g_pool_ctr[PG_POOL_SLOTS * PG_POOL_WORDS];
__device__ unsigned int g_pool_bad;                             // sd3d_pair_pool_check's result
__device__ unsigned int g_pool_bad_seen;                        // workgroups that met a poisoned word since the last check (they fell back to a static split)

// A workgroup CLAIMS its launch's word when it starts - an atomic max with {epoch, 0}, no return value waited for: epochs of a slot only
// grow, so whatever an older launch left (finished or dead) is replaced by the first claim and every later claim is a no-op - and DRAWS
// with one atomic add when it runs dry: its own claim precedes its draw in program order on the same address, so a draw sees this launch's
// epoch or - only after a foreign write - a newer one.  (Rejected forms: a compare-and-swap loop per draw cost 1 - 2 ms per launch, the
// ~500 workgroups of a launch run dry together and retry against each other; claim-on-first-draw tripled the atomics at that moment:
// +25 us on the 400 us layers.)  A newer epoch cannot come from any launch: POOL_POISONED tells the caller to split the pool statically,
// and the event is counted in g_pool_bad_seen for sd3d_pair_pool_check.
#define POOL_POISONED 0xFFFFFFFFu
__device__ __forceinline__ void pool_claim(unsigned long long* ctr, unsigned int epoch) {
    (void)__hip_atomic_fetch_max(ctr, (unsigned long long)epoch << 32, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned int pool_draw(unsigned long long* ctr, unsigned int epoch) {
    const unsigned long long old = __hip_atomic_fetch_add(ctr, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return (unsigned int)(old >> 32) == epoch ? (unsigned int)old : POOL_POISONED;
}
// slots in a state no sequence of finished launches can leave behind: an epoch the host has not handed out yet for that slot
// (`tickets` pooled launches so far on this device's ring: slot s was last owned by epoch ceil((tickets - s) / PG_POOL_SLOTS))
__global__ __launch_bounds__(256) void pool_check_kernel(unsigned long long tickets) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= PG_POOL_SLOTS) return;
    const unsigned long long last = tickets > (unsigned long long)s ? (tickets - 1 - s) / PG_POOL_SLOTS + 1 : 0;
    int bad = 0;
#pragma unroll
    for (int w = 0; w < PG_POOL_WORDS; ++w) {
        const unsigned long long v = g_pool_ctr[(size_t)s * PG_POOL_WORDS + w];
        if ((v >> 32) > last || ((v >> 32) == 0 && v != 0)) ++bad;    // (epoch 0 = never used: the whole word is zero)
    }
    if (bad) atomicAdd(&g_pool_bad, (unsigned int)bad);
}


// scale * x + shift as ONE fused multiply-add in every epilogue of this file, so that the paths agree bit for bit
__device__ __forceinline__ float pg_affine(float x, const float* scale, const float* shift, int n) {
    return __builtin_fmaf(x, scale ? scale[n] : 1.f, shift ? shift[n] : 0.f);
}
// (GELU / sigmoid never follow a sparse convolution in the shipped networks: kept out of line so that the 64 epilogue sites of a
//  kernel do not each carry an inlined erff / expf; that is why this is not common.h's sd3d_act, whose expressions these are)
__device__ __attribute__((noinline)) float pg_act_slow(float t, int act) {
    return act == 2 ? 0.5f * t * (1.f + erff(t * 0.70710678118654752440f)) : 1.f / (1.f + expf(-t));
}
__device__ __forceinline__ float pg_act(float t, int act) {
    if (act == 1) t = fmaxf(t, 0.f);
    else if (act >= 2) t = pg_act_slow(t, act);
    return t;
}

// ---- pass 1, lock-step variant ------------------------------------------------------------------------------------------
// A workgroup walks its range of consecutive 128-pair tiles as ONE flat stream of (tile, 32-channel chunk) steps: the weight chunk
// of step s + 1 is staged global -> registers -> LDS while step s runs on the matrix cores, the gathered activation rows are
// requested TWO steps ahead (three register stages, renamed by unrolling), across tile boundaries.  The four waves share the weight
// chunk (lock-step, one barrier per step); each owns 32 pairs x (32 NT) output columns.
// Round 5 form.  The ISA of the round 1-4 form (hipcc 7.2, -save-temps) showed two full memory round trips outside the matrix work:
// every tile switch loaded the next gather indices and the next tile's offset from global memory and waited for them on the spot
// (`s_waitcnt vmcnt(0)`: the offset must become a scalar, the index register is copied) with all four waves parked behind the
// barrier - every third step of a 96-channel layer, EVERY step of a 32-channel one - and the step at the loop header waited
// `vmcnt(0)` right after it had ISSUED the next weight chunk's loads.  Here the range's metadata (gather rows, offsets) sits in LDS,
// a piece of PG_PIECE tiles at a time, so the steady state has no global load whose value is needed at once, and a step issues its
// requests (next weight chunk, the rows of step s + 2) BEHIND its first group of MFMAs, so whatever the compiler waits for at the top
// of a step was requested a whole step earlier.  Same tiles, same MFMA order per accumulator, same stores: the partial products are
// bit-identical to the old form's.  Measured (tools/r05_pair_ab.sh, profiles/EXPERIMENTS.md): -4 % on the 96-column layers of
// levels 0-1, -1...-3 % elsewhere - the other workgroup of the CU was already covering most of those waits.
#define PG_PIECE 24
// The step is written for few vector instructions (376 instead of ~2400 per 204 MFMAs at NT = 4; it bought ~1 %, which is how the round
// learned that instruction issue is not what bounds this kernel - profiles/EXPERIMENTS.md): the MFMA is issued transposed (A = weights, B = gathered rows: a lane owns one pair row and its accumulator groups are
// four consecutive columns - 4 NT `dwordx4` stores from ONE 64-bit address per tile instead of 16 NT dword stores with an index product
// each), the weight requests are a wave-uniform 64-bit base (scalar unit) + a per-thread 32-bit offset fixed for the launch, a gather
// request is one 64-bit multiply-add per step.
// MODE 0: partial products (pass 2 follows); 1: direct epilogue over out_idx (transposed convolutions); 2: dense rows (the identity as the
// rulebook: the U-Net's 1x1 convolutions, launch_pair_dense) - its own kernel symbols (`pair_dense_kernel_*`), so that a kernel trace lists
// the sparse convolutions the roofline counts apart from the 1x1s
template <int NT, int MODE>
__device__ __forceinline__ void pair_gemm_body(const PGParams& p, float (*Bs)[NT * 32 * PBS_LD], int* Ix, int* Kx) {
    constexpr bool DIRECT = MODE >= 1;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, h = lane >> 5;
    constexpr bool dense = MODE == 2;
    const int n_real = dense ? (int)((p.dense_rows + PT - 1) / PT) : p.tile_k[p.n_tiles];
    const int nchunks = p.Cin >> 5;
    // static part [0, n_static) in equal ranges, then the pool [n_static, n_real) in units of `unit` tiles (see g_pool_ctr above)
    // (not for the 32- / 64-channel layers: a unit of six one- or two-step tiles is shorter than the pipeline restart it costs - measured
    //  +12 % / +4 % on the level-1 32 -> 32 and level-2 64 -> 64 layers, -3 ... -5 % on the 96- ... 192-channel ones)
    const bool pool = p.pool_ctr != nullptr && nchunks >= 3 && n_real >= 6 * (int)gridDim.x;
    int n_static = n_real;
    // (13/16 static and units of six steps: the best of a sweep over 11 - 14 sixteenths x 4 - 12 steps, profiles/r05_pool_sweep.txt)
    const int unit = (6 + nchunks - 1) / nchunks;
    if (pool) {
        if (tid == 0) pool_claim(p.pool_ctr + blockIdx.y, p.pool_epoch);
        n_static = (int)((int64_t)n_real * 13 / 16);
        if (p.chained) while (n_static < n_real && (p.tile_k[n_static - 1] & PG_CHAIN)) ++n_static;
    }
    int range0 = (int)((int64_t)blockIdx.x * n_static / gridDim.x);
    int range1 = (int)((int64_t)(blockIdx.x + 1) * n_static / gridDim.x);
    if (p.chained) {                                           // a chain of sub-tiles (<= 3) is never split between workgroups
        while (range0 > 0 && range0 < n_static && (p.tile_k[range0 - 1] & PG_CHAIN)) ++range0;
        while (range1 > 0 && range1 < n_static && (p.tile_k[range1 - 1] & PG_CHAIN)) ++range1;
    }
    if (range1 <= range0 && !pool) return;                     // uniform over the workgroup
    const int ncol0 = blockIdx.y * NT * 32;
    __shared__ int pool_unit;
    bool poisoned = false;                                     // (uniform) this workgroup met a counter word no launch can have written
    int fallback_round = 0;
    const uint64_t wstride_b = (uint64_t)p.Cout * (uint64_t)p.Cin * 4ull;

    f32x16 acc[NT];
    const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    bool fresh = true;                                         // the next product starts a new tile (chain): its MFMA takes C = 0 instead of 16 NT register clears per tile

    // weight staging: thread f = tid + 256 i moves 16 bytes of row (f >> 3) of the chunk; its byte offset inside W[k] and its LDS slot
    // are fixed for the launch, the (offset, chunk) part of the address is wave-uniform
    f32x4 bst[NT];
    uint32_t woff[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        const int f = tid + i * 256;
        int n = ncol0 + (f >> 3);
        n = n < p.Cout ? n : p.Cout - 1;
        woff[i] = (uint32_t)(n * p.Cin + (f & 7) * 4) * 4u;
    }
    float* const sts = &Bs[0][(tid >> 3) * PBS_LD + (tid & 7) * 4];         // + i * 32 rows, + buf * buffer
    auto stage_load = [&](int kf, int chunk) {
        const int kw = p.k_flip >= 0 ? p.k_flip - (kf & PG_KMASK) : (kf & PG_KMASK);
        const char* Wk = (const char*)p.wt + (uint64_t)(uint32_t)kw * wstride_b + (uint32_t)chunk * 128u;    // scalar
#pragma unroll
        for (int i = 0; i < NT; ++i) bst[i] = *(const f32x4*)(Wk + woff[i]);
    };
    auto stage_store = [&](int buf) {
#pragma unroll
        for (int i = 0; i < NT; ++i) *(f32x4*)(sts + buf * (NT * 32 * PBS_LD) + i * 32 * PBS_LD) = bst[i];
    };
    const uint64_t lane_b = (uint64_t)(h * 64);                 // this lane's 16 channels of a 32-channel chunk
    auto load_a = [&](f32x4 (&a)[4], int row, int chunk) {      // branch-free: row >= 0 always (padding reads row 0)
        const int cc = chunk * 32;                              // wave-uniform from here ...
        const bool first = cc < p.C0;
        const char* base = (const char*)(first ? p.in0 : p.in1) + (uint32_t)(first ? cc : cc - p.C0) * 4u;
        const uint32_t ld4 = (uint32_t)(first ? p.ld0 : p.ld1) * 4u;
        const char* src = base + ((uint64_t)(uint32_t)row * ld4 + lane_b);                 // ... one 64-bit multiply-add per lane
#pragma unroll
        for (int q = 0; q < 4; ++q) a[q] = *(const f32x4*)(src + q * 16);
    };
    const bool full_cols = ncol0 + NT * 32 <= p.Cout;           // every layer of the shipped networks (Cout a multiple of 32 NT)

  for (;;) {                                                     // the static range, then pool units until the pool is empty
    for (int piece0 = range0; piece0 < range1; piece0 += PG_PIECE) {
        const int ntl = range1 - piece0 < PG_PIECE ? range1 - piece0 : PG_PIECE;
        __syncthreads();                                       // nobody still reads the previous piece's metadata / weight buffers
        if (dense) {
            for (int f = tid; f < ntl * PT; f += 256) {
                const int64_t r = (int64_t)piece0 * PT + f;
                Ix[f] = (int)(r < p.dense_rows ? r : p.dense_rows - 1);
            }
            if (tid < PG_PIECE + 2) Kx[tid] = 0;
        } else {
        for (int f = tid; f < ntl * PT; f += 256) {
            const int v = p.in_idx[(int64_t)piece0 * PT + f];
            Ix[f] = v < 0 ? 0 : v;                             // padding gathers row 0: its products are never read back
        }
        if (tid < PG_PIECE + 2) Kx[tid] = tid < ntl ? p.tile_k[piece0 + tid] : 0;
        }
        __syncthreads();
        const int nsteps = ntl * nchunks;
        const int* Iw = Ix + wv * 32 + j;                       // this lane's gather row of tile t: Iw[t * PT]
        int k_cur = __builtin_amdgcn_readfirstlane(Kx[0]), k_nxt = __builtin_amdgcn_readfirstlane(Kx[1]);
        f32x4 a0[4], a1[4], a2[4];
        int pf_t = 0, pf_c = 0;                                 // prefetch pointer = step s + 2
#define PF_ADVANCE() do { if (++pf_c == nchunks) { pf_c = 0; ++pf_t; } } while (0)
#define PF_ROW() Iw[(pf_t < ntl ? pf_t : ntl - 1) * PT]        /* past the end: a harmless reload of the last tile's row */
        load_a(a0, PF_ROW(), pf_c); PF_ADVANCE();
        load_a(a1, PF_ROW(), pf_c); PF_ADVANCE();
        stage_load(k_cur, 0);
        stage_store(0);
        __syncthreads();
        int buf = 0, cur_lt = 0, cur_c = 0, s = 0;
#define PAIR_STEP(CUR, PF)                                                                                            \
    {                                                                                                                 \
        const bool has_next = s + 1 < nsteps;                                                                         \
        const bool last_chunk = cur_c + 1 == nchunks;                                                                 \
        const int pf_row = PF_ROW();                /* LDS: asked for before the matrix work, used behind its first group */ \
        const int k_after = Kx[cur_lt + 2];                                                                           \
        {                                                                                                             \
            const float* bb = &Bs[buf][j * PBS_LD + h * 16];                                                          \
            f32x4 bq[2][NT];                                                                                          \
            _Pragma("unroll") for (int t = 0; t < NT; ++t) bq[0][t] = *(const f32x4*)(bb + t * 32 * PBS_LD);          \
            _Pragma("unroll") for (int q = 0; q < 4; ++q) {                                                           \
                if (q < 3) {                                                                                          \
                    _Pragma("unroll") for (int t = 0; t < NT; ++t)                                                    \
                        bq[(q + 1) & 1][t] = *(const f32x4*)(bb + t * 32 * PBS_LD + (q + 1) * 4);                     \
                }                                                                                                     \
                _Pragma("unroll") for (int e = 0; e < 4; ++e) {                                                       \
                    if (q == 0 && e == 0) {                                                                           \
                        if (fresh) {                                                                                  \
                            _Pragma("unroll") for (int t = 0; t < NT; ++t)                                            \
                                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(bq[0][t][0], CUR[0][0], zero16, 0, 0, 0); \
                        } else {                                                                                      \
                            _Pragma("unroll") for (int t = 0; t < NT; ++t)                                            \
                                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(bq[0][t][0], CUR[0][0], acc[t], 0, 0, 0); \
                        }                                                                                             \
                    } else {                                                                                          \
                        _Pragma("unroll") for (int t = 0; t < NT; ++t)                                                \
                            acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(bq[q & 1][t][e], CUR[q][e], acc[t], 0, 0, 0); \
                    }                                                                                                 \
                }                                                                                                     \
                __builtin_amdgcn_sched_barrier(0);                                                                    \
                if (q == 0) {   /* this step's requests, behind 4 NT MFMAs: next weight chunk first (consumed first) */ \
                    if (has_next) stage_load(last_chunk ? k_nxt : k_cur, last_chunk ? 0 : cur_c + 1);                 \
                    load_a(PF, pf_row, pf_c); PF_ADVANCE();                                                           \
                    __builtin_amdgcn_sched_barrier(0);                                                                \
                }                                                                                                     \
            }                                                                                                         \
        }                                                                                                             \
        if (last_chunk && !(k_cur & PG_CHAIN)) { /* tile (chain) complete: lane = pair row, register group g = columns 8g + 4h .. +3 */ \
            const int64_t prow = (int64_t)(piece0 + cur_lt) * PT + wv * 32 + j;                                       \
            if (DIRECT) {                                      /* one pair per output row: write the row itself */          \
                const int64_t o = dense ? (prow < p.dense_rows ? prow : -1) : (int64_t)p.out_idx[prow];               \
                if (o >= 0) {                                                                                         \
                    _Pragma("unroll") for (int t = 0; t < NT; ++t)                                                    \
                        _Pragma("unroll") for (int g = 0; g < 4; ++g) {                                               \
                            const int c = ncol0 + 4 * h + t * 32 + 8 * g;                                             \
                            if (full_cols || c < p.Cout) {                                                            \
                                f32x4 y;                                                                              \
                                _Pragma("unroll") for (int i = 0; i < 4; ++i) y[i] = pg_affine(acc[t][4 * g + i], p.scale, p.shift, c + i); \
                                if (p.res) y += *(const f32x4*)(p.res + o * p.ld_res + c);                            \
                                *(f32x4*)(p.out + o * p.ld_out + c) = f32x4{pg_act(y[0], p.act), pg_act(y[1], p.act), pg_act(y[2], p.act), pg_act(y[3], p.act)}; \
                            }                                                                                         \
                        }                                                                                             \
                }                                                                                                     \
            } else {                                                                                                  \
                float* dst = p.part + prow * p.Cout + ncol0 + 4 * h;                                                  \
                _Pragma("unroll") for (int t = 0; t < NT; ++t)                                                        \
                    _Pragma("unroll") for (int g = 0; g < 4; ++g)                                                     \
                        if (full_cols || ncol0 + 4 * h + t * 32 + 8 * g < p.Cout)                                     \
                            PART_STORE4(dst + t * 32 + 8 * g, (f32x4{acc[t][4 * g], acc[t][4 * g + 1],                \
                                                                     acc[t][4 * g + 2], acc[t][4 * g + 3]}));         \
            }                                                                                                         \
            fresh = true;                                                                                             \
        } else {                                                                                                      \
            fresh = false;                                                                                            \
        }                                                                                                             \
        if (!has_next) break;                                                                                         \
        stage_store(buf ^ 1);                                                                                         \
        __syncthreads();                                                                                              \
        buf ^= 1;                                                                                                     \
        ++s;                                                                                                          \
        if (last_chunk) {                                                                                             \
            cur_c = 0; ++cur_lt;                                                                                      \
            k_cur = k_nxt; k_nxt = __builtin_amdgcn_readfirstlane(k_after);                                           \
        } else {                                                                                                      \
            ++cur_c;                                                                                                  \
        }                                                                                                             \
    }
        for (;;) {
            PAIR_STEP(a0, a2)
            PAIR_STEP(a1, a0)
            PAIR_STEP(a2, a1)
        }
#undef PAIR_STEP
#undef PF_ADVANCE
#undef PF_ROW
    }
    if (!pool) break;
    __syncthreads();
    if (tid == 0) {
        unsigned int d = poisoned ? POOL_POISONED : pool_draw(p.pool_ctr + blockIdx.y, p.pool_epoch);
        if (d == POOL_POISONED) {                              // a foreign write in the slot: the pool is split statically, unit b, b + grid, ...
            if (!poisoned) atomicAdd(&g_pool_bad_seen, 1u);
            d = blockIdx.x + (unsigned)fallback_round * gridDim.x;
            pool_unit = -1 - (int)d;
        } else {
            pool_unit = (int)d;
        }
    }
    __syncthreads();
    int u = __builtin_amdgcn_readfirstlane(pool_unit);
    if (u < 0) { poisoned = true; ++fallback_round; u = -1 - u; }
    range0 = n_static + u * unit;
    if (range0 >= n_real) break;
    range1 = range0 + unit < n_real ? range0 + unit : n_real;
    if (p.chained) {                                           // the same snapping rule at both ends: the units tile the pool without gaps or overlaps
        while (range0 < n_real && (p.tile_k[range0 - 1] & PG_CHAIN)) ++range0;
        while (range1 < n_real && (p.tile_k[range1 - 1] & PG_CHAIN)) ++range1;
    }
  }
}

#define PAIR_GEMM_ENTRY(NAME, NT, WAVES, MODE)                                                                  \
    __global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(WAVES, WAVES))) void NAME(const PGParams p) { \
        __shared__ __attribute__((aligned(16))) float Bs[2][NT * 32 * PBS_LD];                                  \
        __shared__ int Ix[PG_PIECE * PT];                                                                       \
        __shared__ int Kx[PG_PIECE + 2];                                                                        \
        pair_gemm_body<NT, MODE>(p, Bs, Ix, Kx);                                                               \
    }
PAIR_GEMM_ENTRY(pair_gemm_kernel_1, 1, 3, 0)
PAIR_GEMM_ENTRY(pair_gemm_kernel_2, 2, 2, 0)
PAIR_GEMM_ENTRY(pair_gemm_kernel_3, 3, 2, 0)
PAIR_GEMM_ENTRY(pair_gemm_kernel_4, 4, 2, 0)
PAIR_GEMM_ENTRY(pair_gemm_direct_kernel_1, 1, 3, 1)
PAIR_GEMM_ENTRY(pair_gemm_direct_kernel_2, 2, 2, 1)
PAIR_GEMM_ENTRY(pair_gemm_direct_kernel_3, 3, 2, 1)
PAIR_GEMM_ENTRY(pair_gemm_direct_kernel_4, 4, 2, 1)
PAIR_GEMM_ENTRY(pair_dense_kernel_1, 1, 3, 2)
PAIR_GEMM_ENTRY(pair_dense_kernel_2, 2, 2, 2)
PAIR_GEMM_ENTRY(pair_dense_kernel_3, 3, 2, 2)
PAIR_GEMM_ENTRY(pair_dense_kernel_4, 4, 2, 2)

// ---- pass 1, weight-stationary variant ----------------------------------------------------------
// For layers whose whole W[k] (Cout x Cin fp32, Cout = 32*NT <= 128) fits in LDS next to a second
// workgroup: the workgroup stages W[k] ONCE per run of same-offset tiles and its four waves then walk
// their own 32-pair sub-tiles independently - no per-step barrier, no re-staging of weight chunks.
// The MFMA is issued transposed (A = weights, B = gathered rows) so a lane owns one pair row and its
// accumulator registers are 4-column groups: the partial products leave as dwordx4 stores.
#define WS_RANGE_TILES 24       // most tiles one workgroup may be given: its gather indices live in LDS (12 KB)
#define WS_STAGE_BATCH 16       // 16-byte weight requests per thread in flight while W[k] is staged

// (An inline-asm variant of the gather with hand-counted s_waitcnt vmcnt(N) was tried to keep two steps
// of loads in flight past hipcc's conservative waits: it was not faster - latency is not what limits this
// kernel - and the register copies the compiler places around asm outputs at the loop back-edge read
// registers with loads still in flight.  Plain loads it is.)
#define LOAD_A4(A, PTR)                                                                                            \
    do { _Pragma("unroll") for (int q_ = 0; q_ < 4; ++q_) A[q_] = *(const f32x4*)((PTR) + q_ * 4); } while (0)

// RT = 32-pair row tiles one wave multiplies per weight fragment.  RT = 4 / 2 for the narrow layers
// (Cout = 32 / 64; 4 independent accumulators per fragment read, epilogue amortised over 64 MFMAs per step)
// measured SLOWER than RT = 1 (stem 296 -> 333 us, 32->32 62 -> 72, 64->64 108 -> 121): those layers are
// bound by the gathers and partial stores per flop, not by the matrix pipe, and RT costs them half their
// resident waves.  All variants therefore run RT = 1.
template <int NT, int RT, int ST, bool DIRECT>
__device__ __forceinline__ void pair_gemm_ws_body(const PGParams& p, float* Ws) {   // no __restrict__: LDS shared across waves
    constexpr int UPT = 4 / RT;                                // wave units (RT x 32 pairs) per 128-pair tile
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform values must live in SGPRs (scalar branches)
    const int j = lane & 31, h = lane >> 5;
    const int n_real = p.tile_k[p.n_tiles];
    const int range0 = (int)((int64_t)blockIdx.x * n_real / gridDim.x);
    const int range1 = (int)((int64_t)(blockIdx.x + 1) * n_real / gridDim.x);
    if (range1 <= range0) return;
    const int nchunks = p.Cin >> 5;
    const int ldw = p.Cin + 4;                                 // (Cin + 4) mod 64 is 4 or 36: conflict-free b128 rows
    const int c4 = p.Cin >> 2;
    const int npieces = 32 * NT * c4;
    const int ncol0 = blockIdx.y * NT * 32;                    // column group (256-column layers run as two groups of 128)
    int* Ix = (int*)(Ws + 32 * NT * ldw);                      // gather rows of this workgroup's pairs; padding (-1) -> row 0

    f32x16 acc[RT][NT];
    const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    bool fresh = true;                                         // the next product starts a new unit: its MFMAs take C = 0 (no register clears: VALU time is matrix time here)

  // the range is walked in pieces whose gather indices fit the LDS buffer (the capacity-sized lists of a scene that
  // skipped the rulebook-size read-back can make a range longer than that)
  for (int tile0 = range0; tile0 < range1; tile0 += WS_RANGE_TILES) {
    const int ntl = range1 - tile0 < WS_RANGE_TILES ? range1 - tile0 : WS_RANGE_TILES;
    __syncthreads();                                           // nobody still reads the previous piece's indices
    for (int f = tid; f < ntl * PT; f += 256) {
        const int v = p.in_idx[(int64_t)(tile0 + (f >> 7)) * PT + (f & (PT - 1))];
        Ix[f] = v < 0 ? 0 : v;                                 // their partial products are never read back
    }
    int run_start = 0;
    while (run_start < ntl) {                                  // runs of tiles with the same offset (uniform)
        const int k = p.tile_k[(tile0 + run_start)];
        int run_end = run_start + 1;
        while (run_end < ntl && p.tile_k[(tile0 + run_end)] == k) ++run_end;
        __syncthreads();                                       // everyone is done reading the previous W (and Ix is written)
        {
            const float* __restrict__ W = p.wt + ((int64_t)(p.k_flip >= 0 ? p.k_flip - k : k) * p.Cout + ncol0) * p.Cin;
            // sixteen requests per thread in flight (four before round 5): staging W[k] was 4 - 8 dependent L2 round trips of ~1.5 us before
            // a workgroup's first MFMA - a fifth of a level-3 128 -> 128 launch, where a workgroup has 3.5 tiles.  Unconditional loads
            // (clamped), conditional LDS writes: no exec-masked load for the compiler to wait on.
            constexpr int SB = (NT == 1 || NT == 3) ? WS_STAGE_BATCH / 2 : WS_STAGE_BATCH;    // (the 3- and 4-waves-per-SIMD variants have 128 / 168 registers)
            for (int f0 = 0; f0 < npieces; f0 += 256 * SB) {
                f32x4 v[SB];
#pragma unroll
                for (int u = 0; u < SB; ++u) {
                    const int f = f0 + u * 256 + tid;
                    v[u] = *(const f32x4*)(W + (int64_t)(f < npieces ? f : npieces - 1) * 4);
                }
#pragma unroll
                for (int u = 0; u < SB; ++u) {
                    const int f = f0 + u * 256 + tid;
                    if (f < npieces) {
                        const int row = f / c4, col = f - row * c4;
                        *(f32x4*)(Ws + row * ldw + col * 4) = v[u];
                    }
                }
            }
        }
        __syncthreads();
        // this wave's units of the run: local unit numbers u0, u0 + 4, ...
        const int u0 = run_start * UPT + wv;
        const int ns = (run_end * UPT - u0 + 3) / 4;
        const int nsteps = ns * nchunks;
        if (nsteps > 0) {
            // fragments of step (unit i, chunk c); past the end -> unit 0 (harmless reload)
            auto load_unit = [&](f32x4 (&A)[RT][4], int i, int c) {
                const int ii = i < ns ? i : 0;
                const int cc = c * 32;                          // wave-uniform
                const bool first = cc < p.C0;
                const float* base = first ? p.in0 : p.in1;
                const int ld = first ? p.ld0 : p.ld1;
                const int coff = (first ? cc : cc - p.C0) + h * 16;
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) {
                    const int row = Ix[((u0 + 4 * ii) * RT + rt) * 32 + j];
                    const float* q = base + (int64_t)row * ld + coff;
                    LOAD_A4(A[rt], q);
                }
            };
            // ST register stages: the rows of step s + ST - 1 are requested while step s multiplies.  The ring is
            // rotated by unrolling the loop ST times with the roles renamed (copying a stage would make the
            // compiler wait for the loads still in flight into it).  Narrow layers are latency-bound and want
            // ST = 3-4; the 96/128-column variants are better off with the registers (ST = 2).
            f32x4 a0[RT][4], a1[RT][4], a2[RT][4], a3[RT][4];
            int pf_i = 0, pf_c = 0;
#define WS_PF_ADVANCE() do { if (++pf_c == nchunks) { pf_c = 0; ++pf_i; } } while (0)
            load_unit(a0, pf_i, pf_c); WS_PF_ADVANCE();
            if (ST >= 3) { load_unit(a1, pf_i, pf_c); WS_PF_ADVANCE(); }
            if (ST >= 4) { load_unit(a2, pf_i, pf_c); WS_PF_ADVANCE(); }
            int cur_i = 0, cur_c = 0, s = 0;
#define WS_STEP(CUR, PF)                                                                                              \
    {                                                                                                                 \
        const bool last_chunk = cur_c + 1 == nchunks;                                                                 \
        load_unit(PF, pf_i, pf_c); WS_PF_ADVANCE();             /* next step's rows while this one multiplies */      \
        {                                                                                                             \
            const float* wb = Ws + j * ldw + cur_c * 32 + h * 16;                                                     \
            f32x4 wq[2][NT];                                                                                          \
            _Pragma("unroll") for (int t = 0; t < NT; ++t) wq[0][t] = *(const f32x4*)(wb + t * 32 * ldw);             \
            _Pragma("unroll") for (int q = 0; q < 4; ++q) {                                                           \
                if (q < 3) {                                                                                          \
                    _Pragma("unroll") for (int t = 0; t < NT; ++t)                                                    \
                        wq[(q + 1) & 1][t] = *(const f32x4*)(wb + t * 32 * ldw + (q + 1) * 4);                        \
                }                                                                                                     \
                _Pragma("unroll") for (int e = 0; e < 4; ++e) {                                                       \
                    if (q == 0 && e == 0 && fresh) {                                                                  \
                        _Pragma("unroll") for (int t = 0; t < NT; ++t)                                                \
                            _Pragma("unroll") for (int rt = 0; rt < RT; ++rt)                                         \
                                acc[rt][t] = __builtin_amdgcn_mfma_f32_32x32x2f32(wq[0][t][0], CUR[rt][0][0], zero16, 0, 0, 0); \
                    } else {                                                                                          \
                        _Pragma("unroll") for (int t = 0; t < NT; ++t)                                                \
                            _Pragma("unroll") for (int rt = 0; rt < RT; ++rt)                                         \
                                acc[rt][t] = __builtin_amdgcn_mfma_f32_32x32x2f32(wq[q & 1][t][e], CUR[rt][q][e],     \
                                                                                  acc[rt][t], 0, 0, 0);               \
                    }                                                                                                 \
                }                                                                                                     \
                __builtin_amdgcn_sched_barrier(0);                                                                    \
            }                                                                                                         \
        }                                                                                                             \
        if (last_chunk) { /* unit complete: lane = pair row, register group g = columns 8g + 4h .. +3 */              \
            _Pragma("unroll") for (int rt = 0; rt < RT; ++rt) {                                                       \
                const int ue = (u0 + 4 * cur_i) * RT + rt;          /* 32-pair unit of the piece: tile ue / 4, quarter ue % 4 */ \
                const int64_t prow = (int64_t)(tile0 + (ue >> 2)) * PT + (ue & 3) * 32 + j;                       \
                if (DIRECT) {                                       /* one pair per output row: write the row itself */ \
                    const int64_t o = p.out_idx[prow];                                                                \
                    if (o >= 0) {                                                                                     \
                        _Pragma("unroll") for (int t = 0; t < NT; ++t)                                                \
                            _Pragma("unroll") for (int g = 0; g < 4; ++g) {                                           \
                                const int c = ncol0 + 4 * h + t * 32 + 8 * g;                                         \
                                f32x4 y;                                                                              \
                                _Pragma("unroll") for (int i = 0; i < 4; ++i) y[i] = pg_affine(acc[rt][t][4 * g + i], p.scale, p.shift, c + i); \
                                if (p.res) y += *(const f32x4*)(p.res + o * p.ld_res + c);                            \
                                *(f32x4*)(p.out + o * p.ld_out + c) = f32x4{pg_act(y[0], p.act), pg_act(y[1], p.act), pg_act(y[2], p.act), pg_act(y[3], p.act)}; \
                            }                                                                                         \
                    }                                                                                                 \
                } else {                                                                                              \
                float* dst = p.part + prow * p.Cout + ncol0 + 4 * h;                                                  \
                _Pragma("unroll") for (int t = 0; t < NT; ++t)                                                        \
                    _Pragma("unroll") for (int g = 0; g < 4; ++g)                                                     \
                        PART_STORE4(dst + t * 32 + 8 * g, (f32x4{acc[rt][t][4 * g], acc[rt][t][4 * g + 1],            \
                                                                 acc[rt][t][4 * g + 2], acc[rt][t][4 * g + 3]}));     \
                }                                                                                                     \
            }                                                                                                         \
        }                                                                                                             \
        fresh = last_chunk;                                                                                           \
        if (s + 1 >= nsteps) break;                                                                                   \
        ++s;                                                                                                          \
        if (last_chunk) { cur_c = 0; ++cur_i; } else { ++cur_c; }                                                     \
    }
            if (ST == 2) {
                for (;;) {
                    WS_STEP(a0, a1)
                    WS_STEP(a1, a0)
                }
            } else if (ST == 3) {
                for (;;) {
                    WS_STEP(a0, a2)
                    WS_STEP(a1, a0)
                    WS_STEP(a2, a1)
                }
            } else {
                for (;;) {
                    WS_STEP(a0, a3)
                    WS_STEP(a1, a0)
                    WS_STEP(a2, a1)
                    WS_STEP(a3, a2)
                }
            }
#undef WS_STEP
#undef WS_PF_ADVANCE
        }
        run_start = run_end;
    }
  }
}

#define PAIR_GEMM_WS_ENTRY(NAME, NT, RT, ST, WAVES, DIRECT)                                                        \
    __global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(WAVES, WAVES))) void NAME(const PGParams p) { \
        extern __shared__ __attribute__((aligned(16))) float ws_smem[];                                            \
        pair_gemm_ws_body<NT, RT, ST, DIRECT>(p, ws_smem);                                                         \
    }
PAIR_GEMM_WS_ENTRY(pair_gemm_ws_kernel_1, 1, 1, 3, 4, false)
PAIR_GEMM_WS_ENTRY(pair_gemm_ws_kernel_2, 2, 1, 3, 2, false)
PAIR_GEMM_WS_ENTRY(pair_gemm_ws_kernel_3, 3, 1, 2, 3, false)
PAIR_GEMM_WS_ENTRY(pair_gemm_ws_kernel_4, 4, 1, 2, 2, false)
PAIR_GEMM_WS_ENTRY(pair_gemm_ws_direct_kernel_1, 1, 1, 3, 4, true)
PAIR_GEMM_WS_ENTRY(pair_gemm_ws_direct_kernel_2, 2, 1, 3, 2, true)
PAIR_GEMM_WS_ENTRY(pair_gemm_ws_direct_kernel_3, 3, 1, 2, 3, true)
PAIR_GEMM_WS_ENTRY(pair_gemm_ws_direct_kernel_4, 4, 1, 2, 2, true)

// ---- pass 2: fixed-order reduction over the offsets + epilogue --------------------------------
struct PRParams {
    const int32_t* pos; int K; int64_t M;
    const float* part; int Cout;
    const float* scale; const float* shift;
    const float* res; int ld_res;
    float* out; int ld_out; int act;
};

__global__ __launch_bounds__(256) void pair_reduce_kernel(const PRParams p) {
    const int c4 = p.Cout >> 2;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t r = e / c4;
    if (r >= p.M) return;
    const int q = (int)(e - r * c4) * 4;
    f32x4 a = {0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < p.K; k0 += 8) {
        int ids[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) ids[u] = (k0 + u < p.K) ? p.pos[(int64_t)(k0 + u) * p.M + r] : -1;
        f32x4 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u)
            v[u] = ids[u] >= 0 ? *(const f32x4*)(p.part + (int64_t)ids[u] * p.Cout + q) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (ids[u] >= 0) a += v[u];
    }
    float y[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int n = q + i;
        float t = pg_affine(a[i], p.scale, p.shift, n);
        if (p.res) t += p.res[r * p.ld_res + n];
        y[i] = pg_act(t, p.act);
    }
    *(f32x4*)(p.out + r * p.ld_out + q) = f32x4{y[0], y[1], y[2], y[3]};
}

// ---- pass 2 over the per-row lists ---------------------------------------------------------------
// The same fixed-order sum, but a row walks ITS OWN partial products {count, positions...} (pair_rowlist_batch_kernel) instead of
// all K slots of pos[k][r]: one 16-byte load brings the count and the first three positions.
struct PRLParams {
    const int32_t* rlist; int rl_stride; int64_t M;
    const float* part; int Cout;
    const float* scale; const float* shift;
    const float* res; int ld_res;
    float* out; int ld_out; int act;
};

__global__ __launch_bounds__(256) void pair_reduce_rl_kernel(const PRLParams p) {
    const int c4 = p.Cout >> 2;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t r = e / c4;
    if (r >= p.M) return;
    const int q = (int)(e - r * c4) * 4;
    const int32_t* rl = p.rlist + r * p.rl_stride;
    // the row's whole list in registers first (7 x 16 bytes cover count + 27 positions: every 3^3 table), then the partial
    // products eight at a time: two short dependent steps instead of a position -> product chain per group of four
    int4 hv[7];
    hv[0] = *(const int4*)rl;
    const int cnt = hv[0].x;
#pragma unroll
    for (int g = 1; g < 7; ++g) hv[g] = (4 * g <= cnt) ? *(const int4*)(rl + 4 * g) : int4{0, 0, 0, 0};
    auto id_at = [&](int i) -> int {                            // list entry i (< 27) = int 1 + i of the row; compile-time i after unrolling
        const int4& v = hv[(1 + i) >> 2];
        const int c = (1 + i) & 3;
        return c == 0 ? v.x : (c == 1 ? v.y : (c == 2 ? v.z : v.w));
    };
    f32x4 a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i0 = 0; i0 < 27; i0 += 9) {
        if (i0 < cnt) {
            f32x4 v[9];
#pragma unroll
            for (int u = 0; u < 9; ++u)
                v[u] = i0 + u < cnt ? PART_LOAD4(p.part + (int64_t)id_at(i0 + u) * p.Cout + q) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int u = 0; u < 9; ++u) if (i0 + u < cnt) a += v[u];
        }
    }
    for (int i0 = 27; i0 < cnt; i0 += 4) {                      // longer lists (the 5^3 stem): four at a time from memory (int 1 + 27 = 28: 16-byte aligned)
        const int4 ids = *(const int4*)(rl + 1 + i0);
        f32x4 v[4];
        const int idv[4] = {ids.x, ids.y, ids.z, ids.w};
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = i0 + u < cnt ? PART_LOAD4(p.part + (int64_t)idv[u] * p.Cout + q) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int u = 0; u < 4; ++u) if (i0 + u < cnt) a += v[u];
    }
    float y[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int n = q + i;
        float t = pg_affine(a[i], p.scale, p.shift, n);
        if (p.res) t += p.res[r * p.ld_res + n];
        y[i] = pg_act(t, p.act);
    }
    *(f32x4*)(p.out + r * p.ld_out + q) = f32x4{y[0], y[1], y[2], y[3]};
}

// ---- the shared tail's host side ------------------------------------------------------------------
static std::atomic<unsigned long long*> g_pool_bases[SD3D_MAX_DEVICES];
static std::atomic<unsigned long long> g_pool_tickets[SD3D_MAX_DEVICES];        // pooled launches handed out so far, per device
static std::atomic<int> g_pool_on{-1};                                         // -1: not decided yet (SD3D_PAIR_POOL, default 1)
static bool pool_enabled() {
    int v = g_pool_on.load(std::memory_order_relaxed);
    if (v < 0) {
        const char* e = getenv("SD3D_PAIR_POOL");
        v = e ? (atoi(e) != 0) : 1;
        int expected = -1;
        g_pool_on.compare_exchange_strong(expected, v);
        v = g_pool_on.load(std::memory_order_relaxed);
    }
    return v != 0;
}
extern "C" int sd3d_set_pair_pool(int on) {
    const int prev = pool_enabled() ? 1 : 0;
    g_pool_on.store(on ? 1 : 0, std::memory_order_relaxed);
    return prev;
}
// Number of counter words of the current device's ring in a state no sequence of finished launches leaves behind (an epoch the host has
// not handed out for that slot, or anything in a slot no launch has used) + the workgroups that met such a word since the last call (they
// fell back to a static split of their pool: the results are unaffected, the event is reported here and through sd3d_last_error);
// 0 is the healthy answer.  Synchronises the device.  < 0: error.
extern "C" int sd3d_pair_pool_check(void) {
    const int dev = sd3d_device();
    if (dev < 0) { sd3d_set_error(SD3D_ERR_LAUNCH, "pair_pool_check: no device"); return -1; }
    if (hipDeviceSynchronize() != hipSuccess) { sd3d_set_error(SD3D_ERR_LAUNCH, "pair_pool_check: device synchronisation failed"); return -1; }
    unsigned int zero = 0, bad = 0, seen = 0;
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_pool_bad), &zero, sizeof(zero)) != hipSuccess) { sd3d_set_error(SD3D_ERR_LAUNCH, "pair_pool_check: symbol write failed"); return -1; }
    hipLaunchKernelGGL(pool_check_kernel, dim3(PG_POOL_SLOTS / 256), dim3(256), 0, nullptr, g_pool_tickets[dev].load(std::memory_order_relaxed));
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
        hipMemcpyFromSymbol(&bad, HIP_SYMBOL(g_pool_bad), sizeof(bad)) != hipSuccess ||
        hipMemcpyFromSymbol(&seen, HIP_SYMBOL(g_pool_bad_seen), sizeof(seen)) != hipSuccess ||
        hipMemcpyToSymbol(HIP_SYMBOL(g_pool_bad_seen), &zero, sizeof(zero)) != hipSuccess) { sd3d_set_error(SD3D_ERR_LAUNCH, "pair_pool_check: check kernel failed"); return -1; }
    if (seen) sd3d_set_error(SD3D_ERR_LAUNCH, "pair_pool_check: launches met counter words no launch can have written (they fell back to a static split of their shared tail: results unaffected)");
    bad += seen;                                               // (workgroups that fell back since the last check)
    return (int)bad;
}
// pooled launches so far on the current device (tests: did the pool really run?)
extern "C" int sd3d_pair_pool_launches(int64_t* launches_out) {
    const int dev = sd3d_device();
    if (!launches_out || dev < 0) return sd3d_set_error(SD3D_ERR_ARG, "pair_pool_launches: no device / no output");
    *launches_out = (int64_t)g_pool_tickets[dev].load(std::memory_order_relaxed);
    return SD3D_OK;
}
// Test hook: overwrite the whole ring of the current device with `word` (a launch that died half-way, a foreign write) and forget
// nothing else - the next pooled launches must still produce the same bits (tests/test_gpu_pair_paths.py).
extern "C" int sd3d_pair_pool_poison(int64_t word) {
    unsigned long long* base = nullptr;
    if (hipGetSymbolAddress((void**)&base, HIP_SYMBOL(g_pool_ctr)) != hipSuccess) return sd3d_set_error(SD3D_ERR_LAUNCH, "pair_pool_poison: no symbol");
    std::vector<unsigned long long> h((size_t)PG_POOL_SLOTS * PG_POOL_WORDS, (unsigned long long)word);
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(base, h.data(), h.size() * sizeof(unsigned long long), hipMemcpyHostToDevice) != hipSuccess)
        return sd3d_set_error(SD3D_ERR_LAUNCH, "pair_pool_poison: copy failed");
    return SD3D_OK;
}

// ---- launchers --------------------------------------------------------------------------------
// pass-1 kernels by variant, indexed by [direct epilogue][nt - 1]
typedef void (*PGKernel)(const PGParams);
static const PGKernel k_lockstep[2][4] = {{pair_gemm_kernel_1, pair_gemm_kernel_2, pair_gemm_kernel_3, pair_gemm_kernel_4},
                                          {pair_gemm_direct_kernel_1, pair_gemm_direct_kernel_2, pair_gemm_direct_kernel_3, pair_gemm_direct_kernel_4}};
static const PGKernel k_ws[2][4] = {{pair_gemm_ws_kernel_1, pair_gemm_ws_kernel_2, pair_gemm_ws_kernel_3, pair_gemm_ws_kernel_4},
                                    {pair_gemm_ws_direct_kernel_1, pair_gemm_ws_direct_kernel_2, pair_gemm_ws_direct_kernel_3, pair_gemm_ws_direct_kernel_4}};
static const PGKernel k_dense[4] = {pair_dense_kernel_1, pair_dense_kernel_2, pair_dense_kernel_3, pair_dense_kernel_4};

static std::atomic<int> g_n_cu[SD3D_MAX_DEVICES];                                // CU count per device, 0: not asked yet
static Sd3dLdsRaised g_ws_raised;                                              // the weight-stationary kernels' LDS limit, 80 KB (160 KB at nt = 4)
#define WS_LDS(d, i) {(const void*)k_ws[d][i], (i == 3 ? 160 : 80) * 1024}
static const Sd3dLdsKernel k_ws_lds[8] = {WS_LDS(0, 0), WS_LDS(0, 1), WS_LDS(0, 2), WS_LDS(0, 3), WS_LDS(1, 0), WS_LDS(1, 1), WS_LDS(1, 2), WS_LDS(1, 3)};
#undef WS_LDS

// the current device (the index of its per-device state) and its CU count; -1: no usable device
static int pg_device(int* n_cu) {
    const int dev = sd3d_device();
    if (dev < 0) return -1;
    int n = g_n_cu[dev].load(std::memory_order_relaxed);
    if (!n) {
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) return -1;
        g_n_cu[dev].store(n, std::memory_order_relaxed);
    }
    *n_cu = n;
    return dev;
}

// column tiling of a pass-1 launch: nt 32-column tiles per workgroup (1 - 4), cgs column groups of 32 nt columns
static void pg_col_tiles(int Cout, int* nt_out, int* cgs_out) {
    const int sub = (Cout + 31) / 32;
    int nt = sub >= 4 ? 4 : sub;
    if (sub > 4 && sub % 4) { for (int c = 4; c >= 1; --c) if (sub % c == 0) { nt = c; break; } }
    *nt_out = nt;
    *cgs_out = (int)cdiv(sub, nt);
}

// lock-step kernel: 3 workgroups per CU at nt = 1, 2 otherwise, never more than there are tiles
static dim3 pg_lockstep_grid(int n_cu, int nt, int cgs, int64_t tiles) {
    int gx = n_cu * (nt == 1 ? 3 : 2) / cgs;
    gx = gx < 1 ? 1 : (gx < tiles ? gx : (int)tiles);
    return dim3((unsigned)gx, (unsigned)cgs);
}

// a slot of the shared tail for a lock-step launch on device `dev`; g.pool_ctr stays NULL (static partition) when the pool is off
// (sd3d_set_pair_pool / SD3D_PAIR_POOL=0: every tile dealt out statically, rounds 1-4), the launch has more than PG_POOL_WORDS column
// groups, or the stream is being captured.  (The counters are a per-device symbol: a process that drives several GPUs gets each
// device's own address and its own tickets.)
static void pg_setup_pool(PGParams& g, int dev, int cgs, hipStream_t st) {
    if (!pool_enabled() || cgs > PG_POOL_WORDS) return;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (st != nullptr && (hipStreamIsCapturing(st, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone)) return;
    unsigned long long* base = g_pool_bases[dev].load(std::memory_order_acquire);
    if (!base && hipGetSymbolAddress((void**)&base, HIP_SYMBOL(g_pool_ctr)) == hipSuccess) g_pool_bases[dev].store(base, std::memory_order_release);
    if (!base) return;
    const unsigned long long t = g_pool_tickets[dev].fetch_add(1, std::memory_order_relaxed);
    g.pool_ctr = base + (size_t)(t % PG_POOL_SLOTS) * PG_POOL_WORDS;
    g.pool_epoch = (unsigned int)(t / PG_POOL_SLOTS + 1);
}

// rlist / rl_stride / center / out_idx: optional products of sd3d_pair_lists_desc (NULL / -1: the round-1 path, pass 1 over all
// offsets + pair_reduce_kernel over pos).  out_idx != NULL promises ONE pair per output row (transposed k2s2 convolution).
int launch_pair_conv(const float* in0, int ld0, int C0, const float* in1, int ld1, const int32_t* in_idx, const int32_t* tile_k,
                     int64_t p_cap, const int32_t* pos, const int32_t* rlist, int rl_stride, int center, const int32_t* out_idx,
                     const float* wt, int K, int Cin, int Cout, int64_t M, const float* scale,
                     const float* shift, const float* res, int ld_res, float* out, int ld_out, int act, float* part,
                     size_t part_bytes, hipStream_t st) {
    if (M <= 0 || Cout <= 0) return SD3D_OK;
    if (Cin <= 0 || (Cin & 31)) return sd3d_set_error(SD3D_ERR_ARG, "pair_conv: Cin must be a positive multiple of 32");
    if (Cout & 3) return sd3d_set_error(SD3D_ERR_ARG, "pair_conv: Cout must be a multiple of 4");
    if (in1 && ((C0 & 31) || C0 > Cin)) return sd3d_set_error(SD3D_ERR_ARG, "pair_conv: concat split must be a multiple of 32");
    if (!in1) C0 = Cin;
    if ((ld0 & 3) || (in1 && (ld1 & 3)) || (ld_out & 3)) return sd3d_set_error(SD3D_ERR_ARG, "pair_conv: row strides must be multiples of 4 floats");
    if (p_cap <= 0 || (p_cap % PT)) return sd3d_set_error(SD3D_ERR_ARG, "pair_conv: p_cap must be a positive multiple of 128");
    if (part_bytes < (size_t)p_cap * Cout * sizeof(float)) return sd3d_set_error(SD3D_ERR_ARG, "pair_conv: partial-product buffer too small");
    int n_cu = 0;
    const int dev = pg_device(&n_cu);
    if (dev < 0) return sd3d_set_error(SD3D_ERR_LAUNCH, "pair_conv: no device");
    if ((ld_res & 3) && res) return sd3d_set_error(SD3D_ERR_ARG, "pair_conv: residual row stride must be a multiple of 4 floats");
    const bool mirror_w = center == SD3D_PAIR_MIRROR_W(-1) || center == SD3D_PAIR_MIRROR_W(SD3D_PAIR_CHAINED);
    if (mirror_w) center += 2;
    if (center >= 0 || center < SD3D_PAIR_CHAINED) return sd3d_set_error(SD3D_ERR_ARG, "pair_conv: center must be -1 or SD3D_PAIR_CHAINED, or SD3D_PAIR_MIRROR_W of them (the dense centre kernel of round 3 left the library: profiles/EXPERIMENTS.md)");
    const bool direct = out_idx != nullptr;
    // (lean evaluation tables carry no position table, 'up' tables no row lists: for a C caller that passes neither, pass 2 would walk
    //  pos == NULL - refuse before anything is launched.  ADVICE r5)
    if (!direct && !rlist && !pos)
        return sd3d_set_error(SD3D_ERR_ARG, "pair_conv: pass 2 needs rlist, or pos, or out_idx (direct epilogue); "
                                            "this table was built without a position table (lean evaluation lists)");
    const bool crowded = g_scenes_in_flight.load(std::memory_order_relaxed) > 1;
    PGParams g;
    g.in0 = in0; g.ld0 = ld0; g.C0 = C0; g.in1 = in1; g.ld1 = ld1; g.in_idx = in_idx; g.tile_k = tile_k; g.wt = wt;
    g.Cin = Cin; g.Cout = Cout; g.part = part;
    g.chained = center == SD3D_PAIR_CHAINED ? 1 : 0;
    g.nt_part = crowded ? 1 : 0;                               // (see PART_STORE4)
    g.dense_rows = 0;
    g.pool_ctr = nullptr;
    g.pool_epoch = 0;
    g.k_flip = mirror_w ? K - 1 : -1;
    g.out_idx = out_idx;
    g.scale = scale; g.shift = shift; g.res = res; g.ld_res = ld_res; g.out = out; g.ld_out = ld_out; g.act = act;
    int nt, cgs;
    pg_col_tiles(Cout, &nt, &cgs);
    g.n_tiles = (int)(p_cap / PT);
    // weight-stationary variant: Cout = 32 * nt <= 128 and W[k] (padded rows) <= 68 KB of LDS
    const size_t w_lds = (size_t)Cout * (Cin + 4) * sizeof(float);
    const size_t w_lds_cg = (size_t)(32 * nt) * (Cin + 4) * sizeof(float);       // one column group's share of W[k]
    // several scenes in flight: the 96 / 128-column weight-stationary variants (47-63 KB of LDS per workgroup, 2-3 per CU) leave
    // no room for the other scenes' kernels; measured with 4 scenes in flight 107 -> 112 scenes/s without them, while alone on the
    // GPU they are 0.3 ms per forward faster.
    const bool ws_one = !g.chained && !(crowded && nt >= 3) && cgs == 1 && Cout == 32 * nt && w_lds <= 68 * 1024;
    // wide layers (256 columns = two groups of 128): the group's half of W[k] (133 KB at Cin = 256) still fits LDS with ONE
    // workgroup per CU - no per-step barrier, no re-staging of weight chunks, like the narrow layers
    // (measured: level-3 256->256, 1808 tiles: 358 -> 347 us; level-4, 472 tiles: 104 -> 113 us - too few tiles for half the workgroups)
    const bool ws_two = !g.chained && !crowded && cgs == 2 && nt == 4 && Cout == 256 && g.n_tiles >= 1024 && w_lds_cg + WS_RANGE_TILES * PT * sizeof(int32_t) + 256 <= 160 * 1024;
    if (ws_one || ws_two) {
        if (int rc = sd3d_raise_lds_limit(g_ws_raised, k_ws_lds, 8, dev)) return rc;
        // resident workgroups per CU: the pinned register budgets allow 4 / 3 / 3 / 2; LDS (160 KB) may allow fewer
        int per_cu = nt == 1 ? 4 : (nt == 3 ? 3 : 2);
        const size_t w_need = ws_two ? w_lds_cg : w_lds;
        const int by_lds = (int)((160 * 1024) / (w_need + WS_RANGE_TILES * PT * sizeof(int32_t) + 256));
        per_cu = per_cu < by_lds ? per_cu : by_lds;
        int gx = n_cu * per_cu / (ws_two ? 2 : 1);
        gx = gx < 1 ? 1 : (gx < g.n_tiles ? gx : g.n_tiles);
        const size_t lds = w_need + (size_t)WS_RANGE_TILES * PT * sizeof(int32_t);
        hipLaunchKernelGGL(k_ws[direct][nt - 1], dim3((unsigned)gx, ws_two ? 2u : 1u), dim3(256), lds, st, g);
    } else {
        pg_setup_pool(g, dev, cgs, st);
        hipLaunchKernelGGL(k_lockstep[direct][nt - 1], pg_lockstep_grid(n_cu, nt, cgs, g.n_tiles), dim3(256), 0, st, g);
    }
    if (direct) {                                              // pass 1 wrote the output rows
    } else if (rlist) {
        PRLParams r;
        r.rlist = rlist; r.rl_stride = rl_stride; r.M = M; r.part = part; r.Cout = Cout; r.scale = scale; r.shift = shift; r.res = res;
        r.ld_res = ld_res; r.out = out; r.ld_out = ld_out; r.act = act;
        hipLaunchKernelGGL(pair_reduce_rl_kernel, dim3((unsigned)cdiv(M * (Cout / 4), 256)), dim3(256), 0, st, r);
    } else {
        PRParams r;
        r.pos = pos; r.K = K; r.M = M; r.part = part; r.Cout = Cout; r.scale = scale; r.shift = shift; r.res = res; r.ld_res = ld_res;
        r.out = out; r.ld_out = ld_out; r.act = act;
        hipLaunchKernelGGL(pair_reduce_kernel, dim3((unsigned)cdiv(M * (Cout / 4), 256)), dim3(256), 0, st, r);
    }
    SD3D_CHECK_LAUNCH();
    return SD3D_OK;
}
extern "C" int sd3d_pair_conv_ex(const float* in0, int ld0, int C0, const float* in1, int ld1, const int32_t* in_idx, const int32_t* tile_k,
                                 int64_t p_cap, const int32_t* pos, const int32_t* rlist, int rl_stride, int center, const int32_t* out_idx,
                                 const float* wt, int K, int Cin, int Cout, int64_t M, const float* scale, const float* shift, const float* res,
                                 int ld_res, float* out, int ld_out, int act, float* part, size_t part_bytes, void* stream) {
    return launch_pair_conv(in0, ld0, C0, in1, ld1, in_idx, tile_k, p_cap, pos, rlist, rl_stride, center, out_idx, wt, K, Cin, Cout, M,
                            scale, shift, res, ld_res, out, ld_out, act, part, part_bytes, (hipStream_t)stream);
}

// A dense [M, Cin] x W^T product (+ scale / shift / residual / activation) on the pass-1 kernel: the 1x1 convolutions of the U-Net
// (BasicBlockBase.downsample, minkunet.py:314-328) on tens of thousands of rows.  The one-tile-per-workgroup kernel of gather_gemm.hip
// spends most of such a launch on its prologue and epilogue (Cin / 32 = 4 - 12 steps per workgroup: 49 TFLOP/s at level 0); here a
// persistent workgroup walks its share of the 128-row tiles through the same software pipeline as the sparse convolutions, the
// "rulebook" being the identity (no lists are read) and the epilogue writing the output rows themselves.
int launch_pair_dense(const GGParams& q, hipStream_t st) {
    int n_cu = 0;
    if (pg_device(&n_cu) < 0) return sd3d_set_error(SD3D_ERR_LAUNCH, "pair_dense: no device");
    PGParams g;
    g.in0 = q.in0; g.ld0 = q.ld0; g.C0 = q.in1 ? q.C0 : q.Cin; g.in1 = q.in1; g.ld1 = q.ld1; g.in_idx = nullptr; g.tile_k = nullptr; g.wt = q.wt;
    g.Cin = q.Cin; g.Cout = q.Cout; g.part = nullptr; g.n_tiles = 0; g.out_idx = nullptr; g.scale = q.scale; g.shift = q.shift; g.res = q.res;
    g.ld_res = q.ld_res; g.out = q.out; g.ld_out = q.ld_out; g.act = q.act; g.nt_part = 0; g.chained = 0; g.dense_rows = q.M; g.pool_ctr = nullptr; g.pool_epoch = 0; g.k_flip = -1;
    int nt, cgs;
    pg_col_tiles(q.Cout, &nt, &cgs);
    hipLaunchKernelGGL(k_dense[nt - 1], pg_lockstep_grid(n_cu, nt, cgs, cdiv(q.M, PT)), dim3(256), 0, st, g);
    SD3D_CHECK_LAUNCH();
    return SD3D_OK;
}
