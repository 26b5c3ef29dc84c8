/*
 * segdino3d_hip.h - C ABI of the MI355X-native (gfx950) SegDINO3D forward path.
 *
 * This is the drop-in boundary below the reference's Python operator interface: every entry point
 * replaces a call the reference makes into a third-party CUDA library (MinkowskiEngine, spconv,
 * torch_scatter) or into ATen for the eval-mode `Baseline3D.forward`
 * (segdino3d/models/architecture/baseline3d.py:308-346).  Citations are reference file:line.
 *
 * Conventions
 *   - All pointers are DEVICE pointers unless the name ends in `_host`; tensors are row-major fp32 /
 *     int32 / int64 / uint64 as typed; `ld*` are row strides in elements.
 *   - `stream` is a hipStream_t passed as void*; every function only enqueues work on it and returns
 *     (no device synchronisation, no allocation).  Scratch memory is caller-provided: `ws`/`ws_bytes`,
 *     sized with the matching `*_ws_bytes` query.
 *   - Return value: 0 on success, negative SD3D_ERR_* otherwise; `sd3d_last_error()` gives the text.
 *     The Python host (segdino3d_amd/_lib.py) maps a non-zero status to a RuntimeError.
 *   - No global state besides the last-error string; no internal threads.
 */
#ifndef SEGDINO3D_HIP_H
#define SEGDINO3D_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SD3D_ABI_VERSION 25

int sd3d_abi_version(void);
const char* sd3d_last_error(void);
/* Host-only self test of the Z-order key codec (runs without a GPU); returns 0 when consistent. */
int sd3d_selftest_host(void);
/* Scheduling hint (process-wide, default 1): how many independent scenes the caller keeps in flight on this GPU, each on its
 * own stream (dist_eval.PipelinedRunner).  With more than one, launchers prefer kernel variants with a small LDS footprint
 * that co-schedule with the other scenes' kernels over the ones that are fastest alone on an idle GPU (sd3d_pair_conv_ex: the
 * weight-stationary pass 1 for >= 96 output columns).  Results are bit-identical either way.  Returns the previous value. */
int sd3d_set_scenes_in_flight(int n);

/* The shared tail of the lock-step pass 1 (csrc/pair_gemm.hip "The shared tail of a lock-step launch"): the last 3/16 of a launch's tiles
 * are drawn in small units from an epoch-stamped counter of a per-device ring of launch slots.  Results are the same bits with the tail
 * on or off.  sd3d_set_pair_pool(0 / 1) switches it at run time (default: SD3D_PAIR_POOL, 1) and returns the previous setting.
 * sd3d_pair_pool_check() synchronises the current device and returns the number of counter words of its ring in a state no sequence of
 * finished launches can leave behind (0 = healthy; < 0 = error, see sd3d_last_error).  sd3d_pair_pool_launches(&n): pooled launches handed
 * out on the current device so far.  sd3d_pair_pool_poison(word) is a TEST hook: it overwrites every counter word of the current
 * device's ring (what a launch that died half-way or a foreign write would leave) - later launches must still produce the same bits.
 * A launch on a stream that is being captured into a HIP graph never uses the tail. */
int sd3d_set_pair_pool(int on);
int sd3d_pair_pool_check(void);
int sd3d_pair_pool_launches(int64_t* launches_out);
int sd3d_pair_pool_poison(int64_t word);

/* ---------------------------------------------------------------------------------------------
 * Sort / scan primitives (used by voxelisation, superpoint pooling, top-k)
 * ------------------------------------------------------------------------------------------- */
size_t sd3d_sort_ws_bytes(int64_t n);
/* Stable LSD radix sort of (key, value) pairs on bits [begin_bit, end_bit).  keys_in / vals_in are
 * clobbered.  vals_in may be NULL (value = element index); then vals_scratch [n] must be given.  The radix passes ping-pong
 * between (keys_in, vals_in | vals_scratch) and (keys_out, vals_out); an EVEN number of 8-bit passes leaves the result in the
 * former and sets *landed_in_input = 1, otherwise the result is in *_out and *landed_in_input = 0. */
int sd3d_sort_pairs_u64_ex(uint64_t* keys_in, uint32_t* vals_in, uint64_t* keys_out, uint32_t* vals_out, uint32_t* vals_scratch,
                           int64_t n, int begin_bit, int end_bit, void* ws, size_t ws_bytes, int* landed_in_input, void* stream);
size_t sd3d_scan_ws_bytes(int64_t n);
int sd3d_scan_exclusive_i32(const int32_t* in, int32_t* out, int64_t n, int32_t* total_dev, void* ws, size_t ws_bytes,
                            void* stream);
/* order-preserving key builders */
int sd3d_keys_from_f32(const float* x, int64_t n, int descending, uint64_t* keys, void* stream);
/* keys[i] = x[i] + add (add: the scene's bits of a batch-wide key - superpoint ids of scene b become (b << 32) | id before the batch-wide
 * sort; 0 for one scene).  The checks and the maximum are taken on x[i], not on the key: *flag |= flag_value when an id does not fit `bits`
 * bits (a radix sort over fewer key bits is then not a full sort; bits = 1..64, 64: no width check), *max_out = max(*max_out, largest id,
 * clamped to INT32_MAX) - the caller zeroes it - and an id that is negative or larger than INT32_MAX - 1 ORs 8 into *flag whatever `bits` is
 * (ids are row numbers: int32).  flag and max_out are required.  The superpoint count of a scene (largest id + 1; `minkunet.py:631-639`
 * scatter_mean sizes its output the same way) is known without waiting for the sort of the ids. */
int sd3d_keys_from_i64(const int64_t* x, int64_t n, int64_t add, uint64_t* keys, int bits, int32_t* flag, int flag_value, int32_t* max_out,
                       void* stream);

/* ---------------------------------------------------------------------------------------------
 * Voxelisation and coordinate maps.
 * Replaces ME.utils.batch_sparse_collate + ME.TensorField(...).sparse() + inverse_mapping
 * (minkunet.py:624-630, spconvunet.py:285-315) and the coordinate-manager side of
 * ME.MinkowskiConvolution / spconv indice-pair generation (minkunet.py:146-162, 176-192;
 * spconvunet.py:45-74, 156-201).
 * ------------------------------------------------------------------------------------------- */
/* stats[9] = min xyz, max xyz, sum xyz of points[:, 0:3] (baseline3d.py:285-287 scene range). */
size_t sd3d_scene_stats_ws_bytes(void);
int sd3d_scene_stats(const float* points, int ld, int64_t n, float* stats, void* ws, size_t ws_bytes, void* stream);
/* keys[i] = Z-order key of floor((xyz - (shift_to_min ? min : 0)) * inv_voxel); icoords [n,3] (optional)
 * receives the floor-quantised integer coordinates; origin[3] the key origin; *err_flag |= 1 when
 * the scene exceeds the 16-bit-per-axis key range. */
int sd3d_voxel_keys(const float* points, int ld, int64_t n, float inv_voxel, const float* stats, int shift_to_min,
                    int batch_index, int32_t* origin, uint64_t* keys, int32_t* icoords, int32_t* err_flag, void* stream);
/* Run-length unique over SORTED keys compared after (morton >> shift):
 *   ukeys [<=n], seg_start [<=n+1] (optional), map[src_idx ? src_idx[j] : j] = unique id (optional),
 *   *n_unique_dev = number of unique keys.  n_dev (optional) = device-resident live length <= n_cap.
 * clip_stats != NULL applies spconv's SparseConv3d(k=2, s=2) output-extent rule when creating level
 * clip_level >= 1: parents outside (D - 2) / 2 + 1 per axis (D_0 = max(extent, clip_min_shape),
 * spconvunet.py:309-310) are not created and their children map to -1. */
size_t sd3d_unique_ws_bytes(int64_t n_cap);
int sd3d_unique_sorted(const uint64_t* keys, const uint32_t* src_idx, int64_t n_cap, const int32_t* n_dev, int shift,
                       uint64_t* ukeys, int32_t* seg_start, int32_t* map, int32_t* n_unique_dev, void* ws,
                       size_t ws_bytes, const float* clip_stats, float clip_inv_voxel, int clip_level, int clip_min_shape,
                       void* stream);
/* One scene's voxelisation chain from ONE call (sd3d_scene_stats, sd3d_voxel_keys, the radix sort of the keys, sd3d_voxel_levels_all,
 * the superpoint ids' sort keys): ~28 launches that take the GPU ~0.25 ms
 * but cost a Python host ~0.5 ms when issued one by one in front of everything else of the scene.  Same kernels, same order, same
 * outputs as the separate calls (`minkunet.py:624-630`: batch_sparse_collate + TensorField.sparse() + inverse_mapping).
 *   readback [n_levels + 2] is zeroed here and receives {voxels of level 0 .. n_levels - 1, flags, largest superpoint id}
 *     (flags: 1 = key range exceeded, 2 = a Morton key needs more than key_bits bits, 4 = a superpoint id needs more than sp_bits bits);
 *   the sorted (key, point) pairs ping-pong between (keys_a, vals_a) and (keys_b, vals_b): *sorted_in_a tells where they landed;
 *   superpoints NULL: no ids (sp_keys unused); sp_bits = 64: no check of the ids' width. */
typedef struct sd3d_voxelise_desc {
    const float* points; int64_t n; int ld; int shift_to_min; float inv_voxel; int key_bits; int n_levels; int sp_bits;
    float* stats;                           /* [9] */
    int32_t *origin, *icoords;              /* [3], [n, 3] */
    uint64_t *keys_a, *keys_b;              /* [n] each */
    uint32_t *vals_a, *vals_b;              /* [n] each */
    uint64_t* ukeys0;                       /* [n] */
    int32_t *seg_start, *inverse;           /* [n + 1], [n] */
    uint64_t* const* ukeys;                 /* n_levels - 1 pointers, [n] each */
    int32_t* const* parents;                /* n_levels - 1 pointers, [n] each */
    int32_t* readback;                      /* [n_levels + 2] */
    const int64_t* superpoints; uint64_t* sp_keys;   /* [n] each, optional */
    void* ws; size_t ws_bytes;              /* >= sd3d_voxelise_scene_ws_bytes(n, n_levels) */
} sd3d_voxelise_desc;
size_t sd3d_voxelise_scene_ws_bytes(int64_t n, int n_levels);
int sd3d_voxelise_scene(const sd3d_voxelise_desc* d, int* sorted_in_a, void* stream);
/* EVERY level of a scene in ONE set of four launches, from the sorted POINT keys (level l keeps the runs of Morton >> 3 l): ukeys[l] [<= n]
 * (l = 0 .. n_levels - 1, level 0 included), seg_start [<= n + 1], map[src_idx ? src_idx[j] : j] = level-0 id, parents[l] [<= n] (l < n_levels - 1:
 * level-(l + 1) id of every level-l voxel), counts[l] = voxels of level l.  1 <= n_levels <= 8, no extent clip; entry for entry the arrays of
 * sd3d_unique_sorted(shift 0, seg_start, map) followed by sd3d_unique_sorted(shift 3, map) level after level. */
size_t sd3d_voxel_levels_all_ws_bytes(int64_t n, int n_levels);
int sd3d_voxel_levels_all(const uint64_t* sorted_keys, const uint32_t* src_idx, int64_t n, int n_levels, uint64_t* const* ukeys, int32_t* seg_start,
                          int32_t* map, int32_t* const* parents, int32_t* counts, void* ws, size_t ws_bytes, void* stream);
/* Open-addressing hash table key -> voxel id; capacity = power of two > n. */
int sd3d_hash_build(const uint64_t* ukeys, int64_t n, uint64_t* table_keys, int32_t* table_vals, int64_t capacity,
                    void* stream);
/* nbr[k*n_out + v] = id of the voxel at coord(v) + offsets[k] in the hashed level, or -1.
 * offsets: int8 [K,3] in units of that level's stride.  pair_count (optional, device int32[64],
 * pre-zeroed) accumulates the rulebook size (number of hits) as 64 partial sums - the host adds them
 * and uses the density to pick the convolution kernel. 
 * mirrored = 1: out_keys are the table's own keys and offsets[K-1-k] == -offsets[k] (centred odd kernel): only half the
 * offsets are probed and every hit is written to both mirror slots. */
int sd3d_kernel_map(const uint64_t* out_keys, int64_t n_out, const uint64_t* table_keys, const int32_t* table_vals,
                    int64_t capacity, const int8_t* offsets, int K, int mirrored, int32_t* nbr, int32_t* pair_count, void* stream);
/* The 3^3 kernel maps of EVERY level of a scene (and the 5^3 map of the finest level) from one call, without hash tables: through the
 * hierarchy of the sorted keys (level l + 1 = unique(key >> 3): the children of a coarse voxel are consecutive rows, the neighbour of a
 * voxel lies in one of the 27 cells around its parent).  keys[l] / n[l]: the levels' sorted keys (finest first, as sd3d_voxel_levels_all
 * leaves them), parent[l][j] = row of voxel j's parent on level l + 1 (NULL for the coarsest level; no extent clip: every parent
 * exists), nbr3[l] [27, n_l] outputs, nbr5 [125, n_0] output or NULL, offsets3 / offsets5 device int8 [K, 3] in the enumeration order
 * of the weights, inv27 (HOST) maps (dx + 1) + 3 (dy + 1) + 9 (dz + 1) to the row of offsets3.  pair_counts: NULL or device int32
 * [(n_levels + 1) x 64], zeroed - 64 partial rulebook counters per table (levels 0 .. n_levels - 1, then the 5^3 table).  The tables
 * are those of sd3d_kernel_map, entry for entry (MinkowskiEngine kernel map generation: minkunet.py:146-162).
 * perm8 + nbr_down[l] [8, n_{l+1}] / nbr_up[l] [8, n_l] for l < n_levels - 1 (all optional: NULL): the stride-2 maps of every level pair
 * (the tables of sd3d_stride_maps) from the same launches, every entry written by the thread that owns it (no pre-fill).
 * blk_cnt3 / blk_cnt5 (optional): while a workgroup holds the 256 rows of a block, the entry counts per (offset, 256-row block) of the tables
 * it writes: blk_cnt3[l] (l < n_levels - 1; the array or any entry may be NULL) device int32 [27, ceil(n_l / 256)], blk_cnt5 (NULL or)
 * [125, ceil(n_0 / 256)], count of offset k in rows [256 b, 256 b + 256) at [k * nblk + b] - what sd3d_pair_lists_desc takes as blk_counts
 * in place of its own count pass.  (The coarsest level's map is searched directly and brings no counts.) */
size_t sd3d_kernel_maps_hier_ws_bytes(int n_levels, const int64_t* n);
int sd3d_kernel_maps_hier(int n_levels, const uint64_t* const* keys, const int32_t* const* parent, const int64_t* n,
                          int32_t* const* nbr3, int32_t* nbr5, const int8_t* offsets3, const int8_t* offsets5, const int8_t* inv27,
                          int32_t* pair_counts, const int32_t* perm8, int32_t* const* nbr_down, int32_t* const* nbr_up,
                          int32_t* const* blk_cnt3, int32_t* blk_cnt5, void* ws, size_t ws_bytes, void* stream);
/* 2x2x2 stride-2 maps from the parent array: nbr_down [8, n_coarse], nbr_up [8, n_fine]; perm8[8]
 * maps the child's Z-order position (x | y<<1 | z<<2) to the weight index. */
int sd3d_stride_maps(const uint64_t* fine_keys, const int32_t* parent, int64_t n_fine, int64_t n_coarse,
                     const int32_t* perm8, int32_t* nbr_down, int32_t* nbr_up, void* stream);

/* ---- 1..16 scenes as ONE block-diagonal sparse tensor (the collation of `utils/dataset_utils.py:215-230` collate_fn_3D +
 * ME.utils.batch_sparse_collate, minkunet.py:624-627): the scene index sits in the key bits above the 48-bit Z-order code
 * (sd3d_voxel_keys batch_index), so ONE sort / unique / hash / kernel-map pass serves every scene of the batch and rows of
 * different scenes never become neighbours.  One scene is a batch of one: per voxel / superpoint the arithmetic (point order,
 * sums) does not depend on the number of scenes. ---- */
#define SD3D_MAX_BATCH 16
typedef struct sd3d_scene_src {
    const float* points;     /* [n_points, ld_points] xyz rgb of this scene */
    const float* feats2d;    /* [n_points, F] or NULL (mode 1) */
    const float* stats;      /* the scene's sd3d_scene_stats row */
    int64_t point_off;       /* index of the scene's first point in the batch-global point numbering */
    int64_t n_points;
    int32_t ld_points, pad_;
} sd3d_scene_src;
/* Unweighted per-voxel average of the assembled point feature row (ME quantisation mode used by the reference) over the voxels
 * of all scenes.  mode 0: rgb|f2d, 1: rgb, 2: rgb|xyz-mean|f2d.  out [n_vox, ld_out], zero padded.  Voxel v belongs to scene
 * (ukeys[v] >> 48) & 0xFF; sorted_idx holds batch-global point numbers.  With n_scenes == 1 every voxel belongs to scene 0:
 * ukeys may be NULL and is not read.  `scenes` is a HOST array (copied into the launch); every scene needs points and stats. */
int sd3d_voxel_mean_batch(const sd3d_scene_src* scenes, int n_scenes, int F, int mode, const uint64_t* ukeys,
                          const uint32_t* sorted_idx, const int32_t* seg_start, int64_t n_vox, float* out, int ld_out, void* stream);
/* start[s] = first position of dense superpoint id s in the sorted (scene << 32 | id) keys, start[S] = n: dense id = id_off[scene] + id,
 * S = number of dense ids of the batch.  `id_off` is a HOST array of n_scenes entries.  One scene (n_scenes = 1, id_off = {0}): the keys
 * are plain ids below 2^32 - the product checks ids into [0, 2^31 - 2] and the dataset targets sort over at most 32 bits. */
int sd3d_segment_starts_batch(const uint64_t* sorted_ids, int64_t n, int64_t S, const int32_t* id_off, int n_scenes, int32_t* start,
                              void* stream);
/* Fused `x.slice(field)` + torch_scatter.scatter_mean of features [S,C] and of the floor-quantised
 * coordinates * voxel_size [S,3]  (minkunet.py:631-656; spconvunet.py:390). */
/* C (feature columns) must be a multiple of 4 and <= 96 (round 5: a staged row of 96 columns + 3 coordinates per LDS slot; the shipped networks pool
 * 96 columns; SD3D_ERR_ARG otherwise). */
int sd3d_pool_superpoints(const float* feat, int ld_feat, int C, const int32_t* inverse, const int32_t* icoords,
                          float voxel_size, const uint32_t* sorted_idx, const int32_t* start, int64_t S, float* out_feat,
                          float* out_pos, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Gather-GEMM (fp32 MFMA): sparse convolution and dense Linear in one kernel.
 *   out[r][n] = act(scale[n] * sum_k sum_c in[nbr[k][r]][c] * wt[k][n][c] + shift[n] + res[r][n])
 * Replaces ME.MinkowskiConvolution / ConvolutionTranspose + MinkowskiBatchNorm + MinkowskiReLU
 * (minkunet.py:135-192, 28-38, 234-250), spconv SubMConv3d / SparseConv3d / SparseInverseConv3d
 * (spconvunet.py:45-74, 156-201) and torch.nn.functional.linear in the decoder.
 *   in0 [*, ld0] first C0 channels, in1 [*, ld1] the remaining Cin - C0 (skip concatenation, or NULL)
 *   nbr  [K, M] or NULL (identity rows, K == 1);  wt [K, Cout, Cin] (Cin % 32 == 0)
 *   act: 0 none, 1 ReLU, 2 GELU(erf), 3 sigmoid;  nt: tiling code (0 = auto, see csrc/gather_gemm.hip)
 *   ws / ws_bytes: optional scratch (>= 8 * M * Cout floats enables split-K on small launches)
 * ------------------------------------------------------------------------------------------- */
int sd3d_gather_gemm(const float* in0, int ld0, int C0, const float* in1, int ld1, const int32_t* nbr, const float* wt,
                     int K, int Cin, int Cout, int64_t M, const float* scale, const float* shift, const float* res,
                     int ld_res, float* out, int ld_out, int act, int nt, void* ws, size_t ws_bytes, void* stream);
/* Host-only helper: the value of `nt` that makes sd3d_gather_gemm run a plain Linear (nbr = NULL, K = 1) on ANY number of rows with the
 * kernel - hence the summation order and the bits - it picks by itself for `rows` rows (0 = the lock-step kernel, whose order does
 * not depend on the row count).  The batched evaluation forward runs the rows of several scenes in one launch this way. */
int sd3d_dense_plan_code(int64_t rows, int Cin, int Cout);
/* n <= 8 INDEPENDENT plain Linears in one launch: out_i = act_i([in0_i | in1_i] wt_i^T + shift_i + res_i), wt_i [Cout, Cin]
 * (nn.Linear layout).  For the decoder's chains of few-hundred-row Linears (instance_seg_3d_decoder.py:656-772: the two box MLPs
 * of a layer, projections that share an input) - the same kernel as sd3d_gather_gemm's small-M path, one dispatch. */
typedef struct sd3d_linear_job {
    const float *in0, *in1;            /* in1: optional second source (concatenated channels C0..Cin-1) or NULL */
    const float *wt, *shift, *res;     /* shift / res optional */
    float* out;
    int64_t M;
    int32_t ld0, C0, ld1, Cin, Cout, ld_res, ld_out, act;
} sd3d_linear_job;
int sd3d_linear_group(int n, const sd3d_linear_job* jobs, void* stream);

/* Opt-in variant of sd3d_gather_gemm that evaluates the fp32 products as sums of bf16 MFMA products
 * (csrc/gather_gemm_split.hip).  wt_split = the fp32 weights [K, Cout, Cin] split into bf16 terms,
 * w = t0 + t1 (+ t2) with t_i = bf16_rne(w - sum_{j<i} t_j), laid out [2 or 3][K][Cout][Cin];
 * terms = 3 (two terms per operand, error ~2^-16 per product) or 6 (three terms, ~2^-24: fp32-grade), or
 * terms = 1: plain bf16 operands with fp32 accumulation ([1][K][Cout][Cin]) - the "bf16 decoder" of BASELINE
 * config #3 (autocast(bf16) around the decoder's nn.Linear calls in the reference, train_engine_3d.py:88-100).
 * Not used unless the host asks for it (decoder compute_dtype, or split weights passed explicitly); the default is exact fp32 MFMA. */
int sd3d_gather_gemm_split(const float* in0, int ld0, int C0, const float* in1, int ld1, const int32_t* nbr,
                           const uint16_t* wt_split, int terms, int K, int Cin, int Cout, int64_t M, const float* scale,
                           const float* shift, const float* res, int ld_res, float* out, int ld_out, int act, int nt,
                           void* ws, size_t ws_bytes, void* stream);

/* Pair-major sparse convolution (csrc/pair_gemm.hip) - the same contract as sd3d_gather_gemm with a
 * neighbour table (MinkowskiConvolution / SubMConv3d + folded BN + residual + activation), evaluated
 * over the rulebook laid out offset-major so that every MFMA row is a real (in, out) pair.
 * sd3d_pair_lists_desc builds, for n <= 16 neighbour tables nbr [K, M] in ONE launch set:
 *   pos [K, M]      position of pair (k, r) in the list, -1 where nbr[k][r] < 0
 *   in_idx [p_cap]  gathered input row of each list entry; every offset's segment is padded to a
 *                   multiple of 128 entries with -1
 *   tile_k [p_cap/128 + 1]  offset of each 128-entry tile, -1 past the end of the list; the last entry
 *                   receives the number of real tiles
 * p_cap: multiple of 128, >= (number of pairs) + 127 * K (pairs beyond the capacity are dropped:
 * size it from the pair count sd3d_kernel_map returns).  ws holds the tables' scratch back to back, each rounded up to
 * 256 bytes (sum of align256(sd3d_pair_lists_ws_bytes(K_i, M_i))).
 * sd3d_pair_conv_ex: part = caller scratch of >= p_cap * Cout floats.  Cin % 32 == 0, Cout % 4 == 0.  With plain lists
 * (rlist and out_idx NULL, center -1) pass 2 sums each output row's partial products through pos. */
size_t sd3d_pair_lists_ws_bytes(int K, int64_t M);

/* Round-3 products of the list builder, all optional, and what the convolution does with them (same fixed per-row summation
 * order for a given table description, results reproducible bit for bit):
 *   rlist [M, rl_stride]   per output row {count, list positions of its pairs in offset order}; rl_stride a multiple of 4,
 *                          >= K + 4.  Pass 2 walks a row's own partial products instead of the K slots of pos[k][r].
 *   center                 -1 (plain lists) or SD3D_PAIR_CHAINED (below).  (Round 3 also took an offset number here - a dense
 *                          kernel for the centre offset of a stride-1 table; it measured slower and left the library, see
 *                          profiles/EXPERIMENTS.md.  A value >= 0 is refused with SD3D_ERR_ARG.)
 *   meta                   bit 0: tile_k has p_cap / 128 + 3 entries (two reserved slots, written as zero, behind the tile count);
 *                          bit 1: the capacity behind the last real tile (in_idx, out_idx, tile_k) is left UNWRITTEN - for callers
 *                          whose consumers walk tile_k[p_cap / 128] tiles and nothing else (sd3d_pair_conv_ex / sd3d_run_layers do);
 *                          with worst-case capacities that tail is tens of MB per table.
 *   pos == NULL            (round 5) no position table: needs rlist or out_idx, K <= 128.  The builder then takes the row-block form
 *                          (a workgroup owns 256 rows and walks all offsets; three launches; the per-row lists come out of the fill
 *                          launch).  What an evaluation forward uses: the stem's [125, V] table alone is 69 MB written and read back.
 *   out_idx [p_cap]        output row of every list entry (-1 on padding).  Handing it to the convolution promises ONE pair per
 *                          output row - the transposed k2s2 convolutions (minkunet.py:165-192 `conv_tr`: every fine voxel has one
 *                          parent) - and pass 1 writes act(scale * product + shift + res) to the row directly: no pass 2. */
/* center == SD3D_PAIR_CHAINED (stride-1 table of a voxel set onto itself, odd kernel with symmetric offsets off[K-1-k] == -off[k],
 * centre K / 2): CHAINED lists - the entries of an output row that belong to one mirror group {k, K-1-k}, plus the centre in the
 * row's first non-empty group, share ONE partial product (pass 1 accumulates across up to three consecutive sub-tiles and stores
 * once; tile_k carries bit 30 on all but the last sub-tile of a chain).  27-44 % fewer partial rows on surface-like scenes.  For
 * these tables pos is not written (may be NULL: a row's partial positions are its rlist), rlist is required (rl_stride >= K / 2 + 2), K <= 125, p_cap >=
 * pairs + 127 * (11 * (K / 2) + 1), and the same value goes to sd3d_pair_conv_ex / sd3d_run_layers as `center`. */
#define SD3D_PAIR_CHAINED (-2)
/* sd3d_pair_conv_ex only: `center` - 2 (i.e. -3 for plain, -4 for chained lists) = the same lists with the weight matrices taken in MIRRORED offset
 * order, W[K - 1 - k] for offset k.  The input gradient of a stride-1 convolution is the forward convolution on the same table with the offsets
 * mirrored and the matrices transposed (csrc/pair_wgrad.hip header): a parameter kept as [K, Cin, Cout] (ME.MinkowskiConvolution.kernel) IS that
 * transposed set, so the training step passes it as it lies - no flipped / transposed copy per layer and step. */
#define SD3D_PAIR_MIRROR_W(center) ((center) - 2)
typedef struct sd3d_pair_table_desc {
    const int32_t* nbr;                  /* [K, M] */
    int32_t *pos, *in_idx, *tile_k;      /* see sd3d_pair_lists_desc above */
    int32_t *rlist, *out_idx;            /* optional (NULL) */
    int64_t M, p_cap;
    int32_t K, center, rl_stride, meta;
} sd3d_pair_table_desc;
/* blk_counts: the count pass of some tables already done - (NULL or) [n] pointers, each NULL or device int32 [K, ceil(M / 256)] as
 * sd3d_kernel_maps_hier leaves them in blk_cnt3 / blk_cnt5.  Only a table built in the row-block form (pos == NULL, K <= 128, not chained) may
 * bring counts; it has no workgroups in the count launch, its counts are scanned in place (consumed), and its lists are those of a call
 * without counts bit for bit. */
int sd3d_pair_lists_desc(int n, const sd3d_pair_table_desc* tables, int32_t* const* blk_counts, void* ws, size_t ws_bytes, void* stream);
int sd3d_pair_conv_ex(const float* in0, int ld0, int C0, const float* in1, int ld1, const int32_t* in_idx,
                      const int32_t* tile_k, int64_t p_cap, const int32_t* pos, const int32_t* rlist, int rl_stride, int center,
                      const int32_t* out_idx, const float* wt, int K, int Cin, int Cout, int64_t M, const float* scale,
                      const float* shift, const float* res, int ld_res, float* out, int ld_out, int act, float* part,
                      size_t part_bytes, void* stream);

/* Layer-sequence executor (csrc/executor.hip): a whole sparse U-Net forward from one call.  Replaces the
 * Python-level module loop of Res16UNetBase.forward (minkunet.py:531-601) / UBlock.forward
 * (spconvunet.py:156-201): the plan is built once per model, per scene the caller supplies the
 * neighbour tables and the activation buffers (one arena, carved by the caller); the call only enqueues.
 *   SD3D_LAYER_PAIR_CONV        out = act(scale * conv(cat[src0, src1]; table) + shift + res)   (sd3d_pair_conv_ex)
 *   SD3D_LAYER_DENSE            the same with identity rows, K = 1                                 (sd3d_gather_gemm)
 *   SD3D_LAYER_SCALE_SHIFT_ACT  out = act(cat[src0, src1] * scale + shift) + res, Cin = total channels; res (optional) is
 *                               added AFTER the activation here                                  (sd3d_scale_shift_act_add) */
enum { SD3D_LAYER_PAIR_CONV = 0, SD3D_LAYER_DENSE = 1, SD3D_LAYER_SCALE_SHIFT_ACT = 2 };
typedef struct sd3d_layer {
    int32_t kind, table;               /* table: index into tables[] (PAIR_CONV) */
    int32_t src0, src1, res, dst;      /* buffer ids; src1 / res = -1 when absent */
    int32_t K, Cin, C0, Cout, act;     /* C0 = channels taken from src0 (Cin when src1 is absent) */
    int32_t pad_;
    const float *wt, *scale, *shift;   /* wt [K, Cout, Cin]; scale / shift per output channel or NULL */
} sd3d_layer;
typedef struct sd3d_table {
    const int32_t *in_idx, *tile_k, *pos;   /* from sd3d_pair_lists_desc */
    int64_t p_cap, M;                        /* M = output rows of the table */
    int32_t K, pad_;
    const int32_t *rlist, *out_idx;          /* optional products of sd3d_pair_lists_desc (NULL) */
    int32_t rl_stride, center;               /* -1 or SD3D_PAIR_CHAINED, as in sd3d_pair_table_desc */
} sd3d_table;
typedef struct sd3d_buf {
    float* ptr;
    int64_t rows;
    int32_t ld, pad_;
} sd3d_buf;
int sd3d_run_layers(const sd3d_layer* layers, int n_layers, const sd3d_table* tables, int n_tables, const sd3d_buf* bufs,
                    int n_bufs, float* part, size_t part_bytes, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Decoder kernels (segdino3d/models/decoder/instance_seg_3d_decoder.py:606-799,
 * segdino3d/models/module/attention.py:186-395, segdino3d/models/module/utils.py:53-105)
 * ------------------------------------------------------------------------------------------- */
/* ---- Row-chain executor (csrc/rowchain.hip): the row-local part of a decoder layer as ONE launch ------------------------------
 * Replaces the per-op launches of instance_seg_3d_decoder.py:606-799 between the superpoint cross-attention and the mask-logit
 * product: a workgroup owns 16 (program.tile_rows = 0 / 16) or 4 (tile_rows = 4: csrc/rowchain_narrow.hip, 8 waves) consecutive query
 * rows of one scene, keeps their activations in LDS slots ([rows][260] fp32 each; a buffer wider than 256 columns has row stride
 * width + 4 and spills into the following slots) and interprets `ops` over them.
 * All pointers are device pointers; global tensors hold the query rows of ALL scenes of the call back to back (row = scene.q0 +
 * row in scene).  Slot 0xFF = "none".  Per row the arithmetic does not depend on the other rows of the launch. */
#define SD3D_RC_MAX_OPS 44
#define SD3D_RC_MAX_PROGRAMS 4
enum { SD3D_RC_LOAD = 1,   /* slot dst[:, :cout] = p0[row, :cout] (row stride ld) */
       SD3D_RC_STORE = 2,  /* p0[row, :cout] = slot src0 */
       SD3D_RC_LINEAR = 3, /* dst = act([src0 (k0 ch) | src1 (k1 ch)] . W^T + bias (+ res)); p0 = W [cout, K = k0 + k1] PACKED in MFMA-fragment order
                            * P[tile = col / 16][g = ch / 16][lane = 16 * ((ch % 16) / 4) + col % 16][ch % 4] = W[min(col, cout - 1)][ch] (4-row tiles:
                            * P[tile = col / 64][quad = ch / 4][lane = col % 64][ch % 4]), p1 = bias | NULL,
                            * p2 = optional global copy (row stride ld); flag NO_LDS_DST: only the global copy */
       SD3D_RC_LN = 4,     /* dst = act(LayerNorm_256(src0 (+ res)) * p0 + p1), eps = f0; p2 = optional global copy (ld) */
       SD3D_RC_PE = 5,     /* dst = sine PE (utils.py:53-105) of p0[row, 0:3] in the scene's range; p1 = dim_t [256], p2 = axis int8 [256];
                            * src0 != none: times slot src0[:, a] / p3[row, a] (box modulation, :659-666) */
       SD3D_RC_BOX = 6,    /* box refinement (:735-759): p2[row] = p0[row] + src0[:, 0:3]; with src1: size p3 / metric size p4 from p1 (previous
                            * size) and src1[:, 0:3]; flag NORMALIZE */
       SD3D_RC_MERGE = 7,  /* dst = rows of the superpoint cross-attention: p1 (its output, stride ld) where the scene's key split is 1, else
                            * the combination of its partial states p0 + scene.part_off (sd3d_attention_parts) */
       SD3D_RC_BITS2D = 8, /* LDS bit rows: blocked2d = no superpoint open for the query (p0 + scene.bits_off: blocked bits [nq, nw]) and near
                            * the 2D query (p1 + scene.near_off: [nm - 1, nw]) (:722-726) */
       SD3D_RC_ATTN = 9    /* dst = 8-head attention (32 channels per head) of slot src0 over the scene's keys: K = p0, V = p1 (row stride ld),
                            * key rows scene.q0.. (nq) or, flag KEYS_2D, scene.m0.. (nm); flag MASK_BITS2D: the LDS bit rows; scale f0;
                            * aux = first of two scratch slots */ };
#define SD3D_RC_F_NO_LDS_DST 1
#define SD3D_RC_F_NORMALIZE 2
#define SD3D_RC_F_KEYS_2D 4
#define SD3D_RC_F_MASK_BITS2D 8
#define SD3D_RC_F_INPLACE 16           /* LINEAR: dst overlaps src0 / src1 (a barrier separates the contraction from the stores) */
typedef struct sd3d_rc_op {
    uint8_t type, act, src0, src1, dst, res, flag, aux;
    uint16_t k0, k1, cout, pad_;
    int32_t ld;
    float f0;
    const void *p0, *p1, *p2, *p3, *p4;
} sd3d_rc_op;                                                  /* 64 bytes */
typedef struct sd3d_rc_scene {
    int32_t q0, nq;                                            /* first query row, number of query rows */
    int32_t m0, nm;                                            /* 2D keys: first row, count (incl. the appended dummy key) */
    int32_t bits_off, nw;                                      /* blocked bits of the scene: offset in words, words per row */
    int32_t near_off, ksplit;                                  /* near table offset in words; key split of the cross-attention */
    int64_t part_off;                                          /* offset (floats) of the scene's partial attention states */
} sd3d_rc_scene;                                               /* 40 bytes */
typedef struct sd3d_rc_program {
    int32_t n_scenes, n_programs, n_slots, nw_max, nw2_max, tile_rows;
    const float* rng;                                          /* [n_scenes][6] scene ranges (lo, hi) for PE / BOX */
    int32_t tile0[SD3D_MAX_BATCH + 1];                         /* prefix sums of ceil(nq / tile rows) */
    int32_t prog_begin[SD3D_RC_MAX_PROGRAMS + 1];              /* op ranges of the programs (gridDim.y) */
    sd3d_rc_scene scenes[SD3D_MAX_BATCH];
    sd3d_rc_op ops[SD3D_RC_MAX_OPS];
} sd3d_rc_program;
/* program_host: HOST pointer to the program (passed to the kernel by value). */
int sd3d_row_chain(const sd3d_rc_program* program_host, void* stream);
size_t sd3d_row_chain_program_bytes(void);                     /* sizeof(sd3d_rc_program): bindings check their layout against it */

/* out = act(LayerNorm(x + res) * w + b); nn.LayerNorm (+ the residual adds at decoder :690-691,
 * :708-709, :82-84, :187-188).  act: 0 none, 1 ReLU (input_proj, :228-229). */
int sd3d_layernorm(const float* x, int ld_x, const float* res, int ld_res, const float* w, const float* b, float eps,
                   int64_t M, int D, float* out, int ld_out, int act, void* stream);
/* out = act(LayerNorm(x wt^T + bias + res) * ln_w + ln_b) in ONE launch for few rows (the 200-query tensors of the decoder): the
 * attention out-projection / second FFN Linear with the residual add and norm that follow it (decoder :690-691, :708-709, :82-84,
 * :187-188).  wt [Cout = 256, Cin], Cin a multiple of 16; bias / res optional; fp32 MFMA, two-pass row statistics. */
int sd3d_linear_layernorm(const float* x, int ld_x, int64_t M, int Cin, const float* wt, int Cout, const float* bias, const float* res, int ld_res,
                          const float* ln_w, const float* ln_b, float eps, int act, float* out, int ld_out, void* stream);
/* PositionEmbeddingCoordsSine.get_sine_embeddings (utils.py:53-105) incl. shift_scale_points
 * (pc_util.py:48-76).  A range is (lo[3], hi[3]); dim_t / axis: per output channel (host tables);
 * optional box modulation out *= mod_num / mod_den (decoder :660-663; ld_den may be 0 = broadcast; mod_num without mod_den is refused).
 * ranges / row_scene, here and in sd3d_fourier_pe and sd3d_box_refine: row_scene NULL = ranges is ONE [6] range for every row; otherwise the
 * rows of SEVERAL scenes at once (the decoder of a batched evaluation forward): ranges [n_scenes, 6], row_scene [n] = scene of every row, row r
 * uses ranges[row_scene[r]].  Per row the arithmetic is the same either way. */
int sd3d_sine_pe(const float* xyz, int ld_xyz, int64_t n, const float* ranges, const int32_t* row_scene, const float* dim_t,
                 const int8_t* axis, int d_pos, const float* mod_num, int ld_num, const float* mod_den, int ld_den, float* out,
                 int ld_out, void* stream);
/* PositionEmbeddingCoordsSine.get_fourier_embeddings (utils.py:107-142; decoder `pos_type="fourier"`): out[:, :d/2] = sin(p),
 * out[:, d/2:] = cos(p), p = (2 pi * shift_scale(xyz)) @ gauss_b[:, :d/2]; gauss_b [3, >= d/2] is the module's buffer.  An odd d_pos is refused. */
int sd3d_fourier_pe(const float* xyz, int ld_xyz, int64_t n, const float* ranges, const int32_t* row_scene, const float* gauss_b,
                    int ld_b, int d_pos, float* out, int ld_out, void* stream);
/* Fused multi-head attention (replaces bmm + masked_fill + softmax + bmm of attention.py:361-385 and
 * nn.MultiheadAttention's SDPA at decoder :79).  q / k / v / out hold H heads of head_dim channels side by side; head_dim is 32 or 64
 * (one kernel body, the width a template parameter), any other width returns SD3D_ERR_ARG before anything is launched.  nsrc = 2
 * (q1 / k1 given) concatenates [q0|q1] . [k0|k1] per head (decoder :681-687): the score contraction runs over head_dim channels per
 * source.  mask_bits [Lq, ceil(Lk/32)]: bit = 1 -> blocked.
 * lse: optional [H, Lq] log-sum-exp of the masked, scaled score rows (natural units; the backward pass needs it), NULL = not wanted.
 * bf16 != 0: Q, K, P and V rounded to bf16 for the two contractions (v_mfma_f32_32x32x16_bf16, fp32 accumulate; scores, mask, softmax
 * in fp32): the attention of the "bf16 decoder", BASELINE config #3.
 * ws / ws_bytes: optional scratch (sd3d_attention_ws_bytes; 0 for an unsupported width) that lets few-query launches split the keys
 * over several workgroups and merge the softmax states in a second pass; NULL = single pass.  One partial softmax state per (32-query
 * tile, head, key split) is m[32], l[32], O[head_dim dv][32 q] in the log2 domain = 64 + 32 * head_dim floats, laid out
 * [ceil(Lq/32)][H][ksplit] with ksplit <= 8.  The launcher splits the keys only as far as the workspace it was given holds (ksplit = 1
 * without one) and never writes behind it.
 * key, call, p: dropout of rate p on the softmax probabilities, inside the kernel (nn.MultiheadAttention(dropout=p) in training,
 * attention.py:383): out = (c K o softmax(S)) V with c = 1 / (1 - p); lse, the key split and its workspace are unchanged.
 * The keep mask K is a pure function of (key, call, head, q, k) (csrc/attention.h): Philox4x32-10 keyed by the two words at
 * `key` (device memory) with the counter (k >> 2, q, head, call); element (head, q, k) takes output word k & 3 and is kept iff that
 * word >= floor(p 2^32).  `call` tells the attentions of one step apart.  Neither the launch shape nor the head width enters, so
 * sd3d_attention_backward regenerates the mask the forward drew and sd3d_attention_dropout_keep writes it out
 * (keep[H, Lq, Lk] bytes, 1 = kept).  p == 0 (evaluation; key NULL, call 0) launches the kernels without dropout and ignores key; p outside
 * [0, 1) (NaN included), p > 0 with a NULL key or an unsupported head width returns SD3D_ERR_ARG before anything is launched.
 * sd3d_attention_config: the waves per workgroup and the key split the launcher chooses for one attention given ws_bytes of split
 * workspace (host-only, launches nothing). */
size_t sd3d_attention_ws_bytes(int Lq, int H, int head_dim);
int sd3d_attention(const float* q0, int ldq0, const float* q1, int ldq1, const float* k0, int ldk0, const float* k1, int ldk1,
                   const float* v, int ldv, const uint32_t* mask_bits, int Lq, int Lk, int H, int head_dim, float scale,
                   float* out, int ldo, float* lse, int bf16, void* ws, size_t ws_bytes, const uint32_t* key, int call, float p,
                   void* stream);
int sd3d_attention_config(int Lq, int Lk, int H, int head_dim, size_t ws_bytes, int* waves_out, int* ksplit_out);
int sd3d_attention_dropout_keep(const uint32_t* key, int call, int H, int Lq, int Lk, float p, uint8_t* keep, void* stream);
/* n <= SD3D_MAX_BATCH independent attentions of the same kind (heads, width, scale, one or two sources, fp32 / bf16 contractions) in ONE
 * launch: the decoder of a batched evaluation forward runs the scenes' cross- / self- / 2D-query attentions this way.  blockIdx.x runs
 * over the query tiles of all scenes; each scene keeps the waves per workgroup and the key split its own launch would have, so its rows
 * are the bits of sd3d_attention on that scene alone (scenes whose workgroup shapes differ are launched one by one inside the call).
 * ws: split workspace, scene i's sd3d_attention_ws_bytes(Lq_i, H, head_dim) bytes back to back. */
typedef struct sd3d_attn_job {
    const float *q0, *q1, *k0, *k1, *v;      /* q1 / k1 NULL for one source (all jobs alike) */
    const uint32_t* mask_bits;               /* [Lq, ceil(Lk / 32)] or NULL */
    float* out;
    int32_t ldq0, ldq1, ldk0, ldk1, ldv, ldo, Lq, Lk;
} sd3d_attn_job;
int sd3d_attention_batch(int n, const sd3d_attn_job* jobs, int H, int head_dim, float scale, int bf16, void* ws, size_t ws_bytes,
                         void* stream);
/* The same launch for 32-channel heads WITHOUT the pass that combines the key splits (its consumer does: sd3d_row_chain MERGE, built for
 * that width): on return scene i's rows are final in its `out` where ksplit_out_host[i] == 1, and otherwise wait as partial softmax
 * states [ceil(Lq/32)][H][ksplit][64 + 1024] (m[32], l[32], O[32 dv][32 q], log2 domain) at ws + part_off_out_host[i] floats. */
int sd3d_attention_batch_parts(int n, const sd3d_attn_job* jobs, int H, float scale, int bf16, void* ws, size_t ws_bytes,
                               int32_t* ksplit_out_host, int64_t* part_off_out_host, void* stream);
/* (dist < thr) of torch.cdist(p=1) (:721) as bits near[M, ceil(S/32)]. */
int sd3d_near_bits(const float* sp_pos, int64_t S, const float* centers, int64_t M, float thr, uint32_t* near, int nwords,
                   void* stream);
/* The matrices of 1 <= n <= SD3D_MAX_BATCH scenes in one launch each (host arrays of n entries; one scene is n = 1).
 * mask_bits, the _forward_head mask part (:567-572): bits[i] [Q_i, nwords_i = ceil(S_i/32)] = sigmoid(logits[i]) < thr, dead rows reset to open.
 * dinox_mask_bits: out[i] [Q_i, nwords_out_i = ceil((Mq_i+1)/32)] = ((~blocked[i]).float() @ near[i].float()) == 0, plus the always-open dummy
 * key (:722-726); refused when two (under 2048 query rows in all) or eight query rows of the widest scene exceed 64 KiB of LDS. */
int sd3d_mask_bits_batch(int n, const float* const* logits, const int* ld, const int64_t* Q, const int* S, uint32_t* const* bits,
                         const int* nwords, float thr, void* stream);
int sd3d_dinox_mask_bits_batch(int n, const uint32_t* const* blocked, const uint32_t* const* near, const int* nwords, const int64_t* Q,
                               const int64_t* Mq, uint32_t* const* out, const int* nwords_out, void* stream);
/* centre / size refinement (:735-759, :768-772). d_size may be NULL (no size head).  ranges / row_scene: as in sd3d_sine_pe. */
int sd3d_box_refine(const float* ref_points, const float* d_center, const float* size_prev, int ld_size_prev,
                    const float* d_size, const float* ranges, const int32_t* row_scene, int normalize, int64_t Q, float* center,
                    float* size, float* size_metric, void* stream);
/* out = act(x * scale + shift) + add, x = [x0 (C0 channels) | x1] (x1 may be NULL).  add NULL: the pre-activation
 * BatchNorm1d + ReLU of the spconv residual blocks (spconvunet.py:48-51, 154-156, 184-187, 227-229); with add: the tail of a
 * normalize_before=False residual block - conv -> BatchNorm1d -> ReLU, then the identity branch summed in AFTER the
 * activation (spconvunet.py:66-81, 95-97). */
int sd3d_scale_shift_act_add(const float* x0, int ld0, int C0, const float* x1, int ld1, const float* scale,
                             const float* shift, int act, int64_t M, int C, const float* add, int ld_add, float* out,
                             int ld_out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Post-processing (segdino3d/models/architecture/baseline3d.py)
 * ------------------------------------------------------------------------------------------- */
/* softmax(cls)[:, :C] flattened (:427) and/or its row maximum (:236-238). Either output may be NULL. */
int sd3d_class_scores(const float* cls, int ld, int64_t Q, int C, float* scores, float* rowmax, void* stream);
/* labels / query index of the selected flat indices + mask-quality rescoring (:436-446). */
int sd3d_mask_scores(const float* masks, int ld, int S, const uint32_t* flat_idx, const float* score_in, int n, int C,
                     int normalize, int32_t* labels, int32_t* qidx, float* score_out, void* stream);
/* Index glue of predict_by_feat_instance / mask_matrix_nms as single launches (pure data movement):
 *   take_f32: out[i] = src[idx[i]] (:434-435 `scores[topk_idx]`);  take_pair: labels / scores in the first sort's order (:71-76);
 *   nms_finish: final_scores = scores2[order2], final_labels = labels1[order2], record = order1[order2] (int64, :133-139) and, boxes != NULL,
 *   boxes[i] = [centers | sizes][qidx[record[i]]] ([n, 6], baseline3d.py:447-452; centers / sizes [Q, 3] contiguous). */
int sd3d_take_f32(const float* src, const uint32_t* idx, int n, float* out, void* stream);
/* idx[0..k) = the first k entries of the STABLE descending sort of x[0..n) (ties: lower index first) - what
 * sd3d_keys_from_f32(descending) + sd3d_sort_pairs_u64_ex give, from one launch of one workgroup (radix select + rank of the k survivors).
 * `scores.flatten(0, 1).topk(topk_insts)` of predict_by_feat_instance (baseline3d.py:434).  1 <= k <= 1024, k <= n <= 40 960 (forty scores per thread of the one workgroup, in registers). */
int sd3d_topk_desc_f32(const float* x, int64_t n, int k, uint32_t* idx, void* stream);
/* The data-dependent selections of predict_by_feat_instance (:470-476) for two score thresholds on the device (all outputs sized k):
 * keep / pkeep = rows with score > thr0 / thr1 and count > npoint_thr, ascending; union_rows = rows in either; keep_u / pkeep_u = where
 * the rows of keep / pkeep sit in union_rows; score_mask[i] = score[i] > thr0; npoint_mask = (count > npoint_thr) compacted over the
 * rows with score > thr0; counts[4] = {|keep|, |pkeep|, |union|, |score > thr0|} - the only thing the host has to read. */
int sd3d_select_instances(const float* scores, const int32_t* count, int k, float thr0, float thr1, int npoint_thr, int32_t* keep,
                          int32_t* pkeep, int32_t* union_rows, int32_t* keep_u, int32_t* pkeep_u, uint8_t* score_mask, uint8_t* npoint_mask,
                          int32_t* counts, void* stream);
/* labels_out (int64) / scores_out / boxes_out ([m, 6] or NULL) = rows keep[0..m) of labels / scores / boxes (baseline3d.py:470-476). */
int sd3d_take_instances(const int32_t* keep, int m, const int32_t* labels, const float* scores, const float* boxes, int64_t* labels_out,
                        float* scores_out, float* boxes_out, void* stream);
int sd3d_take_pair(const uint32_t* order, const int32_t* labels, const float* scores, int n, int32_t* labels_out, float* scores_out,
                   void* stream);
int sd3d_nms_finish(const uint32_t* order2, const float* scores2, const int32_t* labels1, const uint32_t* order1, const int32_t* qidx,
                    const float* centers, const float* sizes, int n, float* final_scores, int32_t* final_labels, int64_t* record,
                    float* boxes, void* stream);
/* sig[r] = sigmoid(masks[qidx[order[r]]]) zero-padded to ld_out, area[r] = sum (:441, :66, :80-81). */
int sd3d_gather_sigmoid(const float* masks, int ld, int S, const int32_t* qidx, const uint32_t* order, int n, float* sig,
                        int ld_out, float* area, void* stream);
/* matrix-NMS decay from inter = sig . sig^T (:85-119); comp_ws [n] scratch. */
int sd3d_nms_decay(const float* inter, int ld, const float* area, const int32_t* labels, int n, int gaussian,
                   float sigma, const float* score_in, float* comp_ws, float* score_out, void* stream);
/* superpoint -> point broadcast + threshold + point count + optional box filter (:453-454, :464, :348-371).
 * Mask bytes are 0/1; count[n] counts BEFORE the box filter; boxes [n,6] or NULL.  Superpoint ids must be
 * < ld_sig (the padded row width of sig); ws holds the thresholded rows as a bit table.
 * Two steps, so that the caller applies the score / point-count thresholds BEFORE expanding (count[] comes from step 1):
 * sd3d_mask_rowbits thresholds the rows into the bit table in `ws` (sd3d_expand_masks_ws_bytes) and makes count[n];
 * sd3d_expand_rows writes out[j] = row rows[j] for a list of m rows from the SAME ws (boxes [n, 6] indexed by the row number, or NULL):
 * the whole [n, N] byte table (90 MB at 600 x 150 k; the list 0 .. n - 1) is never made, only the kept rows. */
size_t sd3d_expand_masks_ws_bytes(int n, int ld_sig);
int sd3d_mask_rowbits(const float* sig, int ld_sig, const uint32_t* src_row, int n, const int64_t* superpoints, int64_t N, float sp_thr,
                      int32_t* count, void* ws, size_t ws_bytes, void* stream);
int sd3d_expand_rows(const void* ws, int n, int ld_sig, const int32_t* rows, int m, const int64_t* superpoints, const float* points,
                     int ld_points, int64_t N, const float* boxes, float loose_ratio, uint8_t* out, void* stream);
/* Bit-packed copy of selected rows of the [n, N] byte masks of sd3d_expand_rows, for the device -> host copy of
 * `pts_instance_mask[0]` (baseline3d.py:453-454; evaluator_3d.py:178 reads it on the host): out [n_rows, nb = ceil(N/8)] bytes,
 * bit j of byte b = masks[rows[i]][8 b + j] != 0 (numpy bitorder "little"); rows NULL = rows 0..n_rows-1. */
int sd3d_pack_mask_rows(const uint8_t* masks, int64_t N, const int32_t* rows, int n_rows, uint8_t* out, int64_t nb, void* stream);
/* HOST function (no GPU): packed_host [n_rows, nb] -> out_host [n_rows, N] bytes 0 / 1, the torch.bool / numpy bool layout. */
int sd3d_unpack_bits_host(const uint8_t* packed_host, int64_t n_rows, int64_t N, int64_t nb, uint8_t* out_host);
/* argmax over selected columns (:504) and table gather (:504-507). */
int sd3d_row_argmax(const float* x, int ld, int64_t Q, const int32_t* cols, int ncols, int64_t* out, void* stream);
int sd3d_gather_i64(const int64_t* table, const int64_t* idx, int64_t N, int use_index, int64_t* out, void* stream);
/* panoptic paint + small-segment removal + map composition (:532-556).  rows_desc[n]: mask rows in
 * descending score order; inst_ws [N], hist_ws [n + n_stuff + 1] scratch. */
int sd3d_panoptic(const uint8_t* masks, int64_t N, const int32_t* rows_desc, const int32_t* labels_desc, int n, int n_stuff,
                  int npoint_thr, const int64_t* sem_stuff, int32_t* inst_ws, int32_t* hist_ws, int64_t* sem_map,
                  int64_t* inst_map, void* stream);
/* GT instance centres / sizes attached to the targets before inference (:289-305).  masks: bool bytes,
 * row stride mask_stride; mode 0 = "mean" centre, 1 = "median" (= bbox centre, :299-300). */
size_t sd3d_instance_boxes_ws_bytes(int n_inst);
int sd3d_instance_boxes(const float* points, int ld, int64_t N, const uint8_t* masks, int64_t mask_stride, int n_inst,
                        int mode, float* centers, float* sizes, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * ScanNet AP association (the caller side of the path):
 * evaluation/utils_instance_seg_3d_eval.py:340-371 counts |pred_mask & (gt_ids == id)| per (prediction,
 * ground truth) pair with numpy.  counts[p][c] = number of points of prediction row p (mask byte != 0) whose
 * gt_index is c, for c in [0, n_cols); points with gt_index outside that range are not counted.  The caller
 * maps instance ids to columns (and void points to one extra column), so vert_count = the row sum.
 * masks [n, mask_stride] bytes; counts [n, n_cols] is zeroed by the call; n_cols <= 8192. */
int sd3d_mask_overlaps(const uint8_t* masks, int64_t mask_stride, int n, const int32_t* gt_index, int64_t N, int n_cols,
                       int32_t* counts, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Training criterion, segdino3d/models/loss/loss_3d.py.  One (decoder layer, scene) per call.
 * Shapes: cls [Q, n_cls1] (n_cls1 = instance classes + "no object"), masks [Q, S] logits over superpoints,
 * scores [Q] / centers [Q,3] / sizes [Q,3] nullable; ground truth: labels [G] int64, masks as bit rows
 * gt_bits [G, words] + gt_count [G] (sd3d_pack_mask_bits), gt_centers / gt_sizes [G, >=3] nullable,
 * query_masks [G, Q] bytes nullable ("query q lies in object g", loss_3d.py:358). */

/* bits[r][w] bit b = masks[r][32 w + b] != 0; counts[r] = set bits of the row (nullable). */
int sd3d_pack_mask_bits(const uint8_t* masks, int64_t ld, int n_rows, int n_cols, uint32_t* bits, int words, int32_t* counts,
                        void* stream);

/* cost [Q, G] = w0 * QueryClassificationCost + w1 * MaskBCECost + w2 * MaskDiceCost + w3 * CenterL1Cost + w4 * SizeL1Cost
 * (loss_3d.py:139-271 with the helpers :63-97); entries with query_masks[g][q] == 0 are 1e8 (SparseMatcher, :358-359).
 * weights5 is a HOST array. */
int sd3d_match_costs(const float* cls, int ld_cls, int n_cls1, const float* masks, int ld_masks, int Q, int S, const float* centers,
                     const float* sizes, const int64_t* labels, const uint32_t* gt_bits, int words, const int32_t* gt_count, int G,
                     const float* gt_centers, int ld_gc, const float* gt_sizes, int ld_gs, const uint8_t* query_masks,
                     const float* weights5, float* cost, void* stream);

/* SparseMatcher.__call__ (loss_3d.py:360-365): match[q][g] = cost[q][g] < (topk+1)-th smallest cost of column g. */
int sd3d_sparse_match(const float* cost, int Q, int G, int topk, uint8_t* match, void* stream);

/* HungarianMatcher.__call__ (loss_3d.py:274-312, scipy.optimize.linear_sum_assignment there): the minimum-cost one-to-one
 * assignment of n independent problems in one call (csrc/assign.hip: shortest augmenting paths in fp64, one workgroup per
 * problem).  Problem i is cost[i] [Q[i], G[i]] fp32 row-major; match[i] [Q[i], G[i]] bytes is fully overwritten with exactly
 * min(Q[i], G[i]) ones, at most one per row and per column (all zeros when Q[i] or G[i] is 0).  cost, Q, G, match are HOST
 * arrays of n entries (of device pointers / sizes) copied into the launches; n is not limited (one launch per SD3D_MAX_BATCH
 * problems).  status (device, n words, may be NULL): 0, or 1 where scipy would raise - a NaN or -inf entry, or no finite
 * assignment; the match of such a problem is still one-to-one.  +inf entries are ordinary values.  The result is an optimum;
 * where the optimum is not unique it need not be the one scipy picks. */
size_t sd3d_hungarian_match_ws_bytes(int n, const int* Q, const int* G);
int sd3d_hungarian_match_batch(int n, const float* const* cost, const int* Q, const int* G, uint8_t* const* match, int32_t* status,
                               void* ws, size_t ws_bytes, void* stream);

/* InstanceCriterion's per-scene terms of one layer (loss_3d.py:459-503 / :618-663) for a given match [Q, G] (from
 * sd3d_sparse_match or sd3d_hungarian_match_batch), and their gradients.
 * parts8 (device) = [class CE, mask BCE, mask dice, score MSE, centre L1, size L1, matched pairs, scores kept];
 * d_* = coef6[i] * d(parts[i]) / d(prediction): coef6 (HOST array) carries the loss weight and the batch-size factors
 * of :505-521 / :665-679, so the d_* buffers are the gradients of the total loss.  d_cls [Q, n_cls1], d_masks [Q, S],
 * d_scores [Q], d_centers / d_sizes [Q, 3] are fully overwritten (the nullable ones only when their prediction is given). */
size_t sd3d_instance_loss_ws_bytes(int Q);
int sd3d_instance_loss(const float* cls, int ld_cls, int n_cls1, const float* masks, int ld_masks, int Q, int S, const float* scores,
                       const float* centers, const float* sizes, const int64_t* labels, const uint32_t* gt_bits, int words,
                       const int32_t* gt_count, int G, const float* gt_centers, int ld_gc, const float* gt_sizes, int ld_gs,
                       const uint8_t* match, const float* class_weight, const float* coef6, float* d_cls, float* d_masks,
                       float* d_scores, float* d_centers, float* d_sizes, float* parts8, void* ws, size_t ws_bytes, void* stream);

/* ScanNetSemanticCriterion for one scene (loss_3d.py:37-60): sem [Q, ld] logits of which the first n_logits count,
 * sem_masks [n_rows, Q] bytes (target = first set row, 0 if none), rows with target == ignore_index are skipped.
 * loss[0] = mean NLL; d_sem [Q, ld_d] = coef * d loss / d sem (columns >= n_logits are zeroed). */
size_t sd3d_semantic_loss_ws_bytes(int Q);
int sd3d_semantic_loss(const float* sem, int ld, int Q, int n_rows, int n_logits, const uint8_t* sem_masks, int ignore_index, float coef,
                       float* d_sem, int ld_d, float* loss, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Backward of the pair-major sparse convolution (MinkowskiEngine / spconv autograd in the reference,
 * reached through train_engine_3d.py:88-122).  The input gradient is sd3d_pair_conv_ex on the transposed rulebook with
 * transposed weights; the weight gradient is
 *     dw[k][co][ci] (+)= sum over pairs p of offset k of dy[out_idx[p]][co] * x[in_idx[p]][ci]
 * with in_idx / tile_k from sd3d_pair_lists_desc and out_idx from sd3d_pair_out_rows (out_idx[pos[k][r]] = r, -1 on
 * padding).  dw is [K, Cout, Cin] like the forward weights; exact fp32 MFMA, fixed summation order.
 * flags: bit 0 = accumulate into dw, bit 1 = round both operands to bf16 (nearest even) before multiplying - the numbers
 * of a bf16-operand product with fp32 accumulation, for the bf16 training mode of the decoder; bit 2 (K = 1: a Linear) =
 * dw has Cout more floats after the [Cout, Cin] block and receives the bias gradient there (column sums of dy over the
 * listed rows), formed from the dy rows the kernel has staged anyway. */
#define SD3D_WGRAD_ACCUMULATE 1
#define SD3D_WGRAD_BF16_OPERANDS 2
#define SD3D_WGRAD_BIAS 4
int sd3d_pair_out_rows(const int32_t* pos, int K, int64_t M, int64_t p_cap, int32_t* out_idx, void* stream);
size_t sd3d_pair_wgrad_ws_bytes(int K, int Cin, int Cout);
int sd3d_pair_wgrad(const float* dy, int ld_dy, const float* x, int ld_x, const int32_t* in_idx, const int32_t* out_idx,
                    const int32_t* tile_k, int64_t p_cap, int K, int Cin, int Cout, float* dw, int flags, void* ws, size_t ws_bytes,
                    void* stream);

/* Weight and bias gradient of a Linear on a few thousand rows in ONE launch (the decoder's ~130 Linears per training step):
 * dw [Cout, Cin] (+)= g^T x, db [Cout] (+)= column sums of g (db may be NULL); g [M, ld_g >= round4(Cout)] (act'-scaled output gradient),
 * x [M, ld_x >= round4(Cin)], both strides multiples of 4 floats.  A workgroup owns a 32 x 32 block of dw for all rows (rounds of 128 rows staged
 * in LDS, sixteen waves, their accumulators summed in a fixed order: bit-reproducible).
 * flags: SD3D_WGRAD_ACCUMULATE, SD3D_WGRAD_BF16_OPERANDS.  For tens of thousands of rows sd3d_pair_wgrad (row ranges + reduce) is the one. */
int sd3d_linear_wgrad(const float* g, int ld_g, const float* x, int ld_x, int64_t M, int Cin, int Cout, float* dw, float* db, int flags,
                      void* stream);

/* ---------------------------------------------------------------------------------------------
 * Training-mode BatchNorm over voxel rows (ME.MinkowskiBatchNorm = nn.BatchNorm1d, minkunet.py:302-304) with the
 * BasicBlock's residual add and ReLU folded in (:234-250), and the backward of sd3d_pool_superpoints (:668-676).
 * x, y, dy, dx, res, dres are [M, C] fp32 with row strides in floats; act: 0 none, 1 relu.
 *   sd3d_bn_stats_running: mean[c], var[c] (biased), rstd[c] = 1 / sqrt(var + eps) over the M rows
 *   sd3d_bn_apply:         y = act((x - mean) * rstd * gamma + beta + res)            (res nullable)
 *   sd3d_bn_backward:      g = dy masked by y > 0 when act == relu; dbeta = sum g; dgamma = sum g * xhat;
 *                          dx = gamma * rstd * (g - dbeta / M - xhat * dgamma / M); dres = g (nullable)
 * Reductions run in a fixed order (bit-reproducible) and in double.  ws: sd3d_bn_ws_bytes(M, C), aligned to 8 bytes. */
size_t sd3d_bn_ws_bytes(int64_t M, int C);
/* sd3d_bn_stats_running also advances nn.BatchNorm1d's buffers in place (any of the three may be NULL: then it only computes
 * the statistics): running_mean = (1 - momentum) running_mean + momentum mean, running_var likewise with the UNBIASED batch variance
 * (var * M / (M - 1)), num_batches_tracked += 1 (torch/nn/modules/batchnorm.py semantics behind minkunet.py:302-304). */
int sd3d_bn_stats_running(const float* x, int ld, int64_t M, int C, float eps, float* mean, float* var, float* rstd,
                          float* running_mean, float* running_var, int64_t* num_batches_tracked, float momentum, void* ws,
                          size_t ws_bytes, void* stream);
int sd3d_bn_apply(const float* x, int ld_x, const float* mean, const float* rstd, const float* gamma, const float* beta, const float* res,
                  int ld_res, int64_t M, int C, int act, float* y, int ld_y, void* stream);
int sd3d_bn_backward(const float* dy, int ld_dy, const float* y, int ld_y, const float* x, int ld_x, const float* mean, const float* rstd,
                     const float* gamma, int64_t M, int C, int act, float* dx, int ld_dx, float* dres, int ld_dres, float* dgamma,
                     float* dbeta, void* ws, size_t ws_bytes, void* stream);
/* dfeat[v] = sum over the points p of voxel v (sidx[seg_start[v] .. seg_start[v+1])) of dout[sp[p]] / max(|sp[p]|, 1),
 * with |s| = sp_start[s+1] - sp_start[s]; dout [S, C], C <= 128. */
int sd3d_pool_superpoints_backward(const float* dout, int C, const int64_t* superpoints, const uint32_t* sidx, const int32_t* seg_start,
                                   const int32_t* sp_start, int64_t V, float* dfeat, int ld, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Train-time augmentation, segdino3d/datasets/transform/point_cloud_transforms.py.  The random draws are
 * the caller's (numpy.random in the reference's order); trans3 / color_* are HOST arrays.
 *   sd3d_augment_points:   in place on points[:, 0:3]: flip x / y (:112-117), rotate by `angle` about z (points @ rot_mat_T
 *                          of mmdet3d's rotation_3d_in_axis, :284-300), scale (:312), translate (:255); with color_mean3 also
 *                          points[:, 3:6] = (rgb - mean) / std (:382-387).  Also used for query2d_pos (ld = 3, no colour).
 *   sd3d_voxel_units:      coords [n, 3] = points[:, 0:3] / voxel_size (:417)
 *   sd3d_box_blur3:        scipy.ndimage.convolve(ones(3) / 3 along `axis`, mode="constant") on `grids` volumes (:455-459)
 *   sd3d_elastic_displace: coords += mag * trilinear(noise [3, D0, D1, D2]) on the grid linspace(-(b-1) gran, (b-1) gran, b)
 *                          per axis, zero outside (:461-470) */
int sd3d_augment_points(float* points, int ld, int64_t n, int flip_x, int flip_y, float angle, float scale, const float* trans3,
                        const float* color_mean3, const float* color_std3, void* stream);
int sd3d_voxel_units(const float* points, int ld, int64_t n, float voxel_size, float* coords, void* stream);
int sd3d_box_blur3(const float* in, float* out, int grids, int D0, int D1, int D2, int axis, void* stream);
int sd3d_elastic_displace(float* coords, int64_t n, const float* noise, int D0, int D1, int D2, float gran, float mag, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Backward pieces of the query decoder; torch autograd over nn.Linear / nn.LayerNorm / elementwise ops in
 * the reference (instance_seg_3d_decoder.py:640-797).
 *   sd3d_act_backward:       g[:, :C] = dy * act'(.), g[:, C:C_pad] = 0.  act as in sd3d_gather_gemm; ref = forward OUTPUT for
 *                            relu / sigmoid, PRE-activation for gelu.  The Linear's input / weight gradients are then
 *                            sd3d_gather_gemm(g, W^T) and sd3d_pair_wgrad on identity pair lists, its bias gradient sd3d_col_sums(g).
 *   sd3d_col_sums:           out[c] = sum_r x[r][c], fixed order.
 *   sd3d_layernorm_backward: for y = act(LayerNorm(x + res) * w + b): dxin = d/d(x + res) [M, D], dw, db (act 0 / 1 = relu).
 *   sd3d_sine_pe_mod_backward: gradient of sd3d_sine_pe's box modulation w.r.t. mod_num [n, 3] (positions and mod_den are
 *                            detached in the reference, :740, :753). */
/* ---------------------------------------------------------------------------------------------
 * Training step of a sparse U-Net from two calls (csrc/train_plan.hip; segdino3d_amd/train_plan.py records the plan): the forward of every
 * {sparse convolution -> batch-statistics BatchNorm (+ residual) -> ReLU} layer of Res16UNetBase.forward (minkunet.py:531-601), and the
 * backward of the same list in reverse (what `loss.backward()` of train_engine_3d.py:88-122 gets from MinkowskiEngine's autograd).
 * A buffer (sd3d_buf) may hold the outputs of several layers side by side (`*_col` = first column of a layer's slice): a skip concatenation
 * is the two producers writing into one buffer.  Every pointer is device memory owned by the caller; the calls only enqueue.
 * ------------------------------------------------------------------------------------------- */
typedef struct sd3d_train_table {
    const int32_t *in_idx, *tile_k, *pos, *rlist;   /* sd3d_pair_lists_desc products of the table (plain lists, with the position table) */
    const int32_t *out_rows;                        /* [p_cap] output row of every list entry (sd3d_pair_out_rows / the table's out_idx) */
    int64_t p_cap, M;
    int32_t K, rl_stride, center, direct;           /* direct = 1: one pair per output row (transposed k2s2 convolution): pass 1 writes the rows */
} sd3d_train_table;
typedef struct sd3d_train_layer {
    int32_t table, table_t, mirrored;               /* forward table; table of the transposed rulebook (-1: no input gradient); 1: stride-1 table (its own transpose, offsets mirrored) */
    int32_t src, src_col, res, res_col, dst, dst_col;   /* buffer ids + first column of the slice; res = -1: no residual */
    int32_t raw;                                    /* raw[] id of the convolution output in front of the BatchNorm, [rows, Cout] */
    int32_t K, Cin, Cout, act;                      /* Cin = columns read from src (the stem's are zero-padded to a multiple of 32) */
    int32_t need_dx, dx_accum;                      /* need_dx = 0: the input carries no gradient; dx_accum = 1: grad[src] already holds one when this layer's arrives */
    int32_t stats, pad_;                            /* offset (floats) of {mean, var, rstd} x Cout in the statistics arena */
    float eps, momentum;
    const float *wt_fwd, *kernel;                   /* [K, Cout, Cin] copy for the forward; the parameter [K, Cin, Cout] (input gradient) */
    float* dkernel;                                 /* [K, Cin, Cout] gradient of the parameter */
    const float *gamma, *beta;
    float *dgamma, *dbeta, *running_mean, *running_var;
    int64_t* num_batches;
} sd3d_train_layer;
int sd3d_unet_train_forward(const sd3d_train_layer* layers, int n_layers, const sd3d_train_table* tables, int n_tables, const sd3d_buf* act,
                            int n_bufs, const sd3d_buf* raw, int n_raw, float* stats, float* part, size_t part_bytes, void* ws, size_t ws_bytes,
                            void* stream);
/* grad[]: gradient buffers, ids / shapes of act[] (d loss / d output already in the output's buffer); graw: scratch of max(rows x Cout) floats;
 * ws >= max(sd3d_bn_ws_bytes, sd3d_pair_wgrad_ws_bytes) over the layers. */
int sd3d_unet_train_backward(const sd3d_train_layer* layers, int n_layers, const sd3d_train_table* tables, int n_tables, const sd3d_buf* act,
                             const sd3d_buf* grad, int n_bufs, const sd3d_buf* raw, int n_raw, const float* stats, float* graw, size_t graw_floats,
                             float* part, size_t part_bytes, void* ws, size_t ws_bytes, void* stream);

/* dst_i [cols_i, ld_dst_i] = src_i [rows_i, cols_i]^T, columns rows_i .. ld_dst_i - 1 zero, for n matrices in as few launches as
 * their descriptors fit (112 per launch): all the W^T the Linear input gradients of one backward pass need
 * (`x.grad = dy @ W` of every nn.Linear in instance_seg_3d_decoder.py), made at once instead of one copy kernel per weight. */
typedef struct sd3d_transpose_job {
    const float* src; float* dst;
    int32_t rows, cols, ld_dst, batch;   /* batch > 1: that many matrices back to back in src ([rows, cols] each) and dst ([cols, ld_dst] each): the
                                          * [K, Cin, Cout] -> [K, Cout, Cin] weights of a sparse convolution as ONE job (0 / 1: one matrix) */
} sd3d_transpose_job;
int sd3d_transpose_batch(int n, const sd3d_transpose_job* jobs, void* stream);
int sd3d_act_backward(const float* dy, int ld_dy, const float* ref, int ld_ref, int act, int64_t M, int C, int C_pad, float* g, int ld_g,
                      void* stream);
size_t sd3d_col_sums_ws_bytes(int64_t M, int C);
int sd3d_col_sums(const float* x, int ld, int64_t M, int C, float* out, void* ws, size_t ws_bytes, void* stream);
size_t sd3d_layernorm_backward_ws_bytes(int64_t M, int D);
int sd3d_layernorm_backward(const float* dy, int ld_dy, const float* y, int ld_y, const float* x, int ld_x, const float* res, int ld_res,
                            const float* w, float eps, int64_t M, int D, int act, float* dxin, int ld_dx, float* dw, float* db, void* ws,
                            size_t ws_bytes, void* stream);
/* backward of sd3d_box_refine w.r.t. the two head outputs (d_center, d_size_out nullable = zero gradient). */
int sd3d_box_refine_backward(const float* d_center, const float* d_size_out, const float* size, const float* range, int normalize, int64_t Q,
                             float* d_dc, float* d_ds, void* stream);
int sd3d_sine_pe_mod_backward(const float* d_out, int ld_do, const float* xyz, int ld_xyz, int64_t n, const float* range, const float* dim_t,
                              const int8_t* axis, int d_pos, const float* mod_den, int ld_den, float* d_num, void* stream);

/* Attention for training: sd3d_attention with lse [H, Lq] = log sum exp of every masked, scaled score row kept
 * (fp32 or, for mixed-precision training, the bf16 forward), and the backward pass (gradients of attention.py:361-385 /
 * nn.MultiheadAttention, decoder :79): given out, lse and d_out -> dq0 (dq1), dk0 (dk1), dv with the shapes / strides of their forward
 * tensors.  Exact fp32 MFMA, P recomputed tile by tile, fixed summation order.  head_dim: 32 or 64, else SD3D_ERR_ARG before anything is
 * launched.  ws: sd3d_attention_backward_ws_bytes (one float per head and query, D = dO . O; 0 for an unsupported width).
 * key, call, p: those of the forward call (out and lse as that call left them).  With p > 0: dV = (c K o P)^T dO, dP = c K o (dO V^T),
 * dS = P o (dP - D) with D = dO . O as without dropout; the kernels regenerate the keep mask K.  p == 0 launches the kernels without
 * dropout and ignores key; p outside [0, 1) or p > 0 with a NULL key returns SD3D_ERR_ARG before anything is launched. */
size_t sd3d_attention_backward_ws_bytes(int Lq, int H, int head_dim);
int sd3d_attention_backward(const float* q0, int ldq0, const float* q1, int ldq1, const float* k0, int ldk0, const float* k1, int ldk1,
                            const float* v, int ldv, const uint32_t* mask_bits, int Lq, int Lk, int H, int head_dim, float scale,
                            const float* out, int ldo, const float* lse, const float* d_out, int ld_do, float* dq0, int ld_dq0,
                            float* dq1, int ld_dq1, float* dk0, int ld_dk0, float* dk1, int ld_dk1, float* dv, int ld_dv, void* ws,
                            size_t ws_bytes, const uint32_t* key, int call, float p, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Parameter update of a training iteration (csrc/optim.hip; segdino3d_amd/optim.py builds the tables): gradient-norm clipping, the AdamW
 * step and the weight EMA of train_engine_3d.py:99-120 / ema_utils.py:34-38, each one launch over ALL parameter tensors.
 *
 * Tensor table: one sd3d_mt_tensor per parameter that has a gradient this step.  fp32, contiguous; p / m / v / ema / g must be 4-byte aligned,
 * 16-byte aligned ones take the 16-byte path (an unaligned g alone only makes its loads scalar).  The scalars are this tensor's own (torch
 * keeps `step` per parameter, the groups have their own lr), folded by the caller in double precision and rounded once to float:
 *   decay = 1 - lr * weight_decay, step_size = lr / (1 - beta1^t), rsqrt_bc2 = 1 / sqrt(1 - beta2^t), t = this tensor's step AFTER the increment.
 * Chunk list: chunk c covers elements [index * SD3D_MT_CHUNK, min(n, (index + 1) * SD3D_MT_CHUNK)) of tensors[tensor]; every element of
 * every tensor must be in exactly one chunk (the entry points check that chunks lie inside their tensors, not that they cover them).
 *
 * Both tables are HOST arrays.  A call copies them into ws with hipMemcpyAsync on `stream` and returns without waiting: keep them unchanged
 * until the stream has passed the copy, and keep them in pinned memory if the call is not to block.  table_resident = 1 skips the copy: ws
 * still holds this very table from the previous sd3d_mt_* call (same ws, same stream).  ws: sd3d_mt_ws_bytes, 16-byte aligned, device.
 *
 *   sd3d_mt_grad_norm: norm_out[0] = total_norm = ||all g||_2, norm_out[1] = clip_coef = min(1, max_norm / (total_norm + 1e-6)) (device floats).
 *                      One partial sum per chunk, added in chunk order in double precision: no atomics, the same bits in every run.
 *   sd3d_mt_adamw:     g' = g * *clip_coef (clip_coef = null: g' = g; g itself is never written);  p *= decay;  m += (1 - beta1) (g' - m);
 *                      v = beta2 v + (1 - beta2) g'^2;  p -= step_size * m / (sqrt(v) * rsqrt_bc2 + eps);  and where ema is not null
 *                      ema = (1 - ema_decay) p + ema_decay ema with the new p, in the same pass.
 *   sd3d_mt_ema:       ema = (1 - ema_decay) p + ema_decay ema alone (tensors whose ema is null are skipped; g, m, v are not read).
 * ------------------------------------------------------------------------------------------- */
#define SD3D_MT_CHUNK 4096
typedef struct sd3d_mt_tensor {
    float *p, *m, *v, *ema;                         /* parameter, exp_avg, exp_avg_sq, EMA shadow (null: none) */
    const float* g;                                 /* gradient */
    int64_t n;                                      /* elements */
    float decay, step_size, rsqrt_bc2;
    float one_minus_beta1, beta2, one_minus_beta2, eps;
    float ema_decay, one_minus_ema_decay, pad_;
} sd3d_mt_tensor;
typedef struct sd3d_mt_chunk { int32_t tensor, index; } sd3d_mt_chunk;
size_t sd3d_mt_ws_bytes(int n_tensors, int64_t n_chunks);
int sd3d_mt_grad_norm(const sd3d_mt_tensor* tensors, int n_tensors, const sd3d_mt_chunk* chunks, int64_t n_chunks, float max_norm,
                      float* norm_out, void* ws, size_t ws_bytes, void* stream);
int sd3d_mt_adamw(const sd3d_mt_tensor* tensors, int n_tensors, const sd3d_mt_chunk* chunks, int64_t n_chunks, const float* clip_coef,
                  int table_resident, void* ws, size_t ws_bytes, void* stream);
int sd3d_mt_ema(const sd3d_mt_tensor* tensors, int n_tensors, const sd3d_mt_chunk* chunks, int64_t n_chunks, int table_resident, void* ws,
                size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Dataset targets: raw per-point labels -> the fields the model and the criterion read (the label side of the reference's
 * `Dataset.__getitem__`: scannet200.py:155-193 adjust_class_ids_ / exclude_stuffs_ / merge_stuffs_, :243-253 superpoint votes,
 * :291-326 split_instance_gt, and instance_seg_3d_preparer.py).  Integers only; every result is a pure function of the input.
 *
 *   sd3d_targets_scan(instance_mask, semantic_mask, super_points [n] int64, lut [lut_len] int64, ...): pass 1.
 *     sem = lut[swap_2_3 ? (2 <-> 3)(raw) : raw]; points whose sem is a stuff id (ascending class ids, at most 8) or n_classes get
 *     instance -1; the distinct masked instance ids are ranked.  Writes the header, four int32 at the START of `ws`:
 *       [0] status: OR of SD3D_TARGETS_BAD_*;  [1] G' = distinct masked ids - 1 (new id = rank - 1: with no background point the
 *       smallest instance becomes -1, as in the reference);  [2] S = largest superpoint id + 1;  [3] bit k: stuff id k occurs.
 *     The caller copies these 16 bytes to the host (the one read-back) and sizes the outputs from them.
 *   sd3d_targets_rows(header, n_stuff, val_view): G, the number of mask rows: G' (train view) or G' + present stuff classes.
 *   sd3d_targets_build(n, header (HOST copy), ...): pass 2 on the SAME `ws`.  A non-zero status returns SD3D_ERR_RANGE and names the
 *     status in sd3d_last_error.  Outputs:
 *       masks [G, n] bytes 0/1, labels / area [G] int64 (may be NULL when G = 0): row order = ascending id.  Train view: row g = new id g,
 *         label = sem at the row's lowest point index - n_stuff.  Val view (merge_stuffs_): the present stuff classes first (all points
 *         of the class, label = the class), then the instances, labels not shifted.
 *       seg_start [S + 1], sp_inst [S], sp_sem [S] int32: start of every superpoint in the sorted order; the instance (new id, -1: none)
 *         and class (n_classes: none) that hold MORE THAN HALF of the superpoint's points, 2 k > n.
 *       sp_masks [G' + n_classes + 1, S] bytes 0/1: rows g < G': sp_inst == g; then sp_sem == c.  Votes are taken before the val merge.
 *   ws: sd3d_targets_ws_bytes(n) bytes, untouched between the two calls.  1 <= n <= 0x7F000000.
 * ------------------------------------------------------------------------------------------- */
#define SD3D_TARGETS_BAD_SEMANTIC 1      /* a raw semantic id outside [0, lut_len) */
#define SD3D_TARGETS_BAD_INSTANCE 2      /* a raw instance id outside [-1, 2^20) */
#define SD3D_TARGETS_BAD_SUPERPOINT 4    /* a superpoint id outside [0, 2^31 - 2] */
size_t sd3d_targets_ws_bytes(int64_t n);
int sd3d_targets_scan(const int64_t* instance_mask, const int64_t* semantic_mask, const int64_t* super_points, int64_t n,
                      const int64_t* lut, int64_t lut_len, int n_classes, const int32_t* stuff_ids, int n_stuff, int swap_2_3,
                      void* ws, size_t ws_bytes, void* stream);
int sd3d_targets_rows(const int32_t* header, int n_stuff, int val_view);
int sd3d_targets_build(int64_t n, const int32_t* header, int n_classes, const int32_t* stuff_ids, int n_stuff, int val_view,
                       uint8_t* masks, int64_t* labels, int64_t* area, int32_t* seg_start, int32_t* sp_inst, int32_t* sp_sem,
                       uint8_t* sp_masks, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Benchmark submission text (csrc/submit.hip): the bytes `np.savetxt(path, x, fmt='%d')` writes, made on the device
 * (evaluator_3d.py:351-396 format_results_semantic / save_single_instance).  The host copies them and calls write().
 *
 *   sd3d_mask_text(masks [*, N] bytes, N, rows [n_rows] | NULL = rows 0..n_rows-1, n_rows, out [n_rows, pitch], pitch):
 *     the byte table and row list of sd3d_pack_mask_rows.  out[r * pitch + 2 p] = '0' + (masks[rows[r]][p] != 0),
 *     out[r * pitch + 2 p + 1] = '\n': the first 2 N bytes of row r are the file of mask rows[r]; the bytes behind them are not
 *     written.  pitch >= 2 N, pitch % 16 == 0 and `out` 16-byte aligned, N >= 1, n_rows >= 0 (SD3D_ERR_ARG otherwise); n_rows == 0
 *     does nothing.  Row indices may repeat, in any order.
 *   sd3d_label_text(values [N] int64, N, lut [lut_len] int32 | NULL, lut_len, out [out_cap], out_cap, info [2], ws, ws_bytes):
 *     line p = the decimal text of lut[values[p]] (of values[p] without a table) + '\n', as '%d' prints an int32 ('-', -2147483648
 *     included); the lines stand back to back from out[0] on.  info[0] = length of the whole text in bytes, info[1] = status, OR of
 *     SD3D_LABEL_TEXT_*: a line whose value cannot be printed is left out (no clamp, no wrap), and a text longer than out_cap is cut
 *     at out_cap - nothing is written at or behind out + out_cap (info[0] is still the full length).  `out` 16-byte aligned.
 *     0 <= N <= (2^31 - 1) / 12; N == 0 writes info = {0, 0} only.  ws: sd3d_label_text_ws_bytes(N) bytes.
 * ------------------------------------------------------------------------------------------- */
#define SD3D_LABEL_TEXT_BAD_INDEX 1      /* with a table: a value outside [0, lut_len) */
#define SD3D_LABEL_TEXT_BAD_VALUE 2      /* without a table: a value outside int32 */
#define SD3D_LABEL_TEXT_OVERFLOW 4       /* the text is longer than out_cap */
int sd3d_mask_text(const uint8_t* masks, int64_t N, const int32_t* rows, int n_rows, uint8_t* out, int64_t pitch, void* stream);
size_t sd3d_label_text_ws_bytes(int64_t N);
int sd3d_label_text(const int64_t* values, int64_t N, const int32_t* lut, int lut_len, uint8_t* out, int64_t out_cap, int32_t* info,
                    void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Semantic and panoptic evaluation (csrc/segeval.hip): what mmdet3d's `seg_eval` (fast_hist) and `panoptic_seg_eval`
 * (EvalPanoptic.add_batch_panoptic, the SemanticKITTI protocol) count per scene, added into DEVICE-RESIDENT accumulators that persist
 * across scenes (evaluation/evaluator_3d.py:128-163 collects the inputs, :184-196 would score them).  Both calls only enqueue work.
 * Label arrays are int64 [n] with an element stride each (any stride >= 0: views are read in place), 0 <= n <= 0x7F000000 (n == 0
 * does nothing), 1 <= n_classes <= SD3D_SEG_EVAL_MAX_CLASSES.  `status` is one int64 word, OR of SD3D_SEG_EVAL_*; it is only ever
 * OR-ed into.  Integer results do not depend on the order of the points; iou_sum is added in a fixed order (same bits on every run).
 *
 *   sd3d_semantic_confusion: confusion [n_classes, n_classes] int64, rows = ground truth, columns = prediction.  A point counts when
 *     its ground truth is not ignore_index and lies in [0, n_classes).  A prediction outside [0, n_classes) on such a point sets
 *     SD3D_SEG_EVAL_BAD_PRED_CLASS and the point is skipped (no clamp, no write outside the table).
 *   sd3d_panoptic_accumulate: tp / fp / fn [n_classes] int64, iou_sum [n_classes] double.  Instance ids are shifted by +1 (-1 = no
 *     instance); points whose ground-truth class is one of ignore_ids_host (HOST array, at most SD3D_SEG_EVAL_MAX_IGNORE) are dropped
 *     from both sides.  Per class that is not ignored: segments = distinct positive shifted ids among the points of that class on the
 *     ground-truth / prediction side, area = their point count; a (gt, pred) pair of one class with 2 * inter > area_gt + area_pred -
 *     inter is a true positive and adds inter / union (float64) to iou_sum; unmatched segments of area >= min_num_points count into
 *     fn / fp.  A shifted id outside [0, 2^16) on a kept point sets SD3D_SEG_EVAL_BAD_INSTANCE_ID and counts as "no instance".
 *     More than SD3D_SEG_EVAL_MAX_SEGMENTS segments on one side of one scene set SD3D_SEG_EVAL_TOO_MANY_SEGMENTS; the segments past
 *     the capacity are left out, nothing is written outside a buffer.  ws: sd3d_seg_eval_ws_bytes(n, n_classes) bytes.
 * ------------------------------------------------------------------------------------------- */
#define SD3D_SEG_EVAL_BAD_PRED_CLASS 1         /* a semantic prediction outside [0, n_classes) on a counted point */
#define SD3D_SEG_EVAL_BAD_INSTANCE_ID 2        /* a shifted instance id outside [0, 2^16) */
#define SD3D_SEG_EVAL_TOO_MANY_SEGMENTS 4      /* more than SD3D_SEG_EVAL_MAX_SEGMENTS segments on one side of a scene */
#define SD3D_SEG_EVAL_MAX_CLASSES 1024
#define SD3D_SEG_EVAL_MAX_IGNORE 8
#define SD3D_SEG_EVAL_MAX_SEGMENTS 65536
size_t sd3d_seg_eval_ws_bytes(int64_t n, int n_classes);
int sd3d_semantic_confusion(const int64_t* pred_sem, int64_t pred_stride, const int64_t* gt_sem, int64_t gt_stride, int64_t n,
                            int n_classes, int64_t ignore_index, int64_t* confusion, int64_t* status, void* stream);
int sd3d_panoptic_accumulate(const int64_t* pred_sem, int64_t pred_sem_stride, const int64_t* pred_inst, int64_t pred_inst_stride,
                             const int64_t* gt_sem, int64_t gt_sem_stride, const int64_t* gt_inst, int64_t gt_inst_stride, int64_t n,
                             int n_classes, const int32_t* ignore_ids_host, int n_ignore, int min_num_points, int64_t* tp, int64_t* fp,
                             int64_t* fn, double* iou_sum, int64_t* status, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * ScanNet instance AP, streamed (csrc/apeval.hip): the protocol of evaluation/utils_instance_seg_3d_eval.py (`evaluate_matches`
 * :18-209) decomposed per scene.  sd3d_ap_scene enqueues, for one scene, the association (points -> ground-truth columns,
 * sd3d_mask_overlaps on SD3D_AP_COLS columns) and the greedy matching of every (class, overlap) pair, and leaves ENTRIES in a store
 * that stays on the device; sd3d_ap_finish sorts the entries of all scenes and evaluates the precision / recall curve of every
 * (class, overlap) group.  Both calls only enqueue work.  `status` is one int64 word, OR of SD3D_AP_*; it is only ever OR-ed into.
 *
 *   Entry = one int64 code: ((class * n_overlaps + overlap) << 33) | (sortable(fp32 score) << 1) | true, sortable() the transform of
 *     sd3d_keys_from_f32 (ascending).  The sentinel (n_classes * n_overlaps) << 33 sorts behind every entry and is no entry.
 *   sd3d_ap_scene:
 *     gt_sem / gt_inst: int64 [N] with an element stride each.  id_map != NULL: the reference's `map_inst_markup` is applied first
 *       (ids shifted down by num_stuff, negative instance ids -> -1 and their semantic id -> -1, semantic id -> id_map[id] with an
 *       index in [-map_len, 0) counted from the back; an index outside [-map_len, map_len) reads as -1).  id_map == NULL: ids as given.
 *     class_lut: int32 [lut_len], dataset id -> class index in [0, n_classes) or -1.  A point whose semantic id has a class and whose
 *       instance index i lies in [0, SD3D_AP_INSTANCE_COLS) belongs to ground-truth instance i (column i; instances are processed in
 *       ascending i, the order of the reference's `get_instances`); instance index -1 or a semantic id without a class: the void
 *       column; semantic id 0 with a class and instance index 0: no column (the reference counts such a point nowhere).  An instance
 *       index outside [-1, SD3D_AP_INSTANCE_COLS) sets SD3D_AP_BAD_INSTANCE and the point is void; an instance whose points carry two
 *       classes sets SD3D_AP_MIXED_SEMANTIC (the larger class index is used).
 *       Where this differs from the host route (`rename_gt` + `assign_scene`): only with dataset id 0 among the classes.  There an
 *       instance whose semantic id has NO class keeps an id below 1000 and is read as a ground-truth instance of the class of id 0;
 *       here its points are void, as with every other label set.
 *     masks: uint8 [n, N], row pitch mask_stride, non-zero = member; 0 <= n <= SD3D_AP_MAX_PREDS.  labels: int64 [n] class INDEX,
 *       scores: float [n].  A label outside [0, n_classes) sets SD3D_AP_BAD_LABEL, a non-finite score SD3D_AP_BAD_SCORE; such a
 *       prediction is left out, as is (silently) one with fewer than min_region points.
 *     overlaps: DEVICE double [n_overlaps], each in (0, 1), n_overlaps <= SD3D_AP_MAX_OVERLAPS; slots_host: HOST int32 [n_overlaps],
 *       the entries one prediction can emit at that overlap (max(1, ceil(1 / th) - 1): IoU > th needs inter > th * |pred| and ground
 *       truths are disjoint).  zero_class: the class index of dataset id 0, or -1.
 *     The scene owns the slots store[slot_begin .. slot_begin + n * sum(slots_host)) and writes EVERY one of them that lies below
 *       slot_begin + slot_cap, an entry or the sentinel: slot of entry j of prediction row r at overlap o =
 *       n * sum(slots_host[:o]) + r * slots_host[o] + j.  What does not fit (a slot past slot_cap, more entries than slots_host[o])
 *       is dropped and sets SD3D_AP_STORE_FULL; nothing is written outside the range.
 *     hard_fn int64 [n_classes * n_overlaps] += ground truths of >= min_region points that no prediction matched; has_gt / has_pred
 *       int64 [n_classes] |= 1.  Comparisons are the reference's, in float64: double(inter) / double(gt + pred - inter) > th and
 *       double(void + intersections with ground truth below min_region) / double(pred) <= th.  ws: sd3d_ap_scene_ws_bytes(N, n).
 *   sd3d_ap_finish: codes int64 [n_slots] (clobbered: sorted in place or into the workspace).  ap double [n_classes * n_overlaps],
 *     pr_rc double [2 * n_classes * n_overlaps] (precision, then recall, at the FIRST maximum of f1 = 2 p r / (p + r + 0.0001)).  A class
 *     with ground truth and predictions: the curve over the distinct scores plus the closing point (1, 0), AP = sum prec[i] *
 *     (0.5 r[i-1] - 0.5 r[i+1]) with r[-1] = r[0] and a trailing 0, summed per thread in ascending i and over threads in a fixed tree;
 *     ground truth only: 0, 0, 0; otherwise NaN.  ws: sd3d_ap_finish_ws_bytes(n_slots).
 * ------------------------------------------------------------------------------------------- */
#define SD3D_AP_BAD_INSTANCE 1           /* an instance index outside [-1, SD3D_AP_INSTANCE_COLS) */
#define SD3D_AP_MIXED_SEMANTIC 2         /* one ground-truth instance over two classes */
#define SD3D_AP_BAD_LABEL 4              /* a prediction label outside [0, n_classes) */
#define SD3D_AP_BAD_SCORE 8              /* a non-finite prediction score */
#define SD3D_AP_STORE_FULL 16            /* more entries than the store (or a prediction's slots) holds */
#define SD3D_AP_INSTANCE_COLS 1000
#define SD3D_AP_COLS 1002                /* instances, void, "counted nowhere" */
#define SD3D_AP_MAX_CLASSES 1024
#define SD3D_AP_MAX_OVERLAPS 16
#define SD3D_AP_MAX_PREDS 4096
size_t sd3d_ap_scene_ws_bytes(int64_t N, int n);
int sd3d_ap_scene(const int64_t* gt_sem, int64_t sem_stride, const int64_t* gt_inst, int64_t inst_stride, int64_t N,
                  const int64_t* id_map, int map_len, int num_stuff, const uint8_t* masks, int64_t mask_stride, int n,
                  const int64_t* labels, const float* scores, const int32_t* class_lut, int lut_len, int zero_class, int n_classes,
                  const double* overlaps, const int32_t* slots_host, int n_overlaps, int min_region, int64_t* store,
                  int64_t slot_begin, int64_t slot_cap, int64_t* hard_fn, int64_t* has_gt, int64_t* has_pred, int64_t* status, void* ws,
                  size_t ws_bytes, void* stream);
size_t sd3d_ap_finish_ws_bytes(int64_t n_slots);
int sd3d_ap_finish(int64_t* codes, int64_t n_slots, int n_classes, int n_overlaps, const int64_t* hard_fn, const int64_t* has_gt,
                   const int64_t* has_pred, double* ap, double* pr_rc, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * ScanNet instance AP per scene (csrc/apeval_scene.hip): `compute_each_sample_metrics` (evaluation/evaluator_3d.py:227-321), which
 * scores one scene at a time.  The caller gives every scene its own counter row to sd3d_ap_scene: counters int64
 * [n_scenes, n_classes * n_overlaps + 2 * n_classes], a row = hard_fn [C, O], has_gt [C], has_pred [C].  Both calls only enqueue work.
 *   sd3d_ap_finish_scenes: codes int64 [n_slots], the store as sd3d_ap_scene left it (READ only; a group above the sentinel's reads as
 *     the sentinel).  slot_offsets: DEVICE int64 [n_scenes + 1], ascending from 0 to n_slots: scene s owns the slots
 *     [slot_offsets[s], slot_offsets[s + 1]); empty scenes are allowed.  Every slot gets the key
 *     (s * (C O + 1) + group) << 33 | low 33 bits of its code in the workspace, the keys are sorted, and every (scene, class, overlap)
 *     segment is scored by the curve body of sd3d_ap_finish with the scene's counters: a class without ground truth in THAT scene is
 *     NaN, with ground truth but no prediction in that scene 0.  n_scenes * (C O + 1) must stay below 2^30 (SD3D_ERR_ARG otherwise,
 *     nothing is launched).  ap double [n_scenes, C, O], pr_rc double [2, n_scenes, C, O], summary double [n_scenes, 5]: the means of
 *     `compute_averages` over the scene's finite cells, NaN without one - all_ap (overlaps whose bit is NOT set in mask25), all_ap_50%
 *     (bits of mask50), all_ap_25% (bits of mask25), all_prec_50%, all_rec_50% (mask50); bit o of a mask = overlap o.  Each mean is
 *     summed per lane over cells lane, lane + 64, .. in class-major order and over the 64 lanes in a fixed butterfly, in float64.
 *     ws: sd3d_ap_finish_scenes_ws_bytes(n_slots).
 *   sd3d_ap_reduce_counters: out int64 [C O + 2 C] = the rows of counters reduced in integers, hard_fn added, has_gt / has_pred 0 / 1
 *     (OR): the counters sd3d_ap_scene leaves when all scenes share one row.  n_scenes == 0 gives zeros.
 * ------------------------------------------------------------------------------------------- */
size_t sd3d_ap_finish_scenes_ws_bytes(int64_t n_slots);
int sd3d_ap_finish_scenes(const int64_t* codes, int64_t n_slots, const int64_t* slot_offsets, int n_scenes, int n_classes, int n_overlaps,
                          const int64_t* counters, int mask50, int mask25, double* ap, double* pr_rc, double* summary, void* ws,
                          size_t ws_bytes, void* stream);
int sd3d_ap_reduce_counters(const int64_t* counters, int n_scenes, int n_classes, int n_overlaps, int64_t* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * 3D box AP / AR, streamed (csrc/boxeval.hip): the VOC-style indoor detection protocol for axis-aligned boxes, per class c and IoU
 * threshold t.  All three calls only enqueue work; `status` is the int64 word of sd3d_ap_scene (OR of SD3D_AP_* and SD3D_BOX_*).
 *
 *   Protocol.  Ground truth: one box per instance of a scene.  IoU in float64 from the fp32 values, every operation rounded on its
 *     own: prediction corners centre -+ size / 2, volumes ((dx * dy) * dz), inter = ((ox * oy) * oz) of the overlaps clamped at 0,
 *     iou = inter / ((va + vb) - inter), 0 where that denominator is 0.  Within a scene the predictions of class c are taken in
 *     (score descending, row ascending) order; each takes the ground truth of class c with the largest IoU (the lowest index on equal
 *     IoU); it is a true positive when that IoU is > t and the ground truth is not yet taken at t, a false positive otherwise (also
 *     without any ground truth of its class).  Curve of (c, t): all entries of all scenes in descending score, true before false on
 *     equal scores; recall = tp / npos, precision = tp / max(tp + fp, eps); AP = the area under the precision envelope (recall
 *     padded with 0 and 1, precision with 0 and 0, running maximum from the back, sum of (r[i+1] - r[i]) * p[i+1]); AR = the last
 *     recall.  npos[c] = 0: AP = AR = NaN; ground truth but no entry: 0.
 *   sd3d_gt_boxes: points float [N, ld] (x, y, z first, ld >= 3); gt_sem / gt_inst / id_map / num_stuff / class_lut / n_classes read by
 *     the id rule of sd3d_ap_scene (same columns, same SD3D_AP_BAD_INSTANCE / SD3D_AP_MIXED_SEMANTIC).  corners float
 *     [SD3D_AP_INSTANCE_COLS, 6] = min xyz, max xyz over the points of instance column i (exact, whatever the order of the points; -0
 *     reads as +0), cls int32 [SD3D_AP_INSTANCE_COLS] = its class index, -1 = no such instance (its corners are 0).  An instance with
 *     one point is a ground truth.  A non-finite coordinate in an instance sets SD3D_BOX_BAD_COORD and the instance is left out.
 *     ws: sd3d_gt_boxes_ws_bytes().
 *   sd3d_box_ap_scene: boxes float [n, 6] (centre, size), labels int64 [n] class INDEX, scores float [n], 0 <= n <= SD3D_AP_MAX_PREDS.
 *     A label outside [0, n_classes) sets SD3D_AP_BAD_LABEL, a non-finite score SD3D_AP_BAD_SCORE, a negative or non-finite size or a
 *     non-finite centre SD3D_BOX_BAD_BOX; such a prediction is left out.  gt_corners float [n_gt, 6], gt_cls int32 [n_gt] (-1 = no
 *     ground truth), 0 <= n_gt <= SD3D_AP_INSTANCE_COLS: the output of sd3d_gt_boxes or the caller's own; a class outside
 *     [-1, n_classes) sets SD3D_AP_BAD_LABEL, a non-finite corner or max < min SD3D_BOX_BAD_COORD, and the box is left out.
 *     thresholds: DEVICE double [n_overlaps], n_overlaps <= SD3D_AP_MAX_OVERLAPS.  Prediction r emits exactly one entry per threshold
 *     o, in the code layout of sd3d_ap_scene with group = class * n_overlaps + o, into slot slot_begin + o * n + r; a prediction that
 *     is left out writes the sentinel.  A slot at or past slot_begin + slot_cap is not written and sets SD3D_AP_STORE_FULL.
 *     npos int64 [n_classes] += the scene's ground-truth boxes per class; has_pred int64 [n_classes] |= 1.
 *     ws: sd3d_box_ap_scene_ws_bytes(n, n_gt, n_overlaps).
 *   sd3d_box_ap_finish: codes int64 [n_slots] (clobbered: sorted in place or into the workspace, the sort of sd3d_ap_finish).  ap, ar
 *     double [n_classes * n_overlaps].  The AP sum is taken per thread in ascending index and over the threads in a fixed tree.
 *     ws: sd3d_box_ap_finish_ws_bytes(n_slots).
 * ------------------------------------------------------------------------------------------- */
#define SD3D_BOX_BAD_COORD 32            /* a non-finite point coordinate in an instance, or a bad ground-truth corner */
#define SD3D_BOX_BAD_BOX 64              /* a predicted box with a negative or non-finite size or a non-finite centre */
size_t sd3d_gt_boxes_ws_bytes(void);
int sd3d_gt_boxes(const float* points, int64_t ld, int64_t N, const int64_t* gt_sem, int64_t sem_stride, const int64_t* gt_inst,
                  int64_t inst_stride, const int64_t* id_map, int map_len, int num_stuff, const int32_t* class_lut, int lut_len,
                  int n_classes, float* corners, int32_t* cls, int64_t* status, void* ws, size_t ws_bytes, void* stream);
size_t sd3d_box_ap_scene_ws_bytes(int n, int n_gt, int n_overlaps);
int sd3d_box_ap_scene(const float* boxes, int n, const int64_t* labels, const float* scores, const float* gt_corners, const int32_t* gt_cls,
                      int n_gt, int n_classes, const double* thresholds, int n_overlaps, int64_t* store, int64_t slot_begin,
                      int64_t slot_cap, int64_t* npos, int64_t* has_pred, int64_t* status, void* ws, size_t ws_bytes, void* stream);
size_t sd3d_box_ap_finish_ws_bytes(int64_t n_slots);
int sd3d_box_ap_finish(int64_t* codes, int64_t n_slots, int n_classes, int n_overlaps, const int64_t* npos, double* ap, double* ar,
                       void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Multi-view lifting of posed 2D feature maps onto scene points (csrc/lift2d.hip): the producer of `points_2dfeats`.  The reference
 * has no counterpart (it loads a per-scene dump); tests/lift2d_ref.py restates the rule below in float64.  All three calls only
 * enqueue work, use no atomics, and their results are pure functions of their inputs.
 *
 *   Inputs.  points float [N, ld] (world x, y, z first, ld >= 3); world_to_cam float [V, 12] = the rows of [R | t] of every view;
 *     intrinsics float [V, 4] = fx, fy, cx, cy in pixels of the depth image, pixel centres at integer coordinates; depth [V, Hd, Wd],
 *     uint16 times depth_scale (depth_u16 != 0) or float metres, 0 = invalid.
 *   Visibility of point n in view v.  p_c = R p + t, z = p_c.z, require z > near.  u = fx x / z + cx, v = fy y / z + cy,
 *     ui = floor(u + 0.5), vi likewise, require border <= ui < Wd - border and border <= vi < Hd - border.  d = depth[v, vi, ui],
 *     require d > 0 and |d - z| <= tol_abs + tol_rel d.  Every comparison is made on floats before a value becomes an integer or an
 *     address: NaN, infinite and huge coordinates fail one and the point is not visible.
 *   sd3d_lift_visibility: bits uint32 [N, ceil(V / 32)], bit (v % 32) of word v / 32 of point n = visible (unused high bits 0), every
 *     word written by one thread; count int32 [N] = the set bits of the point, added to `count` when add_count != 0.
 *   sd3d_lift_accumulate: maps [V, Hf, Wf, C] channels-last, __half (maps_f16 != 0) or float, 16-byte aligned, C a multiple of 64 up
 *     to 1024.  For every set bit of views [v0, v1) in ascending order: sample at xf = (u + 0.5) Wf / Wd - 0.5, yf likewise
 *     (align_corners = False), bilinear with the tap indices clamped to the map, and sum[n, c] = fma(w11, t11, fma(w10, t10,
 *     fma(w01, t01, fma(w00, t00, sum[n, c])))) in fp32.  sum float [N, C] is read and written by the one owner of point n, so any cut
 *     of the views into calls and ranges that keeps them ascending gives the same bits.  `bits` need not come from
 *     sd3d_lift_visibility: the tap coordinates are clamped as floats first, whatever the mask says.
 *   sd3d_lift_finish: mean = sum / count, 0 where count == 0.  scale_index 0 starts, later ones add to acc float [N, C] (may be NULL
 *     when n_scales == 1); the last one writes out [N, C] = (acc + mean) / n_scales as float or __half (out_f16 != 0).
 * ------------------------------------------------------------------------------------------- */
int sd3d_lift_visibility(const float* points, int64_t ld, int64_t N, const float* world_to_cam, const float* intrinsics, const void* depth,
                         int depth_u16, float depth_scale, int V, int Hd, int Wd, float near, int border, float tol_abs, float tol_rel,
                         uint32_t* bits, int32_t* count, int add_count, void* stream);
int sd3d_lift_accumulate(const float* points, int64_t ld, int64_t N, const float* world_to_cam, const float* intrinsics, int V, int Hd,
                         int Wd, const uint32_t* bits, const void* maps, int maps_f16, int Hf, int Wf, int C, int v0, int v1, float* sum,
                         void* stream);
int sd3d_lift_finish(const float* sum, const int32_t* count, int64_t N, int C, int scale_index, int n_scales, float* acc, void* out,
                     int out_f16, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Lifting of a 2D detector's queries to 3D centres (csrc/lift_queries.hip): the producer of `query2d_feats` [M, C] and `query2d_pos`
 * [M, 3].  The reference has no counterpart (it loads a per-scene dump, `scannet200.py:218-232`); tests/lift_queries_ref.py restates
 * the rule below in float64.  The calls only enqueue work; their results are pure functions of their inputs, with the same bits under
 * any schedule, cut of the views into calls, or stream: every decision is an integer one or a single rounded fp32 operation, and the
 * centres are sums of int64 fixed-point numbers.
 *
 *   Inputs.  depth [V, Hd, Wd], uint16 times depth_scale (depth_u16 != 0) or float metres; intrinsics float [V, 4] = fx, fy, cx, cy in
 *     pixels of the depth image, pixel centres at integer coordinates; cam_to_world float [V, 12] = the rows of [R | t]; masks uint8
 *     [V, Q, Hm, Wm], non-zero = set (a bool tensor's bytes), at any resolution; Hd Wd <= 2^28 so that the sums cannot overflow.
 *   1. Mask sample.  Depth pixel (vi, ui) reads mask pixel ym = ((2 vi + 1) Hm) / (2 Hd), xm = ((2 ui + 1) Wm) / (2 Wd), integer
 *      divisions: the mask pixel nearest to the depth pixel's centre, exactly.
 *   2. Depth key.  d = depth in fp32 metres (raw * depth_scale in fp32 for uint16); require d > 0; t = d * 1000 + 0.5 in fp32 (two
 *      rounded operations); require t < 65536; k = (int)floor(t), millimetres; require 1 <= k <= far_mm.  Every comparison is made on
 *      floats before anything becomes an integer: NaN, infinite, negative and huge depths are invalid.
 *   3. Median.  Over the n valid masked pixels of (v, q), k_med = the key of rank (n - 1) / 2 in ascending order (the lower median),
 *      exact.  n == 0 gives count = 0, centre = 0, median_mm = 0.
 *   4. Gate.  Keep a pixel iff 1000 |k - k_med| <= 1000 gate_mm + gate_permille k_med (integers): it removes the background a mask
 *      leaks onto at depth edges.
 *   5. Back-projection.  p_c = ((ui - cx) d / fx, (vi - cy) d / fy, d) in fp32, w = R p_c + t, each component as ((r0 x + r1 y) + r2 z)
 *      + t with every operation rounded on its own (no fused multiply-add: the kernel computes what a float32 evaluation of the
 *      restatement computes); require every component finite and |w| < 2^SD3D_LIFTQ_WORLD_BITS, otherwise the pixel is dropped and not
 *      counted.
 *   6. Centre.  Each kept component becomes rint(w * 2^SD3D_LIFTQ_FIXED_BITS) as int64; the three sums are int64; count = the kept
 *      pixels; centre = (float)((double)sum / (double)count / 2^SD3D_LIFTQ_FIXED_BITS), zero where count == 0.
 *   7. Selection.  Row i = v * Q + q of the stores is valid iff score[i] >= score_thr (a NaN fails) and count[i] >= min_pixels.  With
 *      max_queries < 0, or no more valid rows than max_queries, all valid rows are emitted in ascending order; otherwise the
 *      max_queries best by score descending, ties to the lower row, again in ascending row order.  Equal floats are ties; the order
 *      is the one of sd3d_keys_from_f32(descending), under which +0 sorts before -0.
 *   8. Output.  out_feats float [M, C] = the selected rows of feats (__half -> float is exact), out_pos float [M, 3] = of centre.
 *
 *   sd3d_lift_query_centres: centre float [V Q, 3], count int32 [V Q], median_mm int32 [V Q]; one workgroup owns one (v, q).
 *   sd3d_lift_query_select: scores float [n], count int32 [n] -> rows int32 [rows_cap >= min(max_queries, n)], the first *m_dev of
 *     them written, m_dev int32 on the device.  ws: sd3d_lift_query_select_ws_bytes(n), 256-byte aligned.
 *   sd3d_lift_query_gather: feats [n, C] __half (feats_f16 != 0) or float, 16-byte aligned, C a multiple of 8; rows int32 [M] < n.
 * ------------------------------------------------------------------------------------------- */
#define SD3D_LIFTQ_FIXED_BITS 20         /* fixed-point fraction bits of the centre sums */
#define SD3D_LIFTQ_WORLD_BITS 14         /* world coordinates at or beyond 2^14 m are dropped */
int sd3d_lift_query_centres(const void* depth, int depth_u16, float depth_scale, const float* intrinsics, const float* cam_to_world,
                            const void* masks, int V, int Q, int Hd, int Wd, int Hm, int Wm, int far_mm, int gate_mm, int gate_permille,
                            float* centre, int32_t* count, int32_t* median_mm, void* stream);
size_t sd3d_lift_query_select_ws_bytes(int64_t n);
int sd3d_lift_query_select(const float* scores, const int32_t* count, int64_t n, float score_thr, int min_pixels, int64_t max_queries,
                           int32_t* rows, int64_t rows_cap, int32_t* m_dev, void* ws, size_t ws_bytes, void* stream);
int sd3d_lift_query_gather(const void* feats, int feats_f16, const float* centre, const int32_t* rows, int64_t n, int64_t M, int C,
                           float* out_feats, float* out_pos, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Merging of lifted 2D queries across views into one query per object (csrc/merge_queries.hip): the stage between the lifter's
 * stores and the decoder's `query2d_feats` / `query2d_pos`.  The reference has no counterpart; tests/merge_queries_ref.py restates
 * the rule below, and every decision of it is an integer one, so the kernels EQUAL the restatement (the feature mean apart, which is
 * a fixed sequence of rounded fp32 operations).
 *
 *   Inputs.  feats [n, C] __half (feats_f16 != 0) or float, C <= 1024; centre float [n, 3]; scores float [n]; count int32 [n];
 *     view of a row = row / queries_per_view.
 *   1. Valid rows.  score >= score_thr (a NaN fails), count >= min_pixels, every centre component finite with
 *      |c| < 2^SD3D_LIFTQ_WORLD_BITS.  If more than SD3D_MERGE_MAX_ROWS rows are valid the best by score enter, ties to the lower row
 *      (the order of sd3d_lift_query_select).
 *   2. Order.  Entering rows are ranked by score descending, ties to the lower row (sd3d_keys_from_f32(descending)).
 *   3. Fixed-point centre.  p = rint(centre * 1024) per component as int32 (|p| <= 2^24).
 *   4. Quantised feature.  s = max_j |f_j| in fp32; if s is not finite or s < 2^-100 the code is all zero; otherwise with
 *      2^(e-1) <= s < 2^e, q_j = clamp(rint(f_j * 2^(7-e)), -127, 127) as int8; nrm = sum q_j^2 (int32).
 *   5. Adjacency of ranks a < b.  r_q = radius_q = round(radius * 1024) in 1 .. 2^20: dx^2 + dy^2 + dz^2 <= r_q^2 (int64); and, if
 *      sim_q = round(sim * 128) in 1 .. 128 is given (0 = distance only): d = sum q_a q_b > 0 and
 *      (int64) d d 16384 >= (int64) sim_q sim_q nrm_a nrm_b.  A zero code (nrm = 0) is adjacent to nothing, with or without sim_q.
 *   6. Leader clustering.  Walk the ranks upward: an unlabelled rank becomes a seed and labels every later unlabelled rank adjacent to
 *      it (the greedy order of NMS; not a transitive closure).
 *   7. Per cluster, members in ascending row order: w_i = min(count_i, 2^20); pos = (float)((double) sum w_i p_i / (double) sum w_i
 *      / 1024) (int64 sums); views = the distinct row / queries_per_view; score = the seed's; feat = per channel in fp32
 *      acc = acc + (float) w_i * f_i (two rounded operations per member) then acc / (float) sum w_i, or the seed's row (reduce_best).
 *   8. Emit.  Clusters with views < min_views are dropped; if more than max_queries (< 0: no cap) remain, the best by seed score, ties
 *      to the lower seed row; emitted in ascending seed row.  labels int32 [n] = the output index of each row's cluster, or -1.
 *
 *   The four calls share one workspace (sd3d_merge_queries_ws_bytes(n, C), 256-byte aligned) and run in this order on one stream:
 *   sd3d_merge_queries_adjacency (steps 1-5: the bit matrix [M, ceil(M / 64)] in the workspace), sd3d_merge_queries_sweep (step 6),
 *   sd3d_merge_queries_reduce (steps 7-8 but the features: *k_dev int32 = the number of emitted clusters, on the device),
 *   sd3d_merge_queries_emit (K = the value read from k_dev: out_feats float [K, C], out_pos float [K, 3], out_scores float [K],
 *   out_views int32 [K], labels int32 [n]).  sd3d_merge_queries_adjacency_read copies what the first call left: rank_row int32
 *   [Mp] (the row of each rank, -1 beyond M; Mp = min(n, SD3D_MERGE_MAX_ROWS) rounded up to 64) and the bit matrix uint64
 *   [Mp, Mp / 64] with zeros below the diagonal, for tests and tools.
 * ------------------------------------------------------------------------------------------- */
#define SD3D_MERGE_MAX_ROWS 16384        /* rows that enter the clustering */
size_t sd3d_merge_queries_ws_bytes(int64_t n, int C);
int sd3d_merge_queries_adjacency(const void* feats, int feats_f16, const float* centre, const float* scores, const int32_t* count, int64_t n,
                                 int C, float score_thr, int min_pixels, int radius_q, int sim_q, void* ws, size_t ws_bytes, void* stream);
int sd3d_merge_queries_adjacency_read(int64_t n, int C, const void* ws, size_t ws_bytes, int32_t* rank_row, void* adj, void* stream);
int sd3d_merge_queries_sweep(int64_t n, int C, void* ws, size_t ws_bytes, void* stream);
int sd3d_merge_queries_reduce(const float* scores, const int32_t* count, int64_t n, int C, int queries_per_view, float score_thr,
                              int min_views, int64_t max_queries, int32_t* k_dev, void* ws, size_t ws_bytes, void* stream);
int sd3d_merge_queries_emit(const void* feats, int feats_f16, const float* scores, const int32_t* count, int64_t n, int C, int64_t K,
                            int reduce_best, float* out_feats, float* out_pos, float* out_scores, int32_t* out_views, int32_t* labels,
                            const void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Superpoints from a triangle mesh (csrc/superpoints.hip): the graph segmentation ScanNet's segmentator applies to a scan, the input
 * `super_points` of the model.  The reference loads it from a dump; tests/superpoints_ref.py restates the rule below and the kernels
 * EQUAL the restatement label for label.  Every step is one correctly rounded fp32 operation (never contracted) or an exact integer one.
 *
 *   Inputs.  vertices float [N, 3]; faces int32 or int64 (faces_i64 != 0) [F, 3], indices local to the face's scene; 3 F < 2^31;
 *     k_thresh finite >= 0; min_verts >= 1.  A batch is concatenated: vertex_offsets / face_offsets int64 [n_scenes + 1] on the device
 *     ascend from 0 to N / F.  A face with an index outside its scene's [0, N_s) is ignored and counted in bad_faces; a face with a
 *     repeated index is kept (its self-edges join nothing, its normal is zero).
 *   1. Face normal.  a = p1 - p0, b = p2 - p0, n = (a.y b.z - a.z b.y, a.z b.x - a.x b.z, a.x b.y - a.y b.x), every product and
 *      difference rounded; l = sqrt((n.x n.x + n.y n.y) + n.z n.z); valid iff l is finite and > 0, then n /= l per component.
 *   2. Vertex normal.  Each valid face adds rint(n 2^24) to its three vertices (int64 sums); m = (float)(double)sum, normalised as
 *      above; a zero or invalid m is (0, 0, 0).
 *   3. Edges.  Face f = (i, j, k) gives edges 3 f = (i, j), 3 f + 1 = (i, k), 3 f + 2 = (k, j).  For edge (a, b):
 *      dot = (m_a.x m_b.x + m_a.y m_b.y) + m_a.z m_b.z; w = 1 - dot if that is > 0, else 0;
 *      s = (m_b.x (p_b.x - p_a.x) + m_b.y (p_b.y - p_a.y)) + m_b.z (p_b.z - p_a.z); if s > 0 (a NaN is not) w = w w.
 *   4. Order.  Ascending (bits of w as uint32, edge index).
 *   5. Pass 1.  Every vertex is a component with size 1 and thr = k_thresh.  In order: components A != B of the ends join iff
 *      w <= thr[A] and w <= thr[B]; then size = size_A + size_B and thr = w + k_thresh / (float)size (a divide, then an add).
 *   6. Pass 2.  In the same order: A != B join iff size[A] < min_verts or size[B] < min_verts.
 *   7. Output.  labels int64 [N], dense 0 .. S_s - 1 per scene, components numbered by their smallest vertex; info int32
 *      [n_scenes, 2] = {S_s, bad_faces_s}.  A vertex in no face is a component of its own.
 *
 *   Optional outputs (NULL: not written), for tests and tools: normals_out float [N, 3] (step 2), weights_out uint32 [3 F] (the bits
 *   of step 3, 0 for an ignored face), sweep_stats_out int64 [n_scenes, 2] = the edges of pass 1 / pass 2 whose ends lay in different
 *   components (in pass 2: one of them below min_verts) when their batch began: those the sweep settles in LDS.  ws: sd3d_superpoints_ws_bytes, 256-byte aligned.
 * ------------------------------------------------------------------------------------------- */
size_t sd3d_superpoints_ws_bytes(int64_t n_vertices, int64_t n_faces, int n_scenes);
int sd3d_mesh_superpoints(const float* vertices, const void* faces, int faces_i64, const int64_t* vertex_offsets,
                          const int64_t* face_offsets, int64_t n_vertices, int64_t n_faces, int n_scenes, float k_thresh, int min_verts,
                          int64_t* labels, int32_t* info, float* normals_out, void* weights_out, int64_t* sweep_stats_out, void* ws,
                          size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Superpoints from a point cloud (csrc/superpoints.hip): the segmentator's second entry, segment_point(vertices, normals, edges),
 * for scans without faces, with the two steps in front of it: an exact k-nearest-neighbour graph and normals from the neighbourhood.
 * tests/point_superpoints_ref.py restates the three rules below and the kernels EQUAL it bit for bit.  A batch is concatenated;
 * vertex_offsets / edge_offsets int64 [n_scenes + 1] on the device ascend from 0; indices (nbr, ea, eb) are local to their scene.
 *
 * sd3d_graph_superpoints.  points, normals float [N, 3]; ea, eb int32 [E]; E < 2^31.  An edge with an end outside its scene's [0, N_s)
 *   is ignored, counted in info[s][1] (bad_edges) and never looked at.  Otherwise step 3 of the mesh rule on the given normals:
 *   dot = (m_a.x m_b.x + m_a.y m_b.y) + m_a.z m_b.z; w = 1 - dot if that is > 0, else 0; s = (m_b.x (p_b.x - p_a.x) + m_b.y
 *   (p_b.y - p_a.y)) + m_b.z (p_b.z - p_a.z); if s > 0, w = w w.  oriented == 0 (normals without a sign): dot = |dot| before the
 *   subtraction and no squaring.  Steps 4 to 7 are the mesh's, the edge index being the position in the list: both copies of a mutual
 *   edge are kept.  weights_out uint32 [E], sweep_stats_out int64 [n_scenes, 2]: optional, as for the mesh.
 *
 * sd3d_knn_graph.  1 <= k <= 64, 0 < radius <= 4, N k < 2^31.  A point is valid iff its coordinates are finite with |c| < 2^14.
 *   r2 = (float)(radius radius).  For valid i != j of one scene: dx = p_j.x - p_i.x (dy, dz alike), d2 = (dx dx + dy dy) + dz dz, one
 *   fp32 rounding per operation; j is a candidate iff d2 <= r2.  Row i of nbr int32 [N, k] holds the k smallest candidates by
 *   (bits of d2 as uint32, j), ascending; missing slots hold -1; the row of an invalid point is all -1 and it is nobody's neighbour.
 *   d2_out float [N, k] (optional): the distances, +inf in a missing slot.  A hashed uniform grid of fixed-point cells chooses the
 *   pairs that are evaluated and cannot change the answer (the argument: csrc/superpoints.hip).
 *
 * sd3d_point_normals.  nbr int32 [N, k] (k <= 64).  A slot counts iff 0 <= j < N_s and d = p_j - p_i (fp32) has |d| <= 8 in every
 *   component; c = the slots that count.  c < 3: the normal is (0, 0, 0).  Otherwise q = rint(d 2^20) as int64, n = c + 1 (the point
 *   itself, q = 0), exact sums Sq [3] and Sqq [6], C = n Sqq - Sq Sq^T (exact), its six entries converted to fp64; cyclic Jacobi in
 *   fp64, every operation one IEEE rounding: exactly 8 sweeps over (0,1), (0,2), (1,2); a rotation is skipped when a_pq == 0;
 *   theta = (a_qq - a_pp) / (2 a_pq), t = 1 / (|theta| + sqrt(theta theta + 1)), negated when theta < 0, c = 1 / sqrt(t t + 1),
 *   s = t c; a_pp -= t a_pq, a_qq += t a_pq, a_pq = 0, (a_rp, a_rq) = (c a_rp - s a_rq, s a_rp + c a_rq), and the columns p, q of
 *   V (from the identity) alike: (v_ip, v_iq) = (c v_ip - s v_iq, s v_ip + c v_iq); tests/point_superpoints_ref.py has them one
 *   operation per line and is their definition.  The normal is the column of V at the smallest diagonal entry (ties: the lowest
 *   index), cast to fp32 and normalised as a face normal is (a failure gives (0, 0, 0)).  viewpoint float [n_scenes, 3], or [N, 3]
 *   with viewpoint_per_point != 0: the normal is negated iff (n.x (v.x - p.x) + n.y (v.y - p.y)) + n.z (v.z - p.z) < 0 in fp32;
 *   viewpoint NULL: negated so that its first non-zero component is positive (segment such normals with oriented = 0).
 * ------------------------------------------------------------------------------------------- */
size_t sd3d_graph_superpoints_ws_bytes(int64_t n_points, int64_t n_edges, int n_scenes);
int sd3d_graph_superpoints(const float* points, const float* normals, const int32_t* ea, const int32_t* eb,
                           const int64_t* vertex_offsets, const int64_t* edge_offsets, int64_t n_points, int64_t n_edges, int n_scenes,
                           int oriented, float k_thresh, int min_verts, int64_t* labels, int32_t* info, void* weights_out,
                           int64_t* sweep_stats_out, void* ws, size_t ws_bytes, void* stream);
size_t sd3d_knn_graph_ws_bytes(int64_t n_points, int n_scenes);
int sd3d_knn_graph(const float* points, const int64_t* vertex_offsets, int64_t n_points, int n_scenes, int k, float radius, int32_t* nbr,
                   float* d2_out, void* ws, size_t ws_bytes, void* stream);
int sd3d_point_normals(const float* points, const int32_t* nbr, const int64_t* vertex_offsets, int64_t n_points, int n_scenes, int k,
                       const float* viewpoint, int viewpoint_per_point, float* normals, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Fusion of posed RGB-D frames into the scene's point cloud (csrc/fuse_views.hip): the producer of `points [N, 6]` (xyz, rgb on the
 * 0-255 scale), the input of the superpoint, lifting and query stages.  The reference has no counterpart (it reads a `points/` file per scene,
 * made offline from a mesh); tests/fuse_views_ref.py restates the rule below in numpy and the kernels EQUAL it, bit for bit.  The
 * calls only enqueue work.  Every decision is an integer one or a single rounded fp32 operation and the per-cell state is a set of
 * integer sums, so the result is a pure function of the SET of (view, pixel) observations: the same bits however the views are cut
 * into sd3d_fuse_accumulate calls, in whatever order they arrive, and on whatever stream.
 *
 *   Inputs.  depth [V, Hd, Wd], uint16 times depth_scale (depth_u16 != 0) or float metres; intrinsics float [V, 4] = fx, fy, cx, cy in
 *     pixels of the depth image, pixel centres at integer coordinates; cam_to_world float [V, 12] = the rows of [R | t]; colors uint8
 *     [V, Hc, Wc, 3] at any resolution.
 *   1. Pixels.  Depth pixel (vi, ui) of view v takes part iff vi % stride == 0 and ui % stride == 0.  It reads the colour pixel
 *      (((2 vi + 1) Hc) / (2 Hd), ((2 ui + 1) Wc) / (2 Wd)), integer divisions: the sampling rule of sd3d_lift_query_centres.
 *   2. Depth.  d = (float)raw * depth_scale, one rounded fp32 multiply (float depth is used as it is).  The pixel is valid iff d > 0,
 *      d >= near and d <= far, compared in fp32; a NaN fails.
 *   3. Edges (flying pixels at depth discontinuities; skipped when use_edges == 0).  For each of the 4 neighbours (vi +- 1, ui),
 *      (vi, ui +- 1) that lies inside the image, whatever the stride: dn = the neighbour's depth by step 2; it is a jump iff !(dn > 0)
 *      or |dn - d| > edge_abs + edge_rel * d, the right-hand side one rounded multiply then one rounded add, the difference one
 *      rounded subtract.  A pixel with any jump is dropped.
 *   4. Back-projection.  Step 5 of sd3d_lift_query_centres, the same device function (csrc/backproject.h): x = (ui - cx) * d / fx, y
 *      likewise, w_i = ((R_i0 x + R_i1 y) + R_i2 d) + R_i3, every operation rounded on its own, left to right, no fused multiply-add.
 *      Unless all three w_i are finite with |w_i| < 2^SD3D_FUSE_WORLD_BITS the pixel is dropped and counted in out_of_range.
 *   5. Cell.  c_i = floorf(w_i * inv_voxel), one rounded fp32 multiply; inv_voxel = (float)(1.0 / voxel), divided on the host in
 *      double.  Unless -2^SD3D_FUSE_CELL_BITS <= c_i < 2^SD3D_FUSE_CELL_BITS on all axes, compared as floats before anything becomes
 *      an integer, the pixel is dropped and counted in out_of_range.  key = ((c_x + 2^20) << 42) | ((c_y + 2^20) << 21) | (c_z + 2^20).
 *      floor, not truncation: negative coordinates are ordinary.
 *   6. Per cell, integers only.  n += 1; S_i += (int64)rint((double)w_i * 2^SD3D_FUSE_FIXED_BITS); C_j += colour byte j (r, g, b).  All
 *      seven sums are 64-bit: 2^28 observations of one cell cannot overflow them.
 *   7. Output.  The cells with n >= min_obs in ascending key order: xyz_i = (float)((double)S_i / (double)n / 2^SD3D_FUSE_FIXED_BITS),
 *      rgb_j = (float)((double)C_j / (double)n), obs = n.
 *
 *   The state is an open-addressing table of `capacity` slots (a power of two, SD3D_FUSE_MIN_CAPACITY .. SD3D_FUSE_MAX_CAPACITY) of
 *   SD3D_FUSE_SLOT_WORDS 64-bit words = 64 bytes {key, S_x, S_y, S_z, n, C_r, C_g, C_b}, in a caller-owned workspace of
 *   sd3d_fuse_ws_bytes(capacity) bytes (0 for a bad capacity), 256-byte aligned, that also holds five 64-bit counters and the scratch
 *   of the emit.  A cell whose probe sequence finds no slot within SD3D_FUSE_PROBE_LIMIT slots is dropped and its pixels are counted
 *   in `overflow`: nothing is written outside the table, and the caller treats overflow > 0 as an error.  The table does not grow.
 *
 *   sd3d_fuse_reset: empties the table and zeroes the counters.  Required once before the first accumulate.
 *   sd3d_fuse_accumulate: steps 1 to 6 for V views, one launch.
 *   sd3d_fuse_emit: step 7.  points float [out_cap, 6], obs int32 [out_cap], keys_out int64 [out_cap] or NULL: the first
 *     min(N, out_cap) rows are written.  info int64 [SD3D_FUSE_INFO_WORDS] on the device = N, cells (occupied slots), pixels_used
 *     (observations added to a cell), out_of_range, overflow.  The table is left as it is: accumulate may go on.
 * ------------------------------------------------------------------------------------------- */
#define SD3D_FUSE_FIXED_BITS 20          /* fixed-point fraction bits of the position sums */
#define SD3D_FUSE_WORLD_BITS 14          /* world coordinates at or beyond 2^14 m are dropped */
#define SD3D_FUSE_CELL_BITS 20           /* cell indices lie in [-2^20, 2^20): 21 bits per axis of the key */
#define SD3D_FUSE_SLOT_WORDS 8           /* 64-bit words per slot of the table */
#define SD3D_FUSE_PROBE_LIMIT 64         /* slots a cell tries before it counts as overflow */
#define SD3D_FUSE_INFO_WORDS 5           /* N, cells, pixels_used, out_of_range, overflow */
#define SD3D_FUSE_MIN_CAPACITY 16
#define SD3D_FUSE_MAX_CAPACITY (1 << 24)
size_t sd3d_fuse_ws_bytes(int64_t capacity);
int sd3d_fuse_reset(void* ws, size_t ws_bytes, int64_t capacity, void* stream);
int sd3d_fuse_accumulate(const void* depth, int depth_u16, float depth_scale, const float* intrinsics, const float* cam_to_world,
                         const void* colors, int V, int Hd, int Wd, int Hc, int Wc, int stride, float near, float far, float edge_abs,
                         float edge_rel, int use_edges, float inv_voxel, void* ws, size_t ws_bytes, int64_t capacity, void* stream);
int sd3d_fuse_emit(void* ws, size_t ws_bytes, int64_t capacity, int min_obs, float* points, int32_t* obs, int64_t* keys_out,
                   int64_t out_cap, int64_t* info, void* stream);

/* ---------------------------------------------------------------------------------------------
 * TSDF fusion of posed RGB-D frames and a surface-net mesh (csrc/tsdf.hip): the producer of a mesh - vertices [V, 6] in the layout of
 * `points`, faces [F, 3] - for sd3d_mesh_superpoints, the superpoint rule the network saw in training.  The reference has no
 * counterpart (it reads meshes made offline); tests/tsdf_ref.py restates the rule below in numpy and the kernels EQUAL it, bit for
 * bit.  The per-voxel state is integer sums and a view contributes to a voxel only through a block it touched, so the volume and the
 * mesh are a function of the SET of views: the bits do not depend on how the views are cut into calls, on their order, or on the
 * stream.  Every decision is an integer one or a single rounded fp32 operation (no fused multiply-add).
 *
 *   1. Valid pixel.  Steps 1 to 3 of the fusion above with stride 1: d = (float)raw * depth_scale; valid iff d > 0, near <= d <= far
 *      and no 4-neighbour inside the image is a jump (!(dn > 0) or |dn - d| > edge_abs + edge_rel * d); colour pixel
 *      ((2 vi + 1) Hc) / (2 Hd), ((2 ui + 1) Wc) / (2 Wd).
 *   2. Touched blocks.  For a valid pixel and j = -2 .. 2: d_j = d + (float)j * half_step (one rounded add), w = the back-projection
 *      of (vi, ui, d_j) by csrc/backproject.h; unless |w_i| < 2^SD3D_FUSE_WORLD_BITS and c_i = floorf(w_i * inv_voxel) lies in
 *      [-2^20, 2^20) on all axes (as floats) the sample is counted in out_of_range; else the view TOUCHES block b_i = c_i >> 3
 *      (arithmetic), key = ((b_x + 2^17) << 36) | ((b_y + 2^17) << 18) | (b_z + 2^17).  A block that finds no slot within
 *      SD3D_TSDF_PROBE_LIMIT slots counts into overflow (once per image tile that holds it).
 *   3. Integration, per (view, touched block) and per voxel c of the block: p_i = ((float)c_i + 0.5f) * voxel; camera point
 *      ((r0 p_x + r1 p_y) + r2 p_z) + t per row of world_to_cam; z > 0; uf = floorf(((fx * x) / z + cx) + 0.5f), vf likewise;
 *      0 <= uf < Wd and 0 <= vf < Hd as floats; the pixel is valid by step 1 with depth d; sdf = d - z; skipped if sdf < -trunc;
 *      q = (int)rintf(fminf(sdf, trunc) * qscale); W += 1, T += q, C_j += colour byte j - 32-bit integers, |q| <= 4097, so up to
 *      SD3D_TSDF_MAX_VIEWS views of one volume keep |T| < 2^30.
 *   4. A voxel is observed iff W >= min_weight, inside iff T < 0.
 *   5. Vertices.  Cell c (corner voxels c + {0,1}^3) is active iff its eight corners are observed and not all of one sign.  Its 12
 *      edges in the order x-edges (y, z) = (0,0) (0,1) (1,0) (1,1), y-edges (x, z) likewise, z-edges (x, y) likewise, each from its
 *      lower end a to its upper end b; an edge whose ends differ in sign crosses at s = f_a / (f_a - f_b), f = (float)((double)T /
 *      (double)W).  m = the fp32 sums of the crossings' cell coordinates in that order, divided once by their number; vertex_i =
 *      ((float)c_i + (0.5f + m_i)) * voxel; rgb_j = (float)((double)sum C_j / (double)sum W) over the eight corners.  Vertices in
 *      ascending cell key ((c_x + 2^20) << 42) | ((c_y + 2^20) << 21) | (c_z + 2^20).
 *   6. Faces.  A grid edge a -> a + e_k with both ends observed and of different sign emits a quad iff the four cells around it are
 *      active: with (u, w) = (k + 1, k + 2) mod 3, q0 = a - e_u - e_w, q1 = a - e_w, q2 = a, q3 = a - e_u; triangles (q0 q1 q2),
 *      (q0 q2 q3) if a is inside, (q0 q2 q1), (q0 q3 q2) otherwise: the right-hand normal points from the inside end to the outside
 *      end.  Faces in ascending (key of a, k), as indices into the vertex order.
 *
 *   The state is a caller-owned workspace of sd3d_tsdf_ws_bytes(capacity) bytes (0 for a bad capacity), 256-byte aligned, each part
 *   rounded up to 256 bytes: 7 64-bit counters | block keys uint64 [capacity] (SD3D_EMPTY_KEY = free) | touched uint64 [capacity] |
 *   slot list uint32 [capacity] | voxels int32 [capacity][SD3D_TSDF_VOXEL_WORDS][512] = W, T, C_r, C_g, C_b with voxel (lx, ly, lz) at
 *   lx * 64 + ly * 8 + lz | cell table int32 [capacity][512].  `capacity` counts BLOCKS, a power of two.
 *
 *   sd3d_tsdf_reset: empties the table.  Required once before the first touch.
 *   sd3d_tsdf_touch: steps 1 and 2 for V <= SD3D_TSDF_MAX_CALL_VIEWS views; writes vdepth float [V, Hd, Wd], the depth of each valid
 *     pixel and 0 elsewhere.  half_step = trunc / 2.
 *   sd3d_tsdf_integrate: step 3 for the same V views, which must follow their touch; reads its vdepth.  qscale = 4096 / trunc.
 *   sd3d_tsdf_mesh: steps 4 to 6.  vertices float [max_vertices, 6], keys_out int64 [max_vertices] or NULL, faces int32
 *     [6 * max_vertices, 3] (a cell's low corner starts three grid edges: no more than three quads a vertex); scratch of
 *     sd3d_tsdf_mesh_ws_bytes(max_vertices) bytes.  info int64 [SD3D_TSDF_INFO_WORDS] on the device = vertices (found; only the first
 *     max_vertices are written, and then the faces are incomplete: the caller treats vertices > max_vertices as an error), faces,
 *     blocks, voxels_observed, updates, out_of_range, overflow.  The volume is left as it is: touch / integrate may go on.
 * ------------------------------------------------------------------------------------------- */
#define SD3D_TSDF_VOXEL_WORDS 5          /* 32-bit words per voxel: W, T, C_r, C_g, C_b */
#define SD3D_TSDF_PROBE_LIMIT 64         /* slots a block tries before it counts as overflow */
#define SD3D_TSDF_INFO_WORDS 7           /* vertices, faces, blocks, voxels_observed, updates, out_of_range, overflow */
#define SD3D_TSDF_MAX_CALL_VIEWS 64      /* views of one touch / integrate pair: a bit each in a block's `touched` word */
#define SD3D_TSDF_MAX_VIEWS (1 << 17)    /* views of one volume: 2^17 * 4097 < 2^30 */
#define SD3D_TSDF_MIN_CAPACITY 16
#define SD3D_TSDF_MAX_CAPACITY (1 << 20)
#define SD3D_TSDF_MAX_VERTICES (1 << 26)
size_t sd3d_tsdf_ws_bytes(int64_t capacity);
int sd3d_tsdf_reset(void* ws, size_t ws_bytes, int64_t capacity, void* stream);
int sd3d_tsdf_touch(const void* depth, int depth_u16, float depth_scale, const float* intrinsics, const float* cam_to_world, int V, int Hd,
                    int Wd, float near, float far, float edge_abs, float edge_rel, int use_edges, float inv_voxel, float half_step,
                    float* vdepth, void* ws, size_t ws_bytes, int64_t capacity, void* stream);
int sd3d_tsdf_integrate(const float* vdepth, const float* intrinsics, const float* world_to_cam, const void* colors, int V, int Hd, int Wd,
                        int Hc, int Wc, float voxel, float trunc, float qscale, void* ws, size_t ws_bytes, int64_t capacity, void* stream);
size_t sd3d_tsdf_mesh_ws_bytes(int64_t max_vertices);
int sd3d_tsdf_mesh(void* ws, size_t ws_bytes, int64_t capacity, int min_weight, float voxel, int64_t max_vertices, void* scratch,
                   size_t scratch_bytes, float* vertices, int64_t* keys_out, int32_t* faces, int64_t* info, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Nearest point (csrc/transfer.hip): carrying what a forward computed per point onto other points and onto the depth frames.  The
 * results of a forward are indexed by the points it ran on; a labelling tool, a robot or an evaluation needs them on the pixels of
 * the frames, on a mesh's vertices or on another cloud.  The reference has no counterpart (it evaluates on the points it loaded);
 * tests/transfer_ref.py restates the rule below in numpy and the kernels EQUAL it, bit for bit.  The calls only enqueue work.  The
 * answer is a minimum over a set, so it is a pure function of the source cloud and the query: the same bits however the views are
 * cut into calls and on whatever stream.  No float atomics.
 *
 *   Source cloud P float [N, 3], N < 2^31; radius 0 < r <= 4 (the limits of sd3d_knn_graph); r2 = (float)(r r).
 *   1. Valid points.  A source point or a query is valid iff all three coordinates satisfy |c| < 2^14, compared as floats: a NaN or
 *      an infinity fails.  An invalid query answers -1; an invalid source point is never a candidate.
 *   2. Distance.  For query q and valid source j: dx = P[j].x - q.x (dy, dz alike), d2 = (dx dx + dy dy) + dz dz, every operation
 *      rounded on its own in fp32, no fused multiply-add; j is a candidate iff d2 <= r2.
 *   3. Answer.  The candidate with the smallest key (bits of d2 << 32) | j: the nearest, ties to the lower index.  idx int32 (-1 when
 *      there is no candidate) and d2 float (+inf when there is none).
 *   4. Pixel queries.  Pixel (vi, ui) of view v: d by step 2 of the fusion rule ((float)raw * depth_scale; valid iff d > 0, d >= near,
 *      d <= far); no edge test and no stride; w = the back-projection of csrc/backproject.h, every operation rounded on its own; w is
 *      then a query as in steps 1 to 3.  A pixel whose depth is invalid answers -1.
 *   5. Labels.  labels int32 [L, N], 0 <= L <= SD3D_NEAREST_MAX_LABELS: labels_out[l, query] = labels[l, idx], or `fill` where idx < 0,
 *      written by the kernel that found idx.
 *   6. Instance map.  masks uint8 [I, N] (non-zero = set), scores float [I]: map[n] = the i with masks[i, n] set and
 *      scores[i] >= score_thr that has the largest score, compared in fp32; ties go to the lower i; a NaN score never wins;
 *      map[n] = -1 if there is none.
 *
 *   sd3d_point_index_build: the hashed grid of sd3d_knn_graph over P (one definition: csrc/point_grid.h) into a caller-owned workspace
 *     of sd3d_point_index_ws_bytes(N) bytes (0 for a bad N), 256-byte aligned.  Built once per cloud and radius; the queries only read
 *     it and must be given the same n_points and radius.  The grid chooses the pairs that are evaluated and cannot change the answer
 *     (the argument: csrc/transfer.hip).
 *   sd3d_nearest_points: queries float [M, 3], M < 2^31.  idx_out int32 [M], d2_out float [M], labels_out int32 [L, M]: each optional
 *     (labels_out is required when n_labels > 0).
 *   sd3d_nearest_pixels: depth [V, Hd, Wd], uint16 times depth_scale (depth_u16 != 0) or float metres; intrinsics float [V, 4];
 *     cam_to_world float [V, 12]; images up to 16384 a side; one launch over the V views, at most 2^31 - 1 tiles of 8 x 32 pixels.
 *     idx_out int32 [V, Hd, Wd], d2_out float [V, Hd, Wd], labels_out int32 [L, V, Hd, Wd], indexed in 64 bits.
 *   sd3d_instance_map: map int32 [N].
 * ------------------------------------------------------------------------------------------- */
#define SD3D_NEAREST_MAX_LABELS 8
size_t sd3d_point_index_ws_bytes(int64_t n_points);
int sd3d_point_index_build(const float* points, int64_t n_points, float radius, void* ws, size_t ws_bytes, void* stream);
int sd3d_nearest_points(const float* queries, int64_t n_queries, const void* index_ws, size_t ws_bytes, int64_t n_points, float radius,
                        const int32_t* labels, int n_labels, int fill, int32_t* idx_out, float* d2_out, int32_t* labels_out, void* stream);
int sd3d_nearest_pixels(const void* depth, int depth_u16, float depth_scale, const float* intrinsics, const float* cam_to_world, int V,
                        int Hd, int Wd, float near, float far, const void* index_ws, size_t ws_bytes, int64_t n_points, float radius,
                        const int32_t* labels, int n_labels, int fill, int32_t* idx_out, float* d2_out, int32_t* labels_out, void* stream);
int sd3d_instance_map(const void* masks, const float* scores, int n_instances, int64_t n_points, float score_thr, int32_t* map,
                      void* stream);

/* ---------------------------------------------------------------------------------------------
 * Camera tracking against the TSDF volume (csrc/track.hip): frame-to-model alignment of a depth frame on the signed distance field
 * of sd3d_tsdf_*, which turns an ordered stream of UNPOSED frames into the poses the fusion above starts from.  The reference has no
 * counterpart (its poses were made offline); tests/track_ref.py restates the rule below in numpy and the kernels EQUAL it, bit for
 * bit.  segdino3d_amd/track.py has the rule in full.  The calls only enqueue work.
 *
 *   State: cam_to_world [R | t] as double [12]; steps 1 to 4 read its fp32 rounding.  One ITERATION at stride s:
 *   1. Samples: depth pixels (vi, ui) with vi % s == 0 and ui % s == 0, valid by step 1 of the TSDF rule (edge test at full resolution).
 *   2. p by csrc/backproject.h, y_i = (R_i0 p_x + R_i1 p_y) + R_i2 p_z, w_i = y_i + t_i; dropped unless all |w_i| < 2^14 and all
 *      |y_i| <= ymax (ymax = far sqrt(3): what bounds the sums).
 *   3. g_i = w_i * inv_voxel - 0.5f, c_i = floorf(g_i), f_i = g_i - c_i; the eight voxels c + {0,1}^3 must lie in [-2^20, 2^20) (as
 *      floats) and have W >= min_weight; value (float)((double)T / (double)W) * (1 / 4096); phi = the trilinear interpolant, lerped
 *      along x, then y, then z as a + (b - a) * f; n = its analytic gradient: the same lerps over the four corner differences per axis.
 *   4. q = y * inv_voxel; J = (q x n, n), the cross product term by term; Jq_k = (int)rintf(J_k * 1024), rq = (int)rintf(phi * 16384);
 *      int64 sums A += Jq Jq^T (21, the upper triangle row-major), b += Jq rq (6), count += 1, e += rq rq.
 *   5. One lane, double, + - * / only: A_kk *= 1 + (double)damping, an A_kk of exactly 0 becomes 1 (x_k = 0); L D L^T without
 *      pivoting; x = -(A^-1 b) / 16.  The iteration is LOST iff count < min_samples, a pivot is not > 0, x is not finite,
 *      |x_rot|^2 > max_rot^2 or |x_trans voxel|^2 > max_trans^2.
 *   6. a = x_rot / 2, dR = ((1 - a.a) I + 2 a a^T + 2 [a]x) / (1 + a.a); R <- dR R (three-term sums, left to right); t <- t + x_trans
 *      voxel.  After a lost iteration the later iterations of the frame do nothing.
 *
 *   The state is caller-owned, sd3d_track_state_bytes() bytes, 8-byte aligned: pose double [12] | the pose before the frame double
 *   [12] | lost, count, e | the SD3D_TRACK_SUMS sums in flight at word 32 | those of the last iteration that ran at word 64 (A, b,
 *   count, e).  The caller writes the first pose into words 0 .. 11.
 *   sd3d_track_begin: remembers the pose, clears lost and the sums.
 *   sd3d_track_iterate: one iteration of ONE frame (depth [Hd, Wd], intrinsics float [4]) against the volume in `ws` (read only).
 *     Refuses (4096 ymax inv_voxel + 2)^2 * samples >= 2^63.
 *   sd3d_track_end: a lost frame puts the pose back.  pose double [12] (NaN when lost), cam_to_world and world_to_cam float [12] as
 *     sd3d_tsdf_touch / sd3d_tsdf_integrate take them (world_to_cam = [R^T | -(R^T t)], in double, each entry rounded once), info
 *     int64 [SD3D_TRACK_INFO_WORDS] = lost, count and e of the last iteration that ran.
 * ------------------------------------------------------------------------------------------- */
#define SD3D_TRACK_SUMS 29
#define SD3D_TRACK_INFO_WORDS 3
size_t sd3d_track_state_bytes(void);
int sd3d_track_begin(void* state, size_t state_bytes, void* stream);
int sd3d_track_iterate(const void* depth, int depth_u16, float depth_scale, const float* intrinsics, int Hd, int Wd, int stride, float near,
                       float far, float edge_abs, float edge_rel, int use_edges, float inv_voxel, float voxel, float ymax, int min_weight,
                       int min_samples, float damping, float max_rot, float max_trans, void* state, size_t state_bytes, void* ws,
                       size_t ws_bytes, int64_t capacity, void* stream);
int sd3d_track_end(void* state, size_t state_bytes, double* pose, float* cam_to_world, float* world_to_cam, int64_t* info, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Mesh rasteriser (csrc/raster.hip, csrc/raster_rule.h): a triangle mesh drawn into posed views - per pixel the depth of the nearest
 * face, that face, the face's corner nearest the pixel, and label channels read through either.  The depth image is what the RGB-D
 * stages above take as float metres, for frames that have no depth of their own.  The reference has no counterpart;
 * tests/raster_ref.py restates the rule below in numpy and the kernels EQUAL it, bit for bit.  segdino3d_amd/raster.py has the rule
 * in full.  The call only enqueues work.  The images are a minimum over a set of keys, so they are a pure function of mesh, cameras
 * and rule: the same bits whatever the order of the faces in flight, the cut of the views into calls or passes, and the stream.  The
 * only global atomics are 64-bit integer minima and integer sums.
 *
 *   vertices float [Nv, 3], faces int32 [F, 3], Nv, F < 2^31; per view world_to_cam float [12] ([R | t], row-major) and intrinsics
 *   float [4] = (fx, fy, cx, cy); one image size 1 <= H, W <= 16384, pixel centres at integer coordinates; 0 < near <= far.
 *   Every float operation is rounded on its own, no fused multiply-add.  Per (view, face):
 *   1. Bad face: an index outside [0, Nv), or a corner coordinate that fails |c| < 2^14 as floats (NaN and infinity fail).
 *   2. Camera space: x_c = ((r00 x + r01 y) + r02 z) + t0, y_c and z_c alike; any corner with z_c < near drops the face ("near": there
 *      is no near-plane clipping).
 *   3. u = (fx x_c) / z_c + cx, v alike; any corner that fails |u| < 2^14 && |v| < 2^14 drops the face ("guard"); X = (int)rint(u 256),
 *      Y alike.
 *   4. int64 edge functions E(a, b, P) = (bx - ax)(Py - ay) - (by - ay)(Px - ax), P = (256 ui, 256 vi); A = E(v0, v1, v2); A == 0 or a
 *      clamped bounding box without a pixel centre drops the face ("empty"); s = sign(A), w0 = s E(v1, v2, P), w1 = s E(v2, v0, P),
 *      w2 = s E(v0, v1, P); covered iff all three >= 0 (edges inclusive, both windings, no culling).
 *   5. double: q_i = 1 / z_c,i, num = (w0 q0 + w1 q1) + w2 q2, d = (float)(|A| / num); the sample is kept iff near <= d <= far.
 *   6. The pixel keeps the minimum key (bits of d << 32) | face: the nearest face, ties to the lower face index.
 *   7. depth float (0 where nothing was hit), face int32 (-1), vertex int32 = faces[face][i] for the largest w_i, ties to the lowest i
 *      (-1); face_labels int32 [Lf, F] read at `face`, vertex_labels int32 [Lv, Nv] read at `vertex`, `fill` where nothing was hit;
 *      Lf + Lv <= SD3D_RASTER_MAX_LABELS.
 *   8. info int64 [SD3D_RASTER_INFO_WORDS] = drawn, near, guard, empty, bad (each (view, face) pair exactly once, precedence bad, near,
 *      guard, empty, drawn), pixels hit.  The call clears it first.
 *
 *   sd3d_raster_views: the V views in passes of at most views_per_pass that share one key buffer; the result does not depend on it.
 *     Records of drawn pairs split by clamped bounding-box area: up to SD3D_RASTER_SMALL_MAX_PIXELS one lane draws the face, above it
 *     one wave.  depth_out float [V, H, W], face_out, vertex_out int32 [V, H, W], face_labels_out int32 [Lf, V, H, W],
 *     vertex_labels_out int32 [Lv, V, H, W]: each optional, the label outputs required when their labels are given.  A pass must keep
 *     views * F below 2^31.  ws: sd3d_raster_ws_bytes(F, min(views_per_pass, V), H, W) bytes (0 for bad arguments), 256-byte aligned.
 * ------------------------------------------------------------------------------------------- */
#define SD3D_RASTER_MAX_LABELS 8
#define SD3D_RASTER_INFO_WORDS 6
#define SD3D_RASTER_SMALL_MAX_PIXELS 64
size_t sd3d_raster_ws_bytes(int64_t n_faces, int views_per_pass, int H, int W);
int sd3d_raster_views(const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, const float* world_to_cam,
                      const float* intrinsics, int V, int H, int W, float near, float far, int views_per_pass, const int32_t* face_labels,
                      int n_face_labels, const int32_t* vertex_labels, int n_vertex_labels, int fill, float* depth_out, int32_t* face_out,
                      int32_t* vertex_out, int32_t* face_labels_out, int32_t* vertex_labels_out, int64_t* info, void* ws, size_t ws_bytes,
                      void* stream);

/* ---------------------------------------------------------------------------------------------
 * Mesh decimation (csrc/simplify.hip): vertex clustering on a grid - the vertices of one cell become one vertex, faces follow their
 * corners, collapsed and duplicate faces go - with the maps that carry per-vertex results back to the full mesh and face labels
 * forward.  The reference has no counterpart (it loads meshes decimated offline); tests/simplify_ref.py restates the rule below in
 * numpy and the kernels EQUAL it, bit for bit.  segdino3d_amd/simplify.py has the rule in full.  The call only enqueues work.  Every
 * sum is a 64-bit integer sum and every choice a minimum over a set, so the result is a pure function of the mesh and the rule: the
 * same bits whatever the schedule and the stream.  The only global atomics are 64-bit integer sums and minima.
 *
 *   vertices float [V, C], 3 <= C <= SD3D_SIMPLIFY_MAX_CHANNELS (x, y, z, then attributes), faces int32 [F, 3], V, F < 2^31;
 *   inv_cell = (float)(1 / cell) with cell >= 2^-6, so 0 < inv_cell <= 64.  Every float operation is rounded on its own, no fused
 *   multiply-add.
 *   1. A vertex is bad unless all C channels satisfy |c| < 2^14 as floats (NaN and infinity fail): vertex_map = -1.
 *   2. k_i = floorf(x_i inv_cell); key ((k_x + 2^20) << 42) | ((k_y + 2^20) << 21) | (k_z + 2^20).
 *   3. Per cell: n members, S_j = sum of (int64) rintf(c_j 65536.0f) per channel.
 *   4. One output vertex per occupied cell, in ascending key.  nearest == 0: channel j = (float)((double) S_j / ((double) n 65536.0)).
 *      nearest != 0: the row of the member with the smallest (bits of d2 << 32) | vertex index, copied bit for bit, d2 = (dx dx + dy dy)
 *      + dz dz against the float mean of x, y, z.
 *   5. A face with an index outside [0, V) or a bad corner is bad.  Otherwise its corners go through vertex_map; two equal corners:
 *      collapsed.  Otherwise it is rotated so that its smallest index comes first; of the faces with one oriented triple the lowest
 *      original index survives (the others: duplicates); survivors come out in ascending original index, as the rotated triple.
 *   6. keep_unreferenced == 0: output vertices that no surviving face references are dropped (their members' vertex_map = -1), the rest
 *      renumbered in key order.  The counter is filled either way.
 *   7. info int64 [SD3D_SIMPLIFY_INFO_WORDS] = vertices, faces, bad_vertices, bad_faces, collapsed, duplicates, unreferenced.  More than
 *      2^21 occupied cells (vertices + unreferenced) do not fit the 63-bit face key: the caller must refuse the result.
 *
 *   sd3d_simplify_mesh: vertices_out float [V, C] and faces_out int32 [F, 3], face_source int32 [F] at capacity (the first info[0] /
 *     info[1] rows are written), vertex_map int32 [V].  V == 0 and F == 0 are ordinary inputs.  ws: sd3d_simplify_ws_bytes(V, F, C)
 *     bytes (0 when the sizes do not fit), 256-byte aligned.
 * ------------------------------------------------------------------------------------------- */
#define SD3D_SIMPLIFY_INFO_WORDS 7
#define SD3D_SIMPLIFY_MAX_CHANNELS 11
size_t sd3d_simplify_ws_bytes(int64_t n_vertices, int64_t n_faces, int n_channels);
int sd3d_simplify_mesh(const float* vertices, int64_t n_vertices, int n_channels, const int32_t* faces, int64_t n_faces, float inv_cell,
                       int nearest, int keep_unreferenced, float* vertices_out, int32_t* faces_out, int32_t* vertex_map,
                       int32_t* face_source, int64_t* info, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Connected components (csrc/components.hip): the components of a mesh, an edge list or a neighbour table, their sizes and boxes, and
 * the clean that keeps only the components that pass - the stage that throws away the floating shells and specks of a fused TSDF or
 * cloud before simplify_mesh / the superpoints.  The reference has no counterpart (its meshes were cleaned offline);
 * tests/components_ref.py restates the rule below in numpy and the kernels EQUAL it, bit for bit.  segdino3d_amd/components.py has the
 * rule in full.  The call only enqueues work.  Components are a function of the SET of links, every decision is an integer one and
 * every statistic a sum or a minimum over a set: the same bits whatever the schedule and the stream.
 *
 *   n_nodes nodes; links int32, one of three sources:  SD3D_COMPONENTS_FACES [n_links, 3] (a link joins its three corners),
 *   SD3D_COMPONENTS_EDGES [n_links, 2], SD3D_COMPONENTS_TABLE [n_nodes, link_width] (entry j of row i joins i and j; -1 is an empty
 *   slot, skipped and not counted; n_links = n_nodes * link_width, the entries).  coords float [n_nodes, n_channels], 3 <= n_channels <=
 *   SD3D_COMPONENTS_MAX_CHANNELS (x, y, z first), or NULL with n_channels = 0: the pure graph form.  n_nodes, n_links < 2^31.
 *   1. A node is good iff all channels satisfy |c| < 2^14 as floats (a NaN fails; step 1 of the decimation); without coords every node
 *      is good.  A bad node has label -1, is never written out and counts in bad_nodes.
 *   2. A link is good iff every index lies in [0, n_nodes) and every end is good; otherwise it counts in bad_links and joins nothing.
 *      A link with repeated ends is good: it joins its distinct ends and is kept or dropped with its component.
 *   3. Components: the classes of the good nodes under "joined by a good link", closed transitively; a good node in no good link is a
 *      component of one node and counts in isolated.  They are numbered 0 .. K-1 in ascending order of their smallest node.
 *   4. Per component: comp_nodes, comp_links (good links, table entries one each), box float [K, 6] = x lo, x hi, y lo, y hi, z lo, z hi:
 *      the member coordinate that is smallest / largest under the integer key of its bits (b ^ 0x80000000 for b >= 0, ~b otherwise: -0
 *      sorts below +0), bit for bit; extent = max over the axes of (hi - lo), one float subtraction each.  Graph form: zeros.
 *   5. A component passes iff comp_nodes >= min_nodes, comp_links >= min_links and extent >= min_extent.  keep_largest = m > 0: only
 *      the first m passing components in the order (comp_links descending, label ascending) stay.  keep uint8 [K].
 *   6. The clean (every output optional): kept nodes in ascending original index, rows copied bit for bit (nodes_out [., n_channels]);
 *      node_map int32 [n_nodes] old -> new or -1; kept links in ascending original index with renumbered ends (links_out) and their
 *      original rows (link_source); labels_out = the component of each output node, renumbered densely over the kept components.  The
 *      table form writes the cleaned table of the same width at the nodes' new rows: an entry that is not a good link becomes -1, in
 *      place; link_source is not written.
 *   7. info int64 [SD3D_COMPONENTS_INFO_WORDS] = components, kept, nodes (written), links (written), bad_nodes, bad_links, isolated,
 *      unsettled: good links whose ends ended in different components - always 0; the caller must refuse the result otherwise.
 *
 *   sd3d_components: labels, comp_nodes, comp_links int32 [n_nodes] (the first info[0] of the latter two are written; required when
 *     n_nodes > 0); box float [n_nodes, 6], keep uint8 [n_nodes], nodes_out, node_map, links_out (the shape of links), link_source
 *     int32 [n_links], labels_out int32 [n_nodes]: at capacity, NULL = not wanted.  n_nodes == 0 and n_links == 0 are ordinary
 *     inputs.  ws: sd3d_components_ws_bytes(n_nodes, n_links, link_width, n_channels) bytes (0 when the sizes do not fit), 256-byte
 *     aligned.
 * ------------------------------------------------------------------------------------------- */
#define SD3D_COMPONENTS_INFO_WORDS 8
#define SD3D_COMPONENTS_MAX_CHANNELS 11
#define SD3D_COMPONENTS_FACES 0
#define SD3D_COMPONENTS_EDGES 1
#define SD3D_COMPONENTS_TABLE 2
size_t sd3d_components_ws_bytes(int64_t n_nodes, int64_t n_links, int link_width, int n_channels);
int sd3d_components(int source, const int32_t* links, int64_t n_links, int link_width, const float* coords, int64_t n_nodes, int n_channels,
                    int min_nodes, int min_links, float min_extent, int keep_largest, int32_t* labels, int32_t* comp_nodes,
                    int32_t* comp_links, float* box, uint8_t* keep, float* nodes_out, int32_t* node_map, int32_t* links_out,
                    int32_t* link_source, int32_t* labels_out, int64_t* info, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SEGDINO3D_HIP_H */
