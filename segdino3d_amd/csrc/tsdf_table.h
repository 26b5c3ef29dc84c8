// The block table of a TSDF volume's workspace as tsdf.hip (which owns and writes it) and track.hip (which only reads it) see it: the
// key of a block, the read-only probe and the layout of the workspace.  One definition, so that the two files cannot drift apart.
// Integer code only: the `#pragma clang fp contract` state of the including file does not matter here.
#pragma once
#include "common.h"
#include "../../include/segdino3d_hip.h"

#define TS_VOX 512                                      // voxels of a block
#define TS_WORDS SD3D_TSDF_VOXEL_WORDS
#define TS_BLOCK_BIAS (1 << 17)                         // block indices lie in [-2^17, 2^17): 18 bits per axis of the block key
#define TS_CELL_BIAS (1 << 20)
typedef unsigned long long ts_u64;

// the counters at the head of the workspace, 64-bit each
enum { TS_BLOCKS = 0, TS_UPDATES = 1, TS_RANGE = 2, TS_OVERFLOW = 3, TS_NLIST = 4, TS_NVERT = 5, TS_OBSERVED = 6, TS_COUNTERS = 7 };

__device__ __forceinline__ ts_u64 ts_block_key(int bx, int by, int bz) {
    return ((ts_u64)(uint32_t)(bx + TS_BLOCK_BIAS) << 36) | ((ts_u64)(uint32_t)(by + TS_BLOCK_BIAS) << 18) | (ts_u64)(uint32_t)(bz + TS_BLOCK_BIAS);
}
__device__ __forceinline__ void ts_block_coords(ts_u64 key, int& bx, int& by, int& bz) {
    bx = (int)((key >> 36) & 0x3FFFFull) - TS_BLOCK_BIAS;
    by = (int)((key >> 18) & 0x3FFFFull) - TS_BLOCK_BIAS;
    bz = (int)(key & 0x3FFFFull) - TS_BLOCK_BIAS;
}
// the slot of a block key, or -1: a read-only probe of a table nobody is inserting into
__device__ __forceinline__ int ts_find_key(const ts_u64* __restrict__ keys, uint32_t mask, ts_u64 key) {
    uint32_t slot = hash_u64(key) & mask;
    for (int probe = 0; probe < SD3D_TSDF_PROBE_LIMIT; ++probe) {
        const ts_u64 k = keys[slot];
        if (k == key) return (int)slot;
        if (k == SD3D_EMPTY_KEY) return -1;
        slot = (slot + 1) & mask;
    }
    return -1;
}
__device__ __forceinline__ int ts_find(const ts_u64* __restrict__ keys, uint32_t mask, int bx, int by, int bz) {
    if (bx < -TS_BLOCK_BIAS || bx >= TS_BLOCK_BIAS || by < -TS_BLOCK_BIAS || by >= TS_BLOCK_BIAS || bz < -TS_BLOCK_BIAS || bz >= TS_BLOCK_BIAS)
        return -1;
    return ts_find_key(keys, mask, ts_block_key(bx, by, bz));
}

struct TsWs {
    ts_u64 *counters, *keys, *touched;
    uint32_t* list;
    int32_t *vox, *cellvert;
    size_t total;
};
static TsWs ts_ws(void* ws, int64_t capacity) {
    TsWs w;
    char* p = (char*)ws;
    size_t o = 0;
    const size_t m = (size_t)capacity;
    auto take = [&](size_t bytes) { char* q = p + o; o += align_up(bytes, 256); return (void*)q; };
    w.counters = (ts_u64*)take(TS_COUNTERS * 8);
    w.keys = (ts_u64*)take(m * 8);
    w.touched = (ts_u64*)take(m * 8);
    w.list = (uint32_t*)take(m * 4);
    w.vox = (int32_t*)take(m * TS_WORDS * TS_VOX * 4);
    w.cellvert = (int32_t*)take(m * TS_VOX * 4);
    w.total = o;
    return w;
}
static bool ts_capacity_ok(int64_t c) { return c >= SD3D_TSDF_MIN_CAPACITY && c <= SD3D_TSDF_MAX_CAPACITY && (c & (c - 1)) == 0; }
static int ts_check_ws(const char* who, void* ws, size_t ws_bytes, int64_t capacity, TsWs& w) {
    char msg[160];                                      // sd3d_set_error copies it
    if (!ts_capacity_ok(capacity)) {
        snprintf(msg, sizeof msg, "%s: capacity must be a power of two in [2^4, 2^20]", who);
        return sd3d_set_error(SD3D_ERR_ARG, msg);
    }
    if (!ws || ((uintptr_t)ws & 255) != 0) {
        snprintf(msg, sizeof msg, "%s: ws is required and must be 256-byte aligned", who);
        return sd3d_set_error(SD3D_ERR_ARG, msg);
    }
    w = ts_ws(ws, capacity);
    if (ws_bytes < w.total) {
        snprintf(msg, sizeof msg, "%s: workspace too small (sd3d_tsdf_ws_bytes)", who);
        return sd3d_set_error(SD3D_ERR_WS, msg);
    }
    return SD3D_OK;
}
