// Internal helpers shared by the HIP translation units (gfx950 / CDNA4 only, wave = 64 lanes).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
#include <initializer_list>
#include "wave.h"

#define SD3D_OK 0
#define SD3D_ERR_ARG -1
#define SD3D_ERR_WS -2
#define SD3D_ERR_LAUNCH -3
#define SD3D_ERR_RANGE -4

#define SD3D_CHECK_LAUNCH()                                   \
    do {                                                      \
        hipError_t e_ = hipGetLastError();                    \
        if (e_ != hipSuccess) return sd3d_set_error(SD3D_ERR_LAUNCH, hipGetErrorString(e_)); \
    } while (0)

int sd3d_set_error(int code, const char* msg);

static inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// ------------------------------------------------------------------ voxel keys
// key = morton48(x, y, z) with x, y, z < 2^16 (bit 3i = x_i, 3i+1 = y_i, 3i+2 = z_i).  Bits 48..55
// hold the batch index.  Sorting keys therefore sorts voxels along a Z-order curve, and the key of
// the parent voxel at the next coarser level is (key >> 3) (morton part).
#define SD3D_MORTON_BITS 48
#define SD3D_MORTON_MASK ((1ull << 48) - 1ull)
#define SD3D_EMPTY_KEY 0xFFFFFFFFFFFFFFFFull

__host__ __device__ static inline uint64_t spread3_16(uint32_t v) {
    uint64_t x = v & 0xFFFFull;                     // the standard 21-bit ladder, fed 16 bits
    x = (x | (x << 32)) & 0x001f00000000ffffull;
    x = (x | (x << 16)) & 0x001f0000ff0000ffull;
    x = (x | (x << 8)) & 0x100f00f00f00f00full;
    x = (x | (x << 4)) & 0x10c30c30c30c30c3ull;
    x = (x | (x << 2)) & 0x1249249249249249ull;
    return x;
}
__host__ __device__ static inline uint32_t compact3_16(uint64_t x) {
    x &= 0x1249249249249249ull;
    x = (x ^ (x >> 2)) & 0x10c30c30c30c30c3ull;
    x = (x ^ (x >> 4)) & 0x100f00f00f00f00full;
    x = (x ^ (x >> 8)) & 0x001f0000ff0000ffull;
    x = (x ^ (x >> 16)) & 0x001f00000000ffffull;
    x = (x ^ (x >> 32)) & 0x00000000001fffffull;
    return (uint32_t)x;
}
__host__ __device__ static inline uint64_t morton_encode(uint32_t x, uint32_t y, uint32_t z) {
    return spread3_16(x) | (spread3_16(y) << 1) | (spread3_16(z) << 2);
}
__host__ __device__ static inline void morton_decode(uint64_t m, uint32_t& x, uint32_t& y, uint32_t& z) {
    x = compact3_16(m);
    y = compact3_16(m >> 1);
    z = compact3_16(m >> 2);
}

__device__ static inline uint32_t hash_u64(uint64_t k) {
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return (uint32_t)k;
}

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
// The accumulator of a 32x32 MFMA: register r of lane (j = lane & 31, h = lane >> 5) is element (row, col = j) of the tile with
// row = (r&3) + 8*(r>>2) + 4*h - four consecutive rows per group of four registers, the two half-waves interleaved in fours.
__host__ __device__ __forceinline__ int mfma32_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// The fused activation of every epilogue; the codes are ops.ACT: 0 none, 1 relu, 2 gelu(erf), 3 sigmoid.
__device__ __forceinline__ float sd3d_act(float y, int act) {
    if (act == 1) y = fmaxf(y, 0.f);
    else if (act == 2) y = 0.5f * y * (1.f + erff(y * 0.70710678118654752440f));
    else if (act == 3) y = 1.f / (1.f + expf(-y));
    return y;
}

// ------------------------------------------------------------------ per-device state
// A function attribute belongs to the CURRENT device, and one process may drive several through the C ABI: what is set once
// is set once per device.  Per-device tables have SD3D_MAX_DEVICES entries, indexed by sd3d_device().
#define SD3D_MAX_DEVICES 64
static inline int sd3d_device() {                          // the current device's index, or -1
    int dev = 0;
    return hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < SD3D_MAX_DEVICES ? dev : -1;
}
// Raises hipFuncAttributeMaxDynamicSharedMemorySize of a kernel, or of a group of kernels that launch together, once per device.
// `done` is one static object per kernel or group.  Callers may race: the flags are relaxed atomics and setting the attribute
// twice is harmless.  `dev` is the caller's sd3d_device() where it has one already (< 0: asked here).
struct Sd3dLdsRaised { std::atomic<bool> on[SD3D_MAX_DEVICES]; };
struct Sd3dLdsKernel { const void* fn; int bytes; };
static inline int sd3d_raise_lds_limit(Sd3dLdsRaised& done, const Sd3dLdsKernel* kernels, int n, int dev = -1) {
    if (dev < 0) dev = sd3d_device();
    if (dev < 0 || dev >= SD3D_MAX_DEVICES) return sd3d_set_error(SD3D_ERR_LAUNCH, "raise_lds_limit: no device");
    if (done.on[dev].load(std::memory_order_relaxed)) return SD3D_OK;
    for (int i = 0; i < n; ++i)
        if (hipFuncSetAttribute(kernels[i].fn, hipFuncAttributeMaxDynamicSharedMemorySize, kernels[i].bytes) != hipSuccess)
            return sd3d_set_error(SD3D_ERR_LAUNCH, "raise_lds_limit: the runtime refused a kernel's dynamic LDS size");
    done.on[dev].store(true, std::memory_order_relaxed);
    return SD3D_OK;
}
static inline int sd3d_raise_lds_limit(Sd3dLdsRaised& done, std::initializer_list<Sd3dLdsKernel> kernels, int dev = -1) {
    return sd3d_raise_lds_limit(done, kernels.begin(), (int)kernels.size(), dev);
}

// ------------------------------------------------------------------ internal launchers called across translation units
// Declared here once, with names; the defining file includes this header too, so a call and its definition cannot drift apart.
// sort_scan.hip
size_t sort_ws_bytes(int64_t n);
int sort_pairs_u64(uint64_t* keys_in, uint32_t* vals_in, uint64_t* keys_out, uint32_t* vals_out, int64_t n, int begin_bit, int end_bit,
                   void* ws, size_t ws_bytes, hipStream_t st, uint32_t* vals_scratch, int* landed_in_input);
size_t scan_ws_bytes(int64_t n);
int scan_exclusive_i32(const int* in, int* out, int64_t n_cap, const int* n_dev, int* total_dev, void* ws, size_t ws_bytes, hipStream_t st);
int launch_i64_to_sortkey_checked_max(const int64_t* x, int64_t n, uint64_t* keys, int bits, int32_t* flag, int value, int32_t* max_out,
                                      hipStream_t st, uint64_t add);
// dense.hip
int launch_scale_shift_act(const float* x0, int ld0, int C0, const float* x1, int ld1, const float* scale, const float* shift, int act,
                           int64_t M, int C, const float* add, int ld_add, float* out, int ld_out, hipStream_t st);
