// The ground-truth id rule of the streamed evaluations, shared by sd3d_ap_scene (csrc/apeval.hip: point -> column of the count
// matrix) and sd3d_gt_boxes (csrc/boxeval.hip: point -> the instance whose box it widens).  One body, so both read a scene alike.
#pragma once
#include "common.h"
#include "../../include/segdino3d_hip.h"

#define AP_NI SD3D_AP_INSTANCE_COLS
#define AP_VOID SD3D_AP_INSTANCE_COLS                   // the void column
#define AP_NOWHERE (SD3D_AP_INSTANCE_COLS + 1)          // id 0 of the valid semantic id 0: counted in the prediction's size only

// Column of one point: id_map != NULL applies `map_inst_markup` first; the class of the semantic id comes from `lut`; an instance index
// in [0, AP_NI) with a class is its own column, index -1 or no class the void column, semantic id 0 with a class and instance 0 no
// column at all.  *cls: the class index (meaningful when the column is an instance), *bad |= SD3D_AP_BAD_INSTANCE for an index outside
// [-1, AP_NI).
__device__ static inline int ap_point_column(int64_t s, int64_t in, const int64_t* __restrict__ id_map, int map_len, int num_stuff,
                                             const int32_t* __restrict__ lut, int lut_len, int C, int* cls_out, int* bad) {
    if (id_map) {
        in -= num_stuff;
        if (in < 0) in = -1;
        s -= num_stuff;
        if (in == -1) s = -1;
        const int64_t idx = s < 0 ? s + map_len : s;
        s = (idx >= 0 && idx < map_len) ? id_map[idx] : -1;
    }
    const int cls = (s >= 0 && s < lut_len) ? lut[s] : -1;
    *cls_out = cls;
    if (in < -1 || in >= AP_NI) { *bad |= SD3D_AP_BAD_INSTANCE; return AP_VOID; }
    if (cls < 0 || cls >= C || in == -1) return AP_VOID;
    if (s == 0 && in == 0) return AP_NOWHERE;
    return (int)in;
}

__device__ static inline void ap_raise(unsigned long long* status, int bits) {         // every lane of the wave must arrive
    const unsigned long long any = __ballot(bits != 0);
    if (!any) return;
    bits = wave_or(bits);
    if ((threadIdx.x & 63) == 0) atomicOr(status, (unsigned long long)bits);
}

__device__ static inline uint32_t ap_sortable(float s) {
    if (s == 0.0f) s = 0.0f;                            // -0 and +0 are one score
    const uint32_t u = __float_as_uint(s);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ static inline int64_t ap_code(int group, float score, int truth) {
    return (int64_t)(((uint64_t)group << 33) | ((uint64_t)ap_sortable(score) << 1) | (uint64_t)(truth & 1));
}
