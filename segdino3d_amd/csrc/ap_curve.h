// The precision / recall curve of one (class, overlap) group of sorted entry codes, shared by sd3d_ap_finish (csrc/apeval.hip: one group
// per workgroup over the entries of all scenes) and sd3d_ap_finish_scenes (csrc/apeval_scene.hip: one group per workgroup and scene).
// One body, so both routes give the same bits for the same segment.
#pragma once
#include "common.h"

__device__ static inline int64_t ap_lower_bound(const uint64_t* __restrict__ a, int64_t n, uint64_t key) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// inclusive scan of two ints over the 256 threads of the workgroup
__device__ static inline void ap_scan2(int& a, int& b, int (*wsum)[4], int& tot_a, int& tot_b) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int x = __shfl_up(a, d), y = __shfl_up(b, d);
        if (lane >= d) { a += x; b += y; }
    }
    __syncthreads();                                                          // the previous round's readers are done with wsum
    if (lane == 63) { wsum[0][wv] = a; wsum[1][wv] = b; }
    __syncthreads();
    tot_a = tot_b = 0;
    for (int w = 0; w < 4; ++w) {
        if (w < wv) { a += wsum[0][w]; b += wsum[1][w]; }
        tot_a += wsum[0][w];
        tot_b += wsum[1][w];
    }
}

// A workgroup of 256 threads, every thread with the same arguments.  `codes` sorted; the group's entries are codes[lo .. hi) and P / R
// (as long as codes) are its scratch at the same indices.  gt / pred: the class has ground truth / predictions; hf: the group's hard
// false negatives.  Writes *ap_out, *pr_out, *rc_out: the curve with both, 0 with ground truth only, NaN otherwise.  The lower 33 bits of
// a code are (sortable score << 1 | true); whatever lies above them is the same for all entries of the segment.
__device__ static inline void ap_curve_body(const uint64_t* __restrict__ codes, int64_t lo, int64_t hi, int64_t hf, bool gt, bool pred,
                                            double* __restrict__ P, double* __restrict__ R, double* __restrict__ ap_out,
                                            double* __restrict__ pr_out, double* __restrict__ rc_out) {
#pragma clang fp contract(off)
    __shared__ int wsum[2][4];
    __shared__ double part[256], best_f[256];
    __shared__ int64_t best_i[256];
    const int t = threadIdx.x;
    if (!(gt && pred)) {
        if (t == 0) {
            const double v = gt ? 0.0 : __longlong_as_double(0x7FF8000000000000ll);
            *ap_out = *pr_out = *rc_out = v;
        }
        return;
    }
    const int64_t n_ex = hi - lo;
    // number of true entries
    int64_t n_true = 0;
    {
        int cnt = 0, zero = 0, tot = 0, tot0 = 0;
        for (int64_t j = lo + t; j < hi; j += 256) cnt += (int)(codes[j] & 1ull);
        ap_scan2(cnt, zero, wsum, tot, tot0);
        n_true = tot;
    }
    // precision / recall at the first index of every distinct score
    int64_t carry_true = 0, carry_first = 0;
    for (int64_t b = lo; b < hi; b += 256) {
        const int64_t j = b + t;
        const bool valid = j < hi;
        uint64_t code = 0;
        bool first = false;
        if (valid) {
            code = codes[j];
            first = j == lo || (uint32_t)(code >> 1) != (uint32_t)(codes[j - 1] >> 1);
        }
        const int tr = valid ? (int)(code & 1ull) : 0;
        int inc_t = tr, inc_f = first ? 1 : 0, tot_t, tot_f;
        ap_scan2(inc_t, inc_f, wsum, tot_t, tot_f);
        if (first) {
            const int64_t isc = j - lo, cexc = carry_true + inc_t - tr, ir = carry_first + inc_f - 1;
            const int64_t tp = n_true - cexc, fp = n_ex - isc - tp, fn = cexc + hf;
            P[lo + ir] = (double)tp / (double)(tp + fp);
            R[lo + ir] = (double)tp / (double)(tp + fn);
        }
        carry_true += tot_t;
        carry_first += tot_f;
    }
    __syncthreads();                                                          // P / R of this workgroup are read by its other threads below
    const int64_t U = carry_first;                                            // points 0 .. U - 1, and the closing point (1, 0) at U
    double s = 0.0, bf = -1.0;
    int64_t bi = -1;
    for (int64_t i = t; i <= U; i += 256) {
        const double p = i < U ? P[lo + i] : 1.0, r = i < U ? R[lo + i] : 0.0;
        const double r_prev = i == 0 ? r : R[lo + i - 1], r_next = i + 1 < U ? R[lo + i + 1] : 0.0;
        const double w = 0.5 * r_prev - 0.5 * r_next;
        s = s + p * w;
        const double f1 = (2.0 * p * r) / (p + r + 0.0001);
        if (bi < 0 || f1 > bf) { bf = f1; bi = i; }
    }
    part[t] = s;
    best_f[t] = bf;
    best_i[t] = bi;
    __syncthreads();
    for (int d = 128; d >= 1; d >>= 1) {
        if (t < d) {
            part[t] += part[t + d];
            const int64_t oi = best_i[t + d];
            if (oi >= 0 && (best_i[t] < 0 || best_f[t + d] > best_f[t] || (best_f[t + d] == best_f[t] && oi < best_i[t]))) {
                best_f[t] = best_f[t + d];
                best_i[t] = oi;
            }
        }
        __syncthreads();
    }
    if (t == 0) {
        const int64_t i = best_i[0];
        *ap_out = part[0];
        *pr_out = i < U ? P[lo + i] : 1.0;
        *rc_out = i < U ? R[lo + i] : 0.0;
    }
}
