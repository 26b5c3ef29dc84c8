// Parameter update of a training iteration as multi-tensor kernels: gradient-norm clipping (torch.nn.utils.clip_grad_norm_), the AdamW
// step (torch.optim.AdamW, single-tensor arithmetic order) and the exponential moving average of the weights (utils/ema_utils.py:34-38
// of the reference), each as ONE launch over every parameter tensor of the model instead of a few launches per tensor.
//
// A launch reads a tensor table (sd3d_mt_tensor, one per parameter that has a gradient) and a chunk list (sd3d_mt_chunk) that cuts the
// tensors into pieces of at most SD3D_MT_CHUNK elements; a chunk never crosses a tensor, so a 3-element bias is one short chunk and a
// 2.65 M-element kernel is 648 full ones, and a capped grid strides over the chunks with even work per workgroup.  It is all streaming
// work (32 B per value with the norm, 44 with the EMA): 16-byte accesses on the body of a chunk, scalar ones on the tail and on tensors
// whose pointers are not 16-byte aligned (a gradient that is a slice of a flat buffer: only its loads go scalar).
//
// Nothing here depends on scheduling: no atomics, the squared norm is one partial per chunk (a fixed tree inside the workgroup) added in
// chunk order by one workgroup in double precision, and every product below is rounded where it is written (contraction off; the fused
// multiply-adds are spelled out) so that the EMA of mt_adamw and of mt_ema are the same bits.
#include "common.h"
#include "../../include/segdino3d_hip.h"

#pragma clang fp contract(off)

#define MT_THREADS 256
#define MT_GRID 2048                 // 256 CUs x 8 workgroups; the chunks beyond are strided
#define MT_FINAL_THREADS 1024        // the one workgroup that adds the partials: 13 dependent adds per thread on the 528-tensor model

__device__ __forceinline__ bool mt_aligned16(const void* a) { return ((uintptr_t)a & 15) == 0; }

// 4 consecutive floats, as one 16-byte load when the pointer allows it
__device__ __forceinline__ f32x4 mt_load4(const float* a, bool vec) {
    if (vec) return *(const f32x4*)a;
    f32x4 r = {a[0], a[1], a[2], a[3]};
    return r;
}

// ema <- (1 - d) p + d ema, the reference's `(1.0 - decay) * param + decay * shadow` (two products, one sum)
__device__ __forceinline__ float mt_ema1(float p, float e, float omd, float d) { return omd * p + d * e; }

struct MtScalars { float coef, decay, step_size, rsqrt_bc2, omb1, beta2, omb2, eps; };

// torch/optim/adam.py _single_tensor_adam with decoupled weight decay, one element; g is the raw gradient
__device__ __forceinline__ void mt_adamw1(float& p, float& m, float& v, float g, const MtScalars& s) {
    g = g * s.coef;                                   // clip_grad_norm_: grad.mul_(clip_coef)
    p = p * s.decay;                                  // param.mul_(1 - lr * weight_decay)
    m = fmaf(s.omb1, g - m, m);                       // exp_avg.lerp_(grad, 1 - beta1)
    v = fmaf(s.omb2 * g, g, v * s.beta2);             // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    const float denom = sqrtf(v) * s.rsqrt_bc2 + s.eps;   // exp_avg_sq.sqrt() / sqrt(bias_correction2) + eps
    p = p - s.step_size * (m / denom);                // param.addcdiv_(exp_avg, denom, value=-lr / bias_correction1)
}

__global__ __launch_bounds__(MT_THREADS) void mt_adamw_kernel(const sd3d_mt_tensor* __restrict__ tensors, const sd3d_mt_chunk* __restrict__ chunks,
                                                              int64_t n_chunks, const float* __restrict__ clip_coef) {
    const float coef = clip_coef ? *clip_coef : 1.f;
    for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const sd3d_mt_chunk ck = chunks[c];
        const sd3d_mt_tensor t = tensors[ck.tensor];
        const int64_t off = (int64_t)ck.index * SD3D_MT_CHUNK;
        const int len = (int)(t.n - off < SD3D_MT_CHUNK ? t.n - off : SD3D_MT_CHUNK);
        float *p = t.p + off, *m = t.m + off, *v = t.v + off, *e = t.ema ? t.ema + off : nullptr;
        const float* g = t.g + off;
        const MtScalars s = {coef, t.decay, t.step_size, t.rsqrt_bc2, t.one_minus_beta1, t.beta2, t.one_minus_beta2, t.eps};
        const float d = t.ema_decay, omd = t.one_minus_ema_decay;
        const bool vec = mt_aligned16(p) && mt_aligned16(m) && mt_aligned16(v) && mt_aligned16(e), gvec = mt_aligned16(g);
        const int nv = vec ? len >> 2 : 0;
        for (int i = threadIdx.x; i < nv; i += MT_THREADS) {
            f32x4 P = ((const f32x4*)p)[i], M = ((const f32x4*)m)[i], V = ((const f32x4*)v)[i];
            const f32x4 G = mt_load4(g + 4 * i, gvec);
            f32x4 E = {0.f, 0.f, 0.f, 0.f};
            if (e) E = ((const f32x4*)e)[i];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float pk = P[k], mk = M[k], vk = V[k];
                mt_adamw1(pk, mk, vk, G[k], s);
                P[k] = pk; M[k] = mk; V[k] = vk;
            }
            ((f32x4*)p)[i] = P; ((f32x4*)m)[i] = M; ((f32x4*)v)[i] = V;
            if (e) {
#pragma unroll
                for (int k = 0; k < 4; ++k) E[k] = mt_ema1(P[k], E[k], omd, d);
                ((f32x4*)e)[i] = E;
            }
        }
        for (int i = nv * 4 + threadIdx.x; i < len; i += MT_THREADS) {
            float P = p[i], M = m[i], V = v[i];
            mt_adamw1(P, M, V, g[i], s);
            p[i] = P; m[i] = M; v[i] = V;
            if (e) e[i] = mt_ema1(P, e[i], omd, d);
        }
    }
}

__global__ __launch_bounds__(MT_THREADS) void mt_ema_kernel(const sd3d_mt_tensor* __restrict__ tensors, const sd3d_mt_chunk* __restrict__ chunks,
                                                            int64_t n_chunks) {
    for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const sd3d_mt_chunk ck = chunks[c];
        const sd3d_mt_tensor t = tensors[ck.tensor];
        if (!t.ema) continue;
        const int64_t off = (int64_t)ck.index * SD3D_MT_CHUNK;
        const int len = (int)(t.n - off < SD3D_MT_CHUNK ? t.n - off : SD3D_MT_CHUNK);
        const float* p = t.p + off;
        float* e = t.ema + off;
        const float d = t.ema_decay, omd = t.one_minus_ema_decay;
        const int nv = mt_aligned16(p) && mt_aligned16(e) ? len >> 2 : 0;
        for (int i = threadIdx.x; i < nv; i += MT_THREADS) {
            const f32x4 P = ((const f32x4*)p)[i];
            f32x4 E = ((const f32x4*)e)[i];
#pragma unroll
            for (int k = 0; k < 4; ++k) E[k] = mt_ema1(P[k], E[k], omd, d);
            ((f32x4*)e)[i] = E;
        }
        for (int i = nv * 4 + threadIdx.x; i < len; i += MT_THREADS) e[i] = mt_ema1(p[i], e[i], omd, d);
    }
}

// partial[c] = sum of g^2 over chunk c: per-thread sum in element order, then the same shuffle / LDS tree in every run
__global__ __launch_bounds__(MT_THREADS) void mt_sqnorm_kernel(const sd3d_mt_tensor* __restrict__ tensors, const sd3d_mt_chunk* __restrict__ chunks,
                                                               int64_t n_chunks, float* __restrict__ partial) {
    __shared__ float wave_sum[MT_THREADS / 64];
    for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const sd3d_mt_chunk ck = chunks[c];
        const sd3d_mt_tensor* t = tensors + ck.tensor;
        const int64_t n = t->n, off = (int64_t)ck.index * SD3D_MT_CHUNK;
        const int len = (int)(n - off < SD3D_MT_CHUNK ? n - off : SD3D_MT_CHUNK);
        const float* g = t->g + off;
        const int nv = mt_aligned16(g) ? len >> 2 : 0;
        float acc = 0.f;
        for (int i = threadIdx.x; i < nv; i += MT_THREADS) {
            const f32x4 G = ((const f32x4*)g)[i];
            acc = fmaf(G[0], G[0], acc); acc = fmaf(G[1], G[1], acc); acc = fmaf(G[2], G[2], acc); acc = fmaf(G[3], G[3], acc);
        }
        for (int i = nv * 4 + threadIdx.x; i < len; i += MT_THREADS) acc = fmaf(g[i], g[i], acc);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
        if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = acc;
        __syncthreads();
        if (threadIdx.x == 0) partial[c] = (wave_sum[0] + wave_sum[1]) + (wave_sum[2] + wave_sum[3]);
        __syncthreads();
    }
}

// out[0] = total_norm = sqrt(sum of the partials, added in index order: thread i takes i, i + 1024, ..., then a fixed tree),
// out[1] = clip_coef = min(1, max_norm / (total_norm + 1e-6)) (torch's clip_grad_norm_)
__global__ __launch_bounds__(MT_FINAL_THREADS) void mt_norm_final_kernel(const float* __restrict__ partial, int64_t n_chunks, float max_norm,
                                                                   float* __restrict__ out) {
    __shared__ double sm[MT_FINAL_THREADS];
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < n_chunks; i += MT_FINAL_THREADS) acc += (double)partial[i];
    sm[threadIdx.x] = acc;
    __syncthreads();
    for (int o = MT_FINAL_THREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sm[threadIdx.x] += sm[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float total = (float)sqrt(sm[0]);
        const float coef = max_norm / (total + 1e-6f);
        out[0] = total;
        out[1] = coef > 1.f ? 1.f : coef;             // torch.clamp(coef, max=1.0): a NaN norm stays NaN
    }
}

static size_t mt_tensor_bytes(int n_tensors) { return align_up((size_t)n_tensors * sizeof(sd3d_mt_tensor), 256); }
static size_t mt_chunk_bytes(int64_t n_chunks) { return align_up((size_t)n_chunks * sizeof(sd3d_mt_chunk), 256); }

// Every chunk must lie inside its tensor, and every pointer the kernel will follow must be there: the kernels trust the table.
static int mt_check(const sd3d_mt_tensor* tensors, int n_tensors, const sd3d_mt_chunk* chunks, int64_t n_chunks, int need, const char* who) {
    if (!tensors || !chunks || n_tensors <= 0 || n_chunks <= 0) return sd3d_set_error(SD3D_ERR_ARG, who);
    for (int i = 0; i < n_tensors; ++i) {
        const sd3d_mt_tensor& t = tensors[i];
        if (t.n <= 0 || ((need & 1) && !t.g) || ((need & 2) && (!t.p || !t.m || !t.v)) || ((need & 4) && !t.p) || ((uintptr_t)t.p & 3) ||
            ((uintptr_t)t.g & 3) || ((uintptr_t)t.m & 3) || ((uintptr_t)t.v & 3) || ((uintptr_t)t.ema & 3))
            return sd3d_set_error(SD3D_ERR_ARG, "multi-tensor table: empty tensor, missing pointer or pointer not aligned to 4 bytes");
    }
    for (int64_t c = 0; c < n_chunks; ++c) {
        const sd3d_mt_chunk ck = chunks[c];
        if (ck.tensor < 0 || ck.tensor >= n_tensors || ck.index < 0 || (int64_t)ck.index * SD3D_MT_CHUNK >= tensors[ck.tensor].n)
            return sd3d_set_error(SD3D_ERR_RANGE, "multi-tensor table: chunk outside its tensor");
    }
    return SD3D_OK;
}

// ws = [tensor table | chunk list | one float per chunk].  resident = 1: ws already holds this table (uploaded by the previous call).
static int mt_upload(const sd3d_mt_tensor* tensors, int n_tensors, const sd3d_mt_chunk* chunks, int64_t n_chunks, int need, int resident,
                     void* ws, size_t ws_bytes, hipStream_t st, const char* who, const sd3d_mt_tensor** d_tensors, const sd3d_mt_chunk** d_chunks) {
    if (int rc = mt_check(tensors, n_tensors, chunks, n_chunks, need, who)) return rc;
    if (!ws || ((uintptr_t)ws & 15) || ws_bytes < sd3d_mt_ws_bytes(n_tensors, n_chunks)) return sd3d_set_error(SD3D_ERR_WS, who);
    char* base = (char*)ws;
    if (!resident) {
        if (hipMemcpyAsync(base, tensors, (size_t)n_tensors * sizeof(sd3d_mt_tensor), hipMemcpyHostToDevice, st) != hipSuccess ||
            hipMemcpyAsync(base + mt_tensor_bytes(n_tensors), chunks, (size_t)n_chunks * sizeof(sd3d_mt_chunk), hipMemcpyHostToDevice, st) != hipSuccess)
            return sd3d_set_error(SD3D_ERR_LAUNCH, hipGetErrorString(hipGetLastError()));
    }
    *d_tensors = (const sd3d_mt_tensor*)base;
    *d_chunks = (const sd3d_mt_chunk*)(base + mt_tensor_bytes(n_tensors));
    return SD3D_OK;
}

static unsigned mt_grid(int64_t n_chunks) { return (unsigned)(n_chunks < MT_GRID ? n_chunks : MT_GRID); }

#define ST ((hipStream_t)stream)
extern "C" {

size_t sd3d_mt_ws_bytes(int n_tensors, int64_t n_chunks) {
    if (n_tensors <= 0 || n_chunks <= 0) return 0;
    return mt_tensor_bytes(n_tensors) + mt_chunk_bytes(n_chunks) + align_up((size_t)n_chunks * sizeof(float), 256);
}

int sd3d_mt_grad_norm(const sd3d_mt_tensor* tensors, int n_tensors, const sd3d_mt_chunk* chunks, int64_t n_chunks, float max_norm,
                      float* norm_out, void* ws, size_t ws_bytes, void* stream) {
    const sd3d_mt_tensor* dt; const sd3d_mt_chunk* dc;
    if (!norm_out) return sd3d_set_error(SD3D_ERR_ARG, "mt_grad_norm: norm_out is null");
    if (int rc = mt_upload(tensors, n_tensors, chunks, n_chunks, 1, 0, ws, ws_bytes, ST, "mt_grad_norm: bad table or workspace", &dt, &dc)) return rc;
    float* partial = (float*)((char*)ws + mt_tensor_bytes(n_tensors) + mt_chunk_bytes(n_chunks));
    mt_sqnorm_kernel<<<mt_grid(n_chunks), MT_THREADS, 0, ST>>>(dt, dc, n_chunks, partial);
    mt_norm_final_kernel<<<1, MT_FINAL_THREADS, 0, ST>>>(partial, n_chunks, max_norm, norm_out);
    SD3D_CHECK_LAUNCH();
    return SD3D_OK;
}

int sd3d_mt_adamw(const sd3d_mt_tensor* tensors, int n_tensors, const sd3d_mt_chunk* chunks, int64_t n_chunks, const float* clip_coef,
                  int table_resident, void* ws, size_t ws_bytes, void* stream) {
    const sd3d_mt_tensor* dt; const sd3d_mt_chunk* dc;
    if (int rc = mt_upload(tensors, n_tensors, chunks, n_chunks, 3, table_resident, ws, ws_bytes, ST, "mt_adamw: bad table or workspace", &dt, &dc))
        return rc;
    mt_adamw_kernel<<<mt_grid(n_chunks), MT_THREADS, 0, ST>>>(dt, dc, n_chunks, clip_coef);
    SD3D_CHECK_LAUNCH();
    return SD3D_OK;
}

int sd3d_mt_ema(const sd3d_mt_tensor* tensors, int n_tensors, const sd3d_mt_chunk* chunks, int64_t n_chunks, int table_resident, void* ws,
                size_t ws_bytes, void* stream) {
    const sd3d_mt_tensor* dt; const sd3d_mt_chunk* dc;
    if (int rc = mt_upload(tensors, n_tensors, chunks, n_chunks, 4, table_resident, ws, ws_bytes, ST, "mt_ema: bad table or workspace", &dt, &dc))
        return rc;
    mt_ema_kernel<<<mt_grid(n_chunks), MT_THREADS, 0, ST>>>(dt, dc, n_chunks);
    SD3D_CHECK_LAUNCH();
    return SD3D_OK;
}

}  // extern "C"
