// Layer-sequence executor: runs a whole sparse U-Net (or any straight-line list of the layer kinds
// below) from ONE C call.  The Python host used to issue every convolution itself - ~110 ctypes
// calls and as many tensor allocations per scene, all under the GIL (~2 ms of the ~6.5 ms a forward costs on
// the host).  The plan (sd3d_layer[]) is built once per model;
// per scene the caller provides the neighbour tables and ONE arena carved into the activation
// buffers (sd3d_buf[]), so this call neither allocates nor synchronises: it only enqueues.
#include "gg_common.h"
#include "pair_conv.h"

extern "C" int sd3d_run_layers(const sd3d_layer* layers, int n_layers, const sd3d_table* tables, int n_tables, const sd3d_buf* bufs,
                               int n_bufs, float* part, size_t part_bytes, void* ws, size_t ws_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    for (int i = 0; i < n_layers; ++i) {
        const sd3d_layer& L = layers[i];
        if (L.src0 < 0 || L.src0 >= n_bufs || L.dst < 0 || L.dst >= n_bufs || L.src1 >= n_bufs || L.res >= n_bufs)
            return sd3d_set_error(SD3D_ERR_ARG, "run_layers: buffer id out of range");
        const sd3d_buf& a = bufs[L.src0];
        const sd3d_buf* b = L.src1 >= 0 ? &bufs[L.src1] : nullptr;
        const sd3d_buf* r = L.res >= 0 ? &bufs[L.res] : nullptr;
        const sd3d_buf& o = bufs[L.dst];
        int rc = SD3D_OK;
        if (L.kind == SD3D_LAYER_PAIR_CONV) {
            if (L.table < 0 || L.table >= n_tables) return sd3d_set_error(SD3D_ERR_ARG, "run_layers: table id out of range");
            const sd3d_table& T = tables[L.table];
            if (T.K != L.K) return sd3d_set_error(SD3D_ERR_ARG, "run_layers: table / weight offset count mismatch");
            if (o.rows != T.M) return sd3d_set_error(SD3D_ERR_ARG, "run_layers: output buffer rows != table rows");
            rc = launch_pair_conv(a.ptr, a.ld, L.C0, b ? b->ptr : nullptr, b ? b->ld : 0, T.in_idx, T.tile_k, T.p_cap, T.pos, T.rlist,
                                  T.rl_stride, T.center, T.out_idx, L.wt, L.K,
                                  L.Cin, L.Cout, T.M, L.scale, L.shift, r ? r->ptr : nullptr, r ? r->ld : 0, o.ptr, o.ld, L.act, part,
                                  part_bytes, st);
        } else if (L.kind == SD3D_LAYER_DENSE) {
            const GGParams p = gg_params(a.ptr, a.ld, L.C0, b ? b->ptr : nullptr, b ? b->ld : 0, nullptr, L.wt, 1, L.Cin, L.Cout, o.rows, L.scale,
                                         L.shift, r ? r->ptr : nullptr, r ? r->ld : 0, o.ptr, o.ld, L.act);
            rc = launch_gather_gemm(p, 0, ws, ws_bytes, st);
        } else if (L.kind == SD3D_LAYER_SCALE_SHIFT_ACT) {
            rc = launch_scale_shift_act(a.ptr, a.ld, L.C0, b ? b->ptr : nullptr, b ? b->ld : 0, L.scale, L.shift, L.act, o.rows, L.Cin,
                                        r ? r->ptr : nullptr, r ? r->ld : 0, o.ptr, o.ld, st);
        } else {
            return sd3d_set_error(SD3D_ERR_ARG, "run_layers: unknown layer kind");
        }
        if (rc != SD3D_OK) return rc;
    }
    return SD3D_OK;
}
