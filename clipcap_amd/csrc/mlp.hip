// C ABI of the MLP mapping network (include/clipcap_hip.h cc_mlp_*): two GEMMs around a tanh, out of the launchers in gemm_api.h and
// kernels.h.  Like api.hip: no state, no allocation, no synchronisation; everything is enqueued on the caller's stream and lives in
// caller-owned arenas / workspaces.
#include "../../include/clipcap_hip.h"
#include "gemm_api.h"
#include "kernels.h"
#include "shared.h"
#include "layout.h"

using namespace CC_NS;

namespace {

struct MlpWS {
    act_t *x16, *h;             // forward: cast(emb) [B][E], tanh output [B][Hd]
    act_t *t, *g16, *dU;        // save only: 1 - h h [B][Hd], cast(dout) [B][L D], gradient of the pre-activation [B][Hd]
    float* wg_scratch;          // save only: weight-gradient slabs (gemm_api.h gemm_wgrad)
    float* red;                 // save only: partial sums of the cross-block reductions (kernels.h)
    char* x3;                   // bf16x3 build: operand-image scratch of the GEMM in flight (gemm_api.h)
    size_t x3_bytes;
    size_t bytes;
};

void mlp_carve(const cc_mlp_cfg* c, int B, int save, void* ws, MlpWS& w) {
    Carver cv(ws);
    const size_t b = (size_t)B, E = c->E, Hd = c->Hd, LD = (size_t)c->L * c->D;
    w.x16 = cv.take<act_t>(b * E);
    w.h = cv.take<act_t>(b * Hd);
    w.t = w.g16 = w.dU = nullptr;
    w.wg_scratch = w.red = nullptr;
    if (save) {
        w.t = cv.take<act_t>(b * Hd);
        w.g16 = cv.take<act_t>(b * LD);
        w.dU = cv.take<act_t>(b * Hd);
        w.wg_scratch = cv.take<float>(WGRAD_SCRATCH_BYTES / sizeof(float));
        w.red = cv.take<float>(RED_SCRATCH_FLOATS);
    }
    w.x3 = nullptr; w.x3_bytes = 0;
    if (kX3) {
        size_t need = std::max(x3_img(b, E), x3_img(b, Hd));                                    // forward A images
        if (save) need = std::max(need, x3_img(b, LD) + x3_img(b, Hd));                           // dW2's operand pair; dU's A image and dW1's pair are smaller
        w.x3_bytes = need;
        w.x3 = cv.take<char>(need);
    }
    w.bytes = cv.bytes();
}

// Reduction scratch: batch_sum over len = L D columns cuts the batch into at most 1024 / ceil(len / 256) slices of len floats, colsum_bf16 over
// N = Hd into at most 1024 / ceil(N / 64) slices of N (reduce.hip): at most 2^18 and 2^16 floats for ANY width, inside RED_SCRATCH_FLOATS = 2^20
// (E = 512, D = 768, L = 10: 34 x 7680 and 17 x 3840).  Should a launcher's slicing ever change, red_scratch() hands it no scratch for a
// request beyond the buffer and it returns CC_ERR_STATE: it cannot overrun.

// What every pass starts from (the record MapperPass is for the transformer mapper): built from validated arguments, no HIP call.
struct MlpPass {
    hipStream_t st;
    MlpOff o;
    MlpWS w;
    Call cx;
    int E, Hd, LD;
    MlpPass(const cc_mlp_cfg* c, int B, int save, void* ws, void* stream) : st(S_(stream)), o(c), E(c->E), Hd(c->Hd), LD(c->L * c->D) {
        mlp_carve(c, B, save, ws, w);
        cx = Call{st, w.red, w.x3, w.x3_bytes};
    }
};

int mlp_transposes(const cc_mlp_cfg* c, uint16_t* w16, hipStream_t st) {
    if (kX3) return CC_ERR_ARG;      // the operand images are made from the fp32 master (cc_mlp_sync_weights)
    const MlpOff o(c);
    return transpose_bf16(w16 + o.w2, w16 + o.total + o.w2, c->L * c->D, c->Hd, st);      // [L D][Hd] -> [Hd][L D]: the input-gradient GEMM is NT
}

}  // namespace

extern "C" {

int64_t CC_API(cc_mlp_param_count)(const cc_mlp_cfg* cfg) {
    if (!mlp_cfg_ok(cfg)) return CC_ERR_SHAPE;
    return MlpOff(cfg).total;
}

int CC_API(cc_mlp_param_offsets)(const cc_mlp_cfg* cfg, int64_t* offs) {
    if (!mlp_cfg_ok(cfg) || !offs) return CC_ERR_SHAPE;
    const MlpOff o(cfg);
    offs[0] = o.w1; offs[1] = o.b1; offs[2] = o.w2; offs[3] = o.b2;
    return CC_OK;
}

int64_t CC_API(cc_mlp_ws_bytes)(const cc_mlp_cfg* cfg, int32_t B, int32_t save) {
    if (!mlp_cfg_ok(cfg) || B <= 0) return CC_ERR_SHAPE;
    MlpWS w;
    mlp_carve(cfg, B, save, nullptr, w);
    return (int64_t)w.bytes;
}

int CC_API(cc_mlp_sync_weights)(const cc_mlp_cfg* c, const float* w32, uint16_t* w16, void* stream) {
    if (!mlp_cfg_ok(c) || !w32 || !w16) return CC_ERR_ARG;
    hipStream_t st = S_(stream);
    const MlpOff o(c);
#if CC_OP == 2
    const int LD = c->L * c->D;
    X3SplitBatch sb;
    sb.add(w32 + o.w1, W16(w16, o.w1), c->Hd, c->E, 0, 1);
    sb.add(w32 + o.w2, W16(w16, o.w2), LD, c->Hd, 0, 1);
    sb.add(w32 + o.w2, W16(w16, o.total + o.w2), LD, c->Hd, 1, 1);
    return x3_split_multi(sb, st);
#else
    CC_TRY(f32_to_bf16(w32, w16, (size_t)o.total, st));
    return mlp_transposes(c, w16, st);
#endif
}

int CC_API(cc_mlp_transpose_weights)(const cc_mlp_cfg* c, uint16_t* w16, void* stream) {
    if (!mlp_cfg_ok(c) || !w16) return CC_ERR_ARG;
    return mlp_transposes(c, w16, S_(stream));
}

int CC_API(cc_mlp_fwd)(const cc_mlp_cfg* c, int32_t B, const float* w32, const uint16_t* w16, const float* emb, void* ws, float* out, int32_t save,
               void* stream) {
    if (!mlp_cfg_ok(c) || B <= 0 || !w32 || !w16 || !emb || !ws || !out) return CC_ERR_ARG;
    MlpPass ps(c, B, save, ws, stream);
    auto& [st, o, w, cx, E, Hd, LD] = ps;
    CC_TRY(f32_to_act(emb, w.x16, (size_t)B * E, st));
    // h = tanh(x16 W1^T + b1); t = 1 - h h for the backward, which alone reads it
    CC_TRY(gemm_tanh(0, 0, w.x16, E, W16(w16, o.w1), E, B, Hd, E, w.h, Hd, w32 + o.b1, save ? w.t : nullptr, true, cx));
    // out = h W2^T + b2, viewed [B][L][D] by the caller
    return gemm_f32out(0, 0, w.h, Hd, W16(w16, o.w2), Hd, B, LD, Hd, out, LD, w32 + o.b2, 0, 1.0f, 1, cx);
}

int CC_API(cc_mlp_bwd_part)(const cc_mlp_cfg* c, int32_t B, const float* w32, const uint16_t* w16, void* ws, const float* dout, float* g32, int32_t part,
                    void* stream) {
    if (!mlp_cfg_ok(c) || B <= 0 || !w32 || !w16 || !ws || !dout || !g32 || (part != 0 && part != 1)) return CC_ERR_ARG;
    MlpPass ps(c, B, 1, ws, stream);
    auto& [st, o, w, cx, E, Hd, LD] = ps;
    if (part == 1) {
        CC_TRY(f32_to_act(dout, w.g16, (size_t)B * LD, st));
        CC_TRY(batch_sum(dout, (size_t)LD, g32 + o.b2, LD, B, cx));                                              // db2 += sum_b dout, fp32
        CC_TRY(gemm_wgrad(w.g16, LD, w.h, Hd, LD, Hd, B, g32 + o.w2, Hd, w.wg_scratch, cx));                     // dW2 += g16^T h
        const uint16_t* w16t = W16(w16, o.total);
        return gemm_dact(0, 0, w.g16, LD, W16(w16t, o.w2), LD, B, Hd, LD, w.dU, Hd, w.t, 3, cx);                // dU = (g16 W2) * t
    }
    CC_TRY(gemm_wgrad(w.dU, Hd, w.x16, E, Hd, E, B, g32 + o.w1, E, w.wg_scratch, cx));                           // dW1 += dU^T x16
    return colsum_bf16(w.dU, Hd, B, Hd, g32 + o.b1, cx);                                                         // db1 += column sums of dU
}

int CC_API(cc_mlp_bwd)(const cc_mlp_cfg* c, int32_t B, const float* w32, const uint16_t* w16, void* ws, const float* dout, float* g32, void* stream) {
    CC_TRY(CC_API(cc_mlp_bwd_part)(c, B, w32, w16, ws, dout, g32, 1, stream));
    return CC_API(cc_mlp_bwd_part)(c, B, w32, w16, ws, dout, g32, 0, stream);
}

int CC_API(cc_mlp_get)(const cc_mlp_cfg* c, int32_t B, void* ws, int32_t field, void* dst, int64_t dst_bytes, void* stream) {
    if (!mlp_cfg_ok(c) || B <= 0 || !ws || !dst || field < CC_MLP_X16 || field > CC_MLP_DU) return CC_ERR_ARG;
    MlpPass ps(c, B, 1, ws, stream);
    const act_t* src[5] = {ps.w.x16, ps.w.h, ps.w.t, ps.w.g16, ps.w.dU};
    const int width[5] = {ps.E, ps.Hd, ps.Hd, ps.LD, ps.Hd};
    const size_t n = (size_t)B * width[field] * sizeof(act_t);
    if (dst_bytes != (int64_t)n) return CC_ERR_SHAPE;
    return hipMemcpyAsync(dst, src[field], n, hipMemcpyDeviceToDevice, ps.st) == hipSuccess ? CC_OK : CC_ERR_LAUNCH;
}

}  // extern "C"
