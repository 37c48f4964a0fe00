// C ABI (include/clipcap_hip.h) — orchestration of the mapper and GPT-2 training/inference passes out of the HIP
// kernels in gemm.hip.h / kernels.hip / layernorm.hip / reduce.hip / loss.hip / smooth.hip / attention.hip.  No state, no allocation, no synchronisation: everything is enqueued on the
// caller's stream and lives in caller-owned arenas / workspaces.
#include "../../include/clipcap_hip.h"
#include "gemm_api.h"
#include "kernels.h"
#include "shared.h"
#include "layout.h"
#include <vector>

using namespace CC_NS;

namespace {

#define CC_TIMED(site, st, expr)                 \
    do {                                         \
        cc_shared::ProfScope _ps(site, st);      \
        int _e = (expr);                         \
        if (_e != CC_OK) return _e;              \
    } while (0)

// tuning knob (environment, read once): force a GEMM tile kernel at ONE call-site class for A/B measurements —
// CC_TILE_FC = c_fc forward (gelu epilogue, two outputs), CC_TILE_DACT = its activation-gradient dgrad, CC_TILE_PROJ / CC_TILE_PROJ2 = the
// two residual-epilogue c_proj forwards.  Unset = the chooser.
struct TileScope {
    int old;
    bool on;
    explicit TileScope(int mode) : old(cc_shared::g_gemm_tile_mode), on(mode != -2) { if (on) cc_shared::g_gemm_tile_mode = mode; }
    ~TileScope() { if (on) cc_shared::g_gemm_tile_mode = old; }
};
inline int env_tile(const char* name) {
    const char* e = cc_lab_env(name);
    return e ? atoi(e) : -2;
}

// the Call of an entry point: its stream and the scratch of its carved workspace (MapperWS / Gpt2WS)
template <class WS>
inline Call call_of(hipStream_t st, const WS& w) { return Call{st, w.red, w.x3, w.x3_bytes}; }

// ------------------------------------------------------------------------------------------------------------
// mapper
// ------------------------------------------------------------------------------------------------------------
constexpr int kDeferRows = 40960;      // cc_mapper_bwd_range defers the weight gradients of a call up to this many rows (and 8 layers)
struct MapperWS {
    act_t* emb16;
    float* lin_tmp;
    float* x[MAX_LAYERS + 1];
    float* x1[MAX_LAYERS];
    act_t *xn1[MAX_LAYERS], *xn2[MAX_LAYERS], *qkv[MAX_LAYERS], *att[MAX_LAYERS], *h[MAX_LAYERS];
    float *lse[MAX_LAYERS], *mean1[MAX_LAYERS], *rstd1[MAX_LAYERS], *mean2[MAX_LAYERS], *rstd2[MAX_LAYERS];
    // backward scratch
    float* dx32;
    act_t *dx16, *dx16b, *dh16, *dxn16, *datt16, *dqkv16, *dlin16;
    // per-layer copies of the four output gradients that are weight-gradient operands (round 5): with them every layer's weight gradients can
    // wait for ONE grouped launch at the end of the backward call (gdx[l] = d x[l+1], the gradient entering layer l from above).  The bf16x3
    // build splits operands per call and keeps the single buffers: there every entry aliases them.
    act_t *gdx[MAX_LAYERS], *gdxb[MAX_LAYERS], *gdh[MAX_LAYERS], *gdqkv[MAX_LAYERS];
    bool own_grads;     // every layer has its own copies (else they alias the single dx16 / dx16b / dh16 / dqkv16 buffers and weight gradients flush per layer)
    float* wg_scratch;
    float* red;         // partial sums of the cross-block reductions (kernels.h)
    float* adelta;
    uint16_t* gimg;    // bf16x3 build: the [hi | hi | lo] image of the output gradient both GEMMs of a layer step read
    char* x3;          // bf16x3 build: operand-image scratch of the GEMM in flight (gemm_api.h)
    size_t x3_bytes;
    size_t bytes;
};

void mapper_carve(const cc_mapper_cfg* c, int B, int save, void* ws, MapperWS& w) {
    Carver cv(ws);
    const int S = c->W * c->P + c->L;
    const size_t M = (size_t)B * S, D = c->D;
    w.emb16 = cv.take<act_t>((size_t)B * c->W * c->E);
    w.lin_tmp = c->W > 1 ? cv.take<float>((size_t)B * c->W * c->P * D) : nullptr;
    const int nx = save ? c->N + 1 : 2;
    float* xb[MAX_LAYERS + 1];
    for (int i = 0; i < nx; i++) xb[i] = cv.take<float>(M * D);
    for (int l = 0; l <= c->N; l++) w.x[l] = save ? xb[l] : xb[l & 1];
    const int nl = save ? c->N : 1;
    for (int l = 0; l < c->N; l++) {
        const bool fresh = l < nl;      // (a pass that saves nothing reuses layer 0's buffers)
        w.x1[l] = fresh ? cv.take<float>(M * D) : w.x1[0];
        w.xn1[l] = fresh ? cv.take<act_t>(M * D) : w.xn1[0];
        w.xn2[l] = fresh ? cv.take<act_t>(M * D) : w.xn2[0];
        w.qkv[l] = fresh ? cv.take<act_t>(M * 3 * D) : w.qkv[0];
        w.att[l] = fresh ? cv.take<act_t>(M * D) : w.att[0];
        w.h[l] = fresh ? cv.take<act_t>(M * c->Hm) : w.h[0];
        w.lse[l] = fresh ? cv.take<float>((size_t)B * c->H * S) : w.lse[0];
        w.mean1[l] = fresh ? cv.take<float>(M) : w.mean1[0];
        w.rstd1[l] = fresh ? cv.take<float>(M) : w.rstd1[0];
        w.mean2[l] = fresh ? cv.take<float>(M) : w.mean2[0];
        w.rstd2[l] = fresh ? cv.take<float>(M) : w.rstd2[0];
    }
    if (save) {
        w.dx32 = cv.take<float>(M * D);
        w.dx16 = cv.take<act_t>(M * D);
        w.dx16b = cv.take<act_t>(M * D);        // gradient after the LN2 backward: a second buffer so that the layer's four weight
                                                // gradients can run as one grouped launch once all their operands exist
        w.dh16 = cv.take<act_t>(M * c->Hm);
        w.dxn16 = cv.take<act_t>(M * D);
        w.datt16 = cv.take<act_t>(M * D);
        w.dqkv16 = cv.take<act_t>(M * 3 * D);
        w.dlin16 = cv.take<act_t>((size_t)B * c->W * c->P * D);
        // per-layer copies only where cc_mapper_bwd_range can defer (<= kDeferRows rows and <= 8 layers): a B = 4096 call would otherwise
        // carry (N - 1) x M x (5 D + Hm) unused 16-bit elements (~6 GB at D = 768, N = 8) — ADVICE r5
        w.own_grads = !kX3 && M <= (size_t)kDeferRows && c->N <= 8;
        for (int l = 0; l < c->N; l++) {
            const bool own = w.own_grads;                // every layer its own (a deferred weight gradient reads them at the END of the call)
            w.gdx[l] = own ? cv.take<act_t>(M * D) : w.dx16;
            w.gdxb[l] = own ? cv.take<act_t>(M * D) : w.dx16b;
            w.gdh[l] = own ? cv.take<act_t>(M * c->Hm) : w.dh16;
            w.gdqkv[l] = own ? cv.take<act_t>(M * 3 * D) : w.dqkv16;
        }
        w.wg_scratch = cv.take<float>(WGRAD_SCRATCH_BYTES / sizeof(float));
        w.red = cv.take<float>(RED_SCRATCH_FLOATS);
        w.adelta = cv.take<float>((size_t)B * c->H * S);
        // bf16x3: an output gradient is the operand of TWO GEMMs in the same image form (its layer's weight gradient and input gradient):
        // split once into this buffer, read twice (the widest is d qkv)
        w.gimg = kX3 ? reinterpret_cast<uint16_t*>(cv.take<char>(x3_img(M, std::max<size_t>(3 * (size_t)D, c->Hm)))) : nullptr;
    } else {
        w.dx32 = nullptr; w.dx16 = w.dx16b = w.dh16 = w.dxn16 = w.datt16 = w.dqkv16 = w.dlin16 = nullptr; w.wg_scratch = nullptr; w.adelta = nullptr;
        w.red = nullptr;
        w.gimg = nullptr;
        for (int l = 0; l < c->N; l++) w.gdx[l] = w.gdxb[l] = w.gdh[l] = w.gdqkv[l] = nullptr;
        w.own_grads = false;
    }
    w.x3 = nullptr; w.x3_bytes = 0;
    if (kX3) {
        const size_t Hm = c->Hm, Mb = (size_t)B * c->W, PD = (size_t)c->P * D;
        size_t need = std::max(x3_img(Mb, c->E), x3_img(M, std::max(D, Hm)));                          // forward A images
        if (save) {
            need = std::max(need, x3_img(M, 3 * D));                                                     // dgrad through the fused QKV weight
            need = std::max(need, std::max(x3_img(M, D) + x3_img(M, Hm), x3_img(M, 3 * D) + x3_img(M, D)));   // weight-gradient pairs
            need = std::max(need, x3_img(Mb, PD) + x3_img(Mb, c->E));
        }
        w.x3_bytes = need;
        w.x3 = cv.take<char>(need);
    }
    w.bytes = cv.bytes();
}

// What every mapper pass starts from, built from the entry point's (already validated) arguments: the stream, the arena offsets, the carved
// workspace, the Call and the derived dims.  A plain record on the entry point's stack: no state beyond the call, no allocation, no HIP call.
struct MapperPass {
    hipStream_t st;
    MapperOff o;
    MapperWS w;
    Call cx;
    int D, PP, S, M, H, hd, Hm, PD;      // PP = W*P projected prefix rows, S = rows per sample, M = B*S rows, PD = P*D
    MapperPass(const cc_mapper_cfg* c, int B, int save, void* ws, void* stream)
        : st(S_(stream)), o(c), D(c->D), PP(c->W * c->P), S(PP + c->L), M(B * S), H(c->H), hd(c->D / c->H), Hm(c->Hm), PD(c->P * c->D) {
        mapper_carve(c, B, save, ws, w);
        cx = call_of(st, w);
    }
};

// ------------------------------------------------------------------------------------------------------------
// GPT-2
// ------------------------------------------------------------------------------------------------------------
// bf16x3, frozen LM: c_fc's forward epilogue and the gelu' input-gradient epilogue write the [hi | hi | lo] operand image of their consumer
// GEMM directly instead of an fp32 activation that a split pass re-reads (CC_X3_IMG=0: A/B switch)
static bool x3_img_on() {
    static const bool on = []() { const char* e = cc_lab_env("CC_X3_IMG"); return !e || atoi(e) != 0; }();
    return on;
}
// Exponential form of the lm_head outputs (gemm.hip.h EpiLMHead): the bf16 build's training path stores exp(logit - target logit) and
// never materialises the softmax gradient.  fp16 lacks the exponent range, the bf16x3 build keeps fp32 logits.  CC_LM_EXPFORM=0: A/B switch.
// bf16x3: the exponential form for frozen-LM runs (round 4) — E leaves the GEMM as the [hi | hi | lo] operand image of the input-gradient
// GEMM (in the logits buffer, 1.5x), so neither fp32 logits nor the softmax-gradient pass over them exist; the full finetune keeps the
// logit form (its tied weight gradient reads the fp32 gradient).
static bool lm_exp_form(const cc_gpt2_shape* s) {
    static const bool env = []() { const char* e = cc_lab_env("CC_LM_EXPFORM"); return !e || atoi(e) != 0; }();
    if (CC_OP == 0) return env;
    if (CC_OP == 2) return env && x3_img_on() && s->mode == 1;
    return false;
}
// The logits buffer as cc_lmhead_ce_fwd fills it and cc_lmhead_ce_bwd reads it: in the bf16x3 exponential form E leaves the lm_head GEMM
// as the operand image of the input-gradient GEMM.  cc_gpt2_logits_bwd fills the same buffer with plain values and passes the pointer.
static Act lm_logits(const cc_gpt2_cfg* c, const cc_gpt2_shape* s, act_t* logits16) { return Act(logits16, (kX3 && lm_exp_form(s)) ? c->Vp : 0); }

struct Gpt2WS {
    float* x[MAX_LAYERS + 1];
    float* x1[MAX_LAYERS];
    act_t *qkv[MAX_LAYERS], *u[MAX_LAYERS];
    // Act: buffers that hold, in the bf16x3 build, either fp32 activations or the operand image of the one GEMM that reads them; gpt2_carve
    // decides which, and the handle says it to the buffer's producer and to its consumer alike
    Act xn1[MAX_LAYERS], xn2[MAX_LAYERS], att[MAX_LAYERS], hact[MAX_LAYERS];
    float *lse[MAX_LAYERS], *mean1[MAX_LAYERS], *rstd1[MAX_LAYERS], *mean2[MAX_LAYERS], *rstd2[MAX_LAYERS];
    // lm head / loss
    act_t* hf16;       // [Mh, D]   ln_f output rows (Mh = max(B*cap, B*T) so the parity API can use it too)
    float *meanf, *rstdf;
    int *target, *row_map;
    int* keep;         // [B*cap]  scoring pass (mode 0 with caption rows) only: rows whose log-prob counts
    act_t* logits16;   // [B*cap, Vp]  (what it holds depends on who filled it: lm_logits)
    float *pmax, *psum, *tgt_logit, *lse_row, *row_loss;
    float *cref, *lmfac;   // exponential form of the lm_head outputs (bf16 build): reference shift [Mc], row factors {r, w} [Mc][2]
    act_t* hfs16;          // full finetune: r * hf rows, the weight-gradient operand of the exponential form
    // backward
    float* dx32;
    Act dx16, dx16b, du16, dqkv16;
    act_t *dhf16, *dxn16, *datt16;
    float* wg_scratch;
    float* red;        // partial sums of the cross-block reductions (kernels.h)
    void* scat;        // full finetune: scratch of the token-indexed scatters into d wte (kernels.h scatter_rows), for the B*cap caption rows
    float* adelta;
    char* x3;          // bf16x3 build: operand-image scratch
    size_t x3_bytes;
    size_t bytes;
};

// cap: caption rows per sample the loss-side buffers are sized for (s->T - s->L; cc_gpt2_logits_bwd: all s->T)
void gpt2_carve(const cc_gpt2_cfg* c, const cc_gpt2_shape* s, int cap, void* ws, Gpt2WS& w) {
    Carver cv(ws);
    const int B = s->B, T = s->T, hd = c->D / c->H;
    const size_t M = (size_t)B * T, D = c->D, Mc = (size_t)B * cap;
    const bool keep = s->mode >= 1, full = s->mode >= 2;
    // a 16-bit buffer of n elements that may hold a 1.5x operand image instead (bf16x3, frozen LM: 6 B per element)
    const auto take_img = [&](size_t n) { return cv.take<act_t>(n * ((kX3 && !full) ? 3 : 2) / 2); };
    // bf16x3: which buffers are operand images (width of the operand, 0 = fp32 activations).  Frozen LM: no weight gradient reads the
    // normalised rows, the attention output, the MLP hidden or d u, so LayerNorm, attention and the c_fc / gelu' epilogues write what
    // the next GEMM reads; without dropout that also holds for the 16-bit copies of the residual gradient and for d qkv.  Attention
    // writes images only for the shapes its fp32-VALU pair serves (the backward then recomputes what it needs from qkv).
    const bool img = kX3 && !full && x3_img_on();
    const bool bimg = img && keep && s->p_resid == 0.f && s->p_attn == 0.f && s->p_embd == 0.f;
    const int xw = img ? (int)D : 0, attw = (img && attn_fwd_can_image(T, hd)) ? (int)D : 0, hw = img ? 4 * (int)D : 0;
    const int dxw = bimg ? (int)D : 0, dqw = (bimg && attn_bwd_can_image(T, hd)) ? 3 * (int)D : 0;
    const int nx = keep ? c->NL + 1 : 2;
    float* xb[MAX_LAYERS + 1];
    for (int i = 0; i < nx; i++) xb[i] = cv.take<float>(M * D);
    for (int l = 0; l <= c->NL; l++) w.x[l] = keep ? xb[l] : xb[l & 1];
    for (int l = 0; l < c->NL; l++) {
        const bool k0 = keep || l == 0, f0 = full || l == 0;
        w.x1[l] = k0 ? cv.take<float>(M * D) : w.x1[0];
        w.qkv[l] = k0 ? cv.take<act_t>(M * 3 * D) : w.qkv[0];
        w.u[l] = k0 ? cv.take<act_t>(M * 4 * D) : w.u[0];
        w.lse[l] = k0 ? cv.take<float>((size_t)B * c->H * T) : w.lse[0];
        w.mean1[l] = k0 ? cv.take<float>(M) : w.mean1[0];
        w.rstd1[l] = k0 ? cv.take<float>(M) : w.rstd1[0];
        w.mean2[l] = k0 ? cv.take<float>(M) : w.mean2[0];
        w.rstd2[l] = k0 ? cv.take<float>(M) : w.rstd2[0];
        w.xn1[l] = f0 ? Act(take_img(M * D), xw) : w.xn1[0];       // bf16x3, frozen LM: LayerNorm writes c_attn's / c_fc's operand image
        w.xn2[l] = f0 ? Act(take_img(M * D), xw) : w.xn2[0];
        w.att[l] = k0 ? Act(take_img(M * D), attw) : w.att[0];    // attention output: needed by the backward's delta = rowsum(dO*O) (bf16x3, frozen LM: attn.c_proj's operand image)
        w.hact[l] = f0 ? Act(take_img(M * 4 * D), hw) : w.hact[0];    // bf16x3, frozen LM: holds mlp.c_proj's operand IMAGE (6 B / element), written by c_fc's epilogue
    }
    const size_t Mh = std::max(M, Mc);
    w.hf16 = cv.take<act_t>(Mh * D);
    w.meanf = cv.take<float>(Mh);
    w.rstdf = cv.take<float>(Mh);
    w.target = cv.take<int>(Mh);
    w.row_map = cv.take<int>(Mh);
    w.keep = nullptr;
    if (keep) {
        const int npart = c->Vp / 64;
        w.logits16 = take_img(Mc * c->Vp);               // bf16x3, frozen LM: room for E as an operand image (lm_logits)
        w.pmax = cv.take<float>(Mc * npart);
        w.psum = cv.take<float>(Mc * npart);
        w.tgt_logit = cv.take<float>(Mc);
        w.lse_row = cv.take<float>(Mc);
        w.row_loss = cv.take<float>(Mc);
        w.cref = cv.take<float>(Mc);
        w.lmfac = cv.take<float>(2 * Mc);
        w.hfs16 = full ? cv.take<act_t>(Mc * D) : nullptr;
        w.dx32 = cv.take<float>(M * D);
        w.dx16 = Act(take_img(M * D), dxw);                  // bf16x3, frozen LM: operand images written by their producers (LayerNorm backward, attention backward)
        w.dx16b = full ? Act(cv.take<act_t>(M * D)) : w.dx16;    // full finetune: second copy so a layer's weight gradients can run grouped
        w.dhf16 = cv.take<act_t>(Mc * D);
        w.du16 = Act(take_img(M * 4 * D), hw);              // likewise: c_fc's input-gradient operand image, written by the gelu' epilogue
        w.dxn16 = cv.take<act_t>(M * D);
        w.datt16 = cv.take<act_t>(M * D);
        w.dqkv16 = Act(take_img(M * 3 * D), dqw);
        w.wg_scratch = full ? cv.take<float>(WGRAD_SCRATCH_BYTES / sizeof(float)) : nullptr;
        w.red = full ? cv.take<float>(RED_SCRATCH_FLOATS) : nullptr;      // only a full finetune reduces parameter gradients across blocks
        w.scat = full ? cv.take<char>(scatter_ws_bytes((int)Mc, (int)D)) : nullptr;
        w.adelta = cv.take<float>((size_t)B * c->H * T);
    } else {
        w.wg_scratch = nullptr; w.adelta = nullptr; w.red = nullptr; w.scat = nullptr;
        w.logits16 = nullptr; w.pmax = w.psum = w.tgt_logit = w.lse_row = w.row_loss = nullptr;
        w.cref = w.lmfac = nullptr; w.hfs16 = nullptr;
        w.dx32 = nullptr; w.dx16 = w.dx16b = w.du16 = w.dqkv16 = Act(); w.dhf16 = w.dxn16 = w.datt16 = nullptr;
        if (Mc > 0) {      // forward-only pass with caption rows (cc_lmhead_score): the per-row buffers of the loss side, and no logits matrix
            const int npart = c->Vp / 64;
            w.pmax = cv.take<float>(Mc * npart);
            w.psum = cv.take<float>(Mc * npart);
            w.tgt_logit = cv.take<float>(Mc);
            w.lse_row = cv.take<float>(Mc);
            w.keep = cv.take<int>(Mc);
        }
    }
    w.x3 = nullptr; w.x3_bytes = 0;
    if (kX3) {
        size_t need = x3_img(Mh, 4 * D);                                                       // forward A images (mlp.c_proj is the deepest)
        if (keep) need = std::max(need, x3_img(Mc, c->Vp));                                    // lm_head input gradient: A = dlogits
        if (full) need = std::max(need, std::max(x3_img(M, D) + x3_img(M, 4 * D), x3_img(Mc, c->Vp) + x3_img(Mc, D)));   // weight-gradient pairs
        w.x3_bytes = need;
        w.x3 = cv.take<char>(need);
    }
    w.bytes = cv.bytes();
}

// The GPT-2 counterpart of MapperPass.  cap: caption rows per sample the loss side is carved for (gpt2_carve).  M = B*T rows.
struct Gpt2Pass {
    hipStream_t st;
    Gpt2Off o;
    Gpt2WS w;
    Call cx;
    int D, M, H, hd;
    Gpt2Pass(const cc_gpt2_cfg* c, const cc_gpt2_shape* s, int cap, void* ws, void* stream)
        : st(S_(stream)), o(c), D(c->D), M(s->B * s->T), H(c->H), hd(c->D / c->H) {
        gpt2_carve(c, s, cap, ws, w);
        cx = call_of(st, w);
    }
};

}  // namespace

extern "C" {

int CC_API(cc_mapper_bwd_range)(const cc_mapper_cfg* c, int32_t B, const float* w32, const uint16_t* w16, void* ws, const float* dout, float* g32,
                        int32_t l_hi, int32_t l_lo, void* stream);
int CC_API(cc_gpt2_bwd_range)(const cc_gpt2_cfg* c, const cc_gpt2_shape* s, const float* w32, const uint16_t* w16, void* ws, const int64_t* tokens,
                      float* dprefix, float* g32, int32_t l_hi, int32_t l_lo, void* stream);

// ---------------------------------------------------------------- mapper ----------------------------------------
int64_t CC_API(cc_mapper_param_count)(const cc_mapper_cfg* cfg) {
    if (!mapper_cfg_ok(cfg)) return CC_ERR_SHAPE;
    return MapperOff(cfg).total;
}

int CC_API(cc_mapper_param_offsets)(const cc_mapper_cfg* cfg, int64_t* offs) {
    if (!mapper_cfg_ok(cfg) || !offs) return CC_ERR_SHAPE;
    const MapperOff o(cfg);
    *offs++ = o.lin_w; *offs++ = o.lin_b; *offs++ = o.prefix; *offs++ = o.pos;
    for (int l = 0; l < cfg->N; l++) offs = put_layer(offs, o.layer(l));
    return CC_OK;
}

int64_t CC_API(cc_mapper_ws_bytes)(const cc_mapper_cfg* cfg, int32_t B, int32_t save) {
    if (!mapper_cfg_ok(cfg) || B <= 0) return CC_ERR_SHAPE;
    MapperWS w;
    mapper_carve(cfg, B, save, nullptr, w);
    return (int64_t)w.bytes;
}

#if CC_OP == 2
// bf16x3: [hi | lo | hi] images of every GEMM weight and of its transpose, straight from the fp32 master (W16 layout above)
static int mapper_sync_x3(const cc_mapper_cfg* c, const float* w32, uint16_t* w16, hipStream_t st) {
    const MapperOff o(c);
    const int D = c->D, Hm = c->Hm;
    X3SplitBatch sb;
    sb.add(w32 + o.lin_w, W16(w16, o.lin_w), c->P * D, c->E, 0, 1);
    for (int l = 0; l < c->N; l++) {
        const auto y = o.layer(l);
        const int64_t off[4] = {y.wq, y.wp, y.w1, y.w2};
        const int R[4] = {3 * D, D, Hm, D}, C[4] = {D, D, D, Hm};
        for (int i = 0; i < 4; i++) {
            if (sb.n + 2 > 32) { CC_TRY(x3_split_multi(sb, st)); sb.n = 0; }
            sb.add(w32 + off[i], W16(w16, off[i]), R[i], C[i], 0, 1);
            sb.add(w32 + off[i], W16(w16, o.total + off[i]), R[i], C[i], 1, 1);
        }
    }
    return x3_split_multi(sb, st);
}
#endif

static int mapper_transposes(const cc_mapper_cfg* c, uint16_t* w16, hipStream_t st) {
    if (kX3) return CC_ERR_ARG;      // the operand images are made from the fp32 master (cc_mapper_sync_weights)
    const MapperOff o(c);
    op16_t* t = w16 + o.total;
    const int D = c->D, Hm = c->Hm;
    TransposeBatch tb;                      // 8 layers x 4 matrices: one launch per 32 matrices instead of one each
    for (int l = 0; l < c->N; l++) {
        const auto y = o.layer(l);
        tb.add(w16 + y.wq, t + y.wq, 3 * D, D);   // fused [3D, D] -> [D, 3D]
        tb.add(w16 + y.wp, t + y.wp, D, D);
        tb.add(w16 + y.w1, t + y.w1, Hm, D);       // [Hm, D] -> [D, Hm]
        tb.add(w16 + y.w2, t + y.w2, D, Hm);       // [D, Hm] -> [Hm, D]
        if (tb.n == 32) { CC_TRY(transpose_bf16_multi(tb, st)); tb.n = 0; }
    }
    CC_TRY(transpose_bf16_multi(tb, st));
    return CC_OK;
}

int CC_API(cc_mapper_sync_weights)(const cc_mapper_cfg* c, const float* w32, uint16_t* w16, void* stream) {
    if (!mapper_cfg_ok(c) || !w32 || !w16) return CC_ERR_ARG;
    hipStream_t st = S_(stream);
#if CC_OP == 2
    return mapper_sync_x3(c, w32, w16, st);
#else
    CC_TRY(f32_to_bf16(w32, w16, (size_t)MapperOff(c).total, st));
    return mapper_transposes(c, w16, st);
#endif
}

int CC_API(cc_mapper_transpose_weights)(const cc_mapper_cfg* c, uint16_t* w16, void* stream) {
    if (!mapper_cfg_ok(c) || !w16) return CC_ERR_ARG;
    return mapper_transposes(c, w16, S_(stream));
}

int CC_API(cc_mapper_fwd)(const cc_mapper_cfg* c, int32_t B, const float* w32, const uint16_t* w16, const float* emb, void* ws, float* out,
                  int32_t save, void* stream) {
    if (!mapper_cfg_ok(c) || B <= 0 || !w32 || !w16 || !emb || !ws || !out) return CC_ERR_ARG;
    MapperPass ps(c, B, save, ws, stream);
    auto& [st, o, w, cx, D, PP, S, M, H, hd, Hm, PD] = ps;
    // linear (mapper.py:123): [B*W, E] x [P*D, E]^T + b -> rows 0..PP-1 of every sample of x[0]
    CC_TRY(f32_to_act(emb, w.emb16, (size_t)B * c->W * c->E, st));
    if (c->W == 1) {
        CC_TRY(gemm_f32out(0, 0, w.emb16, c->E, W16(w16, o.lin_w), c->E, B, PD, c->E, w.x[0], S * D, w32 + o.lin_b, 0, 1.0f, 1, cx));
    } else {
        CC_TRY(gemm_f32out(0, 0, w.emb16, c->E, W16(w16, o.lin_w), c->E, B * c->W, PD, c->E, w.lin_tmp, PD, w32 + o.lin_b, 0, 1.0f, 1, cx));
        CC_TRY(copy_rows(w.lin_tmp, (size_t)PP * D, w.x[0], (size_t)S * D, PP * D, B, st));
        if (o.pos >= 0) CC_TRY(add_rows(w.x[0], (size_t)S * D, w32 + o.pos, PP * D, B, st));
    }
    // cat learned prefix_const (mapper.py:125-126)
    CC_TRY(broadcast_rows(w.x[0] + (size_t)PP * D, (size_t)S * D, w32 + o.prefix, c->L * D, B, st));
    for (int l = 0; l < c->N; l++) {
        const auto y = o.layer(l);
        // x1 = x + project(attn(LN1 x))  (mapper.py:108, attention.py:17-43)
        CC_TRY(ln_fwd(w.x[l], D, nullptr, w32 + y.n1w, w32 + y.n1b, w.xn1[l], nullptr, w.mean1[l], w.rstd1[l], M, D, st));
        CC_TIMED(CC_SITE_MAPPER_QKV_FWD, st, gemm_bf16out(0, 0, w.xn1[l], D, W16(w16, y.wq), D, M, 3 * D, D, w.qkv[l], 3 * D, nullptr, 0, nullptr, cx));
        CC_TRY(attn_fwd(w.qkv[l], B, S, H, hd, false, w.att[l], w.lse[l], st));
        CC_TRY(gemm_resid(0, 0, w.att[l], D, W16(w16, y.wp), D, M, D, D, w.x1[l], w.x[l], D, w32 + y.bp, cx));
        // x = x1 + fc2(relu(fc1(LN2 x1)))  (mapper.py:109, :82-88)
        CC_TRY(ln_fwd(w.x1[l], D, nullptr, w32 + y.n2w, w32 + y.n2b, w.xn2[l], nullptr, w.mean2[l], w.rstd2[l], M, D, st));
        CC_TIMED(CC_SITE_MAPPER_FC1_FWD, st, gemm_bf16out(0, 0, w.xn2[l], D, W16(w16, y.w1), D, M, Hm, D, w.h[l], Hm, w32 + y.b1, 1, nullptr, cx));
        CC_TRY(gemm_resid(0, 0, w.h[l], Hm, W16(w16, y.w2), Hm, M, D, Hm, w.x[l + 1], w.x1[l], D, w32 + y.b2, cx));
    }
    // out = rows [PP:] (mapper.py:128)
    CC_TRY(copy_rows(w.x[c->N] + (size_t)PP * D, (size_t)S * D, out, (size_t)c->L * D, c->L * D, B, st));
    return CC_OK;
}

int CC_API(cc_mapper_attention_probs)(const cc_mapper_cfg* c, int32_t B, void* ws, int32_t layer, float* out, void* stream) {
    if (!mapper_cfg_ok(c) || B <= 0 || !ws || !out || layer < 0 || layer >= c->N) return CC_ERR_ARG;
    MapperPass ps(c, B, 1, ws, stream);
    return attn_probs(ps.w.qkv[layer], B, ps.S, ps.H, ps.hd, out, ps.st);
}

int CC_API(cc_mapper_bwd)(const cc_mapper_cfg* c, int32_t B, const float* w32, const uint16_t* w16, void* ws, const float* dout, float* g32,
                  void* stream) {
    if (!mapper_cfg_ok(c)) return CC_ERR_ARG;
    return CC_API(cc_mapper_bwd_range)(c, B, w32, w16, ws, dout, g32, c->N, 0, stream);
}

int CC_API(cc_mapper_bwd_range)(const cc_mapper_cfg* c, int32_t B, const float* w32, const uint16_t* w16, void* ws, const float* dout, float* g32,
                        int32_t l_hi, int32_t l_lo, void* stream) {
    if (!mapper_cfg_ok(c) || B <= 0 || !w32 || !w16 || !ws || !dout || !g32 || l_lo < 0 || l_hi > c->N || l_lo > l_hi) return CC_ERR_ARG;
    MapperPass ps(c, B, 1, ws, stream);
    auto& [st, o, w, cx, D, PP, S, M, H, hd, Hm, PD] = ps;
    const uint16_t* w16t = W16(w16, o.total);   // transposed weight copies: dgrad GEMMs are NT
    if (l_hi == c->N) {   // seed: d x[N][:, PP:, :] = dout, rows [0:PP] = 0
        if (hipMemsetAsync(w.dx32, 0, (size_t)M * D * sizeof(float), st) != hipSuccess) return CC_ERR_LAUNCH;
        CC_TRY(copy_rows(dout, (size_t)c->L * D, w.dx32 + (size_t)PP * D, (size_t)S * D, c->L * D, B, st));
        if (c->N > 0) CC_TRY(f32_to_act(w.dx32, w.gdx[c->N - 1], (size_t)M * D, st));      // (a mapper without layers has no 16-bit consumer)
    }
    // The weight gradients are off the dependency chain.  bf16 / fp16 builds (round 5): every layer of this call parks its four problems and
    // ONE grouped launch at the end runs them all — whole-K 256 x 256 tiles that add into dW in their epilogue (8 layers: 576 tiles), no K
    // slices, no slabs, no per-layer reduce launch; their operands live in per-layer buffers (MapperWS::gd*).  A caller that wants the
    // gradients of a layer range early (the DDP reducer's 2-layer slices) gets them at the end of ITS call: the flush is per call.
    // bf16x3 build: per layer, as before (operand images are split per GEMM call).
    WgradBatch wb;
    wb.defer = true;
    constexpr bool kDeferAll = !kX3;
    static const bool defer_all_on = []() { const char* e = cc_lab_env("CC_MAPPER_WGRAD_DEFER"); return !e || atoi(e) != 0; }();     // lab build: A/B switch
    // Whole-K tiles fill the CUs worse than the per-layer launches' K slices (8 layers: 576 tiles = 2.25 rounds); the launch therefore cuts the
    // tiles beyond its last full round into K slices (TTGroup::whole / split: 2 rounds + 64 tiles x 4 slices, slabs + a small reduce).  What the
    // deferred launch saves does not grow with the row count, what is left of the fill loss does: ahead at B = 256 (M = 5120: 2.63 -> 2.50 ms)
    // and B = 1024 (7.64 -> 7.43), behind at B = 4096 (28.04 -> 28.35) — calls above 40 960 rows keep the per-layer form.
    static const int defer_rows = []() { const char* e = cc_lab_env("CC_MAPPER_DEFER_ROWS"); return e ? std::min(atoi(e), kDeferRows) : kDeferRows; }();      // lab build: a lower row limit
    const bool defer_all = kDeferAll && defer_all_on && w.own_grads && 4 * (l_hi - l_lo) <= 32 && M <= defer_rows;
    if (defer_all) { wb.direct = true; wb.cap = 4 * (l_hi - l_lo); }
    ColsumBatch cs;
    // bf16x3: `G2(t, width)` = the tensor as both of its GEMMs take it — split ONCE into w.gimg ([hi | hi | lo], the form of the weight
    // gradient's first operand and of the input gradient's A operand alike)
#if CC_OP == 2
    static const bool share = []() { const char* e = cc_lab_env("CC_X3_SHARE"); return !e || atoi(e) != 0; }();
    int g2rc = CC_OK;
    auto G2 = [&](const act_t* t, int width) -> ActIn {
        if (!share) return t;
        auto& [st, o, w, cx, D, PP, S, M, H, hd, Hm, PD] = ps;      // (C++17 lambdas capture the pass, not its bindings)
        g2rc = x3_split_rows(t, (size_t)width, w.gimg, M, width, 0, st);
        return ActIn(reinterpret_cast<const act_t*>(w.gimg), width);
    };
#else
    auto G2 = [&](const act_t* t, int) -> ActIn { return t; };
    const int g2rc = CC_OK;
#endif
    for (int l = l_hi - 1; l >= l_lo; l--) {
        const auto y = o.layer(l);
        act_t* dx16 = w.gdx[l];                                   // d x[l+1]: written by the seed / by the LN1 backward of layer l + 1
        act_t* dx16b = w.gdxb[l];
        act_t* dh16 = w.gdh[l];
        act_t* dqkv16 = w.gdqkv[l];
        // d x[l] in 16 bits: the gradient entering layer l - 1.  Below layer 0 nobody reads it (the linear's gradient comes from dx32), and it
        // must NOT land in a buffer a deferred weight gradient still has to read: it goes to the attention-gradient scratch, dead by then
        act_t* dx16_below = l > 0 ? w.gdx[l - 1] : w.datt16;
        // fc2: y = h W2^T + b2
        const ActIn gx = G2(dx16, D);
        CC_TRY(g2rc);
        CC_TIMED(CC_SITE_MAPPER_WGRAD_FC2, st, gemm_wgrad(gx, D, w.h[l], Hm, D, Hm, M, g32 + y.w2, Hm, w.wg_scratch, cx, &wb));
        // fc2.bias gradient = column sums of dx16: for every layer but the top one the LN1 backward of the layer above produced
        // them together with dx16 (ln_bwd dcol); the top layer's dx16 comes from the seed
        if (l == c->N - 1) CC_TRY(colsum_bf16(dx16, D, M, D, g32 + y.b2, cx));
        CC_TRY(gemm_dact(0, 0, gx, D, W16(w16t, y.w2), D, M, Hm, D, dh16, Hm, w.h[l], 1, cx));          // W2^T [Hm, D]
        // fc1
        const ActIn gh = G2(dh16, Hm);
        CC_TRY(g2rc);
        CC_TRY(gemm_wgrad(gh, Hm, w.xn2[l], D, Hm, D, M, g32 + y.w1, D, w.wg_scratch, cx, &wb));
        if (defer_all) cs.add(dh16, g32 + y.b1);                  // fc1.bias gradient: with the deferred weight gradients, one launch for all layers
        else CC_TRY(colsum_bf16(dh16, Hm, M, Hm, g32 + y.b1, cx));
        CC_TRY(gemm_bf16out(0, 0, gh, Hm, W16(w16t, y.w1), Hm, M, D, Hm, w.dxn16, D, nullptr, 0, nullptr, cx));   // W1^T [D, Hm]
        CC_TRY(ln_bwd(w.dxn16, w.x1[l], D, nullptr, w.mean2[l], w.rstd2[l], w32 + y.n2w, w.dx32, w.dx32, dx16b, g32 + y.n2w,
                      g32 + y.n2b, M, D, cx, g32 + y.bp));         // + project.bias gradient (column sums of dx16b)
        // project
        const ActIn gb = G2(dx16b, D);
        CC_TRY(g2rc);
        CC_TRY(gemm_wgrad(gb, D, w.att[l], D, D, D, M, g32 + y.wp, D, w.wg_scratch, cx, &wb));
        CC_TRY(gemm_bf16out(0, 0, gb, D, W16(w16t, y.wp), D, M, D, D, w.datt16, D, nullptr, 0, nullptr, cx));     // Wp^T
        CC_TRY(attn_bwd(w.qkv[l], w.datt16, w.att[l], w.lse[l], w.adelta, B, S, H, hd, false, dqkv16, st));
        // fused q/kv projection (to_queries.weight ++ to_keys_values.weight = [3D, D])
        const ActIn gq = G2(dqkv16, 3 * D);
        CC_TRY(g2rc);
        CC_TRY(gemm_wgrad(gq, 3 * D, w.xn1[l], D, 3 * D, D, M, g32 + y.wq, D, w.wg_scratch, cx, &wb));
        CC_TRY(gemm_bf16out(0, 0, gq, 3 * D, W16(w16t, y.wq), 3 * D, M, D, 3 * D, w.dxn16, D, nullptr, 0, nullptr, cx));  // Wqkv^T [D, 3D]
        // per-layer form: the deferred weight gradients read dx16, dh16, dx16b, dqkv16 — run them before the LN1 backward overwrites dx16
        // with the next layer's input gradient (with per-layer buffers nothing is overwritten and the flush waits for the end of the call)
        if (!defer_all) CC_TRY(wgrad_flush(wb, st));
        CC_TRY(ln_bwd(w.dxn16, w.x[l], D, nullptr, w.mean1[l], w.rstd1[l], w32 + y.n1w, w.dx32, w.dx32, dx16_below, g32 + y.n1w,
                      g32 + y.n1b, M, D, cx, l > 0 ? g32 + o.layer(l - 1).b2 : nullptr));   // + fc2.bias gradient of the layer below
    }
    CC_TRY(wgrad_flush(wb, st));
    CC_TRY(colsum_bf16_multi(cs, Hm, M, Hm, cx));
    if (l_lo > 0) return CC_OK;
    // prefix_const, pos_embeddings, linear
    CC_TRY(batch_sum(w.dx32 + (size_t)PP * D, (size_t)S * D, g32 + o.prefix, c->L * D, B, cx));
    if (o.pos >= 0) CC_TRY(batch_sum(w.dx32, (size_t)S * D, g32 + o.pos, PP * D, B, cx));
    CC_TRY(slice_f32_to_bf16(w.dx32, (size_t)S * D, w.dlin16, (size_t)PP * D, PP * D, B, st));
    CC_TRY(gemm_wgrad(w.dlin16, PD, w.emb16, c->E, PD, c->E, B * c->W, g32 + o.lin_w, c->E, w.wg_scratch, cx));
    CC_TRY(colsum_bf16(w.dlin16, PD, B * c->W, PD, g32 + o.lin_b, cx));
    return CC_OK;
}

// ---------------------------------------------------------------- GPT-2 -----------------------------------------
namespace {
// c_fc forward stores gelu_new'(u) where it used to store u (CC_GELU_GRAD_FWD=0: A/B switch; forward and backward read the same setting)
static bool gelu_grad_fwd() {
    static const bool on = []() { const char* e = cc_lab_env("CC_GELU_GRAD_FWD"); return !e || atoi(e) != 0; }();
    return on;
}
static bool shape_ok(const cc_gpt2_cfg* c, const cc_gpt2_shape* s) {
    return s && s->B > 0 && s->T > 0 && s->L >= 0 && s->L <= s->T && s->cap >= s->T - s->L && s->mode >= 0 && s->mode <= 2 && s->T <= c->NPOS &&
           s->p_embd >= 0.f && s->p_embd < 1.f && s->p_attn >= 0.f && s->p_attn < 1.f && s->p_resid >= 0.f && s->p_resid < 1.f;
}
}  // namespace

int64_t CC_API(cc_gpt2_param_count)(const cc_gpt2_cfg* cfg) {
    if (!gpt2_cfg_ok(cfg)) return CC_ERR_SHAPE;
    return Gpt2Off(cfg).total;
}

int CC_API(cc_gpt2_param_offsets)(const cc_gpt2_cfg* cfg, int64_t* offs) {
    if (!gpt2_cfg_ok(cfg) || !offs) return CC_ERR_SHAPE;
    const Gpt2Off o(cfg);
    *offs++ = o.wte; *offs++ = o.wpe;
    for (int l = 0; l < cfg->NL; l++) offs = put_layer(offs, o.layer(l));
    *offs++ = o.lnf_w; *offs++ = o.lnf_b;
    return CC_OK;
}

int64_t CC_API(cc_gpt2_ws_bytes)(const cc_gpt2_cfg* cfg, const cc_gpt2_shape* s) {
    if (!gpt2_cfg_ok(cfg) || !shape_ok(cfg, s)) return CC_ERR_SHAPE;
    Gpt2WS w;
    gpt2_carve(cfg, s, s->T - s->L, nullptr, w);
    return (int64_t)w.bytes;
}

#if CC_OP == 2
static int gpt2_sync_x3(const cc_gpt2_cfg* c, const float* w32, uint16_t* w16, hipStream_t st) {
    const Gpt2Off o(c);
    const int D = c->D;
    X3SplitBatch sb;
    sb.add(w32 + o.wte, W16(w16, o.wte), c->Vp, D, 0, 1);                       // lm_head forward / logits / decode
    sb.add(w32 + o.wte, W16(w16, o.total + o.wte), c->Vp, D, 1, 1);             // [D][3 Vp]: lm_head input gradient
    CC_TRY(x3_split_multi(sb, st));
    sb.n = 0;
    for (int l = 0; l < c->NL; l++) {
        const auto y = o.layer(l);
        const int64_t off[4] = {y.aw, y.pw, y.fw, y.p2w};
        const int R[4] = {D, D, D, 4 * D}, C[4] = {3 * D, D, 4 * D, D};          // Conv1D [in][out]
        for (int i = 0; i < 4; i++) {
            if (sb.n + 2 > 32) { CC_TRY(x3_split_multi(sb, st)); sb.n = 0; }
            sb.add(w32 + off[i], W16(w16, off[i]), R[i], C[i], 0, 1);
            sb.add(w32 + off[i], W16(w16, o.total + off[i]), R[i], C[i], 1, 1);
        }
    }
    return x3_split_multi(sb, st);
}
#endif

static int gpt2_transposes(const cc_gpt2_cfg* c, uint16_t* w16, hipStream_t st) {
    if (kX3) return CC_ERR_ARG;      // the operand images are made from the fp32 master (cc_gpt2_sync_weights)
    const Gpt2Off o(c);
    op16_t* t = w16 + o.total;
    const int D = c->D;
    CC_TRY(transpose_bf16(w16 + o.wte, t + o.wte, c->Vp, D, st));     // [Vp, D] -> [D, Vp]  (lm_head dgrad)
    TransposeBatch tb;
    for (int l = 0; l < c->NL; l++) {
        const auto y = o.layer(l);
        tb.add(w16 + y.aw, t + y.aw, D, 3 * D);    // Conv1D [in,out] -> [out,in]: forward is NT on these
        tb.add(w16 + y.pw, t + y.pw, D, D);
        tb.add(w16 + y.fw, t + y.fw, D, 4 * D);
        tb.add(w16 + y.p2w, t + y.p2w, 4 * D, D);
        if (tb.n == 32) { CC_TRY(transpose_bf16_multi(tb, st)); tb.n = 0; }
    }
    CC_TRY(transpose_bf16_multi(tb, st));
    return CC_OK;
}

int CC_API(cc_gpt2_sync_weights)(const cc_gpt2_cfg* c, const float* w32, uint16_t* w16, void* stream) {
    if (!gpt2_cfg_ok(c) || !w32 || !w16) return CC_ERR_ARG;
    hipStream_t st = S_(stream);
#if CC_OP == 2
    return gpt2_sync_x3(c, w32, w16, st);
#else
    CC_TRY(f32_to_bf16(w32, w16, (size_t)Gpt2Off(c).total, st));
    return gpt2_transposes(c, w16, st);
#endif
}

int CC_API(cc_gpt2_transpose_weights)(const cc_gpt2_cfg* c, uint16_t* w16, void* stream) {
    if (!gpt2_cfg_ok(c) || !w16) return CC_ERR_ARG;
    return gpt2_transposes(c, w16, S_(stream));
}

// GPT-2 dropout (full finetune in train mode) is part of the pass's cc_gpt2_shape: embed / fwd / bwd(_range) of one pass read the
// same (p_embd, p_attn, p_resid, drop_seed); all zero = eval behaviour.
int CC_API(cc_dropout_mask)(uint64_t seed, int32_t site, int32_t layer, float p, int64_t n, uint8_t* out, void* stream) {
    if (!out || n < 0 || site < 0 || site > 3 || layer < 0 || layer > 255 || p < 0.f || p >= 1.f) return CC_ERR_ARG;
    return dropout_mask_u8(out, (size_t)n, make_drop(p, seed, (unsigned)site, (unsigned)layer), S_(stream));
}

int CC_API(cc_gpt2_embed)(const cc_gpt2_cfg* c, const cc_gpt2_shape* s, const float* w32, const float* prefix, const int64_t* tokens, void* ws,
                  void* stream) {
    if (!gpt2_cfg_ok(c) || !shape_ok(c, s) || !w32 || !ws || (s->L > 0 && !prefix) || (s->T > s->L && !tokens)) return CC_ERR_ARG;
    Gpt2Pass ps(c, s, s->T - s->L, ws, stream);
    auto& [st, o, w, cx, D, M, H, hd] = ps;
    CC_TRY(embed_concat(prefix, reinterpret_cast<const long long*>(tokens), s->cap, w32 + o.wte, w32 + o.wpe, w.x[0], s->B, s->L, s->T, D, 0, st));
    // embd dropout on inputs_embeds + position_embeds (hf GPT2Model.forward: self.drop)
    return dropout_f32(w.x[0], (size_t)s->B * s->T * D, make_drop(s->p_embd, s->drop_seed, DROP_EMBD, 0), st);
}

int CC_API(cc_gpt2_embed_from)(const cc_gpt2_cfg* c, const cc_gpt2_shape* s, const float* w32, const float* inputs_embeds, void* ws,
                       void* stream) {
    if (!gpt2_cfg_ok(c) || !shape_ok(c, s) || !w32 || !ws || !inputs_embeds) return CC_ERR_ARG;
    Gpt2Pass ps(c, s, s->T - s->L, ws, stream);
    return embed_concat(inputs_embeds, nullptr, 0, w32 + ps.o.wte, w32 + ps.o.wpe, ps.w.x[0], s->B, s->T, s->T, ps.D, 0, ps.st);
}

int CC_API(cc_gpt2_fwd)(const cc_gpt2_cfg* c, const cc_gpt2_shape* s, const float* w32, const uint16_t* w16, void* ws, void* stream) {
    if (!gpt2_cfg_ok(c) || !shape_ok(c, s) || !w32 || !w16 || !ws) return CC_ERR_ARG;
    Gpt2Pass ps(c, s, s->T - s->L, ws, stream);
    auto& [st, o, w, cx, D, M, H, hd] = ps;
    const uint16_t* w16t = W16(w16, o.total);   // Conv1D weights transposed to [out,in]: every forward GEMM is NT
    for (int l = 0; l < c->NL; l++) {
        const auto y = o.layer(l);
        // hf :262-310: x1 = x + c_proj(attn(c_attn(ln_1 x)))
        CC_TRY(ln_fwd(w.x[l], D, nullptr, w32 + y.l1w, w32 + y.l1b, w.xn1[l], nullptr, w.mean1[l], w.rstd1[l], M, D, st));
        CC_TRY(gemm_bf16out(0, 0, w.xn1[l], D, W16(w16t, y.aw), D, M, 3 * D, D, w.qkv[l], 3 * D, w32 + y.ab, 0, nullptr, cx));
        CC_TRY(attn_fwd(w.qkv[l], s->B, s->T, H, hd, true, w.att[l], w.lse[l], st, make_drop(s->p_attn, s->drop_seed, DROP_ATTN, l)));
        {
            static const int tile_proj = env_tile("CC_TILE_PROJ");
            TileScope ts(tile_proj);
            CC_TRY(gemm_resid(0, 0, w.att[l], D, W16(w16t, y.pw), D, M, D, D, w.x1[l], w.x[l], D, w32 + y.pb, cx,
                              make_drop(s->p_resid, s->drop_seed, DROP_RESID_ATTN, l)));
        }
        // x = x1 + c_proj(gelu_new(c_fc(ln_2 x1)))   (hf :229-243)
        CC_TRY(ln_fwd(w.x1[l], D, nullptr, w32 + y.l2w, w32 + y.l2b, w.xn2[l], nullptr, w.mean2[l], w.rstd2[l], M, D, st));
        {
            static const int tile_fc = env_tile("CC_TILE_FC");
            TileScope ts(tile_fc);
            // act 3: the pre-activation slot receives gelu_new'(u) — one sigmoid serves both, and the backward's epilogue is a multiply
            CC_TIMED(CC_SITE_GPT2_FC_FWD, st, gemm_bf16out(0, 0, w.xn2[l], D, W16(w16t, y.fw), D, M, 4 * D, D, w.hact[l], 4 * D, w32 + y.fb, (s->mode >= 1 && gelu_grad_fwd()) ? 3 : 2,
                                                            s->mode >= 1 ? w.u[l] : nullptr, cx));
        }
        {
            static const int tile_proj2 = env_tile("CC_TILE_PROJ2");
            TileScope ts(tile_proj2);
            CC_TIMED(CC_SITE_GPT2_PROJ2_FWD, st, gemm_resid(0, 0, w.hact[l], 4 * D, W16(w16t, y.p2w), 4 * D, M, D, 4 * D, w.x[l + 1], w.x1[l], D, w32 + y.p2b, cx,
                                                           make_drop(s->p_resid, s->drop_seed, DROP_RESID_MLP, l)));
        }
    }
    return CC_OK;
}

int CC_API(cc_gpt2_logits)(const cc_gpt2_cfg* c, const cc_gpt2_shape* s, const float* w32, const uint16_t* w16, void* ws, float* logits,
                   int64_t ldl, void* stream) {
    if (!gpt2_cfg_ok(c) || !shape_ok(c, s) || !w32 || !w16 || !ws || !logits) return CC_ERR_ARG;
    const int Ns = std::min(c->Vp, rup(c->V, 8));
    if (ldl < Ns || (ldl & 3) || ldl > 0x7fffffff) return CC_ERR_SHAPE;
    Gpt2Pass ps(c, s, s->T - s->L, ws, stream);
    auto& [st, o, w, cx, D, M, H, hd] = ps;
    CC_TRY(ln_fwd(w.x[c->NL], D, nullptr, w32 + o.lnf_w, w32 + o.lnf_b, w.hf16, nullptr, w.meanf, w.rstdf, M, D, st));
    return gemm_f32out(0, 0, w.hf16, D, W16(w16, o.wte), D, M, Ns, D, logits, (int)ldl, nullptr, 0, 1.0f, 1, cx);
}

namespace {
// Label smoothing (cc_lmhead_ce_fwd_smooth / cc_lmhead_ce_bwd_smooth): the caller's scratch, carved.  part: the slice partials of wbar.
struct SmoothScratch {
    float *wbar, *hsum, *zbar, *term, *coef, *part;
    int64_t floats;
    SmoothScratch(const cc_gpt2_cfg* c, const cc_gpt2_shape* s, float* base) {
        const size_t D = c->D, Mc = ((size_t)s->B * (s->T - s->L) + 3) & ~size_t(3);      // every block starts 16-byte aligned
        size_t off = 0;
        const auto take = [&](size_t n) { float* r = base ? base + off : nullptr; off += n; return r; };
        wbar = take(D); hsum = take(D); zbar = take(Mc); term = take(Mc); coef = take(2 * Mc);
        part = take((size_t)smooth_wbar_slices(c->V) * D);
        floats = (int64_t)off;
    }
};
// eps in [0, 1) and a usable scratch; written so that a NaN fails
inline bool smooth_ok(float eps, const float* scratch) { return eps >= 0.f && eps < 1.f && scratch && !((uintptr_t)scratch & 15); }

// the weighted pair: a row_weight, and a scratch unless eps == 0 (then no smoothing launch reads one)
inline bool weighted_ok(const float* row_weight, float eps, const float* scratch) {
    return row_weight && eps >= 0.f && eps < 1.f && (eps == 0.f || scratch) && !((uintptr_t)scratch & 15);
}

// cc_lmhead_ce_fwd (scratch == nullptr: stats of 2 floats), cc_lmhead_ce_fwd_smooth (stats of 3) and cc_lmhead_ce_fwd_w (row_weight set:
// stats of 3, scratch only where eps != 0) share this body
static int lmhead_ce_fwd_body(const cc_gpt2_cfg* c, const cc_gpt2_shape* s, const float* w32, const uint16_t* w16, void* ws, const int64_t* tokens,
                       float eps, float* scratch, float* stats, void* stream, const float* row_weight = nullptr);
static int lmhead_ce_bwd_body(const cc_gpt2_cfg* c, const cc_gpt2_shape* s, const float* w32, const uint16_t* w16, void* ws, const float* denom,
                       const float* loss_scale, float eps, float* scratch, float* g32, void* stream, const float* row_weight = nullptr);
}  // namespace

int CC_API(cc_lmhead_ce_fwd)(const cc_gpt2_cfg* c, const cc_gpt2_shape* s, const float* w32, const uint16_t* w16, void* ws, const int64_t* tokens,
                     float* stats, void* stream) {
    return lmhead_ce_fwd_body(c, s, w32, w16, ws, tokens, 0.f, nullptr, stats, stream);
}

int64_t CC_API(cc_lmhead_smooth_scratch_floats)(const cc_gpt2_cfg* c, const cc_gpt2_shape* s) {
    if (!gpt2_cfg_ok(c) || !shape_ok(c, s)) return CC_ERR_SHAPE;
    return SmoothScratch(c, s, nullptr).floats;
}

int CC_API(cc_lmhead_ce_fwd_smooth)(const cc_gpt2_cfg* c, const cc_gpt2_shape* s, const float* w32, const uint16_t* w16, void* ws, const int64_t* tokens,
                            float eps, float* scratch, float* stats3, void* stream) {
    if (!smooth_ok(eps, scratch)) return CC_ERR_ARG;
    return lmhead_ce_fwd_body(c, s, w32, w16, ws, tokens, eps, scratch, stats3, stream);
}

int CC_API(cc_lmhead_ce_bwd_smooth)(const cc_gpt2_cfg* c, const cc_gpt2_shape* s, const float* w32, const uint16_t* w16, void* ws, const float* denom,
                            const float* loss_scale, float eps, float* scratch, float* g32, void* stream) {
    if (!smooth_ok(eps, scratch)) return CC_ERR_ARG;
    return lmhead_ce_bwd_body(c, s, w32, w16, ws, denom, loss_scale, eps, scratch, g32, stream);
}

int CC_API(cc_lmhead_ce_fwd_w)(const cc_gpt2_cfg* c, const cc_gpt2_shape* s, const float* w32, const uint16_t* w16, void* ws, const int64_t* tokens,
                       const float* row_weight, float eps, float* scratch, float* stats3, void* stream) {
    if (!weighted_ok(row_weight, eps, scratch)) return CC_ERR_ARG;
    return lmhead_ce_fwd_body(c, s, w32, w16, ws, tokens, eps, scratch, stats3, stream, row_weight);
}

int CC_API(cc_lmhead_ce_bwd_w)(const cc_gpt2_cfg* c, const cc_gpt2_shape* s, const float* w32, const uint16_t* w16, void* ws, const float* denom,
                       const float* loss_scale, const float* row_weight, float eps, float* scratch, float* g32, void* stream) {
    if (!weighted_ok(row_weight, eps, scratch)) return CC_ERR_ARG;
    return lmhead_ce_bwd_body(c, s, w32, w16, ws, denom, loss_scale, eps, scratch, g32, stream, row_weight);
}

int CC_API(cc_lmhead_ce_bwd)(const cc_gpt2_cfg* c, const cc_gpt2_shape* s, const float* w32, const uint16_t* w16, void* ws, const float* denom,
                     const float* loss_scale, float* g32, void* stream) {
    return lmhead_ce_bwd_body(c, s, w32, w16, ws, denom, loss_scale, 0.f, nullptr, g32, stream);
}

namespace {
static int lmhead_ce_fwd_body(const cc_gpt2_cfg* c, const cc_gpt2_shape* s, const float* w32, const uint16_t* w16, void* ws, const int64_t* tokens,
                       float eps, float* scratch, float* stats, void* stream, const float* rw) {
    if (!gpt2_cfg_ok(c) || !shape_ok(c, s) || s->mode < 1 || s->L < 1 || !w32 || !w16 || !ws || !tokens || !stats) return CC_ERR_ARG;
    const int cap = s->T - s->L;
    if (cap != s->cap) return CC_ERR_SHAPE;  // the loss consumes every token column (model.py:108-109)
    Gpt2Pass ps(c, s, cap, ws, stream);
    auto& [st, o, w, cx, D, M, H, hd] = ps;
    const int Mc = s->B * cap, npart = c->Vp / 64;
    if (hipMemsetAsync(stats, 0, (rw ? 3 : 2) * sizeof(float), st) != hipSuccess) return CC_ERR_LAUNCH;
    CC_TRY(ce_targets(reinterpret_cast<const long long*>(tokens), w.target, w.row_map, s->B, cap, s->L, s->T, st));
    // ln_f only on the rows the loss reads: L-1 .. T-2 of every sample (model.py:108)
    CC_TRY(ln_fwd(w.x[c->NL], D, w.row_map, w32 + o.lnf_w, w32 + o.lnf_b, w.hf16, nullptr, w.meanf, w.rstdf, Mc, D, st));
    const bool ef = lm_exp_form(s);
    const op16_t* wte_rows = kX3 ? reinterpret_cast<const op16_t*>(w32 + o.wte) : W16(w16, o.wte);      // rows read elementwise: bf16x3 takes the fp32 master
    if (ef) CC_TRY(lm_tgt_ref(w.hf16, wte_rows, D, w.target, w.cref, Mc, st));
    CC_TIMED(CC_SITE_LMHEAD_FWD, st, gemm_lmhead(w.hf16, D, W16(w16, o.wte), D, Mc, c->Vp, c->V, D, lm_logits(c, s, w.logits16), c->Vp, w.pmax, w.psum, npart, w.target, w.tgt_logit, cx,
                                                 ef ? w.cref : nullptr));
    CC_TRY(ce_rows(w.pmax, w.psum, npart, w.target, ef ? w.cref : w.tgt_logit, w.lse_row, w.row_loss, stats, Mc, st, rw));   // cref IS the target logit
    if (!scratch || (rw && eps == 0.f)) return CC_OK;      // with weights ce_rows has written the third float too
    if (eps == 0.f)      // the plain chain, and the third float
        return hipMemcpyAsync(stats + 2, stats, sizeof(float), hipMemcpyDeviceToDevice, st) == hipSuccess ? CC_OK : CC_ERR_LAUNCH;
    // + eps (z_t - zbar) per kept row: wbar from the rows the lm_head GEMM read, zbar a GEMV over the stored hf — no pass over V
    const SmoothScratch sm(c, s, scratch);
    CC_TRY(smooth_wbar(reinterpret_cast<const act_t*>(wte_rows), c->V, D, sm.part, sm.wbar, st));
    return smooth_rows(w.hf16, sm.wbar, D, w.target, ef ? w.cref : w.tgt_logit, eps, sm.zbar, sm.term, stats, Mc, st, rw);
}
}  // namespace

int CC_API(cc_lmhead_score)(const cc_gpt2_cfg* c, const cc_gpt2_shape* s, const float* w32, const uint16_t* w16, void* ws, const int64_t* tokens,
                    int32_t ignore_zero, float* token_logprob, float* sample_stats, void* stream) {
    if (!gpt2_cfg_ok(c) || !shape_ok(c, s) || s->mode != 0 || s->L < 1 || !w32 || !w16 || !ws || !tokens || !token_logprob || !sample_stats)
        return CC_ERR_ARG;
    const int cap = s->T - s->L;
    if (cap < 1 || cap != s->cap) return CC_ERR_SHAPE;      // every token column is scored
    Gpt2Pass ps(c, s, cap, ws, stream);
    auto& [st, o, w, cx, D, M, H, hd] = ps;
    const int Mc = s->B * cap, npart = c->Vp / 64;
    CC_TRY(ce_targets(reinterpret_cast<const long long*>(tokens), w.target, w.row_map, s->B, cap, s->L, s->T, st));
    CC_TRY(score_keep(reinterpret_cast<const long long*>(tokens), w.keep, Mc, ignore_zero, st));
    // ln_f only on the rows that predict a caption token: L-1 .. T-2 of every sample
    CC_TRY(ln_fwd(w.x[c->NL], D, w.row_map, w32 + o.lnf_w, w32 + o.lnf_b, w.hf16, nullptr, w.meanf, w.rstdf, Mc, D, st));
    CC_TIMED(CC_SITE_LMHEAD_FWD, st, gemm_lmhead_score(w.hf16, D, W16(w16, o.wte), D, Mc, c->Vp, c->V, D, w.pmax, w.psum, npart, w.target, w.tgt_logit, cx));
    return score_rows(w.pmax, w.psum, npart, w.keep, w.tgt_logit, w.lse_row, token_logprob, sample_stats, s->B, cap, st);
}

namespace {
static int lmhead_ce_bwd_body(const cc_gpt2_cfg* c, const cc_gpt2_shape* s, const float* w32, const uint16_t* w16, void* ws, const float* denom,
                       const float* loss_scale, float eps, float* scratch, float* g32, void* stream, const float* rw) {
    if (!gpt2_cfg_ok(c) || !shape_ok(c, s) || s->mode < 1 || !w32 || !w16 || !ws || !denom || (s->mode == 2 && !g32)) return CC_ERR_ARG;
    const int cap = s->T - s->L;
    Gpt2Pass ps(c, s, cap, ws, stream);
    auto& [st, o, w, cx, D, M, H, hd] = ps;
    const int Mc = s->B * cap;
    const bool full = s->mode == 2;
    // exponential form: logits16 holds E = exp(logit - cref); d logits = r E - w onehot is never written — the row factors go into the
    // GEMMs' finishing passes (EpiLMHead comment).  Otherwise: the in-place softmax-gradient pass over the stored logits.
    const bool ef = lm_exp_form(s);
    const LmFix fix{w.lmfac, w.target, kX3 ? reinterpret_cast<const op16_t*>(w32 + o.wte) : W16(w16, o.wte)};
    if (ef) CC_TRY(lm_rowfac(w.cref, w.lse_row, w.target, denom, loss_scale, w.lmfac, Mc, st, rw));
    const Act lg = lm_logits(c, s, w.logits16);
    ActIn dlog = lg;                    // the A operand of the input-gradient GEMM (bf16x3 exponential form: E, written as its operand image)
    // bf16x3, frozen LM: nothing but that GEMM reads d logits -> the softmax-gradient pass writes its [hi | hi | lo] operand image straight
    // into the call's operand scratch (sized for exactly this image, gpt2_carve) instead of fp32 values a split pass would re-read
    op16_t* dimg = (kX3 && !ef && !full && x3_img_on()) ? x3_scratch_block(cx, x3_img(Mc, c->Vp)) : nullptr;
    if (dimg) dlog = ActIn(reinterpret_cast<const act_t*>(dimg), c->Vp);
    if (!ef) CC_TRY(ce_dlogits(w.logits16, c->Vp, c->V, w.target, w.lse_row, denom, loss_scale, Mc, st, dimg, rw));
    // logit form with weights: d logits carries |factor|; the factor's sign is applied to the rows of d hf and of the weight-gradient operand
    const bool sgn = rw && !ef;
    if (sgn) CC_TRY(lm_rowsign(w.target, denom, loss_scale, rw, w.lmfac, Mc, st));
    // d hf = dlogits · wte   ([Mc,Vp] x [Vp(k), D(n)])
    // K = Vp is deep and the output narrow: K slices over the idle CUs, slabs parked in du16 (free until the first layer's backward)
    const auto lm_dgrad = [&]() {
        auto& [st, o, w, cx, D, M, H, hd] = ps;      // (C++17 lambdas capture the pass, not its bindings)
        const int rc = gemm_nt_deepk(dlog, c->Vp, W16(w16, o.total + o.wte), c->Vp, Mc, D, c->Vp, w.dhf16, D, reinterpret_cast<float*>(w.du16.p),
                                     (size_t)M * 4 * D * sizeof(act_t), cx, ef ? &fix : nullptr);
        if (rc != CC_ERR_SHAPE) return rc;
        const int rc2 = gemm_bf16out(0, 0, dlog, c->Vp, W16(w16, o.total + o.wte), c->Vp, Mc, D, c->Vp, w.dhf16, D, nullptr, 0, nullptr, cx);
        return (rc2 != CC_OK || !ef) ? rc2 : lm_dgrad_fix(w.dhf16, w.lmfac, w.target, fix.wte, D, Mc, st);
    };
    CC_TIMED(CC_SITE_LMHEAD_DGRAD, st, lm_dgrad());
    if (sgn) CC_TRY(lm_scale_rows_inplace(w.dhf16, w.lmfac, D, Mc, st));
    if (full) {      // tied lm_head: d wte += dlogits^T hf  (= E^T (r hf) - onehot^T (w hf) in the exponential form)
        if (ef) {
            CC_TRY(lm_scale_rows(w.hf16, w.lmfac, w.hfs16, D, Mc, st));
            CC_TRY(gemm_wgrad(lg, c->Vp, w.hfs16, D, c->Vp, D, Mc, g32 + o.wte, D, w.wg_scratch, cx));
            ScatterSrc oh;          // the one-hot term: d wte[target] -= w hf, rows with w == 0 left out
            oh.ids32 = w.target; oh.act = w.hf16; oh.fac = w.lmfac;
            CC_TRY(scatter_rows(oh, Mc, D, c->Vp, g32 + o.wte, w.scat, st));
        } else {
            if (sgn) CC_TRY(lm_scale_rows(w.hf16, w.lmfac, w.hfs16, D, Mc, st));
            CC_TRY(gemm_wgrad(lg, c->Vp, sgn ? w.hfs16 : w.hf16, D, c->Vp, D, Mc, g32 + o.wte, D, w.wg_scratch, cx));
        }
    }
    if (scratch && eps != 0.f) {
        // label smoothing, a pass of its own after the input-gradient GEMM and its fix: d hf += c (wte[t] - wbar) with the forward's wbar;
        // tied lm_head: d wte[t] += c hf (a row scatter, as the one-hot term above) and d wte[v < V] -= (sum of c hf) / V (one vector)
        const SmoothScratch sm(c, s, scratch);
        CC_TRY(smooth_dhf(w.dhf16, w.target, denom, loss_scale, eps, reinterpret_cast<const act_t*>(fix.wte), sm.wbar, sm.coef, D, Mc, st, rw));
        if (full) {
            ScatterSrc sc;
            sc.ids32 = w.target; sc.act = w.hf16; sc.fac = sm.coef;
            CC_TRY(scatter_rows(sc, Mc, D, c->Vp, g32 + o.wte, w.scat, st));
            CC_TRY(smooth_dwte_bcast(w.hf16, sm.coef, D, Mc, c->V, sm.hsum, g32 + o.wte, cx));
        }
    }
    if (hipMemsetAsync(w.dx32, 0, (size_t)M * D * sizeof(float), st) != hipSuccess) return CC_ERR_LAUNCH;
    const size_t dx16_bytes = (size_t)M * D * (w.dx16.img ? 3 * sizeof(op16_t) : sizeof(act_t));     // (an image where the top layer's backward reads one)
    if (hipMemsetAsync(w.dx16.p, 0, dx16_bytes, st) != hipSuccess) return CC_ERR_LAUNCH;
    CC_TRY(ln_bwd(w.dhf16, w.x[c->NL], D, w.row_map, w.meanf, w.rstdf, w32 + o.lnf_w, nullptr, w.dx32, w.dx16, full ? g32 + o.lnf_w : nullptr,
                  full ? g32 + o.lnf_b : nullptr, Mc, D, cx));
    return CC_OK;
}
}  // namespace

// Test hooks around the lm_head / loss chain (tests/lm_ref.py): carve and copy, no kernels of their own.
int CC_API(cc_lmhead_put_x)(const cc_gpt2_cfg* c, const cc_gpt2_shape* s, void* ws, const float* x, void* stream) {
    if (!gpt2_cfg_ok(c) || !shape_ok(c, s) || !ws || !x) return CC_ERR_ARG;
    Gpt2Pass ps(c, s, s->T - s->L, ws, stream);
    const size_t bytes = (size_t)s->B * s->T * c->D * sizeof(float);
    return hipMemcpyAsync(ps.w.x[c->NL], x, bytes, hipMemcpyDeviceToDevice, ps.st) == hipSuccess ? CC_OK : CC_ERR_LAUNCH;
}

int CC_API(cc_lmhead_get)(const cc_gpt2_cfg* c, const cc_gpt2_shape* s, void* ws, int32_t field, void* dst, int64_t dst_bytes, void* stream) {
    if (!gpt2_cfg_ok(c) || !shape_ok(c, s) || !ws || !dst || field < CC_LM_LSE || field > CC_LM_DX32) return CC_ERR_ARG;
    if (s->T - s->L < 1) return CC_ERR_SHAPE;      // no caption rows: the pass has no lm_head / loss side
    Gpt2Pass ps(c, s, s->T - s->L, ws, stream);
    const Gpt2WS& w = ps.w;
    const size_t Mc = (size_t)s->B * (s->T - s->L), M = (size_t)s->B * s->T, D = c->D;
    const void* src = nullptr;
    size_t bytes = 0;
    switch (field) {
        case CC_LM_LSE: src = w.lse_row; bytes = Mc * sizeof(float); break;
        case CC_LM_TGT: src = (s->mode >= 1 && lm_exp_form(s)) ? w.cref : w.tgt_logit; bytes = Mc * sizeof(float); break;
        case CC_LM_ROW_LOSS: src = w.row_loss; bytes = Mc * sizeof(float); break;
        case CC_LM_HF: src = w.hf16; bytes = Mc * D * sizeof(act_t); break;
        case CC_LM_DHF: src = w.dhf16; bytes = Mc * D * sizeof(act_t); break;
        default: src = w.dx32; bytes = M * D * sizeof(float); break;
    }
    if (!src) return CC_ERR_STATE;      // this shape's mode does not carve the field
    if (dst_bytes < 0 || (size_t)dst_bytes != bytes) return CC_ERR_SHAPE;
    return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, ps.st) == hipSuccess ? CC_OK : CC_ERR_LAUNCH;
}

int CC_API(cc_gpt2_logits_bwd)(const cc_gpt2_cfg* c, const cc_gpt2_shape* s, const float* w32, const uint16_t* w16, void* ws, const float* dlogits,
                       int64_t ldl, float* dx0, float* g32, void* stream) {
    if (!gpt2_cfg_ok(c) || !shape_ok(c, s) || s->mode < 1 || s->L != 0 || !w32 || !w16 || !ws || !dlogits || ldl < c->V || (s->mode == 2 && !g32))
        return CC_ERR_ARG;
    Gpt2Pass ps(c, s, s->T, ws, stream);      // L == 0: the loss-side buffers are sized for all B*T rows
    auto& [st, o, w, cx, D, M, H, hd] = ps;
    const bool full = s->mode == 2;
    CC_TRY(f32_to_op16_pad(dlogits, ldl, c->V, w.logits16, c->Vp, M, st));
    // d hf = dlogits · wte ([M,Vp] x [Vp(k), D(n)]); tied lm_head: d wte += dlogits^T hf (hf16 = the rows cc_gpt2_logits normalised)
    CC_TRY(gemm_bf16out(0, 0, w.logits16, c->Vp, W16(w16, o.total + o.wte), c->Vp, M, D, c->Vp, w.dhf16, D, nullptr, 0, nullptr, cx));
    if (full) CC_TRY(gemm_wgrad(w.logits16, c->Vp, w.hf16, D, c->Vp, D, M, g32 + o.wte, D, w.wg_scratch, cx));
    if (hipMemsetAsync(w.dx32, 0, (size_t)M * D * sizeof(float), st) != hipSuccess) return CC_ERR_LAUNCH;
    CC_TRY(ln_bwd(w.dhf16, w.x[c->NL], D, nullptr, w.meanf, w.rstdf, w32 + o.lnf_w, nullptr, w.dx32, w.dx16, full ? g32 + o.lnf_w : nullptr,
                  full ? g32 + o.lnf_b : nullptr, M, D, cx));
    CC_TRY(CC_API(cc_gpt2_bwd_range)(c, s, w32, w16, ws, nullptr, nullptr, g32, c->NL, 0, stream));
    if (dx0 && hipMemcpyAsync(dx0, w.dx32, (size_t)M * D * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess) return CC_ERR_LAUNCH;
    return CC_OK;
}

int CC_API(cc_gpt2_bwd)(const cc_gpt2_cfg* c, const cc_gpt2_shape* s, const float* w32, const uint16_t* w16, void* ws, const int64_t* tokens,
                float* dprefix, float* g32, void* stream) {
    if (!gpt2_cfg_ok(c)) return CC_ERR_ARG;
    return CC_API(cc_gpt2_bwd_range)(c, s, w32, w16, ws, tokens, dprefix, g32, c->NL, 0, stream);
}

int CC_API(cc_gpt2_bwd_range)(const cc_gpt2_cfg* c, const cc_gpt2_shape* s, const float* w32, const uint16_t* w16, void* ws, const int64_t* tokens,
                      float* dprefix, float* g32, int32_t l_hi, int32_t l_lo, void* stream) {
    if (!gpt2_cfg_ok(c) || !shape_ok(c, s) || s->mode < 1 || !w32 || !w16 || !ws || (s->L > 0 && !dprefix) || (s->mode == 2 && !g32) ||
        l_lo < 0 || l_hi > c->NL || l_lo > l_hi)
        return CC_ERR_ARG;
    Gpt2Pass ps(c, s, s->T - s->L, ws, stream);
    auto& [st, o, w, cx, D, M, H, hd] = ps;
    const int D3 = 3 * D, D4 = 4 * D;
    const bool full = s->mode == 2;
    WgradBatch wb;          // full finetune: a layer's four weight gradients as one grouped launch + one slab reduce
    wb.defer = full;
    WgradBatch* wbp = full ? &wb : nullptr;
    // the weight gradients and bias column sums below read these four as plain activations (.p)
    if (full && (w.dx16.img || w.dx16b.img || w.du16.img || w.dqkv16.img)) return CC_ERR_STATE;
    // The 16-bit copy of the residual gradient that feeds a c_proj's backward GEMMs is the dropout-masked one, and the c_proj's bias
    // gradient is its column sum.  Both are produced by the LayerNorm backward that writes the copy (ln_bwd dmask / dcol) — except for
    // the top layer, whose copy comes from ln_f's row-mapped backward and is masked / summed by separate launches.
    for (int l = l_hi - 1; l >= l_lo; l--) {
        const auto y = o.layer(l);
        const bool top = l == c->NL - 1;
        // mlp.c_proj (Conv1D [4D, D]): y = hact W + b
        if (top) CC_TRY(dropout_bf16(w.dx16.p, (size_t)M * D, make_drop(s->p_resid, s->drop_seed, DROP_RESID_MLP, l), st));
        if (full) {
            CC_TRY(gemm_wgrad(w.hact[l], D4, w.dx16.p, D, D4, D, M, g32 + y.p2w, D, w.wg_scratch, cx, wbp));
            if (top) CC_TRY(colsum_bf16(w.dx16.p, D, M, D, g32 + y.p2b, cx));
        }
        {
            static const int tile_dact = env_tile("CC_TILE_DACT");
            TileScope ts(tile_dact);
            CC_TRY(gemm_dact(0, 0, w.dx16, D, W16(w16, y.p2w), D, M, D4, D, w.du16, D4, w.u[l], gelu_grad_fwd() ? 3 : 2, cx));
        }
        // mlp.c_fc (Conv1D [D, 4D])
        if (full) {
            CC_TRY(gemm_wgrad(w.xn2[l], D, w.du16.p, D4, D, D4, M, g32 + y.fw, D4, w.wg_scratch, cx, wbp));
            CC_TRY(colsum_bf16(w.du16.p, D4, M, D4, g32 + y.fb, cx));
        }
        CC_TIMED(CC_SITE_GPT2_FC_DGRAD, st, gemm_bf16out(0, 0, w.du16, D4, W16(w16, y.fw), D4, M, D, D4, w.dxn16, D, nullptr, 0, nullptr, cx));
        CC_TRY(ln_bwd(w.dxn16, w.x1[l], D, nullptr, w.mean2[l], w.rstd2[l], w32 + y.l2w, w.dx32, w.dx32, w.dx16b, full ? g32 + y.l2w : nullptr,
                      full ? g32 + y.l2b : nullptr, M, D, cx, full ? g32 + y.pb : nullptr,
                      make_drop(s->p_resid, s->drop_seed, DROP_RESID_ATTN, l)));
        // attn.c_proj (Conv1D [D, D])
        if (full) CC_TRY(gemm_wgrad(w.att[l], D, w.dx16b.p, D, D, D, M, g32 + y.pw, D, w.wg_scratch, cx, wbp));
        CC_TRY(gemm_bf16out(0, 0, w.dx16b, D, W16(w16, y.pw), D, M, D, D, w.datt16, D, nullptr, 0, nullptr, cx));
        CC_TRY(attn_bwd(w.qkv[l], w.datt16, w.att[l].p, w.lse[l], w.adelta, s->B, s->T, H, hd, true, w.dqkv16, st,
                        make_drop(s->p_attn, s->drop_seed, DROP_ATTN, l)));
        // attn.c_attn (Conv1D [D, 3D])
        if (full) {
            CC_TRY(gemm_wgrad(w.xn1[l], D, w.dqkv16.p, D3, D, D3, M, g32 + y.aw, D3, w.wg_scratch, cx, wbp));
            CC_TRY(colsum_bf16(w.dqkv16.p, D3, M, D3, g32 + y.ab, cx));
        }
        CC_TRY(gemm_bf16out(0, 0, w.dqkv16, D3, W16(w16, y.aw), D3, M, D, D3, w.dxn16, D, nullptr, 0, nullptr, cx));
        // deferred weight gradients: dx16 (masked layer-input gradient), du16, dx16b, dqkv16 are all still intact here
        if (full) CC_TRY(wgrad_flush(wb, st));
        CC_TRY(ln_bwd(w.dxn16, w.x[l], D, nullptr, w.mean1[l], w.rstd1[l], w32 + y.l1w, w.dx32, w.dx32, w.dx16, full ? g32 + y.l1w : nullptr,
                      full ? g32 + y.l1b : nullptr, M, D, cx, (full && l > 0) ? g32 + o.layer(l - 1).p2b : nullptr,
                      l > 0 ? make_drop(s->p_resid, s->drop_seed, DROP_RESID_MLP, l - 1) : Drop()));
    }
    if (l_lo > 0) return CC_OK;
    CC_TRY(dropout_f32(w.dx32, (size_t)M * D, make_drop(s->p_embd, s->drop_seed, DROP_EMBD, 0), st));   // d(inputs + wpe)
    if (s->L > 0) CC_TRY(copy_rows(w.dx32, (size_t)s->T * D, dprefix, (size_t)s->L * D, s->L * D, s->B, st));
    if (full) {     // d wte[max(tok, 0)] += d x0[b, L + c] (the caption rows, fixed-order scatter);  d wpe[t] += sum_b d x0[b, t]
        if (tokens) {
            ScatterSrc e;
            e.ids64 = reinterpret_cast<const long long*>(tokens);
            e.ids_ld = s->cap;
            e.f32 = w.dx32 + (size_t)s->L * D; e.rpb = s->T - s->L; e.bstride = (size_t)s->T * D;
            CC_TRY(scatter_rows(e, s->B * (s->T - s->L), D, c->Vp, g32 + o.wte, w.scat, st));
        }
        CC_TRY(batch_sum(w.dx32, (size_t)s->T * D, g32 + o.wpe, s->T * D, s->B, cx));
    }
    return CC_OK;
}

// ---------------------------------------------------------------- optimizer / casts / test hooks -----------------
int CC_API(cc_adamw_step)(float* p32, const float* g32, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                  float weight_decay, int32_t step, float grad_scale, const float* loss_scale, const float* found_inf, void* stream) {
    if (!p32 || !g32 || !m || !v || n < 0 || step < 0 || (step == 0 && !loss_scale)) return CC_ERR_ARG;
    return adamw(p32, g32, m, v, (size_t)n, lr, beta1, beta2, eps, weight_decay, step, grad_scale, loss_scale, found_inf, S_(stream));
}

int CC_API(cc_adamw_step_cast)(float* p32, const float* g32, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                       float weight_decay, int32_t step, float grad_scale, const float* loss_scale, const float* found_inf, uint16_t* w16, void* stream) {
    if (!p32 || !g32 || !m || !v || !w16 || n < 0 || step < 0 || (step == 0 && !loss_scale)) return CC_ERR_ARG;
    if (kX3) return CC_ERR_ARG;      // bf16x3: the operand images are per-matrix row images, not a flat cast (use cc_adamw_step + cc_*_sync_weights)
    return adamw(p32, g32, m, v, (size_t)n, lr, beta1, beta2, eps, weight_decay, step, grad_scale, loss_scale, found_inf, S_(stream), w16);
}

int CC_API(cc_adamw_step_clip)(float* p32, const float* g32, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                       float weight_decay, int32_t step, float grad_scale, const float* loss_scale, const float* found_inf, const float* clip,
                       uint16_t* w16, void* stream) {
    if (!p32 || !g32 || !m || !v || n < 0 || step < 0 || (step == 0 && !loss_scale)) return CC_ERR_ARG;
    if (w16 && kX3) return CC_ERR_ARG;      // as cc_adamw_step_cast: no flat cast in the bf16x3 mode
    return adamw(p32, g32, m, v, (size_t)n, lr, beta1, beta2, eps, weight_decay, step, grad_scale, loss_scale, found_inf, S_(stream), w16, clip);
}

int CC_API(cc_adamw_step_ema)(float* p32, const float* g32, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                      float weight_decay, int32_t step, float grad_scale, const float* loss_scale, const float* found_inf, const float* clip,
                      uint16_t* w16, float* ema, float ema_decay, void* stream) {
    if (!p32 || !g32 || !m || !v || n < 0 || step < 0 || (step == 0 && !loss_scale)) return CC_ERR_ARG;
    if (w16 && kX3) return CC_ERR_ARG;      // as cc_adamw_step_cast: no flat cast in the bf16x3 mode
    if (!ema || (reinterpret_cast<uintptr_t>(ema) & 15) || !(ema_decay >= 0.f && ema_decay < 1.f)) return CC_ERR_ARG;      // (NaN fails both comparisons)
    const uintptr_t e0 = reinterpret_cast<uintptr_t>(ema), p0 = reinterpret_cast<uintptr_t>(p32), bytes = (uintptr_t)n * sizeof(float);
    if (e0 == p0 || (e0 < p0 + bytes && p0 < e0 + bytes)) return CC_ERR_ARG;      // the average must not alias the parameters
    return adamw(p32, g32, m, v, (size_t)n, lr, beta1, beta2, eps, weight_decay, step, grad_scale, loss_scale, found_inf, S_(stream), w16, clip, ema,
                 ema_decay);
}

int64_t CC_API(cc_grad_norm_scratch_floats)(void) { return (int64_t)GRAD_NORM_BLOCKS; }

int CC_API(cc_cast_op16)(const float* src, uint16_t* dst, int64_t n, void* stream) {
    if (!src || !dst || n < 0 || kX3) return CC_ERR_ARG;
    return f32_to_bf16(src, dst, (size_t)n, S_(stream));
}

int CC_API(cc_gemm_op16_f32)(int32_t al, int32_t bl, const uint16_t* A, int32_t lda, const uint16_t* B, int32_t ldb, int32_t M, int32_t N, int32_t K,
                     float* C, int32_t ldc, const float* bias, int32_t ksplit, void* stream) {
    if (!A || !B || !C || kX3) return CC_ERR_ARG;      // (bf16x3 GEMMs need a workspace for their operand images: no bare hook)
    Call cx{S_(stream)};
    return gemm_f32out(al, bl, reinterpret_cast<const act_t*>(A), lda, B, ldb, M, N, K, C, ldc, ksplit > 1 ? nullptr : bias, ksplit > 1 ? 2 : 0, 1.0f, ksplit, cx);
}

int64_t CC_API(cc_wgrad_scratch_bytes)(void) { return (int64_t)WGRAD_SCRATCH_BYTES; }

int CC_API(cc_gemm_wgrad)(const uint16_t* X, int32_t ldx, const uint16_t* Y, int32_t ldy, int32_t Mw, int32_t Nw, int32_t K, float* dW, int32_t ldw,
                  float* scratch, void* stream) {
    if (!X || !Y || !dW || kX3) return CC_ERR_ARG;
    Call cx{S_(stream)};
    return gemm_wgrad(reinterpret_cast<const act_t*>(X), ldx, reinterpret_cast<const act_t*>(Y), ldy, Mw, Nw, K, dW, ldw, scratch, cx);
}

int CC_API(cc_layernorm_fwd)(const float* x, const float* gamma, const float* beta, uint16_t* y, float* mean, float* rstd, int32_t rows, int32_t D,
                     void* stream) {
    if (!x || !gamma || !beta || !y) return CC_ERR_ARG;
    return ln_fwd(x, D, nullptr, gamma, beta, reinterpret_cast<act_t*>(y), nullptr, mean, rstd, rows, D, S_(stream));
}

// ---- reduction hooks: red_ws is the call's reduction scratch
int64_t CC_API(cc_red_scratch_floats)(void) { return (int64_t)RED_SCRATCH_FLOATS; }

int CC_API(cc_layernorm_bwd)(const uint16_t* dy, const float* x, int32_t ldx, const int32_t* row_map, const float* mean, const float* rstd,
                     const float* gamma, const float* dres, float* dx32, uint16_t* dx16, float* dgamma, float* dbeta, float* dcol, int32_t rows,
                     int32_t D, float* red_ws, void* stream) {
    // (bf16x3: dx16 would be fp32, or a 3-wide operand image when a GEMM asked for one: no bare hook)
    if (!dy || !x || !mean || !rstd || !gamma || !dx32 || !dgamma != !dbeta || kX3) return CC_ERR_ARG;
    Call cx{S_(stream), red_ws};
    return ln_bwd(reinterpret_cast<const act_t*>(dy), x, ldx, row_map, mean, rstd, gamma, dres, dx32, reinterpret_cast<act_t*>(dx16), dgamma,
                  dbeta, rows, D, cx, dcol);
}

int CC_API(cc_colsum_bf16)(const uint16_t* X, int32_t ld, int32_t M, int32_t N, float* out, float* red_ws, void* stream) {
    if (!X || !out || kX3) return CC_ERR_ARG;
    Call cx{S_(stream), red_ws};
    return colsum_bf16(reinterpret_cast<const act_t*>(X), ld, M, N, out, cx);
}

int CC_API(cc_colsum_multi)(const uint16_t* const* X_host, float* const* out_host, int32_t n, int32_t ld, int32_t M, int32_t N, float* red_ws,
                    void* stream) {
    if (!X_host || !out_host || n < 0 || n > 32 || kX3) return CC_ERR_ARG;
    ColsumBatch b;
    for (int i = 0; i < n; i++) {
        if (!X_host[i] || !out_host[i]) return CC_ERR_ARG;
        b.add(reinterpret_cast<const act_t*>(X_host[i]), out_host[i]);
    }
    Call cx{S_(stream), red_ws};
    return colsum_bf16_multi(b, ld, M, N, cx);
}

int CC_API(cc_batch_sum)(const float* src, int64_t src_stride, float* dst, int32_t len, int32_t B, float* red_ws, void* stream) {
    if (!src || !dst || len < 0 || src_stride < len) return CC_ERR_ARG;
    Call cx{S_(stream), red_ws};
    return batch_sum(src, (size_t)src_stride, dst, len, B, cx);
}

int CC_API(cc_attention_fwd)(const uint16_t* qkv, int32_t B, int32_t S, int32_t H, int32_t hd, int32_t causal, uint16_t* out, float* lse, void* stream) {
    if (!qkv || !out) return CC_ERR_ARG;
    return attn_fwd(reinterpret_cast<const act_t*>(qkv), B, S, H, hd, causal != 0, reinterpret_cast<act_t*>(out), lse, S_(stream));
}

int CC_API(cc_attention_bwd)(const uint16_t* qkv, const uint16_t* dout, const uint16_t* o, const float* lse, float* delta_ws, int32_t B, int32_t S,
                     int32_t H, int32_t hd, int32_t causal, uint16_t* dqkv, void* stream) {
    if (!qkv || !dout || !lse || !dqkv) return CC_ERR_ARG;
    return attn_bwd(reinterpret_cast<const act_t*>(qkv), reinterpret_cast<const act_t*>(dout), reinterpret_cast<const act_t*>(o), lse, delta_ws, B, S, H, hd,
                    causal != 0, reinterpret_cast<act_t*>(dqkv), S_(stream));
}

// ---- attention test hooks (tests/test_gpu_attention_ref.py): the same launchers with the call's Drop and Act handles built from arguments
int CC_API(cc_attention_fwd_x)(const uint16_t* qkv, int32_t B, int32_t S, int32_t H, int32_t hd, int32_t causal, uint16_t* out, int32_t out_img, float* lse,
                       float p, uint64_t seed, int32_t layer, void* stream) {
    if (!qkv || !out || !(p >= 0.f && p < 1.f) || layer < 0 || layer > 255 || out_img < 0 || (!kX3 && out_img)) return CC_ERR_ARG;
    return attn_fwd(reinterpret_cast<const act_t*>(qkv), B, S, H, hd, causal != 0, Act(reinterpret_cast<act_t*>(out), out_img), lse, S_(stream),
                    make_drop(p, seed, DROP_ATTN, (unsigned)layer));
}

int CC_API(cc_attention_bwd_x)(const uint16_t* qkv, const uint16_t* dout, const uint16_t* o, const float* lse, float* delta_ws, int32_t B, int32_t S,
                       int32_t H, int32_t hd, int32_t causal, uint16_t* dqkv, int32_t dqkv_img, float p, uint64_t seed, int32_t layer, void* stream) {
    if (!qkv || !dout || !lse || !dqkv || !(p >= 0.f && p < 1.f) || layer < 0 || layer > 255 || dqkv_img < 0 || (!kX3 && dqkv_img)) return CC_ERR_ARG;
    return attn_bwd(reinterpret_cast<const act_t*>(qkv), reinterpret_cast<const act_t*>(dout), reinterpret_cast<const act_t*>(o), lse, delta_ws, B, S, H, hd,
                    causal != 0, Act(reinterpret_cast<act_t*>(dqkv), dqkv_img), S_(stream), make_drop(p, seed, DROP_ATTN, (unsigned)layer));
}

// ---- GEMM wrapper hooks (tests/test_gpu_gemm_epilogues.py): one wrapper call each on caller buffers, the call's image scratch passed in
namespace {
inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
// what every NT hook checks before it builds its Call: operands present and 16-B aligned, leading dimensions cover the rows they stride
inline bool hook_operands_ok(int al, int bl, const void* A, int a_img, int lda, const void* B, int ldb, int M, int N, int K) {
    if (!A || !B || !al16(A) || !al16(B) || M <= 0 || N <= 0 || K <= 0 || a_img < 0) return false;
    if (!kX3 && a_img) return false;
    return lda >= (a_img ? 0 : (al ? M : K)) && ldb >= (bl ? N : K);
}
inline void hook_scratch(Call& cx, void* x3, int64_t x3_bytes) {
    if (kX3 && x3 && x3_bytes > 0 && al16(x3)) { cx.x3 = static_cast<char*>(x3); cx.x3_bytes = (size_t)x3_bytes; }
}
inline bool hook_c_img_ok(int c_img, int N) { return c_img == 0 || (kX3 && c_img == N); }
}  // namespace

int64_t CC_API(cc_x3_image_bytes)(int64_t rows, int64_t depth) {
    if (rows < 0 || depth < 0) return CC_ERR_ARG;
    return (int64_t)x3_img((size_t)rows, (size_t)depth);
}

int CC_API(cc_x3_split_rows)(const float* src, int64_t ld, int32_t rows, int32_t width, int32_t form, uint16_t* dst, void* stream) {
#if CC_OP == 2
    if (!src || !dst || rows < 0 || width < 0 || ld < width || (form != 0 && form != 1)) return CC_ERR_ARG;
    return x3_split_rows(src, (size_t)ld, dst, rows, width, form, S_(stream));
#else
    (void)src; (void)ld; (void)rows; (void)width; (void)form; (void)dst; (void)stream;
    return CC_ERR_ARG;
#endif
}

int CC_API(cc_gemm_act)(int32_t al, int32_t bl, const void* A, int32_t a_img, int32_t lda, const uint16_t* B, int32_t ldb, int32_t M, int32_t N, int32_t K,
                void* C, int32_t c_img, int32_t ldc, const float* bias, int32_t act, void* pre, void* x3, int64_t x3_bytes, void* stream) {
    if (!hook_operands_ok(al, bl, A, a_img, lda, B, ldb, M, N, K) || !C || !al16(C) || !al16(pre) || !al16(bias) || ldc < N || act < 0 || act > 3 ||
        !hook_c_img_ok(c_img, N))
        return CC_ERR_ARG;
    Call cx{S_(stream)};
    hook_scratch(cx, x3, x3_bytes);
    return gemm_bf16out(al, bl, ActIn(static_cast<const act_t*>(A), a_img), lda, B, ldb, M, N, K, Act(static_cast<act_t*>(C), c_img), ldc, bias, act,
                        static_cast<act_t*>(pre), cx);
}

int CC_API(cc_gemm_tanh)(int32_t al, int32_t bl, const void* A, int32_t a_img, int32_t lda, const uint16_t* B, int32_t ldb, int32_t M, int32_t N, int32_t K,
                 void* C, int32_t c_img, int32_t ldc, const float* bias, void* pre, int32_t pre_nt, void* x3, int64_t x3_bytes, void* stream) {
    if (!hook_operands_ok(al, bl, A, a_img, lda, B, ldb, M, N, K) || !C || !al16(C) || !al16(pre) || !al16(bias) || ldc < N || !hook_c_img_ok(c_img, N))
        return CC_ERR_ARG;
    Call cx{S_(stream)};
    hook_scratch(cx, x3, x3_bytes);
    return gemm_tanh(al, bl, ActIn(static_cast<const act_t*>(A), a_img), lda, B, ldb, M, N, K, Act(static_cast<act_t*>(C), c_img), ldc, bias,
                     static_cast<act_t*>(pre), pre_nt != 0, cx);
}

int CC_API(cc_gemm_resid)(int32_t al, int32_t bl, const void* A, int32_t a_img, int32_t lda, const uint16_t* B, int32_t ldb, int32_t M, int32_t N, int32_t K,
                  float* out, const float* res, int32_t ld, const float* bias, float p, uint64_t seed, int32_t site, int32_t layer, void* x3,
                  int64_t x3_bytes, void* stream) {
    if (!hook_operands_ok(al, bl, A, a_img, lda, B, ldb, M, N, K) || !out || !res || !al16(out) || !al16(res) || !al16(bias) || ld < N || site < 0 ||
        site > 3 || layer < 0 || layer > 255 || p < 0.f || p >= 1.f)
        return CC_ERR_ARG;
    Call cx{S_(stream)};
    hook_scratch(cx, x3, x3_bytes);
    return gemm_resid(al, bl, ActIn(static_cast<const act_t*>(A), a_img), lda, B, ldb, M, N, K, out, res, ld, bias, cx,
                      make_drop(p, seed, (unsigned)site, (unsigned)layer));
}

int CC_API(cc_gemm_dact)(int32_t al, int32_t bl, const void* A, int32_t a_img, int32_t lda, const uint16_t* B, int32_t ldb, int32_t M, int32_t N, int32_t K,
                 void* C, int32_t c_img, int32_t ldc, const void* aux, int32_t act, void* x3, int64_t x3_bytes, void* stream) {
    if (!hook_operands_ok(al, bl, A, a_img, lda, B, ldb, M, N, K) || !C || !aux || !al16(C) || !al16(aux) || ldc < N || act < 1 || act > 3 ||
        !hook_c_img_ok(c_img, N))
        return CC_ERR_ARG;
    Call cx{S_(stream)};
    hook_scratch(cx, x3, x3_bytes);
    return gemm_dact(al, bl, ActIn(static_cast<const act_t*>(A), a_img), lda, B, ldb, M, N, K, Act(static_cast<act_t*>(C), c_img), ldc,
                     static_cast<const act_t*>(aux), act, cx);
}

int CC_API(cc_gemm_f32)(int32_t al, int32_t bl, const void* A, int32_t a_img, int32_t lda, const uint16_t* B, int32_t ldb, int32_t M, int32_t N, int32_t K,
                float* C, int32_t ldc, const float* bias, int32_t mode, float alpha, int32_t ksplit, void* x3, int64_t x3_bytes, void* stream) {
    if (!hook_operands_ok(al, bl, A, a_img, lda, B, ldb, M, N, K) || !C || !al16(C) || !al16(bias) || ldc < N || mode < 0 || mode > 2 || ksplit < 1 ||
        (bias && mode != 0))
        return CC_ERR_ARG;
    Call cx{S_(stream)};
    hook_scratch(cx, x3, x3_bytes);
    return gemm_f32out(al, bl, ActIn(static_cast<const act_t*>(A), a_img), lda, B, ldb, M, N, K, C, ldc, bias, mode, alpha, ksplit, cx);
}

int CC_API(cc_gemm_wgrad_split)(const void* X, int32_t x_img, int32_t ldx, const float* Y, int32_t ldy, int32_t Mw, int32_t Nw, int32_t K, float* dW,
                     int32_t ldw, float* scratch, void* x3, int64_t x3_bytes, void* stream) {
#if CC_OP == 2
    if (!X || !Y || !dW || !al16(X) || !al16(Y) || !al16(dW) || Mw <= 0 || Nw <= 0 || K <= 0 || x_img < 0 || (!x_img && ldx < Mw) || ldy < Nw || ldw < Nw)
        return CC_ERR_ARG;
    Call cx{S_(stream)};
    hook_scratch(cx, x3, x3_bytes);
    return gemm_wgrad(ActIn(static_cast<const act_t*>(X), x_img), ldx, Y, ldy, Mw, Nw, K, dW, ldw, scratch, cx);
#else
    (void)X; (void)x_img; (void)ldx; (void)Y; (void)ldy; (void)Mw; (void)Nw; (void)K; (void)dW; (void)ldw; (void)scratch; (void)x3; (void)x3_bytes; (void)stream;
    return CC_ERR_ARG;
#endif
}

}  // extern "C"
