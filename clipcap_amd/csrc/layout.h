// Host-only: where every tensor of the two models sits in its parameter arena, which configs the entry points accept, and the few helpers
// the host orchestration (api.hip, decode.hip) shares.  This is the ONLY place that knows the arena layouts: everything else asks.
#pragma once
#include "../../include/clipcap_hip.h"
#include "common.hip.h"
#include <cstring>

#define CC_TRY(expr)                 \
    do {                             \
        int _e = (expr);             \
        if (_e != CC_OK) return _e;  \
    } while (0)

namespace CC_NS {

constexpr int MAX_LAYERS = 96;       // per-layer pointer tables of the training workspaces (MapperWS / Gpt2WS)

inline hipStream_t S_(void* s) { return static_cast<hipStream_t>(s); }
inline int rup(int x, int m) { return (x + m - 1) / m * m; }

// Operand arena addressing.  16-bit builds: w16[off] is the cast of w32[off], w16[total + off] the transposed copy.  bf16x3 build: every
// 2-D GEMM weight [R][C] at element offset off owns 3*R*C operand elements at 3*off — rows [hi | lo | hi] of 3C (the B-operand image,
// common.hip.h) — and its transposed image [C][3R] at 3*(total + off); the arena has 6*total elements (1-D tensors leave holes).
constexpr int PL = kX3 ? 3 : 1;
inline const uint16_t* W16(const uint16_t* w16, int64_t off) { return w16 + (size_t)PL * off; }
inline uint16_t* W16(uint16_t* w16, int64_t off) { return w16 + (size_t)PL * off; }
// bf16x3: bytes of operand-image scratch for GEMMs whose largest A image is rows x depth (x3_operand rounds each image up to 256 B)
inline size_t x3_img(size_t rows, size_t depth) { return ((rows * 3 * depth * sizeof(op16_t)) + 255) & ~size_t(255); }

// Workspace carving: consecutive buffers, each starting on a 256-byte boundary; a null base only measures.
struct Carver {
    char* base;
    size_t off = 0;
    explicit Carver(void* p) : base(static_cast<char*>(p)) {}
    template <class T>
    T* take(size_t n) {
        off = (off + 255) & ~size_t(255);
        T* r = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += n * sizeof(T);
        return r;
    }
    size_t bytes() const { return (off + 255) & ~size_t(255); }
};

// A layer record is twelve element offsets in arena order; cc_*_param_offsets hand them out in exactly this order (engine.py names them).
template <class Layer>
inline int64_t* put_layer(int64_t* dst, const Layer& y) {
    static_assert(sizeof(Layer) == 12 * sizeof(int64_t), "a layer record is twelve offsets");
    std::memcpy(dst, &y, sizeof y);
    return dst + 12;
}

// ------------------------------------------------------------------------------------------------------------
// mapper arena: linear.weight, linear.bias, prefix_const, [pos_embeddings], N uniform layers
// ------------------------------------------------------------------------------------------------------------
struct MapperOff {
    struct Layer {
        int64_t n1w, n1b, wq, wkv, wp, bp, n2w, n2b, w1, b1, w2, b2;
    };
    int64_t D, Hm;
    int64_t lin_w, lin_b, prefix, pos;      // pos = -1: no learned position embeddings
    int64_t layer0, layer_stride, total;
    explicit MapperOff(const cc_mapper_cfg* c) : D(c->D), Hm(c->Hm) {
        int64_t p = 0;
        const int64_t PD = (int64_t)c->P * D;
        lin_w = p; p += PD * c->E;
        lin_b = p; p += PD;
        prefix = p; p += (int64_t)c->L * D;
        if (c->W > 1 && c->use_pos) { pos = p; p += (int64_t)c->W * PD; } else pos = -1;
        layer0 = p;
        walk(p);
        layer_stride = p - layer0;
        total = layer0 + c->N * layer_stride;
    }
    Layer layer(int l) const {
        int64_t p = layer0 + l * layer_stride;
        return walk(p);
    }

private:
    Layer walk(int64_t& p) const {      // the one place that orders a layer's tensors; leaves p behind the layer
        Layer y;
        y.n1w = p; p += D;
        y.n1b = p; p += D;
        y.wq = p; p += D * D;
        y.wkv = p; p += 2 * D * D;
        y.wp = p; p += D * D;
        y.bp = p; p += D;
        y.n2w = p; p += D;
        y.n2b = p; p += D;
        y.w1 = p; p += Hm * D;
        y.b1 = p; p += Hm;
        y.w2 = p; p += D * Hm;
        y.b2 = p; p += D;
        return y;
    }
};

inline bool mapper_cfg_ok(const cc_mapper_cfg* c) {
    return c && (c->op_dtype == CC_OP) && c->E > 0 && c->D > 0 && c->P > 0 && c->L > 0 && c->H > 0 && c->N >= 0 && c->N <= MAX_LAYERS && c->Hm > 0 && c->W >= 1 &&
           (c->E % 8) == 0 && (c->D % 8) == 0 && (c->Hm % 8) == 0 && (c->D % c->H) == 0 && ((c->D / c->H) % 8) == 0;
}

// ------------------------------------------------------------------------------------------------------------
// MLP mapper arena: model.0.weight [Hd][E], model.0.bias [Hd], model.2.weight [L D][Hd], model.2.bias [L D]
// ------------------------------------------------------------------------------------------------------------
struct MlpOff {
    int64_t w1, b1, w2, b2, total;
    explicit MlpOff(const cc_mlp_cfg* c) {
        const int64_t LD = (int64_t)c->L * c->D;
        w1 = 0;
        b1 = w1 + (int64_t)c->Hd * c->E;
        w2 = b1 + c->Hd;
        b2 = w2 + LD * c->Hd;
        total = b2 + LD;
    }
};
// (Hd % 8 == 0 with Hd == L D / 2 exactly makes L D a multiple of 16; every tensor then starts on a 16-byte boundary in both arenas)
inline bool mlp_cfg_ok(const cc_mlp_cfg* c) {
    return c && (c->op_dtype == CC_OP) && c->E > 0 && c->D > 0 && c->L > 0 && c->Hd > 0 && (c->E % 8) == 0 && (c->D % 8) == 0 && (c->Hd % 8) == 0 &&
           (int64_t)c->L * c->D == 2 * (int64_t)c->Hd && (int64_t)c->L * c->D <= (int64_t)1 << 24;
}

// ------------------------------------------------------------------------------------------------------------
// GPT-2 arena: wte [Vp, D], wpe [NPOS, D], NL uniform layers, ln_f — O(1) to build: the decode step builds one per generated position
// ------------------------------------------------------------------------------------------------------------
struct Gpt2Off {
    struct Layer {
        int64_t l1w, l1b, aw, ab, pw, pb, l2w, l2b, fw, fb, p2w, p2b;
    };
    int64_t D;
    int64_t wte, wpe, layer0, layer_stride, lnf_w, lnf_b, total;
    explicit Gpt2Off(const cc_gpt2_cfg* c) : D(c->D) {
        wte = 0;
        wpe = wte + (int64_t)c->Vp * D;
        layer0 = wpe + (int64_t)c->NPOS * D;
        int64_t p = layer0;
        walk(p);
        layer_stride = p - layer0;
        lnf_w = layer0 + c->NL * layer_stride;      // directly behind the last layer: decode's fused "next LayerNorm" finish relies on it
        lnf_b = lnf_w + D;
        total = lnf_b + D;
    }
    Layer layer(int l) const {
        int64_t p = layer0 + l * layer_stride;
        return walk(p);
    }

private:
    Layer walk(int64_t& p) const {      // the one place that orders a layer's tensors; leaves p behind the layer
        Layer y;
        y.l1w = p; p += D;
        y.l1b = p; p += D;
        y.aw = p; p += D * 3 * D;
        y.ab = p; p += 3 * D;
        y.pw = p; p += D * D;
        y.pb = p; p += D;
        y.l2w = p; p += D;
        y.l2b = p; p += D;
        y.fw = p; p += D * 4 * D;
        y.fb = p; p += 4 * D;
        y.p2w = p; p += 4 * D * D;
        y.p2b = p; p += D;
        return y;
    }
};

// the GPT-2 dims every entry point needs; the decode side asks for nothing more (it keeps no per-layer tables and checks positions per call)
inline bool gpt2_dims_ok(const cc_gpt2_cfg* c) {
    return c && (c->op_dtype == CC_OP) && c->D > 0 && c->H > 0 && c->NL > 0 && c->V > 0 && c->Vp >= c->V && (c->Vp % 128) == 0 && (c->D % 8) == 0 && (c->D % c->H) == 0 &&
           ((c->D / c->H) % 8) == 0;
}
// the training / scoring side: per-layer tables of MAX_LAYERS entries, and a position table to embed from
inline bool gpt2_cfg_ok(const cc_gpt2_cfg* c) { return gpt2_dims_ok(c) && c->NL <= MAX_LAYERS && c->NPOS > 0; }

}  // namespace CC_NS
