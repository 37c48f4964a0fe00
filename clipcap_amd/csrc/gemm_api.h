// Host entry points of the GEMM instantiations (one translation unit per epilogue so they build in parallel).
#pragma once
#include "common.hip.h"
#include "shared.h"

namespace CC_NS {
// NT tile choice (cc_shared::g_gemm_tile_mode): -1 chooser (default; CC_GEMM_S256 in the environment presets it), 0 = 128 x 128 only,
// 3 / 4 / 5 = force the 256 x 192 / 256 x 256 / 320 x 256 kernel wherever it is legal.  g_gemm_s64 > 0: route NT GEMMs with M <= 1024 through the 64-row
// skinny kernel (env CC_GEMM_S64); g_gemm_small_x2: small-grid NT GEMMs on the 8-wave kernel (env CC_GEMM_X2, default 1).  All three
// are test / microbenchmark hooks living in shared.cpp.
// al/bl: 0 = K-contiguous operand ([rows][K]), 1 = K-strided operand ([K][rows]).  See gemm.hip.h.
//
// Operand types.  A is an ACTIVATION (ActIn), B a WEIGHT from the 16-bit operand arena, C / pre / aux activations again.  In the bf16 /
// fp16 builds act_t is the 16-bit operand type and the calls are what they say.  In the bf16x3 build (common.hip.h) activations are
// fp32: a wrapper splits a plain A (A.img == 0) into its [hi | hi | lo] operand image in the call's scratch (Call::x3) and reads an A
// that already is that image (A.img == K) in place; B is the pre-split [hi | lo | hi] image the weight sync left in the operand arena
// (row stride 3 * ldb), and the unchanged NT kernels run with K' = 3 K.  Callers pass the LOGICAL lda / ldb / K in every build.
// Only al = bl = 0 is supported there.  An output C with C.img == n leaves the epilogue as the image of an n-deep A operand (epi_store8).
int gemm_bf16out(int al, int bl, ActIn A, int lda, const op16_t* B, int ldb, int M, int N, int K, Act C, int ldc,
                 const float* bias, int act, act_t* pre, Call& cx);
// C = h = tanh(A B^T + bias); pre (nullable, plain [M][ldc]) = 1 - h^2 from the fp32 h; pre_nt: only a backward pass reads it (gemm.hip.h EpiTanh)
int gemm_tanh(int al, int bl, ActIn A, int lda, const op16_t* B, int ldb, int M, int N, int K, Act C, int ldc,
              const float* bias, act_t* pre, bool pre_nt, Call& cx);
int gemm_resid(int al, int bl, ActIn A, int lda, const op16_t* B, int ldb, int M, int N, int K, float* out, const float* res,
               int ld, const float* bias, Call& cx, Drop drop = Drop());
// mode 0 store (+bias), 1 add, 2 atomic add (required when ksplit > 1)
int gemm_f32out(int al, int bl, ActIn A, int lda, const op16_t* B, int ldb, int M, int N, int K, float* C, int ldc,
                const float* bias, int mode, float alpha, int ksplit, Call& cx);
int gemm_dact(int al, int bl, ActIn A, int lda, const op16_t* B, int ldb, int M, int N, int K, Act C, int ldc,
              const act_t* aux, int act, Call& cx);
// cref != nullptr: exponential form (C = exp(logit - cref[row]), see gemm.hip.h EpiLMHead); only that form writes C as an image
int gemm_lmhead(ActIn A, int lda, const op16_t* B, int ldb, int M, int Vp, int V, int K, Act C, int ldc, float* pmax,
                float* psum, int npart, const int* target, float* tgt_logit, Call& cx, const float* cref = nullptr);
// scoring lm_head (forward only): the same partials over the V real columns and the exact target logit, and no C at all — gemm.hip.h
// EpiLMHeadScore.  pmax / psum [M][npart] (npart >= Vp / 64), target / tgt_logit [M].
int gemm_lmhead_score(ActIn A, int lda, const op16_t* B, int ldb, int M, int Vp, int V, int K, float* pmax, float* psum, int npart,
                      const int* target, float* tgt_logit, Call& cx);

// decode lm_head: fp32 logits [M][ldc] (Ns columns stored, Ns % 8 == 0) + per-(row, 64-column block) softmax partials over the V real
// columns (pmax / psum [M][npart], npart >= ceil(Ns / 64)) — gemm.hip.h EpiLogits
int gemm_logits_part(ActIn A, int lda, const op16_t* B, int ldb, int M, int Ns, int V, int K, float* C, int ldc, float* pmax, float* psum,
                     int npart, Call& cx);

#if CC_OP == 2
// split `rows` x `width` fp32 (row stride ld) into the call's image scratch: form 0 = [hi | hi | lo] (A side), 1 = [hi | lo | hi] (B side).
// first = true restarts the scratch (one GEMM's operands live there at a time; stream order makes reuse by the next GEMM safe).
// Returns nullptr (rc set, CC_ERR_STATE) when the call has no scratch or the image does not fit.
const op16_t* x3_operand(Call& cx, const float* src, size_t ld, int rows, int width, int form, bool first, int* rc);
#endif
// the whole image scratch as one block, for a producer kernel that writes the next GEMM's A image itself; nullptr when it does not fit
inline op16_t* x3_scratch_block(const Call& cx, size_t bytes) { return (cx.x3 && bytes <= cx.x3_bytes) ? reinterpret_cast<op16_t*>(cx.x3) : nullptr; }
// The A operand of an NT wrapper as its kernel reads it (A16; lda / ldb / K become the image's in the bf16x3 build).
inline int nt_operand(Call& cx, ActIn A, int al, int bl, int M, int& lda, int& ldb, int& K, const op16_t*& A16) {
#if CC_OP == 2
    if (al || bl || (A.img && A.img != K)) return CC_ERR_ARG;
    if (A.img) {
        A16 = reinterpret_cast<const op16_t*>(A.p);
    } else {
        int rc = CC_OK;
        A16 = x3_operand(cx, A.p, (size_t)lda, M, K, 0, true, &rc);
        if (!A16) return rc;
    }
    lda = 3 * K; ldb = 3 * ldb; K = 3 * K;
#else
    if (A.img) return CC_ERR_ARG;
    A16 = A.p;
#endif
    return CC_OK;
}
// weight gradient dW[Mw][Nw] += X^T Y with X stored [K][Mw], Y stored [K][Nw].  Split-K for occupancy: the K slices
// write fp32 slabs into `scratch` (plain stores) and a second kernel folds them into dW — fp32 atomics on the same
// tile from 7-14 concurrent blocks measured 3x slower than the whole GEMM (profiles/r01_b_gemm_microbench.md).
constexpr size_t WGRAD_SCRATCH_BYTES = size_t(96) << 20;
// Several weight gradients of one layer can share one slab-reduce launch: pass a WgradBatch, each gemm_wgrad then parks its slabs
// in its own part of `scratch` and wgrad_flush() folds all of them into their dW targets (8 launches per mapper backward instead
// of 32).  A gradient whose slabs do not fit behind the parked ones flushes the batch first.
struct WgradBatch {
    struct Item { const float* slabs; size_t slab; int ks, Nw; float* dW; int ldw; size_t n4; };
    Item it[8];
    int n = 0;
    size_t used = 0;      // bytes of scratch already holding parked slabs
    // defer = true: weight gradients that fit the 128 x 128 TT kernel are not launched by gemm_wgrad but collected (up to 4, same K)
    // and run by wgrad_flush as ONE grouped launch (gemm_tt_glds4_group_kernel) + one slab reduce.  The caller must keep every
    // operand unchanged until the flush.
    bool defer = false;
    struct Deferred { const op16_t* X; const op16_t* Y; int ldx, ldy, Mw, Nw, K; float* dW; int ldw; };      // (never used in the bf16x3 build: operands are split per call)
    Deferred d[32];
    int nd = 0;
    int cap = 4;          // deferred problems per grouped launch (<= 32)
    // direct = true (round 5; with defer): the deferred problems run as ONE launch with a single K slice per tile that adds into dW in its
    // epilogue — no slabs, no reduce launch; meant for many problems at once (all layers of a mapper backward: 576 tiles of 256 x 256),
    // where whole-K tiles still fill the CUs.  The caller keeps every operand unchanged until the flush.
    bool direct = false;
    float* scratch = nullptr;
};
int wgrad_flush(WgradBatch& b, hipStream_t st);
// bf16x3: X and Y are split into the call's image scratch; an X that already is its [hi | hi | lo] image (X.img == Mw: the form the
// input-gradient GEMM of the same tensor reads as its A operand, split once for both) is read in place.
int gemm_wgrad(ActIn X, int ldx, const act_t* Y, int ldy, int Mw, int Nw, int K, float* dW, int ldw, float* scratch,
               Call& cx, WgradBatch* batch = nullptr);
// Skinny-M NT GEMMs (KV-cached decode: M = beams x samples, a handful of 128x128 tiles): split K over blockIdx.z so every CU
// streams a distinct slice of the weights, fp32 slabs in `scratch`, then ONE finishing kernel sums the slabs and applies the
// epilogue (bias, gelu_new, fp32 residual, bf16 / fp32 stores).  Falls back to the single-pass GEMM when the grid is already wide.
// Optional fused tails of the finishing kernel (decode): LayerNorm of the finished fp32 row (N == row width) -> bf16, and the
// append of the K / V thirds of a finished qkv row to the KV cache.
struct SkinnyFuse {
    const float* ln_gamma = nullptr;   // LayerNorm over the N columns of (acc + bias + res): out -> ln_out16 [M, N]
    const float* ln_beta = nullptr;
    act_t* ln_out16 = nullptr;
    act_t* kcache = nullptr;           // qkv rows (N == 3*D): columns [D,2D) -> kcache, [2D,3D) -> vcache at (r*ctx_max + pos0 + t)*D
    act_t* vcache = nullptr;
    int Tn = 1, pos0 = 0, ctx_max = 0;
    const op16_t* bimg = nullptr;      // the weight's fragment-ordered image (k_skinny_image; cc_decode_image): B is then loaded global -> VGPR where the form allows
};
int skinny_image(const op16_t* W, op16_t* img, int N, int K, hipStream_t st);
int gemm_nt_skinny(ActIn A, int lda, const op16_t* B, int ldb, int M, int N, int K, const float* bias, int act, const float* res,
                   float* out32, act_t* out16, int ldo, float* scratch, size_t scratch_bytes, Call& cx,
                   const SkinnyFuse* fuse = nullptr);
// Narrow output, very deep K (the lm_head input gradient: [B*cap, Vp] x [Vp, D] -> 10240 x 768 over K = 50304): the 256 x 256 kernel on
// 120 tiles leaves half the chip idle, so K is cut into as many slices as fill the CUs (fp32 slabs in `scratch`), and one elementwise
// pass sums the slabs into the 16-bit output.  Returns CC_ERR_SHAPE when the shape does not call for it (caller then uses gemm_bf16out).
// fix (optional): out[m][n] = fac[2m] * acc - fac[2m+1] * wte[target[m]][n] — the lm_head input gradient of the exponential form
struct LmFix { const float* fac; const int* target; const op16_t* wte; };
int gemm_nt_deepk(ActIn A, int lda, const op16_t* B, int ldb, int M, int N, int K, act_t* out16, int ldo, float* scratch,
                  size_t scratch_bytes, Call& cx, const LmFix* fix = nullptr);
int skinny_single_min_tiles();   // grids of at least this many 128 x 128 tiles skip split-K (CC_SKINNY_SINGLE; tuning knob)
// whether gemm_nt_skinny will take the slab + row-finish path for this problem (the only path that supports SkinnyFuse)
bool gemm_nt_skinny_can_fuse(int M, int N, int K, size_t scratch_bytes);
}  // namespace CC_NS
