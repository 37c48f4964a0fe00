// Host-side launchers of the non-GEMM kernels (definitions in kernels.hip / layernorm.hip / reduce.hip / loss.hip / attention.hip; the
// gradient utilities of grads.hip are reached through their entry points only).  Internal to the library.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include "common.hip.h"

namespace CC_NS {

// grid of a grid-stride launch over `total` items: per_block items per block, at most `cap` blocks
inline dim3 flat_grid(size_t total, int per_block, int cap) { return dim3((unsigned)std::min<size_t>((total + per_block - 1) / per_block, cap)); }

int f32_to_bf16(const float* src, op16_t* dst, size_t n, hipStream_t st);      // 16-bit operand cast (weights)
int f32_to_act(const float* src, act_t* dst, size_t n, hipStream_t st);         // fp32 -> stored-activation type (a copy in the bf16x3 build)
int slice_f32_to_bf16(const float* src, size_t src_stride, act_t* dst, size_t dst_stride, int len, int B, hipStream_t st);
int broadcast_rows(float* dst, size_t dst_stride, const float* src, int len, int B, hipStream_t st);
int add_rows(float* dst, size_t dst_stride, const float* add, int len, int B, hipStream_t st);
// Reductions across blocks (batch_sum, ln_bwd's parameter gradients, colsum_bf16*) write per-block partials into the call's reduction
// scratch and fold them in a fixed order, so a gradient is the same bit for bit from run to run (fp32 atomics are not).  They take the
// Call, whose `red` is RED_SCRATCH_FLOATS floats of the entry point's workspace; when they need it and it is null: CC_ERR_STATE.
constexpr size_t RED_SCRATCH_FLOATS = size_t(1) << 20;
int batch_sum(const float* src, size_t src_stride, float* dst, int len, int B, Call& cx);
// internal to the reductions (reduce.hip; ln_bwd in layernorm.hip folds its parameter-gradient partials the same way): partials
// part[y][s][j] (y < groups, S slices x n columns) are added onto out[y * k + j / m][j % m] in the fixed order k_fold_partials states
struct FoldOut { float* p[32]; int m; int k; };
inline float* red_scratch(const Call& cx, size_t floats) { return floats <= RED_SCRATCH_FLOATS ? cx.red : nullptr; }
int fold_partials(const float* part, int S, int n, int groups, const FoldOut& o, hipStream_t st);
int copy_rows(const float* src, size_t src_stride, float* dst, size_t dst_stride, int len, int B, hipStream_t st);

int transpose_bf16(const op16_t* src, op16_t* dst, int R, int C, hipStream_t st);
struct TransposeBatch {
    struct Item { const op16_t* src; op16_t* dst; int R, C; };
    Item it[32];
    int n = 0;
    void add(const op16_t* s, op16_t* d, int R, int C) { it[n++] = Item{s, d, R, C}; }
};
int transpose_bf16_multi(const TransposeBatch& b, hipStream_t st);   // up to 32 matrices in one launch

// Outputs of type Act (common.hip.h): a handle with img != 0 is written as the operand image of the GEMM that reads it (bf16x3 build);
// a producer that cannot do that for the shape it is given returns CC_ERR_STATE (ln_bwd with dcol / dmask / ldx != D, attn_* outside
// attn_*_can_image).
int ln_fwd(const float* x, int ldx, const int* row_map, const float* gamma, const float* beta, Act y, float* y32, float* mean,
           float* rstd, int rows, int D, hipStream_t st);
int ln_bwd(const act_t* dy, const float* x, int ldx, const int* row_map, const float* mean, const float* rstd, const float* gamma,
           const float* dres, float* dx32, Act dx16, float* dgamma, float* dbeta, int rows, int D, Call& cx,
           float* dcol = nullptr, Drop dmask = Drop());
// dcol (needs dgamma, dx16, no row_map): += column sums of the 16-bit dx16 (a bias gradient).  dmask: dropout mask applied to the
// 16-bit copy dx16 only (element index row * D + col; dx32 stays unmasked) — the residual dropout of the c_proj that consumes dx16.
int colsum_bf16(const act_t* X, int ld, int M, int N, float* out, Call& cx);
struct ColsumBatch { const act_t* X[32]; float* out[32]; int n = 0; void add(const act_t* x, float* o) { X[n] = x; out[n] = o; n++; } };
int colsum_bf16_multi(const ColsumBatch& b, int ld, int M, int N, Call& cx);      // out[i][c] += sum_r X[i][r][c] for n equally shaped matrices, one launch

int attn_probs(const act_t* qkv, int B, int S, int H, int hd, float* out, hipStream_t st);
int attn_fwd(const act_t* qkv, int B, int S, int H, int hd, bool causal, Act out, float* lse, hipStream_t st, Drop drop = Drop());
// o: forward output (for delta = rowsum(dO*O)); delta: fp32 scratch [B*H*S].  Both may be null -> VALU kernel.
int attn_bwd(const act_t* qkv, const act_t* dout, const act_t* o, const float* lse, float* delta, int B, int S, int H, int hd, bool causal,
             Act dqkv, hipStream_t st, Drop drop = Drop());
// in-place dropout of an fp32 / bf16 buffer of n elements (n % 4 == 0 / n % 8 == 0): x[i] *= keep(i) / (1 - p)
bool attn_fwd_can_image(int S, int hd);      // bf16x3: attn_fwd can write `out` as an operand image (and the backward will not need the fp32 output)
bool attn_bwd_can_image(int S, int hd);      // bf16x3: attn_bwd can write dqkv as an operand image for this shape
int dropout_f32(float* x, size_t n, Drop drop, hipStream_t st);
int dropout_bf16(act_t* x, size_t n, Drop drop, hipStream_t st);
int dropout_mask_u8(unsigned char* out, size_t n, Drop drop, hipStream_t st);   // test hook: out[i] = keep(i)

int embed_concat(const float* prefix, const long long* tokens, int cap, const float* wte, const float* wpe, float* x0, int B, int L,
                 int T, int D, int pos0, hipStream_t st);
int f32_to_op16_pad(const float* src, long long lds, int V, act_t* dst, int ldd, int M, hipStream_t st);
// Deterministic token-indexed scatter-add (no atomics): dst[id(r)][:] += value(r)[:] for rows r < R, bit for bit the same from run to
// run.  Row values: f32 set: value(r)[d] = f32[(r / rpb) * bstride + (r % rpb) * D + d];  act set: value(r)[d] = fl(-fac[2r+1] * act[r*D+d])
// (the one-hot term of the exponential-form lm_head), rows with fac[2r+1] == 0 left out of every list.  Ids from ids32 or ids64,
// id(r) = min(max(ids[(r / rpb) * ids_ld + r % rpb], 0), Vp - 1).  The order, exactly (a float32 emulation reproduces it bit for bit):
//   * the list of id i = its rows in ascending row order; its k-th chunk = list entries [k*SCATTER_CHUNK, (k+1)*SCATTER_CHUNK);
//   * a chunk's sum, per column: s = value(first row); s = s + value(next row) for each further row in list order (fp32, no fused
//     multiply-add with the products above);
//   * a list of one chunk: dst[i] = dst[i] + s_0;  of nk > 1 chunks: t = s_0; t = t + s_k for k = 1 .. nk-1; dst[i] = dst[i] + t.
// Ids without rows are untouched.  ws: scatter_ws_bytes(R, D) bytes of device scratch for this call (the inverted index and the chunk
// partials, rebuilt by every call; nothing survives it); without it, CC_ERR_STATE.  D % 4 == 0.
constexpr int SCATTER_CHUNK = 512;
constexpr unsigned SC_SKIP = 0xffffffffu;       // id field of a left-out row's key: sorted after every list, summed by none
struct ScatterSrc {
    const int* ids32 = nullptr;
    const long long* ids64 = nullptr;
    const float* f32 = nullptr;
    size_t bstride = 0;
    int rpb = 1;
    size_t ids_ld = 1;
    const act_t* act = nullptr;
    const float* fac = nullptr;
};
size_t scatter_ws_bytes(int R, int D);
int scatter_rows(const ScatterSrc& s, int R, int D, int Vp, float* dst, void* ws, hipStream_t st);

// Per-row loss weights (cc_lmhead_ce_fwd_w / _bwd_w): the one place that turns "kept" into a factor.  A row that is not kept (target 0)
// gets 0 by selection, so neither x nor the bits of its weight (NaN, inf) reach anything; a kept row gets x * rw[row] (WT) or x.
// rw == 1.0 gives the bits of the form without weights.  The row_weight arguments below: nullptr launches the <false> forms, what the entry points
// without weights launch.
#ifdef __HIPCC__
template <bool WT>
__device__ __forceinline__ float row_factor(int target, float x, const float* __restrict__ rw, int row) {
    if (target == 0) return 0.f;
    return WT ? x * rw[row] : x;
}
#endif
// row_weight: stats has 3 floats, [sum of rw * row_loss over the kept rows, kept rows, the plain sum]; row_loss stays the plain row loss
int ce_rows(const float* pmax, const float* psum, int npart, const int* target, const float* tgt_logit, float* lse, float* row_loss,
            float* stats, int M, hipStream_t st, const float* row_weight = nullptr);
// scoring: token_logprob[row] = keep[row] ? tgt_logit[row] - lse[row] : 0 (lse folded exactly as ce_rows does), then per sample
// sample_stats[b] = {sum over its cap rows, kept count} in a fixed order (bit-identical from run to run)
int score_rows(const float* pmax, const float* psum, int npart, const int* keep, const float* tgt_logit, float* lse, float* token_logprob,
               float* sample_stats, int B, int cap, hipStream_t st);
int ce_dlogits(act_t* logits, int ld, int V, const int* target, const float* lse, const float* denom, const float* loss_scale, int M,
               hipStream_t st, op16_t* img = nullptr,    // img (bf16x3): write the gradient as the dgrad GEMM's operand image there instead of in place
               const float* row_weight = nullptr);       // row_weight: the factor's MAGNITUDE goes into the gradient; its sign: lm_rowsign
int ce_targets(const long long* tokens, int* target, int* row_map, int B, int cap, int L, int T, hipStream_t st);
int score_keep(const long long* tokens, int* keep, int n, int ignore_zero, hipStream_t st);   // keep[i] = tokens[i] >= 0 (&& != 0 with ignore_zero)
// Exponential form of the lm_head outputs (gemm.hip.h EpiLMHead, bf16 build):
//   lm_tgt_ref   cref[m] = hf[m] . wte[target[m]]  (16-bit operands, fp32 accumulate): the reference shift of row m
//   lm_rowfac    fac[m] = {r, w}: w = (target[m] != 0) * loss_scale / max(denom, 1) (* row_weight[m]), r = exp(cref[m] - lse[m]) * w
//   lm_dgrad_fix dhf[m][:] = r dhf[m][:] - w wte[target[m]][:]  (the path whose GEMM has no finishing pass of its own)
//   lm_scale_rows out[m][:] = r hf[m][:] (weight-gradient operand);  the one-hot term dwte[target[m]][:] -= w hf[m][:] is scatter_rows' act form
int lm_tgt_ref(const act_t* hf, const op16_t* wte, int D, const int* target, float* cref, int M, hipStream_t st);
int lm_rowfac(const float* cref, const float* lse, const int* target, const float* denom, const float* loss_scale, float* fac, int M, hipStream_t st,
              const float* row_weight = nullptr);
//   lm_rowsign   logit form with row weights: fac[m] = {s, 0}, s = the sign of row m's factor (+1 for 0 and for rows that are not kept): ce_dlogits
//                then writes d logits with the factor's magnitude, and lm_scale_rows(_inplace) puts s onto d hf and onto the hf rows
//                of the weight-gradient GEMM, so that a negated weight gives the negated row bit for bit
int lm_rowsign(const int* target, const float* denom, const float* loss_scale, const float* row_weight, float* fac, int M, hipStream_t st);
int lm_dgrad_fix(act_t* dhf, const float* fac, const int* target, const op16_t* wte, int D, int M, hipStream_t st);
int lm_scale_rows(const act_t* hf, const float* fac, act_t* out, int D, int M, hipStream_t st);
int lm_scale_rows_inplace(act_t* x, const float* fac, int D, int M, hipStream_t st);      // x[m][:] = r x[m][:]

// Label smoothing around the chain above (smooth.hip; include/clipcap_hip.h cc_lmhead_ce_fwd_smooth for the algebra).  wte: the rows as
// they are read elementwise ([V][D] of the operand image; bf16x3: of the fp32 master).  All sums in a fixed order, no atomics.
//   smooth_wbar       wbar[d] = (sum over v < V of wte[v][d]) / V: slice partials in part (smooth_wbar_slices(V) * D floats), then folded in one fixed order
//   smooth_rows       zbar[m] = hf[m] . wbar; term[m] = target[m] != 0 ? eps (tgt[m] - zbar[m]) : 0; stats3[2] = stats3[0], stats3[0] += sum of term
//   smooth_dhf        coef[m] = {0, -c_m}, c_m = (target[m] != 0) eps loss_scale / max(denom, 1); dhf[m][:] += c_m (wte[target[m]][:] - wbar[:])
//   smooth_dwte_bcast hsum[:] = sum of c_m hf[m][:] (partials in the call's reduction scratch, fold_partials); dwte[v][:] -= hsum[:] / V, v < V
//                     (the other half, dwte[target[m]][:] += c_m hf[m][:], is scatter_rows' act form fed coef)
// row_weight (smooth_rows, smooth_dhf): term[m] and c_m times row_weight[m] on kept rows; smooth_rows then leaves stats3[2] as ce_rows wrote it
inline int smooth_wbar_slices(int V) { return std::max(1, std::min((V + 127) / 128, 256)); }
int smooth_wbar(const act_t* wte, int V, int D, float* part, float* wbar, hipStream_t st);
int smooth_rows(const act_t* hf, const float* wbar, int D, const int* target, const float* tgt, float eps, float* zbar, float* term,
                float* stats3, int M, hipStream_t st, const float* row_weight = nullptr);
int smooth_dhf(act_t* dhf, const int* target, const float* denom, const float* loss_scale, float eps, const act_t* wte, const float* wbar,
               float* coef, int D, int M, hipStream_t st, const float* row_weight = nullptr);
int smooth_dwte_bcast(const act_t* hf, const float* coef, int D, int M, int V, float* hsum, float* dwte, Call& cx);

int adamw(float* p, const float* g, float* m, float* v, size_t n, float lr, float b1, float b2, float eps, float wd, int step, float gscale,
          const float* loss_scale, const float* found_inf, hipStream_t st, op16_t* w16 = nullptr,   // w16: also store the 16-bit copy of the updated parameters
          const float* clip = nullptr,            // clip (device, nullable): the gradient is also multiplied by clip[0] (grad_clip_coef)
          float* ema = nullptr, float ema_decay = 0.f);      // ema (device, nullable, n floats, not aliasing p): ema = d * ema + (1 - d) * p after an applied step
// grad_sqnorm (grads.hip, behind cc_grad_sqnorm): sumsq[0] += sum of g[i]^2, i < n (n % 4 == 0), bit for bit the same from run to run
// and from box to box: the grid depends on n alone.
// scratch: GRAD_NORM_BLOCKS floats of device scratch for this call.  The order, with n4 = n / 4 float4 groups,
// nb = min(ceil(n4 / GRAD_NORM_THREADS), GRAD_NORM_BLOCKS) blocks and S = nb * GRAD_NORM_THREADS:
//   * group i contributes q_i = (x*x + y*y) + (z*z + w*w) of its four elements (at most 3 roundings on an element's way in);
//   * thread T = block * GRAD_NORM_THREADS + lane visits groups T, T + S, T + 2S, ...; visit k is added to accumulator k % GRAD_NORM_ACC
//     (each starts at 0, visits in ascending k): an accumulator takes at most ceil(ceil(n4 / S) / GRAD_NORM_ACC) additions;
//   * thread sum = (a0 + a1) + (a2 + a3) (2 levels); wave sum = common.hip.h wave_sum (6 levels); block partial =
//     (w0 + w1) + (w2 + w3) over its four waves (2 levels);
//   * fold (one block): thread t adds partials [4t, 4t + 4) below nb in index order to 0 (GRAD_NORM_BLOCKS / GRAD_NORM_THREADS
//     additions), then wave_sum (6 levels) and (w0 + w1) + (w2 + w3) (2 levels); thread 0: sumsq[0] = sumsq[0] + total (1).
constexpr int GRAD_NORM_BLOCKS = 1024;
constexpr int GRAD_NORM_THREADS = 256;
constexpr int GRAD_NORM_ACC = 4;

// bf16x3 build: GEMM operand pairs (common.hip.h).  dst[r][0:3K] = form 0 (A operand): [hi | hi | lo], form 1 (B operand): [hi | lo | hi]
// of src[r][0:K] (fp32, row stride lds); hi = bf16(x), lo = bf16(x - hi).  K % 8 == 0.
int x3_split_rows(const float* src, size_t lds, op16_t* dst, int M, int K, int form, hipStream_t st);
// several weight matrices in one launch: item = fp32 source [R][C]; tr = 0: dst[R][3C] rows of the source, tr = 1: dst[C][3R] rows of
// its transpose.  R, C % 8 == 0.
struct X3SplitBatch {
    struct Item { const float* src; op16_t* dst; int R, C, tr, form; };
    Item it[32];
    int n = 0;
    void add(const float* s, op16_t* d, int R, int C, int tr, int form) { it[n++] = Item{s, d, R, C, tr, form}; }
};
int x3_split_multi(const X3SplitBatch& b, hipStream_t st);

}  // namespace CC_NS
