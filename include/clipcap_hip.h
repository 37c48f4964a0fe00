/* clipcap_hip.h — C ABI of libclipcap_hip.so: the MI355X (gfx950) ClipCap hot path.
 *
 * The reference (TheoCoombes/ClipCap) is 100 % Python and has NO plugin / FFI / operator interface for this path
 * (SURVEY.md §8b): the effective boundary is the nn.Module surface of clipcap/model/{mapper,attention,model}.py and
 * the HF GPT-2 it instantiates.  Each entry point below therefore cites the reference *Python call* it replaces;
 * INTEGRATION.md shows the ctypes binding a reference maintainer would add.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless it says "host".
 *   - the caller owns every buffer (parameters, gradients, optimizer state, workspace, KV cache).  The compute entry
 *     points keep no state and never allocate or synchronise; all work is enqueued on the caller's hipStream_t (passed
 *     as void*; NULL = default stream), so calls on different streams / from different host threads are independent.
 *     Per-step settings (GPT-2 dropout, loss scale) travel in the call's own arguments.  The only process-wide state is
 *     the test / measurement hooks at the end of this file (cc_gemm_tile_mode, cc_gemm_skinny_mode, cc_decode_mode,
 *     cc_prof_*), which the product path never touches.  libclipcap_hip.so does not read the environment
 *     (getenv is not among its imports) and exports exactly the functions declared here (csrc/exports.map).  The kernels and A/B
 *     code paths that were built, measured and lost — the persistent decode-layer launch, the XCD-team decode engine, decode GEMMs on
 *     fragment-ordered weight images, fp32-MFMA attention — their entry points (include/clipcap_hip_lab.h) and the CC_* environment
 *     switches that select them live in the LAB build only (`make -C clipcap_amd/csrc lab` -> libclipcap_hip_lab.so, -DCC_EXPERIMENTS,
 *     csrc/lab_env.h; CLIPCAP_HIP_LIB=lab makes the Python binding load it).
 *   - return value: 0 = ok, <0 = error (CC_ERR_*), never throws across the ABI.
 *   - OPERAND TYPE.  GEMM / attention operands and the stored 16-bit activations are bf16 (CC_OP_BF16, default) or IEEE
 *     fp16 (CC_OP_FP16 = the reference's `--fp-precision 16`, clipcap/train/args.py:30-34), selected per model by
 *     cfg->op_dtype; accumulation, master weights, residual streams, LayerNorm statistics, the loss and the optimizer are
 *     fp32 in both.  16-bit tensors cross the ABI as raw bit patterns (uint16_t), round-to-nearest-even like
 *     torch.bfloat16 / torch.float16.  fp16 training runs its backward pass under a loss scale (cc_lmhead_ce_bwd,
 *     cc_grad_nonfinite, cc_loss_scale_update, cc_adamw_step) exactly as torch.cuda.amp.GradScaler does for the
 *     reference's Lightning fp16 path.
 *     CC_OP_BF16X3 is the reference's DEFAULT precision (`--fp-precision 32`, clipcap/train/args.py:30-34, train.py:82) on a chip
 *     whose fp32 MFMA runs at 1/16 of its bf16 rate (three bf16 terms are ~5x faster than v_mfma_f32_32x32x2_f32): every GEMM operand x is split into bf16 hi = bf16(x), lo = bf16(x - hi) and each product runs as
 *     three bf16 MFMA terms hi*hi + hi*lo + lo*hi with fp32 accumulation (about 16 mantissa bits per operand, a third of the bf16
 *     rate); activations between kernels are fp32 and attention runs in fp32.  This is the mode in which logits match the fp32
 *     reference to 1e-3 at full depth.  Its buffers differ in size only: the operand arena has 6*count 16-bit elements (the
 *     [hi | lo | hi] image of every 2-D weight at 3x its offset, of its transpose at 3*(count + offset)), the KV cache holds fp32
 *     (twice the bytes per element), workspaces are whatever cc_*_ws_bytes says.  cc_*_transpose_weights, cc_adamw_step_cast,
 *     cc_cast_op16 and the bare GEMM hooks (cc_gemm_op16_f32, cc_gemm_wgrad) do not exist in this mode (CC_ERR_ARG): use cc_adamw_step + cc_*_sync_weights.
 *   - parameters live in flat arenas whose element offsets are defined by cc_*_param_offsets(); the fp32 arena is
 *     the master copy (nn.Parameter views alias it).  The 16-bit operand arena has 2*count elements: [0,count) is the
 *     cast of the master (same offsets, reference state-dict layouts: torch.nn.Linear weight [out,in]; HF Conv1D
 *     weight [in,out]); [count, 2*count) holds, at the same offsets, the TRANSPOSE of every 2-D GEMM weight, so that
 *     forward and dgrad GEMMs are both "NT" (both operands K-contiguous, the direct-to-LDS fast path).  It is
 *     refreshed from the master by cc_mapper_sync_weights / cc_gpt2_sync_weights after every optimizer step.
 */
#ifndef CLIPCAP_HIP_H
#define CLIPCAP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CC_OK 0
#define CC_ERR_ARG (-1)
#define CC_ERR_SHAPE (-2)
#define CC_ERR_LAUNCH (-3)
#define CC_ERR_STATE (-4)

/* bumped when an existing entry point changes.  3: cc_loss_scale_update's state is float[3] (applied-step counter in state[2]) and
 * cc_adamw_step / cc_adamw_step_cast accept step == 0 (= take the step number from loss_scale[2]) — a version-2 caller passing float[2]
 * would be written out of bounds, so clipcap_amd/_lib.py refuses a library whose version differs.  Entry points ADDED since 2:
 * cc_adamw_step_cast, cc_mapper_transpose_weights, cc_gpt2_transpose_weights, cc_comm_count, cc_decode_part_floats, cc_decode_fwd_p,
 * cc_beam_step_p; since 3: cc_decode_fwd_g, cc_decode_ws_check, cc_decode_mode, cc_grad_wire_pack, cc_grad_wire_unpack,
 * cc_sample_step_lp, cc_broadcast_bucket, cc_reduce_bucket, cc_embed_tokens_bwd, cc_embed_tokens_bwd_ws,
 * cc_embed_tokens_bwd_ws_bytes, and the GEMM wrapper test hooks cc_x3_image_bytes, cc_x3_split_rows, cc_gemm_act, cc_gemm_resid,
 * cc_gemm_dact, cc_gemm_f32, cc_gemm_wgrad_split, and the attention test hooks cc_attention_fwd_x, cc_attention_bwd_x; operand mode ADDED: CC_OP_BF16X3.  Round 6 (still 3): the default-off decode experiments
 * (cc_decode_image*, cc_decode_xt_image*, cc_decode_fwd_x, cc_decode_ws_check, cc_decode_last_path) moved to include/clipcap_hip_lab.h —
 * the lab library exports them, the product library does not.  ADDED since (still 3: no existing entry point changed): cc_lmhead_score,
 * cc_grad_norm_scratch_floats, cc_grad_sqnorm, cc_grad_clip_coef, cc_adamw_step_clip, cc_logits_constrain, cc_beam_group_step,
 * cc_beam_group_ws_bytes, cc_decode_hidden_unit, cc_contrastive_topk, cc_contrastive_select, the decode-attention test hook
 * cc_decode_attention, and the label-smoothed loss cc_lmhead_smooth_scratch_floats, cc_lmhead_ce_fwd_smooth, cc_lmhead_ce_bwd_smooth,
 * the weight-averaging optimizer step cc_adamw_step_ema, the decode-time guidance cc_logits_guide, the loss with per-token weights
 * cc_lmhead_ce_fwd_w, cc_lmhead_ce_bwd_w, the sampling truncation rules cc_logits_truncate, and stochastic beam search
 * cc_beam_gumbel_ws_bytes, cc_beam_gumbel_step with its noise test hooks cc_gumbel_noise, cc_gumbel_from_bits, the CIDEr-D reward
 * cc_cider_score with its host-only table builder cc_cider_table_build, and lexically constrained beam search cc_beam_lex_ws_bytes,
 * cc_beam_lex_step, and the caption metrics cc_bleu_stats, cc_rouge_l, and the MLP mapping network cc_mlp_param_count,
 * cc_mlp_param_offsets, cc_mlp_ws_bytes, cc_mlp_sync_weights, cc_mlp_transpose_weights, cc_mlp_fwd, cc_mlp_bwd, cc_mlp_bwd_part with
 * its test hooks cc_mlp_get, cc_gemm_tanh. */
#define CC_ABI_VERSION 3
int cc_abi_version(void);

#define CC_OP_BF16 0
#define CC_OP_FP16 1
#define CC_OP_BF16X3 2   /* split operands: the reference's default --fp-precision 32 (see OPERAND TYPE above) */

/* ------------------------------------------------------------------------------------------------------------
 * Mapper: clipcap/model/mapper.py:113-130 TransformerMapper (+ :133-160 windowed), layers :91-110, MLP :70-88,
 * attention clipcap/model/attention.py:4-43.
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct {
    int32_t E;       /* encoder_embedding_size */
    int32_t D;       /* lm_embedding_size */
    int32_t P;       /* projection_length */
    int32_t L;       /* prefix_length */
    int32_t H;       /* num_heads */
    int32_t N;       /* num_layers */
    int32_t Hm;      /* MLP hidden = int(D * 2.0) (mapper.py:10,100) */
    int32_t W;       /* window count (1 = TransformerMapper; window_size+1 for TransformerMapperWindowed, model.py:28) */
    int32_t use_pos; /* windowed: learned pos_embeddings present (mapper.py:142-145) */
    int32_t op_dtype; /* CC_OP_BF16 / CC_OP_FP16: type of the w16 arena and of every 16-bit activation of this model */
} cc_mapper_cfg;

/* number of per-model tensors ahead of the layers (linear.weight, linear.bias, prefix_const, pos_embeddings) */
#define CC_MAPPER_HEAD_TENSORS 4
/* per layer, in arena order: norm1.weight norm1.bias attn.to_queries.weight attn.to_keys_values.weight
 * attn.project.weight attn.project.bias norm2.weight norm2.bias mlp.fc1.weight mlp.fc1.bias mlp.fc2.weight mlp.fc2.bias
 * (to_queries.weight [D,D] is immediately followed by to_keys_values.weight [2D,D]: one fused [3D,D] QKV operand) */
#define CC_MAPPER_LAYER_TENSORS 12

int64_t cc_mapper_param_count(const cc_mapper_cfg* cfg);
/* offsets[CC_MAPPER_HEAD_TENSORS + N*CC_MAPPER_LAYER_TENSORS] element offsets into the arenas (host array);
 * pos_embeddings offset is -1 when absent. */
int cc_mapper_param_offsets(const cc_mapper_cfg* cfg, int64_t* offsets);
/* workspace bytes for batch B; save=1 keeps every layer's activations for cc_mapper_bwd */
int64_t cc_mapper_ws_bytes(const cc_mapper_cfg* cfg, int32_t B, int32_t save);

/* w16[0:count] = bf16(w32); w16[count:2*count] = per-tensor transposes of the GEMM weights (see Conventions) */
int cc_mapper_sync_weights(const cc_mapper_cfg* cfg, const float* w32, uint16_t* w16, void* stream);
/* only the second half: w16[count:2*count] from w16[0:count] — for callers whose optimizer already wrote the cast (cc_adamw_step_cast) */
int cc_mapper_transpose_weights(const cc_mapper_cfg* cfg, uint16_t* w16, void* stream);

/* replaces model.transformer_mapper(embeddings) (mapper.py:122-130; callers model.py:46, inference/generate.py:31,
 * docs/inference.md:24).  emb fp32 [B, W, E]; out fp32 [B, L, D]. */
int cc_mapper_fwd(const cc_mapper_cfg* cfg, int32_t B, const float* w32, const uint16_t* w16, const float* emb, void* ws,
                  float* out, int32_t save, void* stream);
/* the second return value of MultiHeadAttention.forward (attention.py:32-42; Transformer.forward_with_attention, mapper.py:45-52):
 * softmax attention probabilities of one layer, fp32 [B, S, S, H] (query n, key m, head h), recomputed from the activations a
 * save=1 forward left in ws.  Inspection output; not used by training or decode. */
int cc_mapper_attention_probs(const cc_mapper_cfg* cfg, int32_t B, void* ws, int32_t layer, float* out, void* stream);
/* autograd of the above (what loss.backward() does to mapper.py in the reference).  dout fp32 [B, L, D];
 * g32 (flat, same offsets as w32) is ACCUMULATED into.  Requires the workspace of a save=1 forward. */
int cc_mapper_bwd(const cc_mapper_cfg* cfg, int32_t B, const float* w32, const uint16_t* w16, void* ws, const float* dout,
                  float* g32, void* stream);
/* the same, one slice of layers [l_lo, l_hi) at a time, called with descending ranges (first l_hi == N seeds from dout, the call
 * with l_lo == 0 also produces the linear / prefix_const / pos_embeddings gradients).  Lets the caller start the RCCL
 * all-reduce of a layer's gradient slice while the layers below it are still in backward. */
int cc_mapper_bwd_range(const cc_mapper_cfg* cfg, int32_t B, const float* w32, const uint16_t* w16, void* ws, const float* dout,
                        float* g32, int32_t l_hi, int32_t l_lo, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * GPT-2: transformers GPT2LMHeadModel as called by model.py:56 / inference/base.py:81 with inputs_embeds
 * (hf modeling_gpt2.py:514-634, blocks :262-310, attention :54-72,:144-226, MLP :229-243, lm_head :637-725).
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct {
    int32_t D;     /* n_embd */
    int32_t H;     /* n_head */
    int32_t NL;    /* n_layer */
    int32_t V;     /* vocab_size */
    int32_t Vp;    /* vocab rows of the arenas' wte: V rounded up to a multiple of 128 (zero rows) */
    int32_t NPOS;  /* n_positions */
    int32_t op_dtype; /* CC_OP_BF16 / CC_OP_FP16 (see Conventions) */
} cc_gpt2_cfg;

#define CC_GPT2_HEAD_TENSORS 2   /* wte [Vp,D], wpe [NPOS,D] */
/* per layer: ln_1.weight ln_1.bias attn.c_attn.weight[D,3D] attn.c_attn.bias attn.c_proj.weight[D,D] attn.c_proj.bias
 * ln_2.weight ln_2.bias mlp.c_fc.weight[D,4D] mlp.c_fc.bias mlp.c_proj.weight[4D,D] mlp.c_proj.bias */
#define CC_GPT2_LAYER_TENSORS 12
#define CC_GPT2_TAIL_TENSORS 2   /* ln_f.weight ln_f.bias */

/* one training / scoring pass: every GPT-2 entry point of a pass must be given the SAME shape (it fixes the
 * workspace layout).  T = L + cap_used (cap_used <= cap columns of `tokens` are consumed: T - L). */
typedef struct {
    int32_t B;     /* samples */
    int32_t L;     /* prefix rows per sample */
    int32_t T;     /* total rows per sample (prefix + caption tokens) */
    int32_t cap;   /* row stride of `tokens` (int64 [B, cap]); the loss uses T-L = cap columns */
    int32_t mode;  /* 0 inference (no activations kept); 1 training, frozen LM (dgrad only); 2 full finetune (+wgrad) */
    /* GPT-2 dropout of THIS pass (full finetune in train mode: the reference's ClipCapModel leaves the HF GPT-2 in train mode,
     * model.py:19; hf modeling_gpt2.py: embd_pdrop on inputs+positions, attn_pdrop on the attention probabilities, resid_pdrop
     * after both c_proj).  Masks are a counter-based hash of (drop_seed, site, layer, element) regenerated by the backward
     * kernels — nothing is stored; cc_gpt2_embed / cc_gpt2_fwd / cc_gpt2_bwd(_range) of one pass must be given the same values.
     * All-zero probabilities = eval behaviour (ClipCapModelPrefixOnly keeps GPT-2 in eval, model.py:120-123). */
    float p_embd, p_attn, p_resid;
    uint64_t drop_seed;
} cc_gpt2_shape;

int64_t cc_gpt2_param_count(const cc_gpt2_cfg* cfg);
int cc_gpt2_param_offsets(const cc_gpt2_cfg* cfg, int64_t* offsets);
int64_t cc_gpt2_ws_bytes(const cc_gpt2_cfg* cfg, const cc_gpt2_shape* shp);

int cc_gpt2_sync_weights(const cc_gpt2_cfg* cfg, const float* w32, uint16_t* w16, void* stream);
int cc_gpt2_transpose_weights(const cc_gpt2_cfg* cfg, uint16_t* w16, void* stream);   /* as cc_mapper_transpose_weights */

/* x0[b,t,:] = (t<L ? prefix[b,t,:] : wte[max(tok[b,t-L],0),:]) + wpe[t,:]  — model.py:45-49 + hf :571-577.
 * prefix fp32 [B,L,D]; tokens int64 [B, cap] (may be NULL when L == T).  Writes the workspace's layer-0 input. */
int cc_gpt2_embed(const cc_gpt2_cfg* cfg, const cc_gpt2_shape* shp, const float* w32, const float* prefix, const int64_t* tokens,
                  void* ws, void* stream);
/* same, but from a caller-provided inputs_embeds fp32 [B,T,D] (the `language_model(inputs_embeds=...)` call of
 * inference/base.py:81): x0 = inputs_embeds + wpe[arange(T)] */
int cc_gpt2_embed_from(const cc_gpt2_cfg* cfg, const cc_gpt2_shape* shp, const float* w32, const float* inputs_embeds, void* ws,
                       void* stream);
/* transformer body (all blocks; ln_f is applied by the lm_head entry points). */
int cc_gpt2_fwd(const cc_gpt2_cfg* cfg, const cc_gpt2_shape* shp, const float* w32, const uint16_t* w16, void* ws, void* stream);
/* ln_f + tied lm_head on ALL rows -> fp32 logits [B*T, ldl] (what `.logits` holds; hf :703); ldl >= roundup(V,8). */
int cc_gpt2_logits(const cc_gpt2_cfg* cfg, const cc_gpt2_shape* shp, const float* w32, const uint16_t* w16, void* ws, float* logits,
                   int64_t ldl, void* stream);

/* autograd of cc_gpt2_logits for callers that differentiate `.logits` themselves (ClipCapModel.forward(...).logits.backward(), a
 * custom loss): needs a pass run with shape L == 0 (so cap == T) and mode >= 1 — cc_gpt2_embed_from, cc_gpt2_fwd, cc_gpt2_logits —
 * then this.  dlogits fp32 [B*T, ldl] (first V columns read); dx0 fp32 [B, T, D] (nullable) receives d loss / d inputs_embeds;
 * mode 2 accumulates every GPT-2 weight gradient (tied wte through lm_head, wpe, blocks, ln_f) into g32. */
int cc_gpt2_logits_bwd(const cc_gpt2_cfg* cfg, const cc_gpt2_shape* shp, const float* w32, const uint16_t* w16, void* ws,
                       const float* dlogits, int64_t ldl, float* dx0, float* g32, void* stream);

/* training loss of model.py:94-113 on rows L-1..T-2: fused ln_f + lm_head + softmax cross-entropy (ignore_index=0,
 * pads(-1)->0).  stats (2 device floats, zeroed by this call): [0] sum of kept-row losses, [1] number of kept rows. */
int cc_lmhead_ce_fwd(const cc_gpt2_cfg* cfg, const cc_gpt2_shape* shp, const float* w32, const uint16_t* w16, void* ws,
                     const int64_t* tokens, float* stats, void* stream);
/* teacher-forced log-likelihood of tokens[b, :] given the pass's prefix rows: forward only, nothing differentiable kept,
 * no logits stored.  Needs a mode-0 pass with L >= 1 and cap == T - L (cc_gpt2_embed, cc_gpt2_fwd with the same shape).
 * token_logprob fp32 [B, cap]; sample_stats fp32 [B, 2] = {sum of kept log-probs, kept count}.  ignore_zero != 0 reproduces
 * the training loss's ignore_index = 0 (model.py:108-109).  Both outputs are fully written by the call. */
int cc_lmhead_score(const cc_gpt2_cfg* cfg, const cc_gpt2_shape* shp, const float* w32, const uint16_t* w16, void* ws,
                    const int64_t* tokens, int32_t ignore_zero, float* token_logprob, float* sample_stats, void* stream);
/* backward of the above through lm_head and ln_f into the residual-stream gradient kept in the workspace.
 * denom (device float[1]) = divisor of the mean (local or all-reduced kept-row count).  loss_scale (device float[1], NULL = 1):
 * every gradient of this backward pass (dprefix and what is accumulated into the g32 arenas) is multiplied by it — fp16 operands
 * need it to keep d logits = (softmax - onehot) / denom above the fp16 underflow threshold; cc_adamw_step divides it out again.
 * g32 may be NULL unless mode 2. */
int cc_lmhead_ce_bwd(const cc_gpt2_cfg* cfg, const cc_gpt2_shape* shp, const float* w32, const uint16_t* w16, void* ws,
                     const float* denom, const float* loss_scale, float* g32, void* stream);
/* The same loss with label smoothing, F.cross_entropy(..., ignore_index=0, label_smoothing=eps) over the V real classes, as rank-one
 * corrections around the chain above (the GEMMs, their epilogues and the stored logits are the plain chain's):
 *   loss_row(eps) = loss_row(0) + eps (z_t - zbar),  zbar = hf . wbar,  wbar = the mean of the first V rows of wte (rows V..Vp-1 take no
 *   part in it, receive no gradient and stay bit-untouched);  d hf += c (wte[t] - wbar);  mode 2: d wte[t] += c hf,
 *   d wte[v] -= (sum over kept rows of c hf) / V for v < V;  c = eps * loss_scale / max(denom, 1) on kept rows, 0 elsewhere.
 * eps in [0, 1).  scratch: cc_lmhead_smooth_scratch_floats(cfg, shp) device floats of the caller's, 16-byte aligned; the forward call
 * leaves wbar and zbar there and the backward call of the same pass reads them, so hand both the same buffer (the workspace of
 * (cfg, shp) does not grow).  stats3 (3 device floats, fully written): [0] the smoothed loss sum, [1] kept rows, [2] the plain NLL sum
 * = what cc_lmhead_ce_fwd puts in stats[0].  denom = stats3 + 1 (or its all-reduced copy), as above.  eps == 0 launches exactly what
 * cc_lmhead_ce_fwd / cc_lmhead_ce_bwd launch, plus the store of stats3[2].  Every sum runs in a fixed order (no atomics): a mode-2 step is
 * bit-reproducible from run to run.  CC_ERR_ARG with nothing written: eps < 0, eps >= 1 or NaN, a NULL or misaligned scratch, mode 0, and
 * whatever the plain entry points refuse.  cc_lmhead_smooth_scratch_floats: CC_ERR_SHAPE for a cfg / shape the library refuses. */
int64_t cc_lmhead_smooth_scratch_floats(const cc_gpt2_cfg* cfg, const cc_gpt2_shape* shp);
int cc_lmhead_ce_fwd_smooth(const cc_gpt2_cfg* cfg, const cc_gpt2_shape* shp, const float* w32, const uint16_t* w16, void* ws,
                            const int64_t* tokens, float eps, float* scratch, float* stats3, void* stream);
int cc_lmhead_ce_bwd_smooth(const cc_gpt2_cfg* cfg, const cc_gpt2_shape* shp, const float* w32, const uint16_t* w16, void* ws,
                            const float* denom, const float* loss_scale, float eps, float* scratch, float* g32, void* stream);
/* The same loss with a weight per target token (and label smoothing eps, which may be 0):
 *   loss = (1 / max(n, 1)) * sum over kept rows m of row_weight[m] * loss_row(eps)[m],   n = the kept rows (target != 0), NOT the sum of
 *   the weights: a caller who wants that normalisation scales the weights first.  Any finite fp32 weight: negative (the REINFORCE term
 *   of self-critical training, weight = reward(sample) - reward(greedy)), zero (the row still counts in n), large.  Every gradient of the
 *   pass is that of this loss: the row factor loss_scale / max(denom, 1) of a kept row is multiplied by row_weight[m] where d logits (or,
 *   in the exponential form, the pair {r, w}) is formed, and c of the smoothing corrections becomes row_weight[m] * eps * loss_scale /
 *   max(denom, 1); everything after that (the input-gradient GEMM and its fix, the tied weight gradient, its scatters, ln_f) is the
 *   plain chain's code.  Where d logits itself is formed (fp16; split-bf16 mode 2) it carries the factor's magnitude and the sign is put
 *   onto the rows of d hf and of the weight-gradient operand: negating a weight negates its row's gradient bit for bit.  The weight of a row that is not kept is never used in arithmetic (selected away, not multiplied by 0): NaN or inf
 *   there reaches no output.
 * row_weight: device fp32 [B * cap], row-major like tokens; non-NULL; hand both calls of a pass the same values.  scratch: as for the
 * smoothing pair (cc_lmhead_smooth_scratch_floats, 16-byte aligned, the same buffer in both calls); may be NULL only when eps == 0, and
 * with eps == 0 no smoothing launch happens.  stats3 (3 device floats, fully written): [0] the weighted (smoothed) loss sum, [1] kept
 * rows, [2] the plain unweighted NLL sum = what cc_lmhead_ce_fwd puts in stats[0], bit for bit.  denom = stats3 + 1 (or its all-reduced
 * copy).  With every weight 1.0f the outputs are those of cc_lmhead_ce_fwd / _bwd (eps == 0) or of the smoothing pair, bit for bit.
 * Every sum runs in a fixed order (no atomics): a mode-2 step is bit-reproducible from run to run.  CC_ERR_ARG with nothing written: a
 * NULL row_weight, eps < 0, eps >= 1 or NaN, a NULL scratch with eps != 0, a misaligned scratch, mode 0, and whatever the plain entry
 * points refuse.  CC_LM_ROW_LOSS (cc_lmhead_get) stays the plain row loss. */
int cc_lmhead_ce_fwd_w(const cc_gpt2_cfg* cfg, const cc_gpt2_shape* shp, const float* w32, const uint16_t* w16, void* ws,
                       const int64_t* tokens, const float* row_weight, float eps, float* scratch, float* stats3, void* stream);
int cc_lmhead_ce_bwd_w(const cc_gpt2_cfg* cfg, const cc_gpt2_shape* shp, const float* w32, const uint16_t* w16, void* ws,
                       const float* denom, const float* loss_scale, const float* row_weight, float eps, float* scratch, float* g32,
                       void* stream);
/* backward through the blocks.  dprefix fp32 [B, L, D] receives d loss / d prefix (rows 0..L-1 of d x0).
 * mode 2 additionally accumulates all GPT-2 weight gradients (incl. wte/wpe) into g32. */
int cc_gpt2_bwd(const cc_gpt2_cfg* cfg, const cc_gpt2_shape* shp, const float* w32, const uint16_t* w16, void* ws,
                const int64_t* tokens, float* dprefix, float* g32, void* stream);
/* blocks [l_lo, l_hi) only, descending ranges; the call with l_lo == 0 also writes dprefix (and wte/wpe gradients in mode 2) */
int cc_gpt2_bwd_range(const cc_gpt2_cfg* cfg, const cc_gpt2_shape* shp, const float* w32, const uint16_t* w16, void* ws,
                      const int64_t* tokens, float* dprefix, float* g32, int32_t l_hi, int32_t l_lo, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * KV-cached decode (replaces the full re-forward of inference/base.py:81 per step).
 * kv cache: bf16 [NL][2][R][ctx_max][D] owned by the caller (R rows = beams * samples).
 * ------------------------------------------------------------------------------------------------------------ */
int64_t cc_decode_ws_bytes(const cc_gpt2_cfg* cfg, int32_t R, int32_t Tnew);
/* processes Tnew new positions per row (prefill: Tnew = prefix length; step: Tnew = 1) starting at position pos0,
 * appends K/V to the cache (row r writes cache row r) and returns fp32 logits of the LAST new position [R, ldl].
 * x fp32 [R,Tnew,D] WITHOUT wpe.  row_map (int32 [R][ctx_max], may be NULL = identity): cache row that holds position j of
 * row r — a beam reorder (base.py:93,113) then only permutes this small table instead of copying the cache. */
int cc_decode_fwd(const cc_gpt2_cfg* cfg, int32_t R, int32_t Tnew, int32_t pos0, int32_t ctx_max, const float* w32,
                  const uint16_t* w16, const float* x, uint16_t* kv, const int32_t* row_map, void* ws, float* logits, int64_t ldl,
                  void* stream);
/* cc_decode_fwd that also hands out, from the lm_head GEMM's epilogue, the softmax partials of every logits row: lpart (device, may be
 * NULL = plain cc_decode_fwd) = pmax [R][npart] followed by psum [R][npart], npart = ceil(min(Vp, round_up(V, 8)) / 64); pmax = maximum of
 * the row's logits in the 64-column block, psum = sum of exp(logit - pmax) over it (columns >= V excluded).  cc_decode_part_floats = the
 * float count of lpart (2 * R * npart).  cc_beam_step_p uses them to run the whole beam update in one launch without a pass over the
 * logits matrix. */
int64_t cc_decode_part_floats(const cc_gpt2_cfg* cfg, int32_t R);
int cc_decode_fwd_p(const cc_gpt2_cfg* cfg, int32_t R, int32_t Tnew, int32_t pos0, int32_t ctx_max, const float* w32,
                    const uint16_t* w16, const float* x, uint16_t* kv, const int32_t* row_map, void* ws, float* logits, int64_t ldl,
                    float* lpart, void* stream);
/* cc_decode_fwd_p for rows that come in groups of `group` consecutive rows sharing ancestry (beam search: group = beam width, the rows of
 * one caption; R % group == 0, 1 <= group; 1 = cc_decode_fwd_p).  Results are those of cc_decode_fwd_p for ANY row_map; the hint lets the
 * single-position attention step (Tnew == 1, group <= 8) read every distinct (cache row, position) of a group once for all its rows
 * instead of once per row (inference/base.py:80-121 re-forwards every beam separately). */
int cc_decode_fwd_g(const cc_gpt2_cfg* cfg, int32_t R, int32_t Tnew, int32_t pos0, int32_t ctx_max, const float* w32,
                    const uint16_t* w16, const float* x, uint16_t* kv, const int32_t* row_map, int32_t group, void* ws, float* logits,
                    int64_t ldl, float* lpart, void* stream);
/* reorder / expand cache rows after a beam step: kv_dst[:, :, r] = kv_src[:, :, src[r]] for positions < ctx and
 * r < R_dst (base.py:93,113: embeds.expand / embeds[next_tokens_source]); the two caches may have different row counts. */
int cc_decode_reorder(const cc_gpt2_cfg* cfg, int32_t R_src, int32_t R_dst, int32_t ctx, int32_t ctx_max, const uint16_t* kv_src,
                      uint16_t* kv_dst, const int32_t* src, void* stream);
/* one beam-search update for S independent samples of `beam` rows each (base.py:84-119): log-softmax of logits/T,
 * stopped rows -> -inf except col 0 -> 0, length-normalised top-`beam` over beam*V, outputs next token / source row /
 * updated scores, seq_lengths, has_stopped.  first!=0: step 0 (top-beam of the single row, base.py:86-94). */
int cc_beam_step(int32_t S, int32_t beam, int32_t V, const float* logits, int64_t ldl, float temperature, int32_t first,
                 int32_t stop_token, float* scores, float* seq_lengths, uint8_t* has_stopped, int32_t* next_tokens,
                 int32_t* src_rows, void* ws, void* stream);
/* the same update given the logits' partials (lpart / npart as cc_decode_fwd_p writes them for the S * beam rows; NULL = cc_beam_step):
 * row statistics from the partials, every 64-column block bounded by its maximum, only the handful of blocks that can hold a winner
 * read — one launch.  Identical results (arithmetic, tie rule); temperature != 1 or widths other than 1..5, 8 take cc_beam_step's path. */
int cc_beam_step_p(int32_t S, int32_t beam, int32_t V, const float* logits, int64_t ldl, const float* lpart, int32_t npart,
                   float temperature, int32_t first, int32_t stop_token, float* scores, float* seq_lengths, uint8_t* has_stopped,
                   int32_t* next_tokens, int32_t* src_rows, void* ws, void* stream);
int64_t cc_beam_ws_bytes(int32_t S, int32_t beam, int32_t V);
/* Diverse beam search (since 3, added without a version bump; not in the reference: Vijayakumar et al., 2016): cc_beam_step with the `beam`
 * rows of every sample split into `groups` beam groups of W = beam / groups consecutive rows (beam % groups == 0, beam <= 16); beam group
 * g owns rows and output slots g W .. (g + 1) W - 1.  One call advances the beam groups in the order 0 .. groups - 1; beam group g takes
 * cc_beam_step's update on its own W rows (first != 0: on row 0 of the sample, in every beam group), with one change: the log-probability
 * log(softmax(x / T))[v] of a non-stopped row's token v loses diversity_penalty * c(v) in fp32 before the length normalisation, c(v) =
 * how many slots of beam groups 0 .. g - 1 of the sample took token v AT THIS CALL from a source row that had not stopped (the token-0
 * continuation of a stopped beam is padding: neither counted nor penalised).  c(v) == 0 applies no operation, so groups == 1 is
 * cc_beam_step bit for bit, for any penalty, and diversity_penalty == 0 is cc_beam_step at width W on every beam group's rows.  The W
 * best of a beam group's W V candidates fill its slots best first (ties: lowest flat index b_local V + v); the penalised value is what
 * scores keeps.  src_rows = the source row's index inside the SAMPLE (g W + b_local), as cc_beam_advance takes it.
 * 1 + 2 groups launches (row statistics once, then per beam group a selection over 16 slices and a merge + commit), stream-ordered.
 * ws: cc_beam_group_ws_bytes(S, beam, groups, V) bytes.  CC_ERR_ARG: NULL pointers, S < 0, beam outside [1, 16], groups < 1 or not a
 * divisor of beam, V < 1, ldl < V, a penalty that is negative or not finite.  S == 0: CC_OK, nothing is launched. */
int64_t cc_beam_group_ws_bytes(int32_t S, int32_t beam, int32_t groups, int32_t V);
int cc_beam_group_step(int32_t S, int32_t beam, int32_t groups, int32_t V, const float* logits, int64_t ldl, float temperature,
                       float diversity_penalty, int32_t first, int32_t stop_token, float* scores, float* seq_lengths, uint8_t* has_stopped,
                       int32_t* next_tokens, int32_t* src_rows, void* ws, void* stream);
/* Stochastic beam search (since 3, added without a version bump; not in the reference: Kool, van Hoof, Welling, ICML 2019, "Stochastic
 * Beams and Where to Find Them"): one update that gives every sample `beam` continuations sampled WITHOUT replacement from the model, in
 * sampling order.  State per beam row b of a sample: scores[b] = phi_b, the sum of the token log-probabilities so far (NOT
 * length-normalised); gumbels[b] = Gamma_b, the row's perturbed log-probability; seq_lengths, has_stopped as in cc_beam_step.  first != 0:
 * one parent, row 0, with phi = 0, Gamma = 0, not stopped.
 *   Noise of token v of logits row `row` = s * beam + b of this call (first: row s * beam, under that index) at decode step `step` under
 *   `seed`: h = word v & 3 of Philox4x32-10(counter = (v >> 2, row, step, 0), key = (lo32(seed), hi32(seed))); u = (h + 0.5) / 2^32,
 *   n_v = -ln(-ln u), a real in (-3.14, 22.9).  In fp32: E = -logf(((float)h + 0.5f) 2^-32) for h < 2^31, else
 *   E = -log1pf(-((float)(0xffffffff - h) + 0.5f) 2^-32); n = -logf(E): u is never formed near 1.
 *   Stage 1, per parent row.  A stopped parent has exactly one candidate: token 0 (padding) with Gamma_c = Gamma_b, phi_c = phi_b; no
 *   noise is drawn and its logits are not read.  A live parent: x_v = logits[row][v] / T (T <= 0: 1), lp_v = log_softmax(x)_v from
 *   the row's running (max m, sum of exp(x - m)) pair, y_v = x_v + n_v, Y = max_v y_v.  The row keeps its `beam` best tokens by (y_v
 *   descending, v ascending); tokens with x_v = -inf (bans) are no candidates.  Gamma_c below is non-decreasing in y_v within a row, so the
 *   pruning is exact.
 *   Stage 2, per sample, for every kept candidate of parent b: phi_c = phi_b + lp_v; g = phi_c + n_v; delta = Y - y_v >= 0 (from the y
 *   values: exact in fp32 when small); t = Gamma_b - g + log(1 - exp(-delta)) (delta = 0: -inf); Gamma_c = Gamma_b - max(0, t) -
 *   log1p(exp(-|t|)), the stable form of -log(exp(-Gamma_b) - exp(-Z) + exp(-g)).  Gamma_c <= Gamma_b always; the row's best child has
 *   Gamma_c == Gamma_b bit for bit.  A candidate with Gamma_c = -inf is no candidate.
 *   Selection and commit: the `beam` best candidates under (Gamma_c descending, flat index b V + v ascending) fill the slots best first:
 *   next_tokens = v, src_rows = the source row inside the sample (0 on the first step), scores = phi_c, gumbels = Gamma_c, seq_lengths =
 *   the parent's + (stopped ? 0 : 1) (first: 1), has_stopped = the parent's | (v == stop_token).  Fewer candidates than slots (extreme
 *   bans): an empty slot gets token 0, source row 0, scores = gumbels = -inf, has_stopped = 1 and row 0's seq_lengths as a stopped parent
 *   passes it on (first: 1); it stays empty in later steps by the rules above.  Every index written is in bounds.
 * Two launches, stream-ordered, one read of the logits, no atomics, no host sync, no allocation: one block per live parent row (running
 * softmax pair, per-thread sorted lists of the `beam` best (y, v) in fp32 with the fp32 noise above, one Philox call per four tokens;
 * widths 1-5 and 8 with lists of that length, the others with lists of 16), then one 64-thread block per sample over at most beam^2
 * candidates.  Stage 2 is evaluated in fp64 (the kept candidates' noise drawn again from the same bits, x = logit / T, lp = x - m -
 * log(sum) from the row's fp32 softmax pair, y, delta and the transform), phi_c and Gamma_c rounded to fp32 once: fp32 y values would
 * put ~3e-6 into delta, which log(1 - exp(-delta)) amplifies by 1 / delta.  Results are bit-identical from run to run.  ws: cc_beam_gumbel_ws_bytes(S, beam, V) bytes; every byte read was written in this call.  Leading dimension in elements.
 * CC_ERR_ARG: a NULL pointer argument, S < 0, beam outside [1, 16], V < 1, ldl < V, step < 0, a NaN temperature.  CC_ERR_SHAPE:
 * V > 2097152.  S == 0: CC_OK, nothing is launched.  All checks come before anything touches the device. */
int64_t cc_beam_gumbel_ws_bytes(int32_t S, int32_t beam, int32_t V);
int cc_beam_gumbel_step(int32_t S, int32_t beam, int32_t V, const float* logits, int64_t ldl, float temperature, int32_t first,
                        int32_t stop_token, uint64_t seed, int32_t step, float* scores, float* gumbels, float* seq_lengths,
                        uint8_t* has_stopped, int32_t* next_tokens, int32_t* src_rows, void* ws, void* stream);
/* test hooks, like cc_dropout_mask: the noise cc_beam_gumbel_step uses.  cc_gumbel_noise: out[v] = n_v, v in [0, V), of logits row `row`
 * at `step` under `seed` (CC_ERR_ARG: step < 0, row < 0, V < 1, out NULL).  cc_gumbel_from_bits: out[i] = n(h[i]), i in [0, n)
 * (CC_ERR_ARG: n < 0, a NULL pointer; n == 0: nothing is launched). */
int cc_gumbel_noise(uint64_t seed, int32_t step, int32_t row, int32_t V, float* out, void* stream);
int cc_gumbel_from_bits(const uint32_t* h, int32_t n, float* out, void* stream);
/* Lexically constrained beam search with dynamic beam allocation (since 3, added without a version bump; not in the reference: Post &
 * Vilar, NAACL 2018, "Fast Lexically Constrained Decoding with Dynamic Beam Allocation for Neural Machine Translation"; the idea of forcing
 * words into a caption: Anderson et al., EMNLP 2017): one beam update at a fixed width `beam` that tracks per beam row which phrases it has
 * produced and divides the slots between hypotheses by how much of the constraint set they have met.
 *   Phrases: device int32 [S][n_phr][phr_len], -1 after a phrase's last token.  Phrase c of sample s exists iff its first entry is >= 0; its
 *   length is the index of its first negative entry, or phr_len.  0 <= n_phr <= 8, 1 <= phr_len <= 8; n_phr == 0: no phrases, the pointer
 *   is not followed (the same as a table of -1).  Phrase tokens are in [0, V) and never the stop token (the callers validate); on the device
 *   an id outside [0, V) never matches.
 *   Row state: lex_state int32 [S * beam], in place like scores: bits 0-7 met (bit c: phrase c has been produced), bits 8-11 cur + 1 (the
 *   phrase in progress, 0 = none), bits 12-15 pos (the tokens of that phrase matched so far); 0 is the initial state.  full(s) = the mask
 *   of the sample's existing phrases; tokens_met(state) = the summed lengths of the met phrases, plus pos when a phrase is in progress.
 *   Transition for token v from a parent that has not stopped: a phrase in progress whose next token is v moves on (pos + 1; met, with cur
 *   and pos cleared, when that was its last token); otherwise the progress is dropped, and if v is the first token of an unmet existing
 *   phrase the lowest-index such phrase starts (pos = 1, or met at once when its length is 1).  No fallback to a shorter partial match.  A
 *   stopped parent passes its state on unchanged.  (One definition: csrc/lex_state.h.)
 *   Values are cc_beam_step's: the length-normalised sum of softmax().log() over logits / temperature; first != 0 reads row 0 of the sample
 *   with state 0; a stopped parent has the single continuation token 0 at its own average.  A candidate (b, v), flat index b V + v, is
 *   valid iff its value is > -inf and it is not the stop token from a non-stopped parent with met != full(s): a hypothesis may end only when
 *   every phrase has been produced.  The ban is on the candidate, not the logit: the softmax keeps the stop token, so scores stay sums of
 *   the model's own log-probabilities.
 *   Candidate set K of a sample (a set over flat indices; order: value descending, flat index ascending): T, the `beam` best valid
 *   candidates of the sample; B, every parent row's best valid candidate (a stopped parent has exactly one, so a finished caption that
 *   holds every phrase cannot fall out); P, for every non-stopped parent the valid candidates for the next token of its phrase in progress
 *   and for the first token of each of its unmet phrases.
 *   Allocation: every member of K gets its new state and its bank = tokens_met of that state.  The banks are visited from the highest to
 *   the lowest, round after round; each non-empty bank gives its best untaken candidate to the next free slot, until `beam` slots are
 *   filled or K is empty.  Slots are in picking order, so slot 0 has the largest tokens_met.  Commit as cc_beam_step, lex_state = the new
 *   state.  Fewer candidates than slots: an empty slot gets token 0, source row 0, scores = -inf, has_stopped = 1, state 0 and row 0's
 *   seq_lengths as a stopped parent passes it on (first: 1); it stays empty.  Every index written is in bounds.
 *   Without a phrase in the sample there is one bank and the result is cc_beam_step's (without partials) bit for bit, scores included.
 * Three launches, stream-ordered, no atomics, no host sync, no allocation: the row statistics of cc_beam_step; one block per live parent row
 * (per-thread sorted lists of the `beam` best valid (value, token), widths 1-5 and 8 with lists of that length, the others with lists of
 * 16; a direct gather of the at most n_phr + 1 phrase tokens); one 64-thread block per sample over at most beam * (beam + n_phr + 1)
 * candidates.  The logits are read twice.  Results are bit-identical from run to run.  ws: cc_beam_lex_ws_bytes(S, beam, n_phr, V) bytes;
 * every byte read was written in this call.  Leading dimension in elements.
 * CC_ERR_ARG: a NULL pointer argument (phrases only when n_phr > 0), S < 0, beam outside [1, 16], V < 1, ldl < V, n_phr outside [0, 8],
 * phr_len outside [1, 8] when n_phr > 0, a NaN temperature.  CC_ERR_SHAPE: V > 2097152.  S == 0: CC_OK, nothing is launched.  All checks
 * come before anything touches the device; cc_beam_lex_ws_bytes returns < 0 for the same bad arguments. */
int64_t cc_beam_lex_ws_bytes(int32_t S, int32_t beam, int32_t n_phr, int32_t V);
int cc_beam_lex_step(int32_t S, int32_t beam, int32_t V, const float* logits, int64_t ldl, float temperature, int32_t first,
                     int32_t stop_token, const int32_t* phrases, int32_t n_phr, int32_t phr_len, float* scores, float* seq_lengths,
                     uint8_t* has_stopped, int32_t* lex_state, int32_t* next_tokens, int32_t* src_rows, void* ws, void* stream);
/* Constrained decoding (since 3, added without a version bump): token bans on one step's logits [R][ldl], in place, BEFORE the beam update
 * or the sampling step.  A ban sets the token's logit to -inf, i.e. before the softmax (the convention of the reference's
 * top_k_top_p_filtering, utils.py:5-30): its mass is renormalised over the allowed tokens.  The banned set of row r:
 *   - no_repeat_ngram = g >= 1 over the row's history h[0:n) (history + r * hist_stride elements of hist_elem_bytes = 4 (int32) or 8
 *     (int64), n = hist_len, oldest first): for every i in [0, n-g] with h[i : i+g-1] == h[n-g+1 : n], h[i+g-1]; g == 1 bans the whole
 *     history, n < g bans nothing, 0 = off (history may then be NULL);
 *   - ban_token (-1 = none): the host's min_length rule passes the stop token while a caption is too short;
 *   - suppress[0 : n_suppress) (device int32), at every call.
 *   Ids outside [0, V) in the history or the list ban nothing (a history id takes part in the compare with its own value).  skip_rows (nullable, uint8 [R]): rows with a non-zero entry are left alone
 *   (beam search passes has_stopped: the update ignores a stopped beam's logits).
 * lpart / npart (lpart NULL: none): the softmax partials cc_decode_fwd_p wrote for these R rows (pmax [R][npart] then psum [R][npart], one
 *   entry per 64-column block of the V real columns).  The partials of exactly the blocks that received a ban are recomputed from the
 *   banned logits (a block without a finite entry: pmax = -inf, psum = 0), so cc_beam_step_p's one-launch update, which bounds every
 *   block by its pmax and takes the row's softmax denominator from psum, sees consistent inputs.  Blocks without a ban, the padding
 *   columns [V, ldl) and skipped rows are not written.
 * One launch, one workgroup per row; no launch at all when nothing can be banned.  Limits: hist_len <= 1024, n_suppress <= 1023,
 * V <= 2097152 (CC_ERR_SHAPE); npart * 64 >= V, hist_elem_bytes 4 or 8, hist_stride >= hist_len, -1 <= ban_token < V (CC_ERR_ARG). */
int cc_logits_constrain(float* logits, int32_t R, int32_t V, int64_t ldl, float* lpart, int32_t npart, const void* history,
                        int32_t hist_elem_bytes, int64_t hist_stride, int32_t hist_len, int32_t no_repeat_ngram, int32_t ban_token,
                        const int32_t* suppress, int32_t n_suppress, const uint8_t* skip_rows, void* stream);
/* Classifier-free guidance at decode time (since 3, added without a version bump; not in the reference: Kornblith et al., ICCV 2023,
 * "Guiding image captioning models toward more specific captions"; Sanchez et al., 2023): one step's logits of the conditional stream
 * cond [R][ld_c] (the language model behind the image prefix) and of the unconditional stream uncond [R][ld_u] (the same tokens without it)
 * become the guided scores, BEFORE the token bans, the beam update or the sampling step.  Per row r, V real columns, fp32 throughout:
 *     out[r][i] = scale * (cond[r][i] - lse_c) + (1 - scale) * (uncond[r][i] - lse_u)
 *   with lse_* = the log-sum-exp of the row's V real columns of that stream (max-subtracted; -inf entries contribute nothing), i.e.
 *   log_softmax(uncond) + scale * (log_softmax(cond) - log_softmax(uncond)).  scale 1 gives log_softmax(cond), scale 0
 *   log_softmax(uncond); the step that follows renormalises.
 *   - An entry that is -inf in cond OR in uncond is -inf in out (a token banned in either stream stays banned; no inf - inf is formed); a
 *     row whose cond or uncond holds no finite entry is -inf everywhere.  NaN inputs are not supported.
 *   - skip_rows (nullable, uint8 [R]): rows with a non-zero entry are not written (beam search passes has_stopped).
 *   - out == cond, or out NULL (ld_o is then ignored), works in place.  Columns [V, ld) of all three buffers are neither read nor written.
 * One launch, one workgroup per row: a sweep over both rows for the two running (max, sum) pairs, a second sweep (served by L2 / the
 * Infinity Cache) that writes the combination.  16-byte accesses when cond, uncond and out are 16-byte aligned and the three leading
 * dimensions are multiples of 4, scalar accesses otherwise; the arithmetic of an element does not depend on which.  Reductions in a fixed
 * order, no atomics, no scratch: a row's result is bit-identical from run to run and does not depend on R, on the other rows or on their
 * skip flags.  Leading dimensions in floats.  R == 0: CC_OK, nothing is launched.  CC_ERR_ARG: R < 0, V <= 0, a leading dimension < V,
 * scale not finite or < 0, cond or uncond NULL with R > 0.  CC_ERR_SHAPE: V > 2^30. */
int cc_logits_guide(const float* cond, int64_t ld_c, const float* uncond, int64_t ld_u, int32_t R, int32_t V, float scale, float* out,
                    int64_t ld_o, const uint8_t* skip_rows, void* stream);
/* Truncation rules for the sampling decoders (since 3, added without a version bump; not in the reference): min-p (Nguyen et al., 2024),
 * the epsilon and eta cutoffs (Hewitt et al., 2022, "Truncation sampling as language model desmoothing") and locally typical sampling
 * (Meister et al., 2022) on one step's logits [R][ldl], in place, AFTER the guidance and the token bans and immediately BEFORE
 * cc_sample_step / cc_sample_step_lp, called with the same temperature, history, hist_len, hist_ld and repetition_penalty.  The rules act
 * on exactly the values the sampler draws from: v_i = fl32(pen(x_i) * fl32(1 / T)), the repetition penalty applied once to every id of
 * history[r * hist_ld + 0 .. hist_len) that lies in [0, V), before the temperature (temperature <= 0 is taken as 1; no penalty with
 * hist_len == 0, a NULL history or repetition_penalty == 1).  Per row, over the V real columns, with m = max v, lse = log sum exp(v_i)
 * (max-subtracted; -inf adds nothing), p_i = exp(v_i - lse), H = -sum over p_i > 0 of p_i (v_i - lse) in nats, token i is kept iff
 *     min_p > 0           v_i >= m + ln(min_p)                                      (p_i >= min_p * p_max)
 *     epsilon_cutoff > 0  v_i >= lse + ln(epsilon_cutoff)                           (p_i >= epsilon)
 *     eta_cutoff > 0      v_i >= lse + min(ln eta, 0.5 ln eta - H)                  (p_i >= min(eta, sqrt(eta) e^-H))
 *     typical_p < 1       d_i <= d*, d_i = |lse - v_i - H| (+inf for v_i = -inf); with the tokens ordered by d ascending, d* is the d of
 *                         the first token at which the cumulative p reaches >= typical_p (never: the last finite d); ties at d* are kept
 *   for every rule that is on (off values: 0, 0, 0, 1).  The kept set is the intersection, every rule taken against the same p and H of
 *   the incoming row (with one rule on this is what the corresponding HF transformers warper keeps; with several on, transformers
 *   renormalises between them and this does not).  An empty intersection keeps every token with v_i == m.  A row of only -inf is left as
 *   it is.  -0.0 == +0.0.  NaN inputs are not supported.
 *   - Effect: the RAW logit x_i of every removed token becomes -inf; every kept logit is left bit-untouched; columns [V, ldl) are neither
 *     read nor written.  The sampling step that follows sees the truncated row and applies its own top-k / top-p to it: its mode-0 top_p
 *     mass is therefore relative to the truncated row.
 * One launch, one workgroup per row; the row is re-read per pass (L2): maximum; the sums that give lse and H (epsilon, eta, typical
 * only); for typical four passes of a bucket / radix threshold search on the fp32 image of d with masses in 2^-32 fixed point; one more
 * when typical and a threshold rule are both on (the empty-intersection test); the pass that writes.  The masses go through __expf; lse, H and the
 * thresholds are held in fp64.  Integer atomics and fixed-order sums only: a row's result is bit-identical from run to run and does not
 * depend on R or on the other rows.  Leading dimensions in elements.  Nothing is launched, and CC_OK returned, when all four rules are off
 * or R == 0.  CC_ERR_ARG: R < 0, V <= 0, ldl < V, min_p outside [0, 1], typical_p outside (0, 1], epsilon_cutoff or eta_cutoff outside
 * [0, 1), any of them NaN, hist_len < 0, hist_len > 0 with a NULL history or hist_ld < hist_len, logits NULL with R > 0 (a bad argument is
 * one whatever R and the rules are).  CC_ERR_SHAPE: V beyond what the history bitmap in LDS admits: 16928 + 4 * ceil(V / 32) bytes must not exceed
 * 150 KiB, i.e. V <= 1093376. */
int cc_logits_truncate(float* logits, int32_t R, int32_t V, int64_t ldl, float temperature, const int64_t* history, int32_t hist_len,
                       int32_t hist_ld, float repetition_penalty, float min_p, float typical_p, float epsilon_cutoff, float eta_cutoff,
                       void* stream);
/* CIDEr-D over token ids, the reward of self-critical training (since 3, added without a version bump; the metric of the reference's
 * eval/pycocoevalcap/cider/cider_scorer.py: clipped counts, Gaussian length penalty).  Words are TOKEN IDS: nothing is detokenised and no
 * PTB tokenizer runs, so the numbers are CIDEr-D over BPE tokens, not the published word-level metric.  For a caption x of L words and
 * n = 1..4, its n-grams are w[i .. i + n), i in [0, L - n]; tf_x(g) = occurrences of g in x; idf(g) = the table's value, log_ndocs for an
 * n-gram the table does not hold.  For candidate c and the R references of its image:
 *     v_x,n(g) = tf_x(g) idf(g);  norm_x,n = sqrt(sum over the distinct g of x of v_x,n(g)^2)
 *     val_n(c, r) = sum over the distinct g of c of min(v_c,n(g), v_r,n(g)) v_r,n(g),  divided by norm_c,n norm_r,n only if both are non-zero
 *     out[c] = 10 / (4 R) sum_r exp(-(len(c) - len(r))^2 / (2 sigma^2)) sum_n val_n(c, r),   len(x) = max(L_x - 1, 0)
 *   (len counts bigrams: the reference's behaviour, reproduced).  An empty candidate scores 0; an empty reference still counts in R.
 * Candidates: cand int64 [C][cand_ld], cand_len columns read.  A candidate's words run to the first of: a stop_token (excluded; included
 *   when count_stop != 0), a negative id, cand_len.  stop_token < 0: no stop token.  Candidate c belongs to image cand_group[c], or to
 *   c % G when cand_group is NULL (C must then be a multiple of G); a cand_group value outside [0, G) gives out[c] = 0.
 * References: refs int32 [G][Rmax][Lr]; a row ends at its first negative id; image g uses its first ref_count[g] rows (1..Rmax, clamped;
 *   NULL: all Rmax), the other rows are not read.
 * Table: cc_cider_table_build's tab_keys[cap] / tab_idf[cap] in device memory, cap a power of two.  A key is an n-gram of ids in
 *   [0, 65535), 16 bits per token, unused slots 0xFFFF; the slot is the top log2(cap) bits of key * 0x9E3779B97F4A7C15, probed linearly
 *   with wrap-around (clipcap_amd/csrc/cider_table.h).  A token id >= 65535 inside a caption cannot be packed: every n-gram that holds
 *   it misses the table (idf = log_ndocs) and is still compared exactly, token by token, within and between the captions.
 * One launch, one workgroup per candidate, candidate and references in LDS; tf and first occurrence by exact comparison; the references'
 * norms are computed in the same launch.  fp32 sums over n-grams, fp64 for the per-reference scalars, the result rounded once to fp32.
 * Every sum in a fixed order, no floating-point atomics: the same input gives the same bits on every run, and out[c] does not depend on
 * the other candidates.  out[0 .. C) is written, nothing else.
 * Limits (CC_ERR_SHAPE): cand_len <= 256, Lr <= 256, Rmax * Lr <= 4096, stop_token < 65535.
 * CC_ERR_ARG: C < 0, cand_len < 0, cand_ld < cand_len, G < 1, Rmax < 1, Lr < 1, cap not a power of two, sigma <= 0 or not finite,
 * log_ndocs not finite, cand_group NULL with C not a multiple of G; with C > 0, a NULL cand, refs, tab_keys, tab_idf or out.  C == 0:
 * CC_OK, nothing is launched.  All of this is decided before anything touches the device. */
int cc_cider_score(const int64_t* cand, int32_t C, int32_t cand_len, int64_t cand_ld, int32_t stop_token, int32_t count_stop,
                   const int32_t* cand_group, const int32_t* refs, int32_t G, int32_t Rmax, int32_t Lr, const int32_t* ref_count,
                   const uint64_t* tab_keys, const float* tab_idf, int64_t cap, float log_ndocs, float sigma, float* out, void* stream);
/* The table of cc_cider_score in HOST memory (host-only: no device is touched; the caller copies tab_keys / tab_idf to the device): n
 * distinct keys with their idf into tab_keys[cap] / tab_idf[cap].  CC_ERR_ARG, the table's contents then unspecified: cap not a power
 * of two, 2 n > cap (the load factor stays at or below 0.5), a duplicate key, the all-ones key (the empty marker), NULL pointers. */
int cc_cider_table_build(const uint64_t* keys, const float* idf, int64_t n, uint64_t* tab_keys, float* tab_idf, int64_t cap);
/* BLEU-1..4 and ROUGE-L over word ids (since 3, added without a version bump; the metrics of the reference's
 * eval/pycocoevalcap/bleu/bleu_scorer.py as Bleu.compute_score calls it, option "closest", and eval/pycocoevalcap/rouge/rouge.py).  Words
 * are non-negative integers: token ids, or the word ids of clipcap_amd.eval.  Neither entry point hashes or packs anything: n-grams and
 * words are compared exactly, so any id >= 0 is a word and a candidate id >= 2^31 simply matches no reference word.
 * Candidates, references, ref_count and cand_group are cc_cider_score's: cand int64 [C][cand_ld], cand_len columns read; a candidate's
 *   words run to the first of: a stop_token (excluded; included when count_stop != 0), a negative id, cand_len.  stop_token < 0: no stop
 *   token (there is no upper limit on it here).  Candidate c belongs to image cand_group[c], or to c % G when cand_group is NULL (C must
 *   then be a multiple of G).  refs int32 [G][Rmax][Lr]; a row ends at its first negative id; image g uses its first ref_count[g] rows
 *   (clamped to 1..Rmax; NULL: all Rmax), the other rows are not read.
 *
 * cc_bleu_stats: for candidate c of L words, the references r of its image, and n = 1..4
 *     guess[n]   = max(0, L - n + 1)
 *     correct[n] = sum over the distinct n-grams g of c of  min(tf_c(g), max_r tf_r(g))
 *     reflen     = the l among the references' lengths with the smallest (|l - L|, l): a tie goes to the SHORTER reference
 *     p = 1;  for n = 1..4:  p *= (correct[n] + 1e-15) / (guess[n] + 1e-9);  bleu_n = p^(1/n)
 *     ratio = (L + 1e-15) / (reflen + 1e-9);  if ratio < 1:  bleu_n *= exp(1 - 1/ratio)
 *   stats[c][0..10) = L, reflen, guess[1..4], correct[1..4]: exact integers.  The corpus score is the last two lines on the SUMS of the
 *   ten integers over all candidates (the caller's: clipcap_amd.engine.bleu_corpus).  bleu[c][0..4) = the sentence scores, fp64
 *   arithmetic on the integers, rounded once to fp32; bleu may be NULL: only the integers are written.  A cand_group value outside [0, G)
 *   gives an all-zero row of both.  stats[0 .. 10 C) and bleu[0 .. 4 C) are written, nothing else.
 *
 * cc_rouge_l: lcs(c, r) = the length of the longest common subsequence;  P = max_r lcs / L_c,  R = max_r lcs / L_r (the two maxima may
 *   come from different references);  out[c] = (1 + beta^2) P R / (R + beta^2 P), 0 if P = 0 or R = 0 (the reference: beta = 1.2; beta
 *   arrives as fp32 and is widened).  An empty candidate scores 0 and an empty reference adds 0 to both maxima (the reference never sees
 *   an empty list: "".split(" ") is [""]).  P, R and the score are fp64, rounded once to fp32.  lcs, when not NULL: lcs[c][r] = the exact
 *   LCS length for the rows in use, -1 for the rows not in use.  A cand_group value outside [0, G) gives out[c] = 0 and no row in use
 *   (lcs[c][*] = -1).  out[0 .. C) and lcs[0 .. C Rmax) are written, nothing else.
 *
 * One launch each, one workgroup per candidate, candidate and references in LDS.  BLEU: wave n - 1 counts the n-grams of length n, tf and
 * first occurrence by exact comparison.  ROUGE-L: the bit-parallel LCS recurrence on 64-bit ballots, one wave per reference at a time.
 * Integer sums and maxima in a fixed order, nothing added in floating point, no global atomics: the same input gives the same bits on
 * every run, and a row does not depend on the other candidates.
 * Limits (CC_ERR_SHAPE): cand_len <= 256, Lr <= 256, Rmax * Lr <= 4096.
 * CC_ERR_ARG: C < 0, cand_len < 0, cand_ld < cand_len, G < 1, Rmax < 1, Lr < 1, cand_group NULL with C not a multiple of G; cc_rouge_l:
 * beta <= 0 or not finite; with C > 0, a NULL cand or refs, a NULL stats (cc_bleu_stats) or out (cc_rouge_l).  C == 0: CC_OK, nothing
 * is launched.  All of this is decided before anything touches the device. */
int cc_bleu_stats(const int64_t* cand, int32_t C, int32_t cand_len, int64_t cand_ld, int32_t stop_token, int32_t count_stop,
                  const int32_t* cand_group, const int32_t* refs, int32_t G, int32_t Rmax, int32_t Lr, const int32_t* ref_count,
                  int32_t* stats, float* bleu, void* stream);
int cc_rouge_l(const int64_t* cand, int32_t C, int32_t cand_len, int64_t cand_ld, int32_t stop_token, int32_t count_stop,
               const int32_t* cand_group, const int32_t* refs, int32_t G, int32_t Rmax, int32_t Lr, const int32_t* ref_count, float beta,
               int32_t* lcs, float* out, void* stream);
/* Contrastive search (since 3, added without a version bump; not in the reference: Su et al., 2022, "A Contrastive Framework for Neural
 * Text Generation"): at every step the k most probable tokens of a caption are run through the model as k rows of one group, and the
 * token kept is the one with the largest  (1 - alpha) p(c) - alpha max_j cos(h_c, h_j),  h_c = the candidate's final hidden state, h_j =
 * the final hidden states of the context so far.  Three entry points, all fp32 / integer work:
 *
 * cc_decode_hidden_unit: the final hidden states of the LAST cc_decode_fwd / _p / _g call made on `ws` (same cfg, R and Tnew), for all
 * R * Tnew positions: out[r * ld_row + t * ld_pos + 0..D) = ln_f(x) / |ln_f(x)|_2, x = the fp32 residual stream the forward left in the
 * workspace, eps 1e-5, fp32 arithmetic throughout (LayerNorm as every other LayerNorm here: one wave per row, the row in registers); a
 * zero vector stays zero.  The 16-bit ln_f rows the lm_head reads are NOT used: they exist for the last position only and are rounded to
 * the operand type, and the similarity must not depend on the operand mode more than the residual itself does.  Valid after any call
 * sequence that ends in a forward on this ws with these R, Tnew — prefill (Tnew > 1), a single position, with or without group / lpart:
 * every path of the product's forward (fused finishing passes or separate LayerNorm launches) stores the final residual of all R * Tnew
 * rows in fp32 before ln_f is applied.  NOT valid after a forward with other R / Tnew on the same ws (the carving differs), nor after the
 * lab library's persistent engines (cc_decode_mode bits 1 and 2: CC_ERR_STATE while either is on).  One launch.  CC_ERR_ARG: bad cfg, NULL
 * pointers, R < 0, Tnew < 1, out not 16-byte aligned, ld_pos < D, ld_row < (Tnew - 1) * ld_pos + D.  CC_ERR_SHAPE: D > 2048, D % 4,
 * ld_row % 4 or ld_pos % 4.  R == 0: CC_OK, nothing is launched. */
int cc_decode_hidden_unit(const cc_gpt2_cfg* cfg, int32_t R, int32_t Tnew, const float* w32, void* ws, float* out, int64_t ld_row,
                          int64_t ld_pos, void* stream);
/* cc_contrastive_topk: the candidates of S captions.  Caption s reads logits row s * rows_per + (sel ? sel[s] : 0) (fp32 [.][ldl], V real
 * columns; after the prefill rows_per = 1, sel NULL; at a step rows_per = k and sel = cc_contrastive_select's winners).
 * cand_tok[s * k + c] = the ids of the k largest logits, largest first, ties to the lower id (fp32 comparisons: exact);
 * cand_prob[s * k + c] = softmax(row)[id] in fp32, max-subtracted, -inf entries (token bans) contributing nothing.  A slot whose logit is
 * -inf (fewer than k finite logits) holds token 0 and probability -1 = invalid.  A stopped caption (stopped[s] != 0; stopped may be NULL)
 * gets token 0 / probability -1 in every slot and its row is not read.  One launch, one workgroup per caption, the row read once.
 * CC_ERR_ARG: NULL logits / cand_tok / cand_prob, S < 0, rows_per < 1, k outside [1, 8], V < 1, ldl < V.  CC_ERR_SHAPE: V > 2097152.
 * S == 0: CC_OK, nothing is launched. */
int cc_contrastive_topk(const float* logits, int64_t ldl, int32_t S, int32_t rows_per, const int32_t* sel, int32_t V, int32_t k,
                        const uint8_t* stopped, int32_t* cand_tok, float* cand_prob, void* stream);
/* cc_contrastive_select: the degeneration penalty, the scores and the winner.  cand_h fp32 [S * k][D] unit vectors (cc_decode_hidden_unit
 * of the k candidate rows), hist fp32 [S][hist_ld][D] unit vectors of the context.  For a caption that has not stopped:
 *   deg(c) = max over j in [hist_lo, hist_n) of dot(cand_h[s, c], hist[s, j])   (empty range: 0)
 *   score(c) = (1 - alpha) * cand_prob[s, c] - alpha * deg(c)                   over the slots with cand_prob >= 0
 * the winner w has the largest score, ties to the lowest c.  Written: sel[s] = w; captions[s * cap_ld + step] = cand_tok[s, w];
 * hist[s][hist_n] = cand_h[s, w] (a copy, bit for bit); lengths[s] += 1; stopped[s] = (token == stop_token); sel_score[s] = score(w)
 * (sel_score may be NULL); src_rows[s * k + c] = w for every c (what cc_beam_advance takes); skip_rows[s * k + c] = (c != w) ||
 * stopped[s] with the NEW flag (what cc_logits_constrain takes).  No valid slot: the caption stops with stop_token (length + 1, w = 0,
 * score 0, every row skipped, hist untouched).  A caption that had stopped before the call: sel = 0, src_rows = 0, captions[...] = 0
 * (padding, as beam search pads), sel_score = 0, skip_rows = 1; hist, lengths and stopped untouched.
 * One launch, one workgroup (4 waves) per caption: the k candidate vectors sit in LDS (k * D * 4 bytes, 64 KB at k = 8, D = 2048: the
 * largest workgroup allocation, of gfx950's 160 KB per CU; the wave maxima reuse the front of that buffer afterwards), every wave walks its
 * share of the history positions and reads a history row ONCE, in 16-byte loads, for all k dot products.  No float atomics, fixed
 * reduction order: results do not depend on wave scheduling.
 * CC_ERR_ARG: NULL pointers (sel_score excepted), S < 0, k outside [1, 8], D < 4, not 0 <= hist_lo <= hist_n < hist_ld, alpha outside
 * [0, 1] or not finite, step outside [0, cap_ld).  CC_ERR_SHAPE: D % 4, D > 2048.  S == 0: CC_OK, nothing is launched. */
int cc_contrastive_select(int32_t S, int32_t k, int32_t D, const float* cand_h, const float* cand_prob, const int32_t* cand_tok, float* hist,
                          int32_t hist_ld, int32_t hist_lo, int32_t hist_n, float alpha, int32_t stop_token, uint8_t* stopped, int32_t* lengths,
                          int32_t* sel, int32_t* src_rows, uint8_t* skip_rows, int32_t* captions, int32_t cap_ld, int32_t step, float* sel_score,
                          void* stream);
/* gathers wte rows for next tokens: out fp32 [R, D] (base.py:117) */
int cc_embed_tokens(const cc_gpt2_cfg* cfg, int32_t R, const float* w32, const int32_t* tokens, float* out, void* stream);
/* its gradient: dwte fp32 [Vp, D] += scatter of dout fp32 [R, D] by tokens (rows sharing an id accumulate).  The non-deterministic form:
 * fp32 atomics, so rows that share an id add in arrival order.  cc_embed_tokens_bwd_ws is the reproducible one. */
int cc_embed_tokens_bwd(const cc_gpt2_cfg* cfg, int32_t R, const float* dout, const int32_t* tokens, float* dwte, void* stream);
/* the same gradient, bit for bit the same from run to run (no atomics) — what autograd runs for `language_model.get_input_embeddings()(tokens)`
 * in a full finetune driven through Module.forward (clipcap/model/model.py:44).  Ids clamped to [0, Vp-1] like cc_embed_tokens'.  Order:
 * the rows of one id in ascending row order, cut into chunks of 512 rows; each chunk summed in fp32 in that order, starting from its first
 * row; a one-chunk id: dwte[id] = dwte[id] + sum; otherwise the chunk sums are added in chunk order, starting from the first, and
 * dwte[id] = dwte[id] + that total.  ws: device scratch of cc_embed_tokens_bwd_ws_bytes(cfg, R) bytes, used by this call only
 * (NULL: CC_ERR_STATE).  cfg->D % 4 == 0. */
int cc_embed_tokens_bwd_ws(const cc_gpt2_cfg* cfg, int32_t R, const float* dout, const int32_t* tokens, float* dwte, void* ws, void* stream);
int64_t cc_embed_tokens_bwd_ws_bytes(const cc_gpt2_cfg* cfg, int32_t R);
/* Everything between two beam steps in one launch (base.py:104-117): row r continues row g = (r / beam) * beam + src_rows[r] of its beam
 * group (src_rows NULL: g = r).  x_out fp32 [R, D] = wte[next_tokens[r]] (w32 points at wte);  row_map_out[r][j] = row_map_in[g][j] for
 * j < pos, r for the positions still to come (tables int32 [R][ctx_max], see cc_decode_fwd; NULL = skip);  tokens_out[r][:step] =
 * tokens_in[g][:step], tokens_out[r][step] = next_tokens[r] (int32 [R][tok_ld]; NULL = skip).  In / out buffers must differ. */
int cc_beam_advance(const cc_gpt2_cfg* cfg, int32_t R, int32_t beam, const float* w32, const int32_t* next_tokens, const int32_t* src_rows,
                    int32_t pos, int32_t ctx_max, const int32_t* row_map_in, int32_t* row_map_out, int32_t step, int32_t tok_ld,
                    const int32_t* tokens_in, int32_t* tokens_out, float* x_out, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Optimizer / casts: torch.optim.AdamW as configured by model.py:73-77 (lr schedule is computed by the caller,
 * model.py:79-83), flat over one arena.  The gradient used is g32 * grad_scale / (*loss_scale) (loss_scale: device float[1],
 * NULL = 1).  found_inf (device float[1], NULL = never): a non-zero value skips the update of every element — the step a
 * GradScaler drops when the scaled fp16 backward overflowed — and leaves m, v and the parameters untouched.
 * step >= 1 is Adam's step number (bias correction).  step == 0 (needs loss_scale): the number is taken from the device,
 * 1 + loss_scale[2], the loss scaler's count of steps actually applied (cc_loss_scale_update) — a skipped step must not advance
 * the bias correction, and the host cannot know which steps were skipped without a synchronisation.
 * ------------------------------------------------------------------------------------------------------------ */
int cc_adamw_step(float* p32, const float* g32, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                  float weight_decay, int32_t step, float grad_scale, const float* loss_scale, const float* found_inf, void* stream);
/* cc_adamw_step that also stores w16[0:n] = cast of the updated parameters to op_dtype (untouched when the step is skipped), so that
 * the refresh of the operand arena after a step is cc_*_transpose_weights alone: one pass over the arena less per step. */
int cc_adamw_step_cast(int32_t op_dtype, float* p32, const float* g32, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                       float eps, float weight_decay, int32_t step, float grad_scale, const float* loss_scale, const float* found_inf,
                       uint16_t* w16, void* stream);
/* dst = cast of src to the 16-bit operand type op_dtype */
int cc_cast_op16(int32_t op_dtype, const float* src, uint16_t* dst, int64_t n, void* stream);
/* bf16 gradient wire of the N-rank all-reduce (train/train.py:77-85 runs DDP; clipcap_amd/train/ddp.py): wire[0:n] = bf16(g32[0:n]) (round to
 * nearest even) before the collective, g32[0:n] = fp32(wire[0:n]) after it.  Any n and any element alignment (a layer's gradient slice
 * starts wherever its first parameter does); always bf16, whatever the operand mode. */
int cc_grad_wire_pack(const float* g32, uint16_t* wire, int64_t n, void* stream);
int cc_grad_wire_unpack(const uint16_t* wire, float* g32, int64_t n, void* stream);
/* Dynamic loss scaling for CC_OP_FP16 training (torch.cuda.amp.GradScaler semantics; what Lightning wraps around the reference's
 * model when --fp-precision 16, clipcap/train/train.py:77-85), entirely on the device:
 *   cc_grad_nonfinite: *found_inf = 1 if any of the n gradients is inf / nan (never clears it; call once per arena, after the
 *                      all-reduce in a multi-GPU step so that every rank takes the same decision);
 *   cc_loss_scale_update: state (device float[3]): [0] = scale, [1] = consecutive good steps, [2] = optimizer steps applied so far.
 *                      found_inf != 0: scale *= backoff, counter = 0; else counter += 1 (at `interval`: scale *= growth, counter = 0)
 *                      and state[2] += 1.  Clears *found_inf. */
int cc_grad_nonfinite(const float* g32, int64_t n, float* found_inf, void* stream);
int cc_loss_scale_update(float* state, float* found_inf, float growth, float backoff, int32_t interval, void* stream);
/* Global gradient-norm clipping (torch.nn.utils.clip_grad_norm_, which Lightning's gradient_clip_val runs for the reference's trainer,
 * clipcap/train/train.py:77-85), entirely on the device:
 *   cc_grad_sqnorm: sumsq[0] += sum of g32[i]^2, i < n (n % 4 == 0, else CC_ERR_SHAPE and nothing is written; n == 0: no-op).  Call it
 *                      once per gradient arena (or per owned slice, then SUM sumsq over the ranks) into a zeroed sumsq.  scratch = device
 *                      scratch of cc_grad_norm_scratch_floats() floats, used by this call only.  No atomics: the result is the same bit for
 *                      bit from run to run and from machine to machine.  The order — grid constants CC_GRAD_NORM_BLOCKS, _THREADS, _ACC —
 *                      with n4 = n / 4, nb = min(ceil(n4 / THREADS), BLOCKS) blocks, S = nb * THREADS: float4 group i contributes
 *                      (x*x + y*y) + (z*z + w*w) (<= 3 roundings per element); thread T visits groups T, T + S, T + 2S, ..., visit k
 *                      added to its accumulator k % ACC (<= ceil(ceil(n4 / S) / ACC) additions each); (a0 + a1) + (a2 + a3) (2 levels);
 *                      a 64-lane tree (6 levels); the block's 4 waves as (w0 + w1) + (w2 + w3) (2 levels) -> one partial per block.  A
 *                      second launch of one block folds them: thread t adds its BLOCKS / THREADS consecutive partials in index order,
 *                      the same 6 + 2 levels follow, and one thread does sumsq[0] = sumsq[0] + total.
 *   cc_grad_clip_coef: clip (device float[2]): clip[1] = sqrt(sumsq[0]) * grad_scale / (loss_scale ? loss_scale[0] : 1), the norm of the
 *                      gradient cc_adamw_step would use; clip[0] = min(1, max_norm / (clip[1] + 1e-6)).  A norm that is not finite gives
 *                      clip[0] = NaN; max_norm = +inf gives exactly 1.0f (report the norm, clip nothing).  max_norm >= 0.
 *   cc_adamw_step_clip: cc_adamw_step (w16 NULL) / cc_adamw_step_cast (w16 given) whose gradient is also multiplied by clip[0]
 *                      (clip: device float[1], NULL = 1).  clip NULL or clip[0] == 1.0f: bit for bit the step without it. */
#define CC_GRAD_NORM_BLOCKS 1024
#define CC_GRAD_NORM_THREADS 256
#define CC_GRAD_NORM_ACC 4
int64_t cc_grad_norm_scratch_floats(void);
int cc_grad_sqnorm(const float* g32, int64_t n, float* scratch, float* sumsq, void* stream);
int cc_grad_clip_coef(const float* sumsq, float max_norm, float grad_scale, const float* loss_scale, float* clip, void* stream);
int cc_adamw_step_clip(int32_t op_dtype, float* p32, const float* g32, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                       float eps, float weight_decay, int32_t step, float grad_scale, const float* loss_scale, const float* found_inf,
                       const float* clip, uint16_t* w16 /* nullable: no cast */, void* stream);
/* Exponential moving average of the parameters, updated where they sit in registers: cc_adamw_step_clip (p32, m, v and w16 come out
 * bit for bit as it leaves them) plus, after an APPLIED step, ema[i] = ema_decay * ema[i] + (1 - ema_decay) * p32[i] over the
 * parameters the step just wrote — the convex form in fp32, 1 - ema_decay formed in fp32, so ema_decay = 0 gives ema == p32 as numbers
 * and one update stays within 4 * 2^-24 * max(|ema|, |p32|) of the exact value.  A step skipped on *found_inf leaves ema untouched.
 * ema: n floats on the device, 16-byte aligned, not overlapping p32; ema NULL / misaligned / overlapping, or ema_decay outside [0, 1)
 * (NaN included): CC_ERR_ARG before any launch.  n % 4 != 0: CC_ERR_SHAPE; n == 0: no-op.  w16 given in the bf16x3 mode: CC_ERR_ARG.
 * Costs 4 B read + 4 B written per parameter on top of the step's 16 B + 12 B. */
int cc_adamw_step_ema(int32_t op_dtype, float* p32, const float* g32, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                      float eps, float weight_decay, int32_t step, float grad_scale, const float* loss_scale, const float* found_inf,
                      const float* clip /* nullable */, uint16_t* w16 /* nullable */, float* ema, float ema_decay, void* stream);

/* test hook for the dropout of cc_gpt2_shape: keep flags of one mask stream — site 0 embd [B*T*D], 1 attention [B*H*T*T],
 * 2 residual after attn.c_proj [B*T*D], 3 residual after mlp.c_proj [B*T*D]. */
int cc_dropout_mask(uint64_t seed, int32_t site, int32_t layer, float p, int64_t n, uint8_t* out, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Data-parallel collective: SUM all-reduce of a gradient bucket over RCCL / xGMI, one communicator per process
 * (= per GPU).  What Lightning / DeepSpeed do implicitly around the reference's training_step (clipcap/train/train.py:77-85).
 * The communicator handle is the only object the library allocates; it carries no other state.
 *   rank 0: cc_comm_unique_id(uid) -> the caller ships the 128 bytes to the other ranks (MPI, a TCP store, torch.distributed ...)
 *   every rank, with its GPU current (hipSetDevice): cc_comm_create(&comm, nranks, rank, uid)
 *   per step: cc_allreduce_bucket(comm, g32 + lo, hi - lo, CC_RED_F32, stream) for each finished slice of the gradient arena
 *             (cc_*_bwd_range), enqueued on a side stream that waits on the backward stream — in place, asynchronous
 *   cc_comm_destroy(comm)
 * RCCL is bound at run time; CC_ERR_STATE = no librccl could be loaded.
 * ------------------------------------------------------------------------------------------------------------ */
#define CC_COMM_UID_BYTES 128
#define CC_RED_F32 0
#define CC_RED_BF16 1
#define CC_RED_F16 2
int cc_comm_unique_id(uint8_t* uid_host);
int cc_comm_create(void** comm, int32_t nranks, int32_t rank, const uint8_t* uid_host);
int cc_allreduce_bucket(void* comm, void* buf, int64_t count, int32_t dtype, void* stream);
/* In-place ncclBroadcast of buf[0, count) from rank `root`: with optimizer-state sharding (--deepspeed-strategy stage 1 / 2 of
 * clipcap/train/args.py:87-92) every rank runs cc_adamw_step on its own slice of the parameter arena and the owners' slices are
 * broadcast back, one call per owner. */
int cc_broadcast_bucket(void* comm, void* buf, int64_t count, int32_t dtype, int32_t root, void* stream);
/* In-place ncclReduce (SUM) of buf[0, count) onto rank `root`; the other ranks' buffers keep their own contribution.  Gradient
 * partitioning (--deepspeed-strategy stage 2 / 3, clipcap/train/args.py:87-92): a slice of the gradient arena is summed only where it is
 * consumed — on the rank that owns the matching AdamW moments — which moves half of an all-reduce's bytes over xGMI. */
int cc_reduce_bucket(void* comm, void* buf, int64_t count, int32_t dtype, int32_t root, void* stream);
/* ncclCommCount of the communicator: the number of ranks RCCL actually connected (what bench.py prints as rccl_ranks) */
int cc_comm_count(void* comm, int32_t* nranks);
int cc_comm_destroy(void* comm);

/* ------------------------------------------------------------------------------------------------------------
 * Sampling decoders (replaces the per-step torch ops of clipcap/inference/base.py:159-184 generate_nucleus_sampling and
 * :233-262 generate_no_beam + utils.py:5-37): one step for R rows of fp32 logits [R][ld].
 *   x = logits (history tokens first scaled by the repetition penalty, utils.py:33-37) / temperature (<= 0 -> 1, base.py:163)
 *   mode 0 (nucleus): p = softmax(x); the top_k largest (<= 0 or >= V: all); minimal descending prefix with cumulative p >= top_p
 *                     (mass relative to the FULL softmax, base.py:170-176); renormalised
 *   mode 1 (filter):  keep x >= the top_k-th largest (ties kept, utils.py:14-17), then the minimal descending prefix whose softmax
 *                     mass over that set is > top_p (utils.py:19-29; top_p <= 0: off); softmax of the rest
 *   next_token[r] = inverse CDF, in token-id order, of that distribution at u[r] in [0,1).  probs_out (nullable, [R][V]) receives
 *   the distribution itself.  history: int64 [R][hist_ld], first hist_len entries per row (nullable; penalty 1.0 = off).
 * No sort, no host sync; deterministic for given (logits, u).
 * ------------------------------------------------------------------------------------------------------------ */
int cc_sample_step(const float* logits, int32_t R, int32_t V, int32_t ld, float temperature, int32_t top_k, float top_p, int32_t mode,
                   const int64_t* history, int32_t hist_len, int32_t hist_ld, float repetition_penalty, const float* u, int32_t* next_token,
                   float* probs_out, void* stream);
/* The same step with generate_no_beam's sentence-length penalty (clipcap/inference/no_beam.py:55-60 -> utils.py:40-51): AFTER the
 * filter and before the softmax, a history token whose value EQUALS float(stop_token) is multiplied by length_penalty
 * (= current_length / desired_sentence_length * sentence_length_factor; the reference compares the gathered logit VALUES with the
 * token id, and so does this).  stop_token < 0 or an empty history: exactly cc_sample_step. */
int cc_sample_step_lp(const float* logits, int32_t R, int32_t V, int32_t ld, float temperature, int32_t top_k, float top_p, int32_t mode,
                      const int64_t* history, int32_t hist_len, int32_t hist_ld, float repetition_penalty, int32_t stop_token,
                      float length_penalty, const float* u, int32_t* next_token, float* probs_out, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Unit-test hooks (first argument op_dtype = CC_OP_BF16 / CC_OP_FP16: the type of the 16-bit tensors).
 * cc_gemm_op16_f32: one MFMA GEMM C = A·B (+bias) with fp32 output, any of the three operand layouts
 * (al/bl: 0 = [rows][K], 1 = [K][rows]); ksplit>1 accumulates atomically into C (caller zeroes C).
 * ------------------------------------------------------------------------------------------------------------ */
int cc_gemm_op16_f32(int32_t op_dtype, int32_t al, int32_t bl, const uint16_t* A, int32_t lda, const uint16_t* B, int32_t ldb, int32_t M, int32_t N,
                     int32_t K, float* C, int32_t ldc, const float* bias, int32_t ksplit, void* stream);
/* Weight-gradient GEMM as the backward passes run it: dW[Mw][Nw] += X^T Y with X stored [K][Mw], Y stored [K][Nw] (bf16), fp32
 * accumulation into dW; K is split into slices whose partial sums go through `scratch` (cc_wgrad_scratch_bytes() bytes, device). */
int64_t cc_wgrad_scratch_bytes(void);
int cc_gemm_wgrad(int32_t op_dtype, const uint16_t* X, int32_t ldx, const uint16_t* Y, int32_t ldy, int32_t Mw, int32_t Nw, int32_t K, float* dW, int32_t ldw,
                  float* scratch, void* stream);
/* The four GEMM wrappers every GEMM of a training step leaves through (csrc/gemm_api.h), one call each on caller buffers, in all three
 * operand modes.  Test hooks: they keep no state and the product path never calls them; cc_gemm_tile_mode / cc_gemm_skinny_mode select
 * the tile kernel as for cc_gemm_op16_f32.  Common arguments: al / bl, lda / ldb, M, N, K as cc_gemm_op16_f32 (LOGICAL sizes in every
 * mode).  A: CC_OP_BF16 / CC_OP_FP16 16-bit elements, a_img = 0.  CC_OP_BF16X3: a_img = 0 -> fp32 [M][lda], split per call into the
 * image scratch; a_img = K -> A already is its [hi | hi | lo] image (rows of 3 K 16-bit elements, lda ignored); any other a_img, or
 * al / bl != 0 in that mode: CC_ERR_ARG.  B: 16-bit [N][ldb]; CC_OP_BF16X3: the [hi | lo | hi] image, rows of 3 ldb (cc_x3_split_rows
 * form 1 of an fp32 [N][ldb] matrix).  x3 / x3_bytes: the call's image scratch (Call::x3; 16-B aligned, ignored outside CC_OP_BF16X3);
 * a plain A of M x K needs cc_x3_image_bytes(M, K) of it — missing or too small: CC_ERR_STATE and nothing is written.  C / pre / aux
 * are activations: 16-bit, or fp32 in CC_OP_BF16X3; c_img = N (CC_OP_BF16X3 only) writes C as the [hi | hi | lo] image of an N-deep A
 * operand instead (rows of 3 N 16-bit elements, ldc then strides only pre / aux), any other non-zero c_img: CC_ERR_ARG.
 *   cc_x3_image_bytes: bytes one rows x depth image takes in the scratch (rounded up to 256).
 *   cc_x3_split_rows (CC_OP_BF16X3 only): dst [rows][3 width] = image of src fp32 [rows][ld]; form 0 = [hi | hi | lo], 1 = [hi | lo | hi];
 *                      hi = bf16(x), lo = bf16(x - hi).
 *   cc_gemm_act:   C = act(A B^T + bias); act 0 none, 1 relu, 2 gelu_new, 3 gelu_new with pre receiving gelu_new'(u); pre (nullable)
 *                  otherwise receives u = A B^T + bias.
 *   cc_gemm_tanh:  C = h = tanh(A B^T + bias); pre (nullable, always the plain [M][ldc] layout) receives 1 - h h computed from the fp32 h
 *                  (the multiplier of cc_gemm_dact act 3); pre_nt != 0 stores it with non-temporal stores (same values).
 *   cc_gemm_resid: out = res + drop(A B^T + bias), fp32 rows of stride ld, out may alias res.  drop: residual dropout with probability p
 *                  on the mask stream (seed, site, layer) of cc_dropout_mask, element index row * ld + col; p = 0: off.
 *   cc_gemm_dact:  C = (A B^T) * act'(aux); act 1 relu (aux = post-activation), 2 gelu_new (aux = pre-activation), 3 multiply by aux.
 *   cc_gemm_f32:   fp32 C: mode 0 = alpha A B^T + bias, 1 += alpha A B^T, 2 atomic += (required when ksplit > 1; bias must be NULL
 *                  in modes 1 and 2).
 *   cc_gemm_wgrad_split (CC_OP_BF16X3 only): cc_gemm_wgrad with fp32 X [K][ldx], Y [K][ldy]; x_img = Mw: X already is its [hi | hi | lo]
 *                  image [K][3 Mw].  Both (x_img = 0) or Y alone are split into the image scratch. */
int64_t cc_x3_image_bytes(int64_t rows, int64_t depth);
int cc_x3_split_rows(int32_t op_dtype, const float* src, int64_t ld, int32_t rows, int32_t width, int32_t form, uint16_t* dst, void* stream);
int cc_gemm_act(int32_t op_dtype, int32_t al, int32_t bl, const void* A, int32_t a_img, int32_t lda, const uint16_t* B, int32_t ldb, int32_t M, int32_t N,
                int32_t K, void* C, int32_t c_img, int32_t ldc, const float* bias, int32_t act, void* pre, void* x3, int64_t x3_bytes, void* stream);
int cc_gemm_tanh(int32_t op_dtype, int32_t al, int32_t bl, const void* A, int32_t a_img, int32_t lda, const uint16_t* B, int32_t ldb, int32_t M, int32_t N,
                 int32_t K, void* C, int32_t c_img, int32_t ldc, const float* bias, void* pre, int32_t pre_nt, void* x3, int64_t x3_bytes, void* stream);
int cc_gemm_resid(int32_t op_dtype, int32_t al, int32_t bl, const void* A, int32_t a_img, int32_t lda, const uint16_t* B, int32_t ldb, int32_t M, int32_t N,
                  int32_t K, float* out, const float* res, int32_t ld, const float* bias, float p, uint64_t seed, int32_t site, int32_t layer,
                  void* x3, int64_t x3_bytes, void* stream);
int cc_gemm_dact(int32_t op_dtype, int32_t al, int32_t bl, const void* A, int32_t a_img, int32_t lda, const uint16_t* B, int32_t ldb, int32_t M, int32_t N,
                 int32_t K, void* C, int32_t c_img, int32_t ldc, const void* aux, int32_t act, void* x3, int64_t x3_bytes, void* stream);
int cc_gemm_f32(int32_t op_dtype, int32_t al, int32_t bl, const void* A, int32_t a_img, int32_t lda, const uint16_t* B, int32_t ldb, int32_t M, int32_t N,
                int32_t K, float* C, int32_t ldc, const float* bias, int32_t mode, float alpha, int32_t ksplit, void* x3, int64_t x3_bytes,
                void* stream);
int cc_gemm_wgrad_split(int32_t op_dtype, const void* X, int32_t x_img, int32_t ldx, const float* Y, int32_t ldy, int32_t Mw, int32_t Nw, int32_t K,
                     float* dW, int32_t ldw, float* scratch, void* x3, int64_t x3_bytes, void* stream);
/* PROCESS-WIDE test knob.  NT GEMM tile choice: -1 = cost-model chooser (default), 0 = 128x128 kernels only (also for cc_gemm_wgrad), 3 / 4 / 5 / 6 =
 * force the 256x192 / 256x256 / 320x256 / 160x256 (8-wave staggered) kernel wherever it is legal; 7 = 160x256 on the persistent 4-wave kernel with the
 * instruction-level K loop (what the chooser launches for that tile when K % 128 == 0 and K >= 256), the staggered one otherwise.  Returns the previous
 * mode.  For tests and tools/gemm_bench.py only. */
int cc_gemm_tile_mode(int32_t mode);
/* Decode-sized NT GEMMs (M <= 640 rows: cc_decode_fwd's c_attn / c_proj / c_fc at rows x beams = 320) run on 64-row tiles
 * (gemm_nt_s64_kernel).  -1 = default (those call sites only), 0 = never, 1 / 2 / 3 / 4 = additionally route cc_gemm_bf16_f32's NT launches with
 * M <= 1024 through the 64 x 64 / 64 x 128 / 64 x 64 K-split-over-waves (3) / 80 x 64 K-split-over-waves (4) form.  PROCESS-WIDE test knob; returns the previous mode.  For tests and
 * tools/small_gemm_bench.py. */
int cc_gemm_skinny_mode(int32_t mode);
/* How cc_decode_fwd_g runs a single-position group step.  bit 0 (default on): beam-group attention (every distinct KV row of a group read
 * once; off = one attention launch per row set, the A/B arm of tests/test_gpu_decode_group.py).  The other bits select lab-build experiments
 * (include/clipcap_hip_lab.h) and do nothing in the product library.  mode < 0 only queries.  PROCESS-WIDE test knob; returns the previous mode. */
int cc_decode_mode(int32_t mode);
/* The KV-cached attention step of ONE layer as cc_decode_fwd_g launches it, on a caller's buffers (the same dispatch function: the
 * per-row kernel k_decode_attn, or k_group_union + k_decode_attn_group when Tnew == 1, 2 <= group <= 8, head dim 64, the group's list
 * fits 64 KiB of LDS and bit 0 of cc_decode_mode is set).  Test hook: the product path never calls it.  "Stored type" = the operand
 * type's 16-bit element, fp32 in CC_OP_BF16X3; head dim = cfg->D / cfg->H.
 *   qkv       stored type [R*Tnew][3 D]: q | k | v of the new positions (what c_attn wrote)
 *   kv_layer  stored type: K [R][ctx_max][D] followed by V [R][ctx_max][D], one layer of the cache
 *   row_map   int32 [R][ctx_max] (NULL = identity): cache row that holds position j < pos0 of row r, as cc_decode_fwd
 *   group     as cc_decode_fwd_g (1 <= group, R % group == 0)
 *   append    1: the kernels store the K / V slices of the new positions into cache row r, slots pos0 .. pos0 + Tnew - 1, and read them
 *             from qkv;  0: the caller has stored them already (what the fused c_attn epilogue does) and they are read from the cache
 *   ws        the workspace of cc_decode_ws_bytes(cfg, R, Tnew) (the group form keeps its union list there)
 *   out       stored type [R*Tnew][D]: query (r, t) attends to positions 0 .. pos0 + t
 *   path      HOST int32 (nullable): 0 = the per-row kernel was launched, 1 = union + group kernel
 * CC_ERR_ARG: NULL pointers, R / Tnew <= 0, pos0 < 0, group < 1 or not a divisor of R, append not 0 / 1.  CC_ERR_SHAPE: pos0 + Tnew beyond
 * ctx_max or cfg->NPOS, or a ctx_max whose per-row kernel needs more than 64 KiB of LDS (4 * (2 ctx_max + 8 head dim) * 4 bytes).  Nothing
 * is launched or written on an error. */
int cc_decode_attention(const cc_gpt2_cfg* cfg, int32_t R, int32_t Tnew, int32_t pos0, int32_t ctx_max, const uint16_t* qkv, uint16_t* kv_layer,
                        const int32_t* row_map, int32_t group, int32_t append, void* ws, uint16_t* out, int32_t* path, void* stream);
int cc_layernorm_fwd(int32_t op_dtype, const float* x, const float* gamma, const float* beta, uint16_t* y, float* mean, float* rstd, int32_t rows,
                     int32_t D, void* stream);
int cc_attention_fwd(int32_t op_dtype, const uint16_t* qkv, int32_t B, int32_t S, int32_t H, int32_t hd, int32_t causal, uint16_t* out, float* lse,
                     void* stream);
/* o = forward output and delta_ws = fp32 scratch [B*H*S] select the MFMA kernels (hd 64/96/128); NULL -> LDS/VALU kernel */
int cc_attention_bwd(int32_t op_dtype, const uint16_t* qkv, const uint16_t* dout, const uint16_t* o, const float* lse, float* delta_ws, int32_t B, int32_t S,
                     int32_t H, int32_t hd, int32_t causal, uint16_t* dqkv, void* stream);
/* The same two launchers with attention-probability dropout and the operand-image outputs of the split-bf16 build.  Test hooks: the
 * product path never calls them.  p = 0: no dropout; otherwise the mask stream cc_dropout_mask(seed, 1, layer, p, ...) returns, element
 * index ((b H + h) S + i) S + j (query i, key j), kept probabilities scaled by 1 / (1 - p); p outside [0, 1) or layer outside 0..255:
 * CC_ERR_ARG.  Dropout needs causal != 0 and a kernel that carries it (CC_ERR_SHAPE otherwise, nothing is written).  out_img / dqkv_img:
 * 0, or (CC_OP_BF16X3 only) H hd / 3 H hd: out / dqkv receive the [hi | hi | lo] operand image of the GEMM that reads them (rows of
 * 3 H hd / 9 H hd 16-bit elements, cc_x3_split_rows form 0 of the fp32 rows); a shape whose kernels cannot write images returns
 * CC_ERR_STATE, any other non-zero value in that build CC_ERR_STATE, a non-zero value in the 16-bit builds CC_ERR_ARG. */
int cc_attention_fwd_x(int32_t op_dtype, const uint16_t* qkv, int32_t B, int32_t S, int32_t H, int32_t hd, int32_t causal, uint16_t* out, int32_t out_img,
                       float* lse, float p, uint64_t seed, int32_t layer, void* stream);
int cc_attention_bwd_x(int32_t op_dtype, const uint16_t* qkv, const uint16_t* dout, const uint16_t* o, const float* lse, float* delta_ws, int32_t B, int32_t S,
                       int32_t H, int32_t hd, int32_t causal, uint16_t* dqkv, int32_t dqkv_img, float p, uint64_t seed, int32_t layer, void* stream);
/* The lm_head / loss chain (cc_lmhead_ce_fwd, cc_lmhead_ce_bwd, cc_lmhead_score) on a caller's input, and its per-row state.  Test hooks:
 * the product path never calls them.  Both carve the workspace of (cfg, shp) exactly as the entry points of the pass do and copy with
 * hipMemcpyAsync on the call's stream; they launch no kernel and do not change cc_gpt2_ws_bytes.
 * cc_lmhead_put_x: x fp32 [B*T][D] becomes the final residual stream of the pass (what cc_gpt2_fwd leaves for ln_f).
 * cc_lmhead_get: copies one field into dst, dst_bytes = the field's exact byte count (CC_ERR_SHAPE otherwise; CC_ERR_STATE for a field
 * the shape's mode does not carve: a mode-0 pass keeps only CC_LM_LSE, CC_LM_TGT and CC_LM_HF; CC_ERR_SHAPE also for a shape without
 * caption rows, T == L; CC_ERR_ARG for NULL pointers or an unknown
 * field).  Rows are the B*cap caption rows (cap = T - L), row b*cap + c = position L-1+c of sample b; "stored type" = the operand type's
 * 16-bit element, fp32 in CC_OP_BF16X3. */
#define CC_LM_LSE 0        /* fp32 [B*cap]: log-sum-exp of the row's logits */
#define CC_LM_TGT 1        /* fp32 [B*cap]: the target logit the loss used (the reference shift of the exponential form, the epilogue's value otherwise) */
#define CC_LM_ROW_LOSS 2   /* fp32 [B*cap]: lse - target logit, 0 on ignored rows */
#define CC_LM_HF 3         /* stored type [B*cap][D]: ln_f output rows */
#define CC_LM_DHF 4        /* stored type [B*cap][D]: gradient of the ln_f output rows (after cc_lmhead_ce_bwd) */
#define CC_LM_DX32 5       /* fp32 [B*T][D]: gradient of the final residual stream (after cc_lmhead_ce_bwd) */
int cc_lmhead_put_x(const cc_gpt2_cfg* cfg, const cc_gpt2_shape* shp, void* ws, const float* x, void* stream);
int cc_lmhead_get(const cc_gpt2_cfg* cfg, const cc_gpt2_shape* shp, void* ws, int32_t field, void* dst, int64_t dst_bytes, void* stream);
/* The cross-block reductions of the backward passes, one call each (the training step reaches them only inside cc_mapper_bwd*,
 * cc_gpt2_bwd* and cc_lmhead_ce_bwd).  Test hooks: the product path never calls them.  Every gradient output is ACCUMULATED (+=).
 * red_ws = device scratch of cc_red_scratch_floats() floats for the per-block partial sums, used by this call only; a shape whose
 * sum spans several blocks returns CC_ERR_STATE without it and writes nothing.  bf16 / fp16 operands only (CC_OP_BF16X3: CC_ERR_ARG).
 * cc_layernorm_bwd: LayerNorm backward of `rows` rows of width D.  dy [rows][D] 16-bit, mean / rstd [rows]; x, dres, dx32 fp32 and dx16
 * 16-bit rows of stride ldx, row r of them at row_map[r] (row_map NULL: at r).  dx32 = dres (nullable) + d LayerNorm input; dx16
 * (nullable) = its 16-bit copy; dgamma / dbeta [D] (both or neither) += the parameter gradients; dcol [D] (nullable, needs dgamma and
 * dx16, no row_map) += the column sums of the 16-bit dx16 values. */
int64_t cc_red_scratch_floats(void);
int cc_layernorm_bwd(int32_t op_dtype, const uint16_t* dy, const float* x, int32_t ldx, const int32_t* row_map, const float* mean,
                     const float* rstd, const float* gamma, const float* dres, float* dx32, uint16_t* dx16, float* dgamma, float* dbeta,
                     float* dcol, int32_t rows, int32_t D, float* red_ws, void* stream);
/* out[n] += sum over m of X[m][n]  (X 16-bit [M][ld], N % 8 == 0, ld % 8 == 0) */
int cc_colsum_bf16(int32_t op_dtype, const uint16_t* X, int32_t ld, int32_t M, int32_t N, float* out, float* red_ws, void* stream);
/* the same for n <= 32 equally shaped matrices in one launch (n > 32: CC_ERR_ARG); X_host[i] / out_host[i] = host arrays of device pointers */
int cc_colsum_multi(int32_t op_dtype, const uint16_t* const* X_host, float* const* out_host, int32_t n, int32_t ld, int32_t M, int32_t N,
                    float* red_ws, void* stream);
/* dst[i] += sum over b < B of src[b * src_stride + i], i < len  (fp32) */
int cc_batch_sum(const float* src, int64_t src_stride, float* dst, int32_t len, int32_t B, float* red_ws, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * MLP mapping network (the ClipCap paper's other mapper; the `clip_project` of the original checkpoints):
 *   prefix = reshape(Linear(Hd -> L D)(tanh(Linear(E -> Hd)(emb))), [B][L][D]),   Hd = L D / 2.
 * Two GEMMs whose cost is weight bytes.  Arena order (state-dict names of the original's nn.Sequential): model.0.weight [Hd][E],
 * model.0.bias [Hd], model.2.weight [L D][Hd], model.2.bias [L D].  The w16 arena follows the conventions above: [0, n) the cast,
 * [n, 2n) the transposed copy of model.2.weight at its own offset (model.0.weight has none: no gradient flows to emb); CC_OP_BF16X3:
 * 6n elements, the [hi | lo | hi] images of both weights at 3 off and of model.2.weight's transpose at 3 (n + off).
 * E, D and Hd must be multiples of 8, Hd == L D / 2 exactly (so L D is a multiple of 16) and L D <= 2^24: CC_ERR_SHAPE from the count / offset / size
 * calls, CC_ERR_ARG from the passes, before anything is launched.
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct {
    int32_t E;        /* encoder_embedding_size */
    int32_t D;        /* lm_embedding_size */
    int32_t L;        /* prefix_length */
    int32_t Hd;       /* hidden width = (L * D) / 2 */
    int32_t op_dtype; /* CC_OP_BF16 / CC_OP_FP16 / CC_OP_BF16X3 */
} cc_mlp_cfg;
#define CC_MLP_TENSORS 4
int64_t cc_mlp_param_count(const cc_mlp_cfg* cfg);
int cc_mlp_param_offsets(const cc_mlp_cfg* cfg, int64_t* offsets /* [CC_MLP_TENSORS] */);
/* save != 0: the workspace also carries what cc_mlp_bwd needs (t, the backward's buffers and scratch).  B <= 0: CC_ERR_SHAPE */
int64_t cc_mlp_ws_bytes(const cc_mlp_cfg* cfg, int32_t B, int32_t save);
int cc_mlp_sync_weights(const cc_mlp_cfg* cfg, const float* w32, uint16_t* w16, void* stream);
int cc_mlp_transpose_weights(const cc_mlp_cfg* cfg, uint16_t* w16, void* stream);      /* the [n, 2n) half only (CC_OP_BF16X3: CC_ERR_ARG) */
/* x16 = cast(emb [B][E]); h = tanh(x16 W1^T + b1) (and, save != 0, t = 1 - h h from the fp32 h); out [B][L D] fp32 = h W2^T + b2 */
int cc_mlp_fwd(const cc_mlp_cfg* cfg, int32_t B, const float* w32, const uint16_t* w16, const float* emb, void* ws, float* out, int32_t save,
               void* stream);
/* After cc_mlp_fwd(save = 1) on the same workspace.  g32 is ACCUMULATED into.  g16 = cast(dout [B][L D]); db2 += sum_b dout (fp32);
 * dW2 += g16^T h; dU = (g16 W2) * t; dW1 += dU^T x16; db1 += column sums of dU.  No gradient for emb.  Every cross-block sum folds in a
 * fixed order through the workspace's reduction scratch (no atomics): the same bits from run to run.
 * cc_mlp_bwd_part: part 1 = g16, db2, dW2, dU (the gradients of model.2.*, 94 % of the arena at E = 512, D = 768, L = 10); part 0 = dW1,
 * db1 (model.0.*), which reads the dU part 1 left: call part 1 first.  cc_mlp_bwd = part 1 then part 0.  Any other part: CC_ERR_ARG. */
int cc_mlp_bwd(const cc_mlp_cfg* cfg, int32_t B, const float* w32, const uint16_t* w16, void* ws, const float* dout, float* g32, void* stream);
int cc_mlp_bwd_part(const cc_mlp_cfg* cfg, int32_t B, const float* w32, const uint16_t* w16, void* ws, const float* dout, float* g32, int32_t part,
                    void* stream);
/* Test hook: a raw copy (hipMemcpyAsync on the call's stream, no kernel) of one field of the save = 1 workspace of (cfg, B) into dst;
 * dst_bytes = the field's exact byte count (CC_ERR_SHAPE otherwise; CC_ERR_ARG for NULL pointers or an unknown field).  Every field is
 * plain row-major in the stored type: the operand type's 16-bit element, fp32 in CC_OP_BF16X3 (where the GEMMs split it at their boundary). */
#define CC_MLP_X16 0      /* [B][E]    cast of emb */
#define CC_MLP_H 1        /* [B][Hd]   tanh output */
#define CC_MLP_T 2        /* [B][Hd]   1 - h h */
#define CC_MLP_G16 3      /* [B][L D]  cast of dout (after cc_mlp_bwd_part 1) */
#define CC_MLP_DU 4       /* [B][Hd]   gradient of the pre-activation (after cc_mlp_bwd_part 1) */
int cc_mlp_get(const cc_mlp_cfg* cfg, int32_t B, void* ws, int32_t field, void* dst, int64_t dst_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Measurement aid for bench.py's roofline line: brackets every launch of ONE GEMM call site — or, with CC_SITE_ALL_GEMMS, every
 * GEMM host launch of the library — with HIP events recorded on the launch stream.  PROCESS-WIDE, off by default, never used by
 * the product path.
 * ------------------------------------------------------------------------------------------------------------ */
#define CC_SITE_LMHEAD_FWD 1      /* [B*cap, D] x wte^T           (cc_lmhead_ce_fwd, cc_lmhead_score) */
#define CC_SITE_LMHEAD_DGRAD 2    /* dlogits [B*cap, Vp] x wte    (cc_lmhead_ce_bwd) */
#define CC_SITE_GPT2_FC_FWD 3     /* c_fc  [B*T, D] x [D, 4D]     (cc_gpt2_fwd, per layer) */
#define CC_SITE_GPT2_PROJ2_FWD 4  /* mlp.c_proj [B*T, 4D] x [4D, D] (cc_gpt2_fwd) */
#define CC_SITE_GPT2_FC_DGRAD 5   /* d u-> d xn2  [B*T, 4D] x [4D(k), D] (cc_gpt2_bwd) */
#define CC_SITE_MAPPER_FC1_FWD 6  /* fc1 [B*S, D] x [Hm, D]^T     (cc_mapper_fwd) */
#define CC_SITE_MAPPER_QKV_FWD 7  /* fused q/kv projection         (cc_mapper_fwd) */
#define CC_SITE_MAPPER_WGRAD_FC2 8 /* dW2 = dx^T h (split-K)       (cc_mapper_bwd) */
#define CC_SITE_ALL_GEMMS 100      /* every MFMA GEMM launch (forward, dgrad, wgrad, lm_head, decode), with its 2*M*N*K */
int cc_prof_start(int32_t site, int32_t max_samples);
/* waits for the recorded events; writes up to *n (in: capacity, out: count) durations in milliseconds and (flops_host nullable) the
 * algorithmic FLOPs 2*M*N*K of each bracketed launch (host arrays) */
int cc_prof_stop(float* ms_host, double* flops_host, int32_t* n_host);

#ifdef __cplusplus
}
#endif
#endif /* CLIPCAP_HIP_H */
