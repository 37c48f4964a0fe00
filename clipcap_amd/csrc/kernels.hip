// Operand plumbing of the ClipCap path for gfx950: casts, slices, row copies, transposes, dropout, embedding assembly, AdamW (it writes
// the operand type) and the split-bf16 operand images.  LayerNorm lives in layernorm.hip, the deterministic reductions in reduce.hip, the
// lm_head loss rows in loss.hip, the gradient utilities in grads.hip, attention in attention.hip.
// All are wave64 code; memory accesses are 16-B vectors wherever the layout allows.
#include "kernels.h"
#include "gemm_api.h"

namespace CC_NS {

// ------------------------------------------------------------------------------------------------------------
// element-wise helpers
// ------------------------------------------------------------------------------------------------------------
// eight consecutive floats as two 16-B loads (p aligned to 16 B)
__device__ __forceinline__ void ld8_f32(const float* p, float (&v)[8]) {
    const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
__global__ void k_f32_to_bf16(const float* __restrict__ src, op16_t* __restrict__ dst, size_t n8) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (size_t)gridDim.x * blockDim.x) {
        float v[8];
        ld8_f32(src + 8 * i, v);
        reinterpret_cast<uint4*>(dst)[i] = pack8(v);
    }
}
int f32_to_bf16(const float* src, op16_t* dst, size_t n, hipStream_t st) {
    if (n & 7) return CC_ERR_SHAPE;
    const size_t n8 = n >> 3;
    if (!n8) return CC_OK;
    hipLaunchKernelGGL(k_f32_to_bf16, flat_grid(n8, 256, 2048), dim3(256), 0, st, src, dst, n8);
    return CC_OK;
}

int f32_to_act(const float* src, act_t* dst, size_t n, hipStream_t st) {
    if constexpr (kX3) {
        if (!n) return CC_OK;
        return hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyDeviceToDevice, st) == hipSuccess ? CC_OK : CC_ERR_LAUNCH;
    } else {
        return f32_to_bf16(src, reinterpret_cast<op16_t*>(dst), n, st);
    }
}

// dst[b*dst_stride + i] = (bf16) src[b*src_stride + i], i < len (len % 8 == 0)
__global__ void k_slice_f32_to_bf16(const float* __restrict__ src, size_t src_stride, act_t* __restrict__ dst,
                                    size_t dst_stride, int len8, int B) {
    const size_t total = (size_t)len8 * B;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int b = (int)(i / len8), c = (int)(i % len8);
        const float* s = src + b * src_stride + (size_t)c * 8;
        float v[8];
        ld8_f32(s, v);
        act_st8(dst + b * dst_stride + (size_t)c * 8, v);
    }
}
int slice_f32_to_bf16(const float* src, size_t src_stride, act_t* dst, size_t dst_stride, int len, int B, hipStream_t st) {
    if (len & 7) return CC_ERR_SHAPE;
    const size_t total = (size_t)(len >> 3) * B;
    if (!total) return CC_OK;
    hipLaunchKernelGGL(k_slice_f32_to_bf16, flat_grid(total, 256, 2048), dim3(256), 0, st, src, src_stride, dst, dst_stride, len >> 3, B);
    return CC_OK;
}

// dst[b*dst_stride + i] = src[i] (+ add[i])  — broadcast a learned block (prefix_const) into every sample
__global__ void k_broadcast_rows(float* __restrict__ dst, size_t dst_stride, const float* __restrict__ src, int len4, int B) {
    const size_t total = (size_t)len4 * B;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int b = (int)(i / len4), c = (int)(i % len4);
        reinterpret_cast<float4*>(dst + b * dst_stride)[c] = reinterpret_cast<const float4*>(src)[c];
    }
}
int broadcast_rows(float* dst, size_t dst_stride, const float* src, int len, int B, hipStream_t st) {
    if (len & 3) return CC_ERR_SHAPE;
    const size_t total = (size_t)(len >> 2) * B;
    if (!total) return CC_OK;
    hipLaunchKernelGGL(k_broadcast_rows, flat_grid(total, 256, 2048), dim3(256), 0, st, dst, dst_stride, src, len >> 2, B);
    return CC_OK;
}

// dst[b*dst_stride + i] += add[i]  (positional embeddings of the windowed mapper)
__global__ void k_add_rows(float* __restrict__ dst, size_t dst_stride, const float* __restrict__ add, int len, int B) {
    const size_t total = (size_t)len * B;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int b = (int)(i / len), c = (int)(i % len);
        dst[b * dst_stride + c] += add[c];
    }
}
int add_rows(float* dst, size_t dst_stride, const float* add, int len, int B, hipStream_t st) {
    const size_t total = (size_t)len * B;
    if (!total) return CC_OK;
    hipLaunchKernelGGL(k_add_rows, flat_grid(total, 256, 2048), dim3(256), 0, st, dst, dst_stride, add, len, B);
    return CC_OK;
}

// dst[b*dst_stride + i] = src[b*src_stride + i]  fp32 strided copy (len % 4 == 0)
__global__ void k_copy_rows(const float* __restrict__ src, size_t src_stride, float* __restrict__ dst, size_t dst_stride, int len4, int B) {
    const size_t total = (size_t)len4 * B;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int b = (int)(i / len4), c = (int)(i % len4);
        reinterpret_cast<float4*>(dst + b * dst_stride)[c] = reinterpret_cast<const float4*>(src + b * src_stride)[c];
    }
}
int copy_rows(const float* src, size_t src_stride, float* dst, size_t dst_stride, int len, int B, hipStream_t st) {
    if (len & 3) return CC_ERR_SHAPE;
    const size_t total = (size_t)(len >> 2) * B;
    if (!total) return CC_OK;
    hipLaunchKernelGGL(k_copy_rows, flat_grid(total, 256, 2048), dim3(256), 0, st, src, src_stride, dst, dst_stride, len >> 2, B);
    return CC_OK;
}

// dst[c][r] = src[r][c] for bf16 matrices [R][C] (R, C multiples of 8): 64x64 tiles through LDS, 16-B global accesses both ways.
// Several matrices in one launch (the per-step weight sync transposes 4 small matrices per layer): blockIdx.z picks the matrix, blocks
// outside its extents exit.
__global__ __launch_bounds__(256) void k_transpose_bf16_multi(TransposeBatch b) {
    const TransposeBatch::Item& m = b.it[blockIdx.z];
    if ((int)blockIdx.x * 64 >= m.C || (int)blockIdx.y * 64 >= m.R) return;
    __shared__ op16_t tile[64][66];
    const int r0 = blockIdx.y * 64, c0 = blockIdx.x * 64, R = m.R, C = m.C;
    const int cg = threadIdx.x & 7, rl = threadIdx.x >> 3;  // 8 column groups x 32 rows, two passes
#pragma unroll
    for (int p = 0; p < 2; p++) {
        const int r = r0 + rl + 32 * p, c = c0 + cg * 8;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (r < R && c < C) v = *reinterpret_cast<const uint4*>(m.src + (size_t)r * C + c);
        const op16_t* e = reinterpret_cast<const op16_t*>(&v);
#pragma unroll
        for (int k = 0; k < 8; k++) tile[rl + 32 * p][cg * 8 + k] = e[k];
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < 2; p++) {
        const int c = c0 + rl + 32 * p, r = r0 + cg * 8;   // output row = source column
        if (c < C && r < R) {
            op16_t e[8];
#pragma unroll
            for (int k = 0; k < 8; k++) e[k] = tile[cg * 8 + k][rl + 32 * p];
            *reinterpret_cast<uint4*>(m.dst + (size_t)c * R + r) = *reinterpret_cast<const uint4*>(e);
        }
    }
}
int transpose_bf16_multi(const TransposeBatch& b, hipStream_t st) {
    if (b.n <= 0) return CC_OK;
    int mr = 0, mc = 0;
    for (int i = 0; i < b.n; i++) {
        if ((b.it[i].R & 7) || (b.it[i].C & 7)) return CC_ERR_SHAPE;
        mr = std::max(mr, b.it[i].R);
        mc = std::max(mc, b.it[i].C);
    }
    hipLaunchKernelGGL(k_transpose_bf16_multi, dim3((mc + 63) / 64, (mr + 63) / 64, b.n), dim3(256), 0, st, b);
    return hipGetLastError() == hipSuccess ? CC_OK : CC_ERR_LAUNCH;
}
int transpose_bf16(const op16_t* src, op16_t* dst, int R, int C, hipStream_t st) {
    if ((R & 7) || (C & 7)) return CC_ERR_SHAPE;
    if (R <= 0 || C <= 0) return CC_OK;
    TransposeBatch b;      // one matrix = a batch of one: the same grid, no block outside the extents
    b.add(src, dst, R, C);
    return transpose_bf16_multi(b, st);
}

// ------------------------------------------------------------------------------------------------------------
// GPT-2 input assembly: x0[b,t,:] = (t < L ? prefix[b,t,:] : wte[tok[b,t-L],:]) + wpe[pos0 + t,:]   (fp32)
// (clipcap/model/model.py:45-49 + hf modeling_gpt2.py:571-577).  tokens < 0 (pads) are read as id 0 (model.py:104).
// ------------------------------------------------------------------------------------------------------------
// In-place dropout (common.hip.h: counter-based mask): embedding dropout on x0 / dx0 (fp32) and the masked bf16 copy of the residual
// gradient that feeds a c_proj backward.
// ------------------------------------------------------------------------------------------------------------
__global__ void k_dropout_f32(float* __restrict__ x, size_t n4, Drop d) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        float4 v = reinterpret_cast<float4*>(x)[i];
        const unsigned e = (unsigned)(i * 4);
        float m0, m1, m2, m3;
        drop_mul_pair(d, e, m0, m1);
        drop_mul_pair(d, e + 2, m2, m3);
        v.x *= m0; v.y *= m1; v.z *= m2; v.w *= m3;
        reinterpret_cast<float4*>(x)[i] = v;
    }
}
__global__ void k_dropout_bf16(act_t* __restrict__ x, size_t n8, Drop d) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (size_t)gridDim.x * blockDim.x) {
        float f[8];
        act_ld8(x + i * 8, f);
        const unsigned e = (unsigned)(i * 8);
#pragma unroll
        for (int k = 0; k < 8; k += 2) {
            float m0, m1;
            drop_mul_pair(d, e + k, m0, m1);
            f[k] *= m0; f[k + 1] *= m1;
        }
        act_st8(x + i * 8, f);
    }
}
__global__ void k_dropout_mask(unsigned char* __restrict__ out, size_t n, Drop d) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        out[i] = (d.thresh == 0 || drop_keep(d, (unsigned)i)) ? 1 : 0;
}
int dropout_f32(float* x, size_t n, Drop d, hipStream_t st) {
    if (!d.thresh || !n) return CC_OK;
    if (n & 3) return CC_ERR_SHAPE;
    hipLaunchKernelGGL(k_dropout_f32, flat_grid(n / 4, 256, 4096), dim3(256), 0, st, x, n / 4, d);
    return CC_OK;
}
int dropout_bf16(act_t* x, size_t n, Drop d, hipStream_t st) {
    if (!d.thresh || !n) return CC_OK;
    if (n & 7) return CC_ERR_SHAPE;
    hipLaunchKernelGGL(k_dropout_bf16, flat_grid(n / 8, 256, 4096), dim3(256), 0, st, x, n / 8, d);
    return CC_OK;
}
int dropout_mask_u8(unsigned char* out, size_t n, Drop d, hipStream_t st) {
    if (!n) return CC_OK;
    hipLaunchKernelGGL(k_dropout_mask, flat_grid(n, 256, 4096), dim3(256), 0, st, out, n, d);
    return CC_OK;
}

// ------------------------------------------------------------------------------------------------------------
__global__ void k_embed_concat(const float* __restrict__ prefix, const long long* __restrict__ tokens, int cap,
                               const float* __restrict__ wte, const float* __restrict__ wpe, float* __restrict__ x0,
                               int B, int L, int T, int D, int pos0) {
    const int d4n = D >> 2;
    const size_t total = (size_t)B * T * d4n;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % d4n);
        const int t = (int)((i / d4n) % T), b = (int)(i / ((size_t)d4n * T));
        float4 v;
        if (t < L)
            v = reinterpret_cast<const float4*>(prefix + ((size_t)b * L + t) * D)[c];
        else {
            long long id = tokens[(size_t)b * cap + (t - L)];
            if (id < 0) id = 0;
            v = reinterpret_cast<const float4*>(wte + (size_t)id * D)[c];
        }
        const float4 p = reinterpret_cast<const float4*>(wpe + (size_t)(pos0 + t) * D)[c];
        reinterpret_cast<float4*>(x0)[i] = make_float4(v.x + p.x, v.y + p.y, v.z + p.z, v.w + p.w);
    }
}
int embed_concat(const float* prefix, const long long* tokens, int cap, const float* wte, const float* wpe, float* x0, int B, int L,
                 int T, int D, int pos0, hipStream_t st) {
    if (D & 3) return CC_ERR_SHAPE;
    const size_t total = (size_t)B * T * (D >> 2);
    if (!total) return CC_OK;
    hipLaunchKernelGGL(k_embed_concat, flat_grid(total, 256, 4096), dim3(256), 0, st, prefix, tokens, cap, wte, wpe, x0, B, L, T, D, pos0);
    return CC_OK;
}

// dst[r][c] = op16(src[r][c]) for c < V, 0 for V <= c < ldd (gradient of caller-visible fp32 logits -> the GEMM operand layout)
__global__ __launch_bounds__(256) void k_f32_to_op16_pad(const float* __restrict__ src, long long lds, int V, act_t* __restrict__ dst, int ldd,
                                                         int M) {
    const size_t total = (size_t)M * ldd;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % ldd);
        const size_t r = i / ldd;
        dst[i] = c < V ? f2act(src[r * lds + c]) : (act_t)0;
    }
}
int f32_to_op16_pad(const float* src, long long lds, int V, act_t* dst, int ldd, int M, hipStream_t st) {
    const size_t total = (size_t)M * ldd;
    if (!total) return CC_OK;
    hipLaunchKernelGGL(k_f32_to_op16_pad, flat_grid(total, 256, 8192), dim3(256), 0, st, src, lds, V, dst, ldd, M);
    return CC_OK;
}

// ------------------------------------------------------------------------------------------------------------
// Flat AdamW (torch.optim.AdamW math, decoupled decay) over one parameter arena.  HBM-bound: 16 B read + 12 B written per
// parameter.  inv_scale (device, nullable) = loss scale to divide out of the gradients; found_inf (device, nullable) != 0 skips
// the whole step (the GradScaler rule for an overflowed fp16 backward).
// ------------------------------------------------------------------------------------------------------------
template <bool DEVSTEP, bool EMA>      // DEVSTEP: Adam's step number is read from the loss scaler's device-side count (a separate instantiation: the
                             // pow evaluation must not cost the common kernel its registers — it measured 184 -> 223 us as a run-time branch)
                             // EMA: also ema = d * ema + (1 - d) * p over the parameters just written (+4 B read, +4 B written per parameter); a
                             // separate instantiation for the same reason, so the two plain forms compile from the text they always had
__global__ __launch_bounds__(256) void k_adamw(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                               float* __restrict__ v, size_t n4, float lr, float b1, float b2, float eps, float wd, float bc1,
                                               float bc2_sqrt, float gscale, const float* __restrict__ loss_scale,
                                               const float* __restrict__ found_inf, op16_t* __restrict__ w16,
                                               const float* __restrict__ clip, float* __restrict__ ema, float d) {
    if (found_inf && found_inf[0] != 0.f) return;      // a skipped step skips the average too
    if (loss_scale) gscale /= loss_scale[0];
    if (clip) gscale *= clip[0];      // global-norm clip coefficient (k_grad_clip_coef); 1.0f leaves gscale's bits as they are
    if constexpr (DEVSTEP) {      // step number = 1 + the loss scaler's count of APPLIED steps (loss_scale[2]): a skipped step does not advance Adam's bias correction
        const float t = loss_scale[2] + 1.0f;
        bc1 = 1.0f - __builtin_amdgcn_exp2f(t * __log2f(b1));
        bc2_sqrt = sqrtf(1.0f - __builtin_amdgcn_exp2f(t * __log2f(b2)));
    }
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        float4 P = reinterpret_cast<float4*>(p)[i], G = reinterpret_cast<const float4*>(g)[i];
        float4 M = reinterpret_cast<float4*>(m)[i], V = reinterpret_cast<float4*>(v)[i];
        float4 E;
        if constexpr (EMA) E = reinterpret_cast<float4*>(ema)[i];
        float* pp = &P.x; float* gg = &G.x; float* mm = &M.x; float* vv = &V.x;
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const float gr = gg[e] * gscale;
            pp[e] *= (1.0f - lr * wd);
            mm[e] = b1 * mm[e] + (1.0f - b1) * gr;
            vv[e] = b2 * vv[e] + (1.0f - b2) * gr * gr;
            const float denom = sqrtf(vv[e]) / bc2_sqrt + eps;
            pp[e] -= (lr / bc1) * (mm[e] / denom);
        }
        reinterpret_cast<float4*>(p)[i] = P;
        reinterpret_cast<float4*>(m)[i] = M;
        reinterpret_cast<float4*>(v)[i] = V;
        // the 16-bit operand copy of the updated parameters, while they are in registers: saves the separate cast pass over the arena
        if (w16) reinterpret_cast<uint2*>(w16)[i] = make_uint2(pack2op(P.x, P.y), pack2op(P.z, P.w));
        if constexpr (EMA) {      // the convex form (d = 0 gives ema == p exactly), never e + (1 - d)(p - e): p - e can overflow or cancel
            const float omd = 1.0f - d;
            E.x = d * E.x + omd * P.x; E.y = d * E.y + omd * P.y; E.z = d * E.z + omd * P.z; E.w = d * E.w + omd * P.w;
            reinterpret_cast<float4*>(ema)[i] = E;
        }
    }
}
int adamw(float* p, const float* g, float* m, float* v, size_t n, float lr, float b1, float b2, float eps, float wd, int step, float gscale,
          const float* loss_scale, const float* found_inf, hipStream_t st, op16_t* w16, const float* clip, float* ema, float ema_decay) {
    if (n & 3) return CC_ERR_SHAPE;
    if (!n) return CC_OK;
    if (step < 1 && !loss_scale) return CC_ERR_ARG;
    const float bc1 = 1.0f - powf(b1, (float)std::max(step, 1));
    const float bc2s = sqrtf(1.0f - powf(b2, (float)std::max(step, 1)));
    const size_t n4 = n >> 2;
    const dim3 gr = flat_grid(n4, 256, 4096);
#define CC_ADAMW_(DEVSTEP, EMA) \
    hipLaunchKernelGGL((k_adamw<DEVSTEP, EMA>), gr, dim3(256), 0, st, p, g, m, v, n4, lr, b1, b2, eps, wd, bc1, bc2s, gscale, loss_scale, found_inf, w16, clip, ema, ema_decay)
    if (ema) {
        if (step < 1) CC_ADAMW_(true, true);
        else CC_ADAMW_(false, true);
    } else if (step < 1) CC_ADAMW_(true, false);
    else CC_ADAMW_(false, false);
#undef CC_ADAMW_
    return CC_OK;
}

#if CC_OP == 2
// ------------------------------------------------------------------------------------------------------------
// bf16x3 operand pairs (common.hip.h): x -> hi = bf16(x), lo = bf16(x - hi) (x - hi is exact in fp32), laid out along K so that the
// unchanged NT kernels, run over K' = 3K, compute hi*hi + hi*lo + lo*hi:  A operand [hi | hi | lo],  B operand [hi | lo | hi].
// ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_x3_split_rows(const float* __restrict__ src, size_t lds, op16_t* __restrict__ dst, int M, int K, int form) {
    const int k8 = K >> 3;
    const size_t total = (size_t)M * k8;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t r = i / k8;
        const int c = (int)(i - r * k8) * 8;
        float f[8];
        ld8_f32(src + r * lds + c, f);
        uint4 hi, lo;
        x3_pair8(f, hi, lo);
        x3_store(dst + r * 3 * (size_t)K, K, c, form, hi, lo);
    }
}
int x3_split_rows(const float* src, size_t lds, op16_t* dst, int M, int K, int form, hipStream_t st) {
    if ((K & 7) || (lds & 3) || ((uintptr_t)src & 15) || ((uintptr_t)dst & 15)) return CC_ERR_SHAPE;
    const size_t total = (size_t)M * (K >> 3);
    if (!total) return CC_OK;
    hipLaunchKernelGGL(k_x3_split_rows, flat_grid(total, 256, 8192), dim3(256), 0, st, src, lds, dst, M, K, form);
    return hipGetLastError() == hipSuccess ? CC_OK : CC_ERR_LAUNCH;
}
// weights: 64 x 64 source tiles; tr = 1 goes through LDS so that both the fp32 reads and the 16-bit writes are row-contiguous
__global__ __launch_bounds__(256) void k_x3_split_multi(X3SplitBatch b) {
    const X3SplitBatch::Item& m = b.it[blockIdx.z];
    if ((int)blockIdx.x * 64 >= m.C || (int)blockIdx.y * 64 >= m.R) return;
    __shared__ float tile[64][65];
    const int r0 = blockIdx.y * 64, c0 = blockIdx.x * 64, R = m.R, C = m.C;
    const int cg = threadIdx.x & 7, rl = threadIdx.x >> 3;      // 8 chunks of 8 columns x 32 rows, two passes
    if (!m.tr) {
#pragma unroll
        for (int p = 0; p < 2; p++) {
            const int r = r0 + rl + 32 * p, c = c0 + cg * 8;
            if (r < R && c < C) {
                float f[8];
                ld8_f32(m.src + (size_t)r * C + c, f);
                uint4 hi, lo;
                x3_pair8(f, hi, lo);
                x3_store(m.dst + (size_t)r * 3 * C, C, c, m.form, hi, lo);
            }
        }
        return;
    }
#pragma unroll
    for (int p = 0; p < 2; p++) {
        const int r = r0 + rl + 32 * p, c = c0 + cg * 8;
        float f[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (r < R && c < C) ld8_f32(m.src + (size_t)r * C + c, f);
#pragma unroll
        for (int k = 0; k < 8; k++) tile[rl + 32 * p][cg * 8 + k] = f[k];
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < 2; p++) {
        const int c = c0 + rl + 32 * p, r = r0 + cg * 8;       // output row = source column c, 8 consecutive source rows
        if (c < C && r < R) {
            float f[8];
#pragma unroll
            for (int k = 0; k < 8; k++) f[k] = tile[cg * 8 + k][rl + 32 * p];
            uint4 hi, lo;
            x3_pair8(f, hi, lo);
            x3_store(m.dst + (size_t)c * 3 * R, R, r, m.form, hi, lo);
        }
    }
}
int x3_split_multi(const X3SplitBatch& b, hipStream_t st) {
    if (b.n <= 0) return CC_OK;
    int mr = 0, mc = 0;
    for (int i = 0; i < b.n; i++) {
        if ((b.it[i].R & 7) || (b.it[i].C & 7)) return CC_ERR_SHAPE;
        mr = std::max(mr, b.it[i].R);
        mc = std::max(mc, b.it[i].C);
    }
    hipLaunchKernelGGL(k_x3_split_multi, dim3((mc + 63) / 64, (mr + 63) / 64, b.n), dim3(256), 0, st, b);
    return hipGetLastError() == hipSuccess ? CC_OK : CC_ERR_LAUNCH;
}

const op16_t* x3_operand(Call& cx, const float* src, size_t ld, int rows, int width, int form, bool first, int* rc) {
    if (first) cx.x3_used = 0;
    const size_t need = (((size_t)rows * 3 * width * sizeof(op16_t)) + 255) & ~size_t(255);
    if (!cx.x3 || cx.x3_used + need > cx.x3_bytes) { *rc = CC_ERR_STATE; return nullptr; }
    op16_t* dst = reinterpret_cast<op16_t*>(cx.x3 + cx.x3_used);
    cx.x3_used += need;
    *rc = x3_split_rows(src, ld, dst, rows, width, form, cx.st);
    return *rc == CC_OK ? dst : nullptr;
}
#endif   // CC_OP == 2

}  // namespace CC_NS
