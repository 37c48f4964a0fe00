// Gradient utilities of the training step for gfx950: the bf16 wire format of the gradient all-reduce, the non-finite scan and the
// loss-scale update (torch.cuda.amp.GradScaler semantics), the global squared norm and the clip coefficient.  fp32 / integer work only,
// so this unit is built once (Makefile) and its entry points are the *_bf16 symbols.
#include "kernels.h"
#include "layout.h"

namespace CC_NS {

// gradient wire format of the N-rank all-reduce (train/ddp.py, bf16 wire): fp32 arena slice <-> bf16 staging slice, any length / alignment
// (a layer's slice starts wherever its first parameter does).  Always bf16 (round to nearest even), whatever the operand build.
__device__ __forceinline__ unsigned short wire_bf16(float f) {
    const unsigned u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 0x40u);      // NaN stays NaN
    return (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
__global__ void k_wire_pack(const float* __restrict__ src, unsigned short* __restrict__ dst, size_t n) {
    for (size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += (size_t)gridDim.x * blockDim.x * 4) {
        if (i + 4 <= n && ((reinterpret_cast<size_t>(src + i) & 15) == 0) && ((reinterpret_cast<size_t>(dst + i) & 7) == 0)) {
            const float4 a = *reinterpret_cast<const float4*>(src + i);
            *reinterpret_cast<uint2*>(dst + i) = make_uint2(wire_bf16(a.x) | ((unsigned)wire_bf16(a.y) << 16), wire_bf16(a.z) | ((unsigned)wire_bf16(a.w) << 16));
        } else {
            for (size_t j = i; j < n && j < i + 4; j++) dst[j] = wire_bf16(src[j]);
        }
    }
}
__global__ void k_wire_unpack(const unsigned short* __restrict__ src, float* __restrict__ dst, size_t n) {
    for (size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += (size_t)gridDim.x * blockDim.x * 4) {
        if (i + 4 <= n && ((reinterpret_cast<size_t>(dst + i) & 15) == 0) && ((reinterpret_cast<size_t>(src + i) & 7) == 0)) {
            const uint2 a = *reinterpret_cast<const uint2*>(src + i);
            *reinterpret_cast<float4*>(dst + i) = make_float4(__uint_as_float(a.x << 16), __uint_as_float(a.x & 0xffff0000u), __uint_as_float(a.y << 16),
                                                              __uint_as_float(a.y & 0xffff0000u));
        } else {
            for (size_t j = i; j < n && j < i + 4; j++) dst[j] = __uint_as_float((unsigned)src[j] << 16);
        }
    }
}
static int wire_pack(const float* src, unsigned short* dst, size_t n, hipStream_t st) {      // grids: + 256 items = one block beyond ceil((n / 4) / 256)
    if (!n) return CC_OK;
    hipLaunchKernelGGL(k_wire_pack, flat_grid(n / 4 + 256, 256, 2048), dim3(256), 0, st, src, dst, n);
    return CC_OK;
}
static int wire_unpack(const unsigned short* src, float* dst, size_t n, hipStream_t st) {
    if (!n) return CC_OK;
    hipLaunchKernelGGL(k_wire_unpack, flat_grid(n / 4 + 256, 256, 2048), dim3(256), 0, st, src, dst, n);
    return CC_OK;
}

// ---- dynamic loss scaling (fp16 operands; torch.cuda.amp.GradScaler semantics, all on the device) ----
__global__ __launch_bounds__(256) void k_grad_nonfinite(const float* __restrict__ g, size_t n4, float* __restrict__ found_inf) {
    bool bad = false;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        const float4 G = reinterpret_cast<const float4*>(g)[i];
        // (x - x) is 0 for finite x and NaN for inf / NaN
        const float z = (G.x - G.x) + (G.y - G.y) + (G.z - G.z) + (G.w - G.w);
        bad |= !(z == 0.f);
    }
    if (__any(bad) && (threadIdx.x & 63) == 0) found_inf[0] = 1.0f;      // benign race: every writer stores the same value
}
static int grad_nonfinite(const float* g, size_t n, float* found_inf, hipStream_t st) {
    if (n & 3) return CC_ERR_SHAPE;
    if (!n) return CC_OK;
    const size_t n4 = n >> 2;
    hipLaunchKernelGGL(k_grad_nonfinite, flat_grid(n4, 256, 2048), dim3(256), 0, st, g, n4, found_inf);
    return CC_OK;
}
__global__ void k_loss_scale_update(float* state, float* found_inf, float growth, float backoff, int interval) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (found_inf[0] != 0.f) {
        state[0] = fmaxf(state[0] * backoff, 1.0f);
        state[1] = 0.f;
    } else {
        const float good = state[1] + 1.f;
        if (good >= (float)interval) {
            state[0] = fminf(state[0] * growth, 16777216.0f);
            state[1] = 0.f;
        } else {
            state[1] = good;
        }
        state[2] += 1.f;      // optimizer steps actually applied (read by the next cc_adamw_step called with step = 0)
    }
    found_inf[0] = 0.f;
}
static int loss_scale_update(float* state, float* found_inf, float growth, float backoff, int interval, hipStream_t st) {
    hipLaunchKernelGGL(k_loss_scale_update, dim3(1), dim3(64), 0, st, state, found_inf, growth, backoff, interval);
    return CC_OK;
}

// ---- global gradient norm + clip coefficient (torch.nn.utils.clip_grad_norm_, all on the device) ----
// sumsq[0] += sum g[i]^2 over a flat fp32 slice.  HBM-bound: 4 B read per parameter (AdamW moves 28).  Streaming-reduction shape: 16-byte
// loads, GRAD_NORM_ACC independent accumulators per thread (that many loads in flight), DPP wave_sum, cross-wave fold through LDS, one
// partial per block; a second, single-block launch folds the partials.  No atomics: the order is fixed by n alone (kernels.h states it).
__device__ __forceinline__ float sq4(const float4 G) { return (G.x * G.x + G.y * G.y) + (G.z * G.z + G.w * G.w); }
__global__ __launch_bounds__(GRAD_NORM_THREADS) void k_grad_sqnorm(const float* __restrict__ g, size_t n4, float* __restrict__ part) {
    static_assert(GRAD_NORM_THREADS == 256 && GRAD_NORM_ACC == 4, "the fold below is written for 4 waves and 4 accumulators");
    __shared__ float red[4];
    const float4* g4 = reinterpret_cast<const float4*>(g);
    const size_t S = (size_t)gridDim.x * GRAD_NORM_THREADS;
    size_t i = (size_t)blockIdx.x * GRAD_NORM_THREADS + threadIdx.x;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    for (; i + 3 * S < n4; i += 4 * S) {      // four visits per round: the loads are independent, each feeds its own accumulator
        const float4 G0 = g4[i], G1 = g4[i + S], G2 = g4[i + 2 * S], G3 = g4[i + 3 * S];
        a0 += sq4(G0); a1 += sq4(G1); a2 += sq4(G2); a3 += sq4(G3);
    }
    if (i < n4) a0 += sq4(g4[i]);             // the last (partial) round: visit k still goes to accumulator k % 4
    if (i + S < n4) a1 += sq4(g4[i + S]);
    if (i + 2 * S < n4) a2 += sq4(g4[i + 2 * S]);
    // every lane reaches the reduction (no early exit; a lane without elements brings 0): wave_sum's full-wave precondition
    const float w = wave_sum((a0 + a1) + (a2 + a3));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}
__global__ __launch_bounds__(GRAD_NORM_THREADS) void k_grad_sqnorm_fold(const float* __restrict__ part, int nb, float* __restrict__ sumsq) {
    __shared__ float red[4];
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < GRAD_NORM_BLOCKS / GRAD_NORM_THREADS; e++) {      // thread t: its run of consecutive partials, in index order
        const int j = threadIdx.x * (GRAD_NORM_BLOCKS / GRAD_NORM_THREADS) + e;
        if (j < nb) s += part[j];
    }
    const float w = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0) sumsq[0] += (red[0] + red[1]) + (red[2] + red[3]);
}
static int grad_sqnorm(const float* g, size_t n, float* scratch, float* sumsq, hipStream_t st) {
    if (n & 3) return CC_ERR_SHAPE;
    if (!n) return CC_OK;
    const size_t n4 = n >> 2;
    const int nb = (int)flat_grid(n4, GRAD_NORM_THREADS, GRAD_NORM_BLOCKS).x;
    hipLaunchKernelGGL(k_grad_sqnorm, dim3(nb), dim3(GRAD_NORM_THREADS), 0, st, g, n4, scratch);
    hipLaunchKernelGGL(k_grad_sqnorm_fold, dim3(1), dim3(GRAD_NORM_THREADS), 0, st, scratch, nb, sumsq);
    return CC_OK;
}
// clip[1] = sqrt(sumsq[0]) * grad_scale / (loss_scale ? loss_scale[0] : 1), the true (unscaled) norm; clip[0] = min(1, max_norm /
// (clip[1] + 1e-6)); a norm that is not finite gives clip[0] = NaN; max_norm = +inf gives exactly 1.0f
__global__ void k_grad_clip_coef(const float* sumsq, float max_norm, float grad_scale, const float* loss_scale, float* clip) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float norm = sqrtf(sumsq[0]) * grad_scale;
    if (loss_scale) norm /= loss_scale[0];
    clip[1] = norm;
    clip[0] = (norm - norm == 0.f) ? fminf(1.0f, max_norm / (norm + 1e-6f)) : __builtin_nanf("");
}
static int grad_clip_coef(const float* sumsq, float max_norm, float grad_scale, const float* loss_scale, float* clip, hipStream_t st) {
    hipLaunchKernelGGL(k_grad_clip_coef, dim3(1), dim3(64), 0, st, sumsq, max_norm, grad_scale, loss_scale, clip);
    return CC_OK;
}
}  // namespace CC_NS

using namespace CC_NS;

extern "C" {

int CC_API(cc_grad_sqnorm)(const float* g32, int64_t n, float* scratch, float* sumsq, void* stream) {
    if (!g32 || !scratch || !sumsq || n < 0) return CC_ERR_ARG;
    return grad_sqnorm(g32, (size_t)n, scratch, sumsq, S_(stream));
}

int CC_API(cc_grad_clip_coef)(const float* sumsq, float max_norm, float grad_scale, const float* loss_scale, float* clip, void* stream) {
    if (!sumsq || !clip || !(max_norm >= 0.f)) return CC_ERR_ARG;
    return grad_clip_coef(sumsq, max_norm, grad_scale, loss_scale, clip, S_(stream));
}

int CC_API(cc_grad_wire_pack)(const float* g32, uint16_t* wire, int64_t n, void* stream) {
    if (!g32 || !wire || n < 0) return CC_ERR_ARG;
    return wire_pack(g32, wire, (size_t)n, S_(stream));
}

int CC_API(cc_grad_wire_unpack)(const uint16_t* wire, float* g32, int64_t n, void* stream) {
    if (!g32 || !wire || n < 0) return CC_ERR_ARG;
    return wire_unpack(wire, g32, (size_t)n, S_(stream));
}

int CC_API(cc_grad_nonfinite)(const float* g32, int64_t n, float* found_inf, void* stream) {
    if (!g32 || !found_inf || n < 0) return CC_ERR_ARG;
    return grad_nonfinite(g32, (size_t)n, found_inf, S_(stream));
}

int CC_API(cc_loss_scale_update)(float* state, float* found_inf, float growth, float backoff, int32_t interval, void* stream) {
    if (!state || !found_inf || growth < 1.f || backoff <= 0.f || backoff > 1.f || interval < 1) return CC_ERR_ARG;
    return loss_scale_update(state, found_inf, growth, backoff, interval, S_(stream));
}

}  // extern "C"
