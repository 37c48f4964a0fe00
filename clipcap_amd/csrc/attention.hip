// Attention of the ClipCap path for gfx950 (declarations in kernels.h): the fp32 LDS-tile kernels, the 16-bit MFMA forward / backward, the
// split-bf16 three-term MFMA kernels, the one-wave-per-row kernels of long sequences, and the dispatchers attn_fwd / attn_bwd.
// All are wave64 code.  profiles/r09_a_attention_refactor_isa.md records which pieces are shared between the kernels and which are not.
#include "kernels.h"

namespace CC_NS {

// ------------------------------------------------------------------------------------------------------------
// Small-sequence attention (mapper: S=20, hd=96, full; GPT-2 training: T<=74, hd=64, causal).  One workgroup per
// (batch, head); Q/K/V staged in LDS as fp32 rows of hd+4 floats (16-B aligned, rows 4 banks apart so that a
// wave's b128 reads of consecutive rows are conflict-free).  qkv is [B*S][3*D] = [q | k | v], head h at h*hd.
// Saves the log-sum-exp per (b,h,row) for the backward pass (probabilities are recomputed there).
// ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void load_head_rows(float* dst, int hdp, const act_t* src, size_t ld, int S, int hd) {
    const int c8n = hd >> 3;
    for (int idx = threadIdx.x; idx < S * c8n; idx += blockDim.x) {
        const int r = idx / c8n, c = idx % c8n;
        float f[8];
        act_ld8(src + (size_t)r * ld + c * 8, f);
        float* d = dst + r * hdp + c * 8;
        *reinterpret_cast<float4*>(d) = make_float4(f[0], f[1], f[2], f[3]);
        *reinterpret_cast<float4*>(d + 4) = make_float4(f[4], f[5], f[6], f[7]);
    }
}

// Launch with `sh` bytes of dynamic LDS: beyond the 64 KiB default the kernel's limit is raised first (the size follows S, so every such call sets it).
template <auto Kernel, class... Args>
static void attn_launch(dim3 grid, dim3 block, size_t sh, hipStream_t st, const Args&... args) {
    if (sh > 64 * 1024) (void)hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh);
    hipLaunchKernelGGL(Kernel, grid, block, sh, st, args...);
}
// The dropout / causal / plain ladder of every launcher: LAUNCH(CAUSAL, DROP) with the instantiation the call needs.  Dropout is a GPT-2
// (causal) feature: the launchers refuse it without the mask before they come here.
#define ATTN_LADDER(LAUNCH) { if (drop.thresh) { LAUNCH(true, true); } else if (causal) { LAUNCH(true, false); } else { LAUNCH(false, false); } }

// Counter of the attention-probability dropout mask for probability (sample b, head h, query q, key k).  A lane whose query or key lies
// beyond S passes it clamped to S - 1: what it masks is an exact zero, but the counter stays inside this head's S x S range.
__device__ __forceinline__ unsigned attn_drop_idx(int b, int H, int h, int S, int q, int k) { return ((unsigned)(b * H + h) * S + q) * S + k; }
// whether probability (query q, key k) exists: both inside the sequence and, under the causal mask, the key not after the query
template <bool CAUSAL>
__device__ __forceinline__ bool attn_live(int q, int k, int S) { return q < S && k < S && (!CAUSAL || k <= q); }

template <bool CAUSAL, bool DROP = false>
__global__ __launch_bounds__(256) void k_attn_fwd(const act_t* __restrict__ qkv, int S, int H, int hd, float scale,
                                                  act_t* __restrict__ out, float* __restrict__ lse, Drop drop = Drop(), int img = 0) {
    // img (bf16x3 build): out receives the [hi | hi | lo] operand image (rows of 3 D 16-bit elements) of attn.c_proj's GEMM
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int D = H * hd, hdp = hd + 4, Sp = S + 1;
    float* Qs = sm;
    float* Ks = Qs + S * hdp;
    float* Vs = Ks + S * hdp;
    float* Ps = Vs + S * hdp;
    const int b = blockIdx.x / H, h = blockIdx.x % H;
    const act_t* base = qkv + (size_t)b * S * 3 * D + h * hd;
    load_head_rows(Qs, hdp, base, 3 * D, S, hd);
    load_head_rows(Ks, hdp, base + D, 3 * D, S, hd);
    load_head_rows(Vs, hdp, base + 2 * D, 3 * D, S, hd);
    __syncthreads();
    // scores: thread -> (block of 4 queries, key j)
    const int nib = (S + 3) >> 2;
    for (int idx = threadIdx.x; idx < nib * S; idx += 256) {
        const int ib = idx / S, j = idx % S, i0 = ib * 4;
        if (CAUSAL && j > i0 + 3) {
#pragma unroll
            for (int ii = 0; ii < 4; ii++)
                if (i0 + ii < S) Ps[(i0 + ii) * Sp + j] = -INFINITY;
            continue;
        }
        float a0 = 0, a1 = 0, a2 = 0, a3 = 0;
        const float* kr = Ks + j * hdp;
        const float* q0 = Qs + min(i0, S - 1) * hdp;
        const float* q1 = Qs + min(i0 + 1, S - 1) * hdp;
        const float* q2 = Qs + min(i0 + 2, S - 1) * hdp;
        const float* q3 = Qs + min(i0 + 3, S - 1) * hdp;
        for (int d = 0; d < hd; d += 4) {
            const float4 k = *reinterpret_cast<const float4*>(kr + d);
            const float4 x0 = *reinterpret_cast<const float4*>(q0 + d), x1 = *reinterpret_cast<const float4*>(q1 + d);
            const float4 x2 = *reinterpret_cast<const float4*>(q2 + d), x3 = *reinterpret_cast<const float4*>(q3 + d);
            a0 += x0.x * k.x + x0.y * k.y + x0.z * k.z + x0.w * k.w;
            a1 += x1.x * k.x + x1.y * k.y + x1.z * k.z + x1.w * k.w;
            a2 += x2.x * k.x + x2.y * k.y + x2.z * k.z + x2.w * k.w;
            a3 += x3.x * k.x + x3.y * k.y + x3.z * k.z + x3.w * k.w;
        }
        const float a[4] = {a0, a1, a2, a3};
#pragma unroll
        for (int ii = 0; ii < 4; ii++)
            if (i0 + ii < S) Ps[(i0 + ii) * Sp + j] = (CAUSAL && j > i0 + ii) ? -INFINITY : a[ii] * scale;
    }
    __syncthreads();
    // softmax: one wave per row
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i = wave; i < S; i += 4) {
        float m = -INFINITY;
        for (int j = lane; j < S; j += 64) m = fmaxf(m, Ps[i * Sp + j]);
        m = wave_max(m);
        float s = 0.f;
        for (int j = lane; j < S; j += 64) {
            const float e = __expf(Ps[i * Sp + j] - m);
            Ps[i * Sp + j] = e;
            s += e;
        }
        s = wave_sum(s);
        const float inv = 1.f / s;
        for (int j = lane; j < S; j += 64) Ps[i * Sp + j] = act_round(Ps[i * Sp + j] * inv);   // P enters the PV product in the operand type (as in the MFMA kernel); fp32 in the bf16x3 build
        if (lane == 0 && lse) lse[((size_t)b * H + h) * S + i] = m + __logf(s);
    }
    __syncthreads();
    // O = P V: thread -> (row i, 4 columns)
    const int d4n = hd >> 2;
    for (int idx = threadIdx.x; idx < S * d4n; idx += 256) {
        const int i = idx / d4n, d0 = (idx % d4n) * 4;
        float4 o = make_float4(0, 0, 0, 0);
        const int jmax = CAUSAL ? i + 1 : S;
        for (int j = 0; j < jmax; j++) {
            float p = Ps[i * Sp + j];
            if (DROP) p *= drop_mul(drop, attn_drop_idx(b, H, h, S, i, j));      // attention-probability dropout: P V only, as in the MFMA kernel
            const float4 v = *reinterpret_cast<const float4*>(Vs + j * hdp + d0);
            o.x += p * v.x; o.y += p * v.y; o.z += p * v.z; o.w += p * v.w;
        }
#if CC_OP == 2
        if (img) {
            const unsigned h01 = pack2op(o.x, o.y), h23 = pack2op(o.z, o.w);
            float a0, a1, a2, a3;
            unpack2(h01, a0, a1);
            unpack2(h23, a2, a3);
            const uint2 hi = make_uint2(h01, h23), lo = make_uint2(pack2op(o.x - a0, o.y - a1), pack2op(o.z - a2, o.w - a3));
            op16_t* r3 = reinterpret_cast<op16_t*>(out) + ((size_t)b * S + i) * 3 * D + h * hd + d0;
            *reinterpret_cast<uint2*>(r3) = hi;
            *reinterpret_cast<uint2*>(r3 + D) = hi;
            *reinterpret_cast<uint2*>(r3 + 2 * D) = lo;
            continue;
        }
#endif
        act_st4(out + ((size_t)b * S + i) * D + h * hd + d0, o.x, o.y, o.z, o.w);
    }
}

// ------------------------------------------------------------------------------------------------------------
// MFMA attention forward (head dim 64 / 96 / 128): one wave per (sample, head, 32-query block), flash-style loop
// over 32-key blocks with v_mfma_f32_32x32x16_bf16.
//   S^T[key][query] = K·Q^T: both operands are d-contiguous, so A (K rows) and B (Q rows) fragments are plain 16-B
//   global loads — no LDS.  The accumulator layout puts ONE query per lane (col = lane&31) and 16 keys in its
//   registers (the other 16 in lane^32), so softmax statistics are lane-local + one cross-half shuffle.
//   O^T[d][query] += V^T·P^T: the B fragment of k-step t is the lane's own p[8t..8t+7] (k-slot s <-> key
//   (s&3) + 8(2t + (s>>2)) + 4(lane>>5)); the A fragment gathers the same keys of one d column from a wave-private LDS
//   copy of the V block (8 x ds_read_u16).
// ------------------------------------------------------------------------------------------------------------
typedef __attribute__((ext_vector_type(16))) float f32x16;

// C layout of a 32 x 32 MFMA accumulator: register r of a lane holds column lane & 31 of row c_row(r, lane >> 5)
__device__ __forceinline__ int c_row(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }
__device__ __forceinline__ void acc_zero(f32x16& a) {
#pragma unroll
    for (int r = 0; r < 16; r++) a[r] = 0.f;
}
template <int N>
__device__ __forceinline__ void acc_zero(f32x16 (&a)[N]) {
#pragma unroll
    for (int n = 0; n < N; n++) acc_zero(a[n]);
}
__device__ __forceinline__ op16x8 pack_frag(const float* p) {
    return __builtin_bit_cast(op16x8, make_uint4(pack2op(p[0], p[1]), pack2op(p[2], p[3]), pack2op(p[4], p[5]), pack2op(p[6], p[7])));
}
// Row loads are branch-free: the caller clamps the row index into range and the value is zeroed by a select.  A predicated
// load (`if (ok) v = *p`) puts every load in its own basic block — 43 branches in the dkv loop — and the loads stop overlapping.
__device__ __forceinline__ op16x8 load_frag(const op16_t* row_ptr, bool ok) {
    uint4 v = *reinterpret_cast<const uint4*>(row_ptr);
    if (!ok) v = make_uint4(0, 0, 0, 0);
    return __builtin_bit_cast(op16x8, v);
}
// accumulators (C layout, this lane's output row) -> the row's HD 16-bit elements at `row`: registers 4 g .. 4 g + 3 are columns
// 32 nb + 8 g + 4 half .. + 3.  MUL: times f (the forward's 1 / l)
template <int NB, bool MUL = false>
__device__ __forceinline__ void store_acc_row(op16_t* row, const f32x16 (&acc)[NB], int half, float f = 1.f) {
#pragma unroll
    for (int nb = 0; nb < NB; nb++)
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const float a0 = MUL ? acc[nb][g * 4 + 0] * f : acc[nb][g * 4 + 0], a1 = MUL ? acc[nb][g * 4 + 1] * f : acc[nb][g * 4 + 1];
            const float a2 = MUL ? acc[nb][g * 4 + 2] * f : acc[nb][g * 4 + 2], a3 = MUL ? acc[nb][g * 4 + 3] * f : acc[nb][g * 4 + 3];
            *reinterpret_cast<uint2*>(row + nb * 32 + 8 * g + 4 * half) = make_uint2(pack2op(a0, a1), pack2op(a2, a3));
        }
}

// Wave-private LDS copy of a [32 rows][HD] block, rows ATT_LD(HD) elements apart (192 B for HD 64 / 96, 320 B for 128: the four
// rows a 32-lane half of a transpose read touches fall into four different 64-B bank slots), and the A fragment of k-step t
// read from it with ds_read_b64_tr_b16: lane (row d = 32 nb + (lane & 31), half) needs rows {16 t + 4 half + 0..3} and
// {16 t + 8 + 4 half + 0..3} of column d — the k-slot order the accumulator layout gives P / dS — i.e. two [4 row][16 col]
// transpose reads per 16-lane group instead of 8 ds_read_u16 + 4 packs.
template <int HD> struct AttLd { static constexpr int v = HD == 128 ? 160 : 96; };
template <int HD>
__device__ __forceinline__ op16x8 frag_tr(const op16_t* blk, int nb, int t, int lane) {
    typedef __attribute__((ext_vector_type(4))) short s16x4_t;
    typedef __attribute__((address_space(3))) s16x4_t* lp_t;
    constexpr int LD = AttLd<HD>::v;
    const int half = lane >> 5, j = lane & 15, dsub = (lane >> 4) & 1;
    const op16_t* p = blk + (16 * t + 4 * half + (j >> 2)) * LD + nb * 32 + 16 * dsub + 4 * (j & 3);
    const s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp_t)p);
    const s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp_t)(p + 8 * LD));
    typedef __attribute__((ext_vector_type(8))) short s16x8_t;
    const s16x8_t v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(op16x8, v);
}

#if CC_OP == 2
// ------------------------------------------------------------------------------------------------------------
// The same forward for the split-bf16 build (round 4; fp32 activations in, fp32 or operand-image out): every product is the three bf16
// MFMA terms hi*hi + hi*lo + lo*hi of the GEMMs — Q, K rows and the probabilities are split in registers, the V block sits
// in LDS as a hi plane and a lo plane.  Softmax statistics, the running rescale and the output stay fp32.  Replaces the fp32 VALU
// LDS-tile kernel (k_attn_fwd) for head dims 64 / 96 / 128 (CC_ATTN_X3MFMA=0 switches back); any S (the windowed mapper's 180 too).
// ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void x3_split8(const float (&f)[8], op16x8& hi, op16x8& lo) {
    const uint4 h = pack8(f);
    float hf[8], d[8];
    unpack8(h, hf);
#pragma unroll
    for (int e = 0; e < 8; e++) d[e] = f[e] - hf[e];
    hi = __builtin_bit_cast(op16x8, h);
    lo = __builtin_bit_cast(op16x8, pack8(d));
}
template <int HD, bool CAUSAL, bool DROP = false>
__global__ __launch_bounds__(256, 2) void k_attn_fwd_mfma3(const float* __restrict__ qkv, int B, int S, int H, float scale, float* __restrict__ out,
                                                           float* __restrict__ lse_out, Drop drop, int img) {
    constexpr int KK = HD / 16, NB = HD / 32, C8 = HD / 8, LD = AttLd<HD>::v;
    __shared__ __attribute__((aligned(16))) op16_t vsm[4][2][32 * LD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nqb = (S + 31) >> 5;
    const int item = blockIdx.x * 4 + wave;
    if (item >= B * H * nqb) return;  // wave-uniform; no block-level barrier is used below
    const int qb = item % nqb, h = (item / nqb) % H, b = item / (nqb * H);
    const int D = H * HD;
    const size_t rs = (size_t)3 * D;
    const float* base = qkv + (size_t)b * S * rs + h * HD;
    const int half = lane >> 5, q = qb * 32 + (lane & 31);
    op16_t* vh = vsm[wave][0];
    op16_t* vl = vsm[wave][1];
    auto ld8 = [](const float* p, bool ok, float (&f)[8]) {      // p is a clamped (always valid) address: load, then zero by select — no branch around the load
        const float4 a = *reinterpret_cast<const float4*>(p), c = *reinterpret_cast<const float4*>(p + 4);
        f[0] = ok ? a.x : 0.f; f[1] = ok ? a.y : 0.f; f[2] = ok ? a.z : 0.f; f[3] = ok ? a.w : 0.f;
        f[4] = ok ? c.x : 0.f; f[5] = ok ? c.y : 0.f; f[6] = ok ? c.z : 0.f; f[7] = ok ? c.w : 0.f;
    };
    op16x8 qh[KK], ql[KK];
#pragma unroll
    for (int kk = 0; kk < KK; kk++) {
        float f[8];
        ld8(base + (size_t)min(q, S - 1) * rs + kk * 16 + half * 8, q < S, f);
        x3_split8(f, qh[kk], ql[kk]);
    }
    f32x16 o[NB];
    acc_zero(o);
    float m = -INFINITY, l = 0.f;
    const int nkb = CAUSAL ? qb + 1 : nqb;
    const int key_l = lane & 31;
    for (int kb = 0; kb < nkb; kb++) {
        // V block -> wave-private LDS planes [32 keys][LD] (hi, lo); the previous block's fragment reads were consumed by its MFMAs
#pragma unroll
        for (int c = 0; c < HD / 16; c++) {
            const int idx = lane + 64 * c;
            const int vk = idx / C8, vc = idx % C8;
            float f[8];
            ld8(base + 2 * D + (size_t)min(kb * 32 + vk, S - 1) * rs + vc * 8, kb * 32 + vk < S, f);
            op16x8 a, c2;
            x3_split8(f, a, c2);
            *reinterpret_cast<op16x8*>(vh + vk * LD + vc * 8) = a;
            *reinterpret_cast<op16x8*>(vl + vk * LD + vc * 8) = c2;
        }
        f32x16 s;
        acc_zero(s);
#pragma unroll
        for (int kk = 0; kk < KK; kk++) {
            float f[8];
            const int key = kb * 32 + key_l;
            ld8(base + D + (size_t)min(key, S - 1) * rs + kk * 16 + half * 8, key < S, f);
            op16x8 kh, kl;
            x3_split8(f, kh, kl);
            s = CC_MFMA_32x32x16(kl, qh[kk], s);          // small terms first
            s = CC_MFMA_32x32x16(kh, ql[kk], s);
            s = CC_MFMA_32x32x16(kh, qh[kk], s);
        }
        float mx = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int kr = kb * 32 + c_row(r, half);
            const bool ok = kr < S && (!CAUSAL || kr <= q);
            s[r] = ok ? s[r] * scale : -INFINITY;
            mx = fmaxf(mx, s[r]);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m, mx);
        const float alpha = (m == -INFINITY) ? 0.f : __expf(m - m_new);
        float p[16], ps = 0.f;
#pragma unroll
        for (int r = 0; r < 16; r++) {
            p[r] = (m_new == -INFINITY) ? 0.f : __expf(s[r] - m_new);
            ps += p[r];
        }
        ps += __shfl_xor(ps, 32, 64);
        l = l * alpha + ps;
        m = m_new;
#pragma unroll
        for (int nb = 0; nb < NB; nb++)
#pragma unroll
            for (int r = 0; r < 16; r++) o[nb][r] *= alpha;
        if (DROP) {     // attention-probability dropout: P V only, the row sum l stays (as in the 16-bit kernel)
            const unsigned rowbase = attn_drop_idx(b, H, h, S, min(q, S - 1), 0);
#pragma unroll
            for (int r = 0; r < 16; r++) p[r] *= drop_mul(drop, rowbase + min(kb * 32 + c_row(r, half), S - 1));
        }
        op16x8 ph[2], pl[2];
#pragma unroll
        for (int t = 0; t < 2; t++) {
            const float f[8] = {p[t * 8 + 0], p[t * 8 + 1], p[t * 8 + 2], p[t * 8 + 3], p[t * 8 + 4], p[t * 8 + 5], p[t * 8 + 6], p[t * 8 + 7]};
            x3_split8(f, ph[t], pl[t]);
        }
#pragma unroll
        for (int t = 0; t < 2; t++)
#pragma unroll
            for (int nb = 0; nb < NB; nb++) {
                const op16x8 fh = frag_tr<HD>(vh, nb, t, lane), fl = frag_tr<HD>(vl, nb, t, lane);
                o[nb] = CC_MFMA_32x32x16(fl, ph[t], o[nb]);
                o[nb] = CC_MFMA_32x32x16(fh, pl[t], o[nb]);
                o[nb] = CC_MFMA_32x32x16(fh, ph[t], o[nb]);
            }
    }
    if (q < S) {
        const float inv = l > 0.f ? 1.f / l : 0.f;
#pragma unroll
        for (int nb = 0; nb < NB; nb++)
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const int d0 = nb * 32 + 8 * g + 4 * half;
                const float o0 = o[nb][g * 4 + 0] * inv, o1 = o[nb][g * 4 + 1] * inv, o2 = o[nb][g * 4 + 2] * inv, o3 = o[nb][g * 4 + 3] * inv;
                if (img) {                                  // [hi | hi | lo] operand image of attn.c_proj's GEMM (rows of 3 D 16-bit elements)
                    const unsigned h01 = pack2op(o0, o1), h23 = pack2op(o2, o3);
                    float a0, a1, a2, a3;
                    unpack2(h01, a0, a1);
                    unpack2(h23, a2, a3);
                    const uint2 hi = make_uint2(h01, h23), lo = make_uint2(pack2op(o0 - a0, o1 - a1), pack2op(o2 - a2, o3 - a3));
                    op16_t* r3 = reinterpret_cast<op16_t*>(out) + ((size_t)b * S + q) * 3 * D + h * HD + d0;
                    *reinterpret_cast<uint2*>(r3) = hi;
                    *reinterpret_cast<uint2*>(r3 + D) = hi;
                    *reinterpret_cast<uint2*>(r3 + 2 * D) = lo;
                } else {
                    *reinterpret_cast<float4*>(out + ((size_t)b * S + q) * D + h * HD + d0) = make_float4(o0, o1, o2, o3);
                }
            }
        if (half == 0 && lse_out) lse_out[((size_t)b * H + h) * S + q] = m + __logf(l);
    }
}
template <int HD>
static int attn_fwd_mfma3_launch(const float* qkv, int B, int S, int H, bool causal, float* out, float* lse, hipStream_t st, Drop drop, int img) {
    const int items = B * H * ((S + 31) / 32);
    const float scale = 1.0f / sqrtf((float)HD);
    if (drop.thresh && !causal) return CC_ERR_SHAPE;
#define CC_L(C, DR) attn_launch<k_attn_fwd_mfma3<HD, C, DR>>(dim3((items + 3) / 4), dim3(256), 0, st, qkv, B, S, H, scale, out, lse, drop, img)
    ATTN_LADDER(CC_L)
#undef CC_L
    return hipGetLastError() == hipSuccess ? CC_OK : CC_ERR_LAUNCH;
}
// ------------------------------------------------------------------------------------------------------------
// Backward of the same attention as three-term bf16 MFMA products (round 4; S <= 64, head dim 64 / 96): one workgroup per (sample, head),
// every operand staged ONCE into LDS as a hi plane and a lo plane (the GEMMs' split, common.hip.h::x3_pair8's arithmetic), so that
// every MFMA fragment is a plain 16-B read (k along the row) or a ds_read_b64_tr_b16 pair (k down the rows).  Phases, a block barrier apart:
//   0  qkv / dO rows (fp32) -> planes Q, K, V, dO [R][LD]
//   1  tile jobs: S = Q K^T and dP = dO V^T (fp32 scratch in the P / dS plane area)
//   2  per row: P = exp(S scale - lse), delta = sum P dP, dS = P (dP - delta) scale -> planes P, dS [R][LDP]
//   3  tile jobs: dQ = dS K, dK = dS^T Q, dV = P^T dO, accumulators [32 rows][32 d-columns] -> global rows (fp32, or the consumer GEMM's
//      [hi | hi | lo] operand image).  Causal launches skip the tiles above the diagonal.
// Replaces the fp32 VALU LDS-tile kernels (k_attn_bwd / _small) where it applies (CC_ATTN_X3MFMA=0 switches back).
// ------------------------------------------------------------------------------------------------------------
template <int LD>
__device__ __forceinline__ op16x8 frag_tr_p(const op16_t* blk, int nb, int t, int lane) {      // frag_tr with the row pitch as a parameter
    typedef __attribute__((ext_vector_type(4))) short s16x4_t;
    typedef __attribute__((address_space(3))) s16x4_t* lp_t;
    const int half = lane >> 5, j = lane & 15, dsub = (lane >> 4) & 1;
    const op16_t* p = blk + (16 * t + 4 * half + (j >> 2)) * LD + nb * 32 + 16 * dsub + 4 * (j & 3);
    const s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp_t)p);
    const s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp_t)(p + 8 * LD));
    typedef __attribute__((ext_vector_type(8))) short s16x8_t;
    const s16x8_t v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(op16x8, v);
}
// k-slot order of the transpose reads, for an operand whose k runs ALONG its row: elements {16 t + 4 half + 0..3} and {16 t + 8 + 4 half + 0..3}
__device__ __forceinline__ op16x8 frag_row_p(const op16_t* row, int t, int half) {
    const uint2 a = *reinterpret_cast<const uint2*>(row + 16 * t + 4 * half), c = *reinterpret_cast<const uint2*>(row + 16 * t + 8 + 4 * half);
    return __builtin_bit_cast(op16x8, make_uint4(a.x, a.y, c.x, c.y));
}
#define CC_MFMA3(AH, AL, BH, BL, ACC) { ACC = CC_MFMA_32x32x16(AL, BH, ACC); ACC = CC_MFMA_32x32x16(AH, BL, ACC); ACC = CC_MFMA_32x32x16(AH, BH, ACC); }
template <int HD, int NBLK> struct AttM3 {
    static constexpr int R = 32 * NBLK, LD = AttLd<HD>::v, LDP = NBLK == 2 ? 96 : 32, SP = NBLK == 2 ? 68 : 32, NW = NBLK == 2 ? 8 : 4;
    static constexpr int PLANE = R * LD, PPLANE = R * LDP;
    static constexpr size_t lds = (size_t)8 * PLANE * 2 + (size_t)4 * PPLANE * 2 + R * 4;
};
template <int HD, int NBLK, bool CAUSAL, bool DROP>
__global__ __launch_bounds__(NBLK == 2 ? 512 : 256, 1) void k_attn_bwd_m3(const float* __restrict__ qkv, const float* __restrict__ dout,
                                                                              const float* __restrict__ lse, int B, int S, int H, float scale,
                                                                              float* __restrict__ dqkv, Drop drop, int img) {
    typedef AttM3<HD, NBLK> G;
    constexpr int R = G::R, LD = G::LD, LDP = G::LDP, SP = G::SP, NW = G::NW, NB = HD / 32, KK = HD / 16, C8 = HD / 8, NT = 64 * NW;
    static_assert((size_t)2 * R * SP * 4 <= (size_t)4 * G::PPLANE * 2, "the fp32 scratch lives in the P / dS plane area");
    extern __shared__ __attribute__((aligned(16))) unsigned char m3raw[];
    op16_t* pl = reinterpret_cast<op16_t*>(m3raw);                 // planes: Qh Ql Kh Kl Vh Vl Oh Ol
    op16_t* Qh = pl, *Ql = pl + G::PLANE, *Kh = pl + 2 * G::PLANE, *Kl = pl + 3 * G::PLANE, *Vh = pl + 4 * G::PLANE, *Vl = pl + 5 * G::PLANE;
    op16_t* Oh = pl + 6 * G::PLANE, *Ol = pl + 7 * G::PLANE;
    op16_t* pp = pl + 8 * G::PLANE;                                // planes: Ph Pl Dh Dl
    op16_t* Ph = pp, *Pl = pp + G::PPLANE, *Dh = pp + 2 * G::PPLANE, *Dl = pp + 3 * G::PPLANE;
    float* scrS = reinterpret_cast<float*>(pp);                    // phase 1 -> 2 scratch: S [R][SP], dP [R][SP]
    float* scrD = scrS + R * SP;
    float* lse_s = reinterpret_cast<float*>(pp + 4 * G::PPLANE);   // [R]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const int D = H * HD, nitems = B * H;
    const size_t rs = (size_t)3 * D;
    // Persistent over the (sample, head) items of this workgroup (grid = one workgroup per CU): the NEXT item's rows are requested into
    // registers as soon as the current item's have been written to the planes, so they travel under phases 1-3 — with one workgroup per CU
    // (the planes fill the LDS) and every CU in the same phase, loads, arithmetic and stores otherwise took turns on an idle memory system.
    constexpr int PER = 4 * R * C8 / NT;
    static_assert(PER * NT == 4 * R * C8, "staging items tile the threads");
    float4 x[PER], y[PER];
    float lse_r = 0.f;
    auto request = [&](int item) {
        const int b_ = item / H, h_ = item - b_ * H;
        const float* base = qkv + (size_t)b_ * S * rs + h_ * HD;
        const float* dbase = dout + (size_t)b_ * S * D + h_ * HD;
#pragma unroll
        for (int it = 0; it < PER; it++) {
            const int idx = tid + it * NT;
            const int which = idx / (R * C8), rem = idx - which * (R * C8), row = rem / C8, c = rem - row * C8;
            const float* src = which == 3 ? dbase + (size_t)min(row, S - 1) * D + c * 8 : base + which * D + (size_t)min(row, S - 1) * rs + c * 8;
            x[it] = *reinterpret_cast<const float4*>(src);
            y[it] = *reinterpret_cast<const float4*>(src + 4);
        }
        if (tid < R) lse_r = lse[((size_t)b_ * H + h_) * S + min(tid, S - 1)];
    };
    if ((int)blockIdx.x < nitems) request(blockIdx.x);
    for (int item = blockIdx.x; item < nitems; item += gridDim.x) {
    const int b = item / H, h = item - b * H;
    // ---- phase 0: rows -> planes
    {
#pragma unroll
        for (int it = 0; it < PER; it++) {
            const int idx = tid + it * NT;
            const int which = idx / (R * C8), rem = idx - which * (R * C8), row = rem / C8, c = rem - row * C8;
            const bool ok = row < S;
            const float f[8] = {ok ? x[it].x : 0.f, ok ? x[it].y : 0.f, ok ? x[it].z : 0.f, ok ? x[it].w : 0.f,
                                ok ? y[it].x : 0.f, ok ? y[it].y : 0.f, ok ? y[it].z : 0.f, ok ? y[it].w : 0.f};
            op16x8 hi, lo;
            x3_split8(f, hi, lo);
            *reinterpret_cast<op16x8*>(pl + (2 * which) * G::PLANE + row * LD + c * 8) = hi;
            *reinterpret_cast<op16x8*>(pl + (2 * which + 1) * G::PLANE + row * LD + c * 8) = lo;
        }
        if (tid < R) lse_s[tid] = tid < S ? lse_r : 0.f;
    }
    if (item + (int)gridDim.x < nitems) request(item + gridDim.x);
    __syncthreads();
    // ---- phase 1: jobs (tile (i, j), product)
    {
        constexpr int NTILE = CAUSAL ? NBLK * (NBLK + 1) / 2 : NBLK * NBLK;
        for (int job = wave; job < 2 * NTILE; job += NW) {
            const int prod = job & 1, tl = job >> 1;
            int i, j;
            if (CAUSAL) { i = tl == 0 ? 0 : 1; j = tl == 2 ? 1 : 0; if (NBLK == 1) { i = 0; j = 0; } }
            else { i = tl / NBLK; j = tl % NBLK; }
            const op16_t* ah = (prod ? Oh : Qh) + (i * 32 + l31) * LD + 8 * half;
            const op16_t* al = (prod ? Ol : Ql) + (i * 32 + l31) * LD + 8 * half;
            const op16_t* bh = (prod ? Vh : Kh) + (j * 32 + l31) * LD + 8 * half;
            const op16_t* bl = (prod ? Vl : Kl) + (j * 32 + l31) * LD + 8 * half;
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; r++) acc[r] = 0.f;
#pragma unroll
            for (int kk = 0; kk < KK; kk++) {
                const op16x8 a_h = *reinterpret_cast<const op16x8*>(ah + kk * 16), a_l = *reinterpret_cast<const op16x8*>(al + kk * 16);
                const op16x8 b_h = *reinterpret_cast<const op16x8*>(bh + kk * 16), b_l = *reinterpret_cast<const op16x8*>(bl + kk * 16);
                CC_MFMA3(a_h, a_l, b_h, b_l, acc)
            }
            float* dst = (prod ? scrD : scrS) + j * 32 + l31;
#pragma unroll
            for (int r = 0; r < 16; r++) dst[(i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half) * SP] = acc[r];
        }
    }
    __syncthreads();
    // ---- phase 2: a thread owns 8 consecutive keys of a row (R / 8 neighbouring lanes share the row)
    {
        constexpr int CPR = R / 8;                                // chunks (threads) per row
        const int q = tid / CPR, c = tid - q * CPR;
        const bool act = q < R;                                   // R = 32: 128 of the 256 threads
        float pm[8], ds[8];
        {
            float sv[8], dv[8];
            const float* ps = scrS + (act ? q : 0) * SP + c * 8;
            const float* pd = scrD + (act ? q : 0) * SP + c * 8;
            const float4 s0 = *reinterpret_cast<const float4*>(ps), s1 = *reinterpret_cast<const float4*>(ps + 4);
            const float4 d0 = *reinterpret_cast<const float4*>(pd), d1 = *reinterpret_cast<const float4*>(pd + 4);
            sv[0] = s0.x; sv[1] = s0.y; sv[2] = s0.z; sv[3] = s0.w; sv[4] = s1.x; sv[5] = s1.y; sv[6] = s1.z; sv[7] = s1.w;
            dv[0] = d0.x; dv[1] = d0.y; dv[2] = d0.z; dv[3] = d0.w; dv[4] = d1.x; dv[5] = d1.y; dv[6] = d1.z; dv[7] = d1.w;
            const float lq = lse_s[act ? q : 0];
            float dpm[8], dl = 0.f;
#pragma unroll
            for (int e = 0; e < 8; e++) {
                const int key = c * 8 + e;
                const bool ok = act && attn_live<CAUSAL>(q, key, S);
                const float pe = ok ? __expf(sv[e] * scale - lq) : 0.f;
                const float mk = DROP ? drop_mul(drop, attn_drop_idx(b, H, h, S, min(q, S - 1), min(key, S - 1))) : 1.f;
                dpm[e] = ok ? dv[e] * mk : 0.f;
                dl += pe * dpm[e];
                pm[e] = pe;                                       // mask applied below, after delta
                ds[e] = mk;
            }
#pragma unroll
            for (int o = CPR / 2; o > 0; o >>= 1) dl += __shfl_xor(dl, o, 64);
#pragma unroll
            for (int e = 0; e < 8; e++) {
                const float mk = ds[e];
                ds[e] = pm[e] * (dpm[e] - dl) * scale;            // pm = 0 where masked
                pm[e] *= mk;
            }
        }
        __syncthreads();                                          // every S / dP value is in registers: the area becomes the P / dS planes
        if (act) {
            op16x8 ph, plo, dh, dlo;
            x3_split8(pm, ph, plo);
            x3_split8(ds, dh, dlo);
            *reinterpret_cast<op16x8*>(Ph + q * LDP + c * 8) = ph;
            *reinterpret_cast<op16x8*>(Pl + q * LDP + c * 8) = plo;
            *reinterpret_cast<op16x8*>(Dh + q * LDP + c * 8) = dh;
            *reinterpret_cast<op16x8*>(Dl + q * LDP + c * 8) = dlo;
        }
    }
    __syncthreads();
    // ---- phase 3: jobs (kind, row block, 32-column block of d)
    for (int job = wave; job < 3 * NBLK * NB; job += NW) {
        const int kind = job / (NBLK * NB), rem = job - kind * (NBLK * NB), blk = rem / NB, nb = rem - blk * NB;
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; r++) acc[r] = 0.f;
        if (kind == 0) {                                        // dQ[q][d] = sum over keys dS[q][key] K[key][d]
            const int jn = CAUSAL ? blk + 1 : NBLK;
            for (int j = 0; j < jn; j++)
#pragma unroll
                for (int t = 0; t < 2; t++) {
                    const op16x8 a_h = frag_row_p(Dh + (blk * 32 + l31) * LDP + j * 32, t, half), a_l = frag_row_p(Dl + (blk * 32 + l31) * LDP + j * 32, t, half);
                    const op16x8 b_h = frag_tr_p<LD>(Kh + j * 32 * LD, nb, t, lane), b_l = frag_tr_p<LD>(Kl + j * 32 * LD, nb, t, lane);
                    CC_MFMA3(a_h, a_l, b_h, b_l, acc)
                }
        } else {                                                // dK[key][d] = sum over q dS[q][key] Q[q][d];  dV[key][d] = sum over q P[q][key] dO[q][d]
            const op16_t* Ah = kind == 1 ? Dh : Ph, *Al = kind == 1 ? Dl : Pl, *Bh = kind == 1 ? Qh : Oh, *Bl = kind == 1 ? Ql : Ol;
            for (int i = CAUSAL ? blk : 0; i < NBLK; i++)
#pragma unroll
                for (int t = 0; t < 2; t++) {
                    const op16x8 a_h = frag_tr_p<LDP>(Ah + i * 32 * LDP, blk, t, lane), a_l = frag_tr_p<LDP>(Al + i * 32 * LDP, blk, t, lane);
                    const op16x8 b_h = frag_tr_p<LD>(Bh + i * 32 * LD, nb, t, lane), b_l = frag_tr_p<LD>(Bl + i * 32 * LD, nb, t, lane);
                    CC_MFMA3(a_h, a_l, b_h, b_l, acc)
                }
        }
        const int d = nb * 32 + l31;
        if (img) {                                              // rows of 9 D 16-bit elements: [hi (q k v) | hi | lo]
            // lanes d, d + 1 trade one value per register pair: the even lane stores row r's two columns, the odd lane row r + 1's — 4-byte
            // stores (64 lanes x 4 B = two 64-B row segments per instruction) instead of 2-byte ones
            const int odd = lane & 1;
            op16_t* r3 = reinterpret_cast<op16_t*>(dqkv) + (size_t)b * S * 9 * D + kind * D + h * HD + (d & ~1);
#pragma unroll
            for (int rp = 0; rp < 8; rp++) {
                const float v0 = acc[2 * rp], v1 = acc[2 * rp + 1];
                const float got = __shfl_xor(odd ? v0 : v1, 1, 64);
                const float a0 = odd ? got : v0, a1 = odd ? v1 : got;           // columns d & ~1, (d & ~1) + 1 of this lane's row
                const int row = blk * 32 + ((2 * rp) & 3) + 8 * ((2 * rp) >> 2) + 4 * half + odd;
                const unsigned hi = pack2op(a0, a1);
                float h0, h1;
                unpack2(hi, h0, h1);
                const unsigned lo = pack2op(a0 - h0, a1 - h1);
                if (row < S) {
                    op16_t* o3 = r3 + (size_t)row * 9 * D;
                    *reinterpret_cast<unsigned*>(o3) = hi;
                    *reinterpret_cast<unsigned*>(o3 + 3 * D) = hi;
                    *reinterpret_cast<unsigned*>(o3 + 6 * D) = lo;
                }
            }
        } else {
            float* o1 = dqkv + (size_t)b * S * rs + kind * D + h * HD + d;
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int row = blk * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (row < S) o1[(size_t)row * rs] = acc[r];
            }
        }
    }
    __syncthreads();                                            // the planes are rewritten by the next item's phase 0
    }
}
template <int HD, int NBLK>
static int attn_bwd_m3_launch(const float* qkv, const float* dout, const float* lse, int B, int S, int H, bool causal, float* dqkv, hipStream_t st,
                              Drop drop, int img) {
    typedef AttM3<HD, NBLK> G;
    const float scale = 1.0f / sqrtf((float)HD);
    static int ncu = 0;
    if (!ncu) {
        int dev = 0;
        hipDeviceProp_t pr;
        if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&pr, dev) != hipSuccess) return CC_ERR_STATE;
        ncu = pr.multiProcessorCount;
    }
    const int per_cu = (int)((size_t)160 * 1024 / G::lds);       // resident workgroups per CU (LDS-limited)
    const dim3 grid(min(B * H, ncu * max(1, per_cu))), blk(64 * G::NW);
    if (drop.thresh && !causal) return CC_ERR_SHAPE;
#define CC_L(C, DR) attn_launch<k_attn_bwd_m3<HD, NBLK, C, DR>>(grid, blk, G::lds, st, qkv, dout, lse, B, S, H, scale, dqkv, drop, img)
    ATTN_LADDER(CC_L)
#undef CC_L
    return hipGetLastError() == hipSuccess ? CC_OK : CC_ERR_LAUNCH;
}
static bool attn_x3mfma_on();
static bool attn_bwd_m3_ok(int S, int hd) { return attn_x3mfma_on() && (hd == 64 || hd == 96) && S > 0 && S <= 64; }
static bool attn_x3mfma_on() {
    static const bool on = !(cc_lab_env("CC_ATTN_X3MFMA") && atoi(cc_lab_env("CC_ATTN_X3MFMA")) == 0) && !cc_lab_env("CC_ATTN_F32MFMA");
    return on;
}
#endif   // CC_OP == 2

#if CC_OP != 2      // the 16-bit MFMA attention kernels; the bf16x3 build runs the three-term form above and the fp32 VALU backward below
template <int HD, bool CAUSAL, bool DROP = false>
__global__ __launch_bounds__(256, HD == 64 ? 3 : 2) void k_attn_fwd_mfma(const op16_t* __restrict__ qkv, int B, int S, int H, float scale,
                                                       op16_t* __restrict__ out, float* __restrict__ lse_out, Drop drop = Drop()) {
    constexpr int KK = HD / 16, NB = HD / 32, C8 = HD / 8;
    __shared__ __attribute__((aligned(16))) op16_t vsm[4][32 * AttLd<HD>::v];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nqb = (S + 31) >> 5;
    const int item = blockIdx.x * 4 + wave;
    if (item >= B * H * nqb) return;  // wave-uniform; no block-level barrier is used below
    const int qb = item % nqb, h = (item / nqb) % H, b = item / (nqb * H);
    const int D = H * HD;
    const size_t rs = (size_t)3 * D;
    const op16_t* base = qkv + (size_t)b * S * rs + h * HD;
    const int half = lane >> 5, q = qb * 32 + (lane & 31);
    op16_t* vs = vsm[wave];

    op16x8 qf[KK];
#pragma unroll
    for (int kk = 0; kk < KK; kk++) {
        qf[kk] = load_frag(base + (size_t)min(q, S - 1) * rs + kk * 16 + half * 8, q < S);
    }
    f32x16 o[NB];
    acc_zero(o);
    float m = -INFINITY, l = 0.f;
    const int nkb = CAUSAL ? qb + 1 : nqb;
    // K fragments and the V block's 16-B chunks are loaded one key block ahead of their use
    uint4 kq[KK], vq[HD / 16];
    auto fetch = [&](int kb, uint4 (&kd)[KK], uint4 (&vd)[HD / 16]) {
        const int key = kb * 32 + (lane & 31);
#pragma unroll
        for (int kk = 0; kk < KK; kk++) {
            kd[kk] = *reinterpret_cast<const uint4*>(base + D + (size_t)min(key, S - 1) * rs + kk * 16 + half * 8);
            if (key >= S) kd[kk] = make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int c = 0; c < HD / 16; c++) {
            const int idx = lane + 64 * c;
            const int vk = idx / C8, vc = idx % C8;
            vd[c] = *reinterpret_cast<const uint4*>(base + 2 * D + (size_t)min(kb * 32 + vk, S - 1) * rs + vc * 8);
            if (kb * 32 + vk >= S) vd[c] = make_uint4(0, 0, 0, 0);
        }
    };
    fetch(0, kq, vq);
    for (int kb = 0; kb < nkb; kb++) {
        uint4 kn[KK], vn[HD / 16];
        fetch(kb + 1, kn, vn);
        f32x16 s;
        acc_zero(s);
#pragma unroll
        for (int kk = 0; kk < KK; kk++) s = CC_MFMA_32x32x16(__builtin_bit_cast(op16x8, kq[kk]), qf[kk], s);
        // V block -> wave-private LDS, row-major [32 keys][ATT_LD]
#pragma unroll
        for (int c = 0; c < HD / 16; c++) {
            const int idx = lane + 64 * c;
            *reinterpret_cast<uint4*>(vs + (idx / C8) * AttLd<HD>::v + (idx % C8) * 8) = vq[c];
        }
        float mx = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int kr = kb * 32 + c_row(r, half);
            const bool ok = kr < S && (!CAUSAL || kr <= q);
            s[r] = ok ? s[r] * scale : -INFINITY;
            mx = fmaxf(mx, s[r]);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m, mx);
        const float alpha = (m == -INFINITY) ? 0.f : __expf(m - m_new);
        float p[16], ps = 0.f;
#pragma unroll
        for (int r = 0; r < 16; r++) {
            p[r] = (m_new == -INFINITY) ? 0.f : __expf(s[r] - m_new);
            ps += p[r];
        }
        ps += __shfl_xor(ps, 32, 64);
        l = l * alpha + ps;
        m = m_new;
#pragma unroll
        for (int nb = 0; nb < NB; nb++)
#pragma unroll
            for (int r = 0; r < 16; r++) o[nb][r] *= alpha;
        if (DROP) {     // attention-probability dropout (hf sdpa dropout_p): applied to P for the PV product only, the row sum l stays
            const unsigned rowbase = attn_drop_idx(b, H, h, S, min(q, S - 1), 0);
#pragma unroll
            for (int r = 0; r < 16; r++) p[r] *= drop_mul(drop, rowbase + min(kb * 32 + c_row(r, half), S - 1));
        }
        op16x8 pf[2];
#pragma unroll
        for (int t = 0; t < 2; t++) pf[t] = pack_frag(p + t * 8);
#pragma unroll
        for (int t = 0; t < 2; t++)          // t outer: consecutive MFMAs go to different accumulators (no back-to-back RAW stall)
#pragma unroll
            for (int nb = 0; nb < NB; nb++) o[nb] = CC_MFMA_32x32x16(frag_tr<HD>(vs, nb, t, lane), pf[t], o[nb]);
#pragma unroll
        for (int kk = 0; kk < KK; kk++) kq[kk] = kn[kk];
#pragma unroll
        for (int c = 0; c < HD / 16; c++) vq[c] = vn[c];
    }
    if (q < S) {
        const float inv = l > 0.f ? 1.f / l : 0.f;
        op16_t* orow = out + ((size_t)b * S + q) * D + h * HD;
        store_acc_row<NB, true>(orow, o, half, inv);
        if (half == 0 && lse_out) lse_out[((size_t)b * H + h) * S + q] = m + __logf(l);
    }
}

template <int HD>
static int attn_fwd_mfma_launch(const op16_t* qkv, int B, int S, int H, bool causal, op16_t* out, float* lse, hipStream_t st, Drop drop) {
    const int items = B * H * ((S + 31) / 32);
    const float scale = 1.0f / sqrtf((float)HD);
    if (drop.thresh && !causal) return CC_ERR_SHAPE;      // dropout is a GPT-2 (causal) feature
#define CC_L(C, DR) attn_launch<k_attn_fwd_mfma<HD, C, DR>>(dim3((items + 3) / 4), dim3(256), 0, st, qkv, B, S, H, scale, out, lse, drop)
    ATTN_LADDER(CC_L)
#undef CC_L
    return hipGetLastError() == hipSuccess ? CC_OK : CC_ERR_LAUNCH;
}

// ------------------------------------------------------------------------------------------------------------
// MFMA attention backward (head dim 64 / 96 / 128), two kernels, no atomics, no transposes through HBM
// (delta[b,h,q] = sum_d dO[q,d] O[q,d] is computed and stored by the dQ kernel, which runs first):
//   k_attn_bwd_dkv (one wave per (b,h,key block j), loops over query blocks): "S orientation" — lane <-> key (col),
//       registers <-> 16 queries — so bf16(P) and bf16(dS) are directly the B fragments of
//       dV^T[d][key] += dO^T[d][q] P[q][key]   and   dK^T[d][key] += Q^T[d][q] dS[q][key];
//       the A fragments (dO^T, Q^T) gather 8 queries of one d column from wave-private LDS copies of the row-major blocks.
//   k_attn_bwd_dq (one wave per (b,h,query block i), loops over key blocks): "S^T orientation" as in the forward —
//       lane <-> query — so bf16(dS^T) is the B fragment of dQ^T[d][q] += K^T[d][key] dS^T[key][q] (K block via LDS).
// P is recomputed from the saved log-sum-exp; dS = P (dP - delta) * scale.
// ------------------------------------------------------------------------------------------------------------

template <int HD, bool CAUSAL, bool DROP = false>
__global__ __launch_bounds__(256, HD == 64 ? 2 : 1) void k_attn_bwd_dkv(const op16_t* __restrict__ qkv, const op16_t* __restrict__ dout,
                                                      const float* __restrict__ lse, const float* __restrict__ delta, int B, int S, int H,
                                                      float scale, op16_t* __restrict__ dqkv, Drop drop = Drop()) {
    constexpr int KK = HD / 16, NB = HD / 32;
    __shared__ __attribute__((aligned(16))) op16_t qsm[4][32 * AttLd<HD>::v];
    __shared__ __attribute__((aligned(16))) op16_t dsm[4][32 * AttLd<HD>::v];
    __shared__ __attribute__((aligned(16))) float ldsm[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nblk = (S + 31) >> 5;
    const int item = blockIdx.x * 4 + wave;
    if (item >= B * H * nblk) return;
    const int j = item % nblk, h = (item / nblk) % H, b = item / (nblk * H);
    const int D = H * HD;
    const size_t rs = (size_t)3 * D;
    const op16_t* base = qkv + (size_t)b * S * rs + h * HD;
    const op16_t* dbase = dout + (size_t)b * S * D + h * HD;
    const float* lrow = lse + ((size_t)b * H + h) * S;
    const float* drow = delta + ((size_t)b * H + h) * S;
    const int half = lane >> 5, key = j * 32 + (lane & 31);
    op16x8 kf[KK], vf[KK];
#pragma unroll
    for (int kk = 0; kk < KK; kk++) {
        kf[kk] = load_frag(base + D + (size_t)min(key, S - 1) * rs + kk * 16 + half * 8, key < S);
        vf[kk] = load_frag(base + 2 * D + (size_t)min(key, S - 1) * rs + kk * 16 + half * 8, key < S);
    }
    f32x16 dk[NB], dv[NB];
#pragma unroll
    for (int nb = 0; nb < NB; nb++)
#pragma unroll
        for (int r = 0; r < 16; r++) { dk[nb][r] = 0.f; dv[nb][r] = 0.f; }
    // The Q / dO fragments of query block i are loaded one iteration ahead (the loop is a chain of dependent global round trips
    // otherwise) and the row-major LDS copies the dK / dV products need are written from those same registers: the lanes'
    // fragments (row lane & 31, columns 16 kk + 8 half .. + 7) tile the block exactly.
    const int i0 = CAUSAL ? j : 0;
    op16x8 qf[KK], df[KK];
    {
        const int qa = i0 * 32 + (lane & 31);
#pragma unroll
        for (int kk = 0; kk < KK; kk++) {
            qf[kk] = load_frag(base + (size_t)min(qa, S - 1) * rs + kk * 16 + half * 8, qa < S);
            df[kk] = load_frag(dbase + (size_t)min(qa, S - 1) * D + kk * 16 + half * 8, qa < S);
        }
    }
    for (int i = i0; i < nblk; i++) {
        op16x8 qn[KK], dn[KK];
        {
            const int qa = (i + 1) * 32 + (lane & 31);      // block i + 1 (clamped rows; unused after the last iteration)
#pragma unroll
            for (int kk = 0; kk < KK; kk++) {
                qn[kk] = load_frag(base + (size_t)min(qa, S - 1) * rs + kk * 16 + half * 8, qa < S);
                dn[kk] = load_frag(dbase + (size_t)min(qa, S - 1) * D + kk * 16 + half * 8, qa < S);
            }
        }
        f32x16 s, dp;
#pragma unroll
        for (int r = 0; r < 16; r++) { s[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
        for (int kk = 0; kk < KK; kk++) {
            s = CC_MFMA_32x32x16(qf[kk], kf[kk], s);
            dp = CC_MFMA_32x32x16(df[kk], vf[kk], dp);
            *reinterpret_cast<op16x8*>(qsm[wave] + (lane & 31) * AttLd<HD>::v + kk * 16 + half * 8) = qf[kk];
            *reinterpret_cast<op16x8*>(dsm[wave] + (lane & 31) * AttLd<HD>::v + kk * 16 + half * 8) = df[kk];
        }
        // log-sum-exp and delta of the block's 32 queries: one coalesced load each into a wave-private LDS row, read back as
        // 4 x float4 per lane (queries 4 half + 8 g + 0..3) instead of 32 scalar global loads per iteration
        {
            const int qq = min(i * 32 + (lane & 31), S - 1);
            ldsm[wave][lane] = half ? drow[qq] : lrow[qq];          // [0,32): lse, [32,64): delta
        }
        float lq[16], dq_[16];
#pragma unroll
        for (int g4 = 0; g4 < 4; g4++) {
            const float4 a = *reinterpret_cast<const float4*>(&ldsm[wave][4 * half + 8 * g4]);
            const float4 b = *reinterpret_cast<const float4*>(&ldsm[wave][32 + 4 * half + 8 * g4]);
            lq[g4 * 4 + 0] = a.x; lq[g4 * 4 + 1] = a.y; lq[g4 * 4 + 2] = a.z; lq[g4 * 4 + 3] = a.w;
            dq_[g4 * 4 + 0] = b.x; dq_[g4 * 4 + 1] = b.y; dq_[g4 * 4 + 2] = b.z; dq_[g4 * 4 + 3] = b.w;
        }
        float p[16], ds[16];
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int qr = i * 32 + c_row(r, half);
            const bool ok = attn_live<CAUSAL>(qr, key, S);
            p[r] = ok ? __expf(s[r] * scale - lq[r]) : 0.f;
            if (DROP) {     // A_d = M A / (1-p): dV uses A_d, dA = M dA_d / (1-p), dS = A (dA - delta)  (delta = rowsum(dO O) = rowsum(A_d dA_d))
                const float mk = drop_mul(drop, attn_drop_idx(b, H, h, S, min(qr, S - 1), min(key, S - 1)));
                ds[r] = p[r] * (mk * dp[r] - dq_[r]) * scale;
                p[r] *= mk;
            } else {
                ds[r] = p[r] * (dp[r] - dq_[r]) * scale;
            }
        }
        const op16x8 pf[2] = {pack_frag(p), pack_frag(p + 8)};
        const op16x8 dsf[2] = {pack_frag(ds), pack_frag(ds + 8)};
#pragma unroll
        for (int t = 0; t < 2; t++)
#pragma unroll
            for (int nb = 0; nb < NB; nb++) {
                dv[nb] = CC_MFMA_32x32x16(frag_tr<HD>(dsm[wave], nb, t, lane), pf[t], dv[nb]);
                dk[nb] = CC_MFMA_32x32x16(frag_tr<HD>(qsm[wave], nb, t, lane), dsf[t], dk[nb]);
            }
#pragma unroll
        for (int kk = 0; kk < KK; kk++) { qf[kk] = qn[kk]; df[kk] = dn[kk]; }
    }
    if (key < S) {
        op16_t* orow = dqkv + ((size_t)b * S + key) * rs + h * HD;
#pragma unroll
        for (int nb = 0; nb < NB; nb++)
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const int d0 = nb * 32 + 8 * g + 4 * half;
                *reinterpret_cast<uint2*>(orow + D + d0) =
                    make_uint2(pack2op(dk[nb][g * 4 + 0], dk[nb][g * 4 + 1]), pack2op(dk[nb][g * 4 + 2], dk[nb][g * 4 + 3]));
                *reinterpret_cast<uint2*>(orow + 2 * D + d0) =
                    make_uint2(pack2op(dv[nb][g * 4 + 0], dv[nb][g * 4 + 1]), pack2op(dv[nb][g * 4 + 2], dv[nb][g * 4 + 3]));
            }
    }
}

template <int HD, bool CAUSAL, bool DROP = false>
__global__ __launch_bounds__(256, HD == 64 ? 3 : (HD == 96 ? 2 : 1)) void k_attn_bwd_dq(const op16_t* __restrict__ qkv, const op16_t* __restrict__ dout, const op16_t* __restrict__ o,
                                                     const float* __restrict__ lse, float* __restrict__ delta, int B, int S, int H,
                                                     float scale, op16_t* __restrict__ dqkv, Drop drop = Drop()) {
    constexpr int KK = HD / 16, NB = HD / 32;
    __shared__ __attribute__((aligned(16))) op16_t ksm[4][32 * AttLd<HD>::v];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nblk = (S + 31) >> 5;
    const int item = blockIdx.x * 4 + wave;
    if (item >= B * H * nblk) return;
    const int i = item % nblk, h = (item / nblk) % H, b = item / (nblk * H);
    const int D = H * HD;
    const size_t rs = (size_t)3 * D;
    const op16_t* base = qkv + (size_t)b * S * rs + h * HD;
    const op16_t* dbase = dout + (size_t)b * S * D + h * HD;
    const int half = lane >> 5, q = i * 32 + (lane & 31);
    const float my_lse = q < S ? lse[((size_t)b * H + h) * S + q] : 0.f;
    op16x8 qf[KK], dof[KK];
    // delta[q] = sum_d dO[q,d] O[q,d]: in this orientation a lane owns half of its query's row, so the dot product is 4 fragment
    // products + one cross-half shuffle.  Computed here and stored for the dK/dV kernel, which runs after this one (the separate
    // k_attn_delta launch is gone).
    float my_delta = 0.f;
#pragma unroll
    for (int kk = 0; kk < KK; kk++) {
        qf[kk] = load_frag(base + (size_t)min(q, S - 1) * rs + kk * 16 + half * 8, q < S);
        dof[kk] = load_frag(dbase + (size_t)min(q, S - 1) * D + kk * 16 + half * 8, q < S);
        const op16x8 of = load_frag(o + ((size_t)b * S + min(q, S - 1)) * D + h * HD + kk * 16 + half * 8, q < S);
        float x[8], y[8];
        unpack8(__builtin_bit_cast(uint4, dof[kk]), x);
        unpack8(__builtin_bit_cast(uint4, of), y);
#pragma unroll
        for (int e = 0; e < 8; e++) my_delta += x[e] * y[e];
    }
    my_delta += __shfl_xor(my_delta, 32, 64);
    if (half == 0 && q < S) delta[((size_t)b * H + h) * S + q] = my_delta;
    f32x16 dq[NB];
#pragma unroll
    for (int nb = 0; nb < NB; nb++)
#pragma unroll
        for (int r = 0; r < 16; r++) dq[nb][r] = 0.f;
    const int jend = CAUSAL ? i + 1 : nblk;
    // K / V fragments one key block ahead; the row-major K copy for dQ^T += K^T dS^T is written from the K fragment registers
    op16x8 kf[KK], vf[KK];
    {
        const int key = lane & 31;
#pragma unroll
        for (int kk = 0; kk < KK; kk++) {
            kf[kk] = load_frag(base + D + (size_t)min(key, S - 1) * rs + kk * 16 + half * 8, key < S);
            vf[kk] = load_frag(base + 2 * D + (size_t)min(key, S - 1) * rs + kk * 16 + half * 8, key < S);
        }
    }
    for (int j = 0; j < jend; j++) {
        op16x8 kn[KK], vn[KK];
        {
            const int key = (j + 1) * 32 + (lane & 31);
#pragma unroll
            for (int kk = 0; kk < KK; kk++) {
                kn[kk] = load_frag(base + D + (size_t)min(key, S - 1) * rs + kk * 16 + half * 8, key < S);
                vn[kk] = load_frag(base + 2 * D + (size_t)min(key, S - 1) * rs + kk * 16 + half * 8, key < S);
            }
        }
        f32x16 st, dpt;
#pragma unroll
        for (int r = 0; r < 16; r++) { st[r] = 0.f; dpt[r] = 0.f; }
#pragma unroll
        for (int kk = 0; kk < KK; kk++) {
            st = CC_MFMA_32x32x16(kf[kk], qf[kk], st);
            dpt = CC_MFMA_32x32x16(vf[kk], dof[kk], dpt);
            *reinterpret_cast<op16x8*>(ksm[wave] + (lane & 31) * AttLd<HD>::v + kk * 16 + half * 8) = kf[kk];
        }
        float ds[16];
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int kr = j * 32 + c_row(r, half);
            const bool ok = kr < S && q < S && (!CAUSAL || kr <= q);
            const float p = ok ? __expf(st[r] * scale - my_lse) : 0.f;
            const float mk = DROP ? drop_mul(drop, attn_drop_idx(b, H, h, S, min(q, S - 1), min(kr, S - 1))) : 1.0f;
            ds[r] = p * (mk * dpt[r] - my_delta) * scale;
        }
        const op16x8 dsf[2] = {pack_frag(ds), pack_frag(ds + 8)};
#pragma unroll
        for (int t = 0; t < 2; t++)
#pragma unroll
            for (int nb = 0; nb < NB; nb++)
                dq[nb] = CC_MFMA_32x32x16(frag_tr<HD>(ksm[wave], nb, t, lane), dsf[t], dq[nb]);
#pragma unroll
        for (int kk = 0; kk < KK; kk++) { kf[kk] = kn[kk]; vf[kk] = vn[kk]; }
    }
    if (q < S) {
        op16_t* orow = dqkv + ((size_t)b * S + q) * rs + h * HD;
        store_acc_row<NB>(orow, dq, half);
    }
}

// ------------------------------------------------------------------------------------------------------------
// One-pass backward for S <= 64 (the training shapes: 10 + 40 GPT-2 positions, 20 mapper rows): one wave per (sample, head) computes
// delta itself and walks the (key block j, query block i) pairs once, in the "S orientation" only (lane <-> key): bf16(P) and
// bf16(dS) are the B fragments of the dV / dK products as in k_attn_bwd_dkv, and dS goes through a wave-private [32 key][32 query]
// LDS tile whose transpose read is the B fragment of dQ_i^T[d][q] += K_j^T[d][key] dS^T[key][q] (same k-slot order as frag_tr's A
// fragments of the K copy).  One read of qkv / dO / O and one launch instead of two, no second score / exp pass.
// NBLK = number of 32-row blocks (1 or 2).  Q / dO of the next pair and K / V of the next key block are requested as soon as the
// current pair's score MFMAs have consumed their registers.
// ------------------------------------------------------------------------------------------------------------
#ifndef CC_ATTN_FUSED_OCC
#define CC_ATTN_FUSED_OCC 2
#endif
// ROWS < 32: the tile holds rows 0 .. ROWS-1 only; reads of the rows above are redirected to row ROWS-1 (finite values that the
// caller multiplies by exact zeros: those rows belong to keys / queries >= S)
template <int LD, int ROWS = 32>
__device__ __forceinline__ op16x8 frag_tr_ld(const op16_t* blk, int nb, int t, int lane) {
    typedef __attribute__((ext_vector_type(4))) short s16x4_t;
    typedef __attribute__((address_space(3))) s16x4_t* lp_t;
    const int half = lane >> 5, j = lane & 15, dsub = (lane >> 4) & 1;
    const int r0 = 16 * t + 4 * half + (j >> 2);
    const op16_t* col = blk + nb * 32 + 16 * dsub + 4 * (j & 3);
    const op16_t* p = col + (ROWS < 32 ? min(r0, ROWS - 1) : r0) * LD;
    const op16_t* ph = col + (ROWS < 32 ? min(r0 + 8, ROWS - 1) : r0 + 8) * LD;
    const s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp_t)p);
    const s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp_t)ph);
    typedef __attribute__((ext_vector_type(8))) short s16x8_t;
    const s16x8_t v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(op16x8, v);
}

// Accumulator tile (C layout: lane <-> row of the output block, registers <-> 16 of its HD columns) -> global rows, through a
// wave-private row-major LDS tile so that the stores are whole 16-B chunks of consecutive lanes (8 lanes per 128-B row at head
// dim 64) instead of 8-B pieces 4.5 KB apart: the scattered form cost 15 of the kernel's 40 us.
template <int HD>
__device__ __forceinline__ void attn_store_tile(op16_t* T, const f32x16 (&acc)[HD / 32], op16_t* gblock, size_t gstride, int rows_left, int lane) {
    constexpr int LD = AttLd<HD>::v, C8 = HD / 8;
    const int half = lane >> 5, l31 = lane & 31;
#pragma unroll
    for (int nb = 0; nb < HD / 32; nb++)
#pragma unroll
        for (int g = 0; g < 4; g++)
            *reinterpret_cast<uint2*>(T + l31 * LD + nb * 32 + 8 * g + 4 * half) =
                make_uint2(pack2op(acc[nb][g * 4 + 0], acc[nb][g * 4 + 1]), pack2op(acc[nb][g * 4 + 2], acc[nb][g * 4 + 3]));
#pragma unroll
    for (int it = 0; it < C8 / 2; it++) {
        const int idx = lane + 64 * it, row = idx / C8, chunk = idx % C8;
        const uint4 v = *reinterpret_cast<const uint4*>(T + row * LD + chunk * 8);
        if (row < rows_left) *reinterpret_cast<uint4*>(gblock + (size_t)row * gstride + chunk * 8) = v;
    }
}

// DR: rows of the dS^T tile (its own LDS tile when the K copy has no spare columns).  Head dim 96 misses two resident workgroups per CU by
// 2 KiB of LDS with 32 rows; with S <= 24 (the mapper: S = 20) the tile holds 24 and the launch asks for OCC = 2 — one round of 2048
// (sample, head) waves instead of two rounds at one wave per SIMD.
template <int HD, bool CAUSAL, bool DROP, int NBLK, int OCC, int DR = 32>
__global__ __launch_bounds__(256, OCC) void k_attn_bwd_fused(const op16_t* __restrict__ qkv, const op16_t* __restrict__ dout, const op16_t* __restrict__ o,
                                                             const float* __restrict__ lse, int B, int S, int H, float scale,
                                                             op16_t* __restrict__ dqkv, Drop drop = Drop()) {
    // the dS^T tile lives in the 32 spare columns of the K copy's rows when there are any (row pitch 96 / 160 for head dim 64 / 128),
    // otherwise in its own tile with 64-B rows (the 4 rows of a transpose read fall into 4 different bank slots either way)
    constexpr int KK = HD / 16, NB = HD / 32, LD = AttLd<HD>::v;
    constexpr bool SPARE = LD >= HD + 32;
    constexpr int LT = SPARE ? LD : 32;
    __shared__ __attribute__((aligned(16))) op16_t ksm[4][32 * LD];
    __shared__ __attribute__((aligned(16))) op16_t qsm[4][32 * LD];
    __shared__ __attribute__((aligned(16))) op16_t dsm[4][32 * LD];
    static_assert(DR == 32 || (!SPARE && NBLK == 1), "the short dS^T tile is for the single-block form with its own tile");
    __shared__ __attribute__((aligned(16))) op16_t dtx[SPARE ? 1 : 4][SPARE ? 8 : DR * 32];
    __shared__ __attribute__((aligned(16))) float ldsm[4][NBLK][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int item = blockIdx.x * 4 + wave;
    if (item >= B * H) return;          // wave-uniform; only wave-private LDS below, no block barrier
    const int h = item % H, b = item / H;
    const int D = H * HD;
    const size_t rs = (size_t)3 * D;
    const op16_t* base = qkv + (size_t)b * S * rs + h * HD;
    const op16_t* dbase = dout + (size_t)b * S * D + h * HD;
    const op16_t* obase = o + (size_t)b * S * D + h * HD;
    const float* lrow = lse + ((size_t)b * H + h) * S;
    const int half = lane >> 5, l31 = lane & 31;
    const int coff = half * 8;
    op16_t* dtm = SPARE ? ksm[wave] + HD : dtx[SPARE ? 0 : wave];

    op16x8 qf[KK], dof[KK], kf[KK], vf[KK];
    auto load_q = [&](int i) {
        const int q = i * 32 + l31, qc = min(q, S - 1);
#pragma unroll
        for (int kk = 0; kk < KK; kk++) {
            qf[kk] = load_frag(base + (size_t)qc * rs + kk * 16 + coff, q < S);
            dof[kk] = load_frag(dbase + (size_t)qc * D + kk * 16 + coff, q < S);
        }
    };
    auto load_k = [&](int j) {
        const int key = j * 32 + l31, kc = min(key, S - 1);
#pragma unroll
        for (int kk = 0; kk < KK; kk++) {
            kf[kk] = load_frag(base + D + (size_t)kc * rs + kk * 16 + coff, key < S);
            vf[kk] = load_frag(base + 2 * D + (size_t)kc * rs + kk * 16 + coff, key < S);
        }
    };
    load_k(0);
    load_q(0);
    // lse and delta = sum_d dO O of every query, row layout (lane <-> query, half <-> column half) -> LDS rows read back per pair
#pragma unroll
    for (int i = 0; i < NBLK; i++) {
        const int q = i * 32 + l31, qc = min(q, S - 1);
        float acc = 0.f;
#pragma unroll
        for (int kk = 0; kk < KK; kk++) {
            const op16x8 df = load_frag(dbase + (size_t)qc * D + kk * 16 + coff, q < S);
            const op16x8 of = load_frag(obase + (size_t)qc * D + kk * 16 + coff, q < S);
            float x[8], y[8];
            unpack8(__builtin_bit_cast(uint4, df), x);
            unpack8(__builtin_bit_cast(uint4, of), y);
#pragma unroll
            for (int e = 0; e < 8; e++) acc += x[e] * y[e];
        }
        acc += __shfl_xor(acc, 32, 64);
        ldsm[wave][i][lane] = half ? acc : lrow[qc];          // [0,32): lse, [32,64): delta
    }
    f32x16 dq[NBLK][NB];

#pragma unroll
    for (int j = 0; j < NBLK; j++) {
        const int key = j * 32 + l31;
#pragma unroll
        for (int kk = 0; kk < KK; kk++) *reinterpret_cast<op16x8*>(ksm[wave] + l31 * LD + kk * 16 + coff) = kf[kk];
        f32x16 dk[NB], dv[NB];
#pragma unroll
        for (int nb = 0; nb < NB; nb++)
#pragma unroll
            for (int r = 0; r < 16; r++) { dk[nb][r] = 0.f; dv[nb][r] = 0.f; }
#pragma unroll
        for (int i = 0; i < NBLK; i++) {
            if (CAUSAL && i < j) continue;
            const int ifirst = CAUSAL ? j : 0;
            // qf / dof hold block i here; the LDS copies are still valid if the previous pair had the same i
            if (!(j > 0 && i == ifirst && i == NBLK - 1)) {
#pragma unroll
                for (int kk = 0; kk < KK; kk++) {
                    *reinterpret_cast<op16x8*>(qsm[wave] + l31 * LD + kk * 16 + coff) = qf[kk];
                    *reinterpret_cast<op16x8*>(dsm[wave] + l31 * LD + kk * 16 + coff) = dof[kk];
                }
            }
            f32x16 s, dp;
#pragma unroll
            for (int r = 0; r < 16; r++) { s[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
            for (int kk = 0; kk < KK; kk++) {
                s = CC_MFMA_32x32x16(qf[kk], kf[kk], s);
                dp = CC_MFMA_32x32x16(dof[kk], vf[kk], dp);
            }
            // next operands
            if (i + 1 < NBLK) {
                load_q(i + 1);
            } else if (j + 1 < NBLK) {
                const int ni = CAUSAL ? j + 1 : 0;
                if (ni != i) load_q(ni);
                load_k(j + 1);
            }
            if (j == 0) {
#pragma unroll
                for (int nb = 0; nb < NB; nb++)
#pragma unroll
                    for (int r = 0; r < 16; r++) dq[i][nb][r] = 0.f;
            }
            float p[16], ds[16];
#pragma unroll
            for (int g4 = 0; g4 < 4; g4++) {
                const float4 lq = *reinterpret_cast<const float4*>(&ldsm[wave][i][4 * half + 8 * g4]);
                const float4 dl = *reinterpret_cast<const float4*>(&ldsm[wave][i][32 + 4 * half + 8 * g4]);
                const float lqa[4] = {lq.x, lq.y, lq.z, lq.w}, dla[4] = {dl.x, dl.y, dl.z, dl.w};
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const int r = g4 * 4 + e;
                    const int qr = i * 32 + c_row(r, half);
                    const bool ok = qr < S && key < S && (!CAUSAL || key <= qr);
                    p[r] = ok ? __expf(s[r] * scale - lqa[e]) : 0.f;
                    if (DROP) {
                        const float mk = drop_mul(drop, attn_drop_idx(b, H, h, S, min(qr, S - 1), min(key, S - 1)));
                        ds[r] = p[r] * (mk * dp[r] - dla[e]) * scale;
                        p[r] *= mk;
                    } else {
                        ds[r] = p[r] * (dp[r] - dla[e]) * scale;
                    }
                }
            }
            const op16x8 pf[2] = {pack_frag(p), pack_frag(p + 8)};
            const op16x8 dsf[2] = {pack_frag(ds), pack_frag(ds + 8)};
            // dS^T tile: row = key (this lane), columns = queries 8 g + 4 half + 0..3 (the register order of the accumulator layout)
            if (DR == 32 || l31 < DR) {        // short tile: keys >= DR are >= S, their dS is zero and their rows are never stored
#pragma unroll
                for (int t = 0; t < 2; t++) {
                    const uint4 w = __builtin_bit_cast(uint4, dsf[t]);
                    *reinterpret_cast<uint2*>(dtm + l31 * LT + 16 * t + 4 * half) = make_uint2(w.x, w.y);
                    *reinterpret_cast<uint2*>(dtm + l31 * LT + 16 * t + 8 + 4 * half) = make_uint2(w.z, w.w);
                }
            }
#pragma unroll
            for (int t = 0; t < 2; t++)
#pragma unroll
                for (int nb = 0; nb < NB; nb++) {
                    dv[nb] = CC_MFMA_32x32x16(frag_tr<HD>(dsm[wave], nb, t, lane), pf[t], dv[nb]);
                    dk[nb] = CC_MFMA_32x32x16(frag_tr<HD>(qsm[wave], nb, t, lane), dsf[t], dk[nb]);
                }
#pragma unroll
            for (int t = 0; t < 2; t++) {
                const op16x8 dst = frag_tr_ld<LT, DR>(dtm, 0, t, lane);
#pragma unroll
                for (int nb = 0; nb < NB; nb++) dq[i][nb] = CC_MFMA_32x32x16(frag_tr<HD>(ksm[wave], nb, t, lane), dst, dq[i][nb]);
            }
            if (j == (CAUSAL ? i : NBLK - 1)) {        // last key block that reaches query block i
                // block i's Q copy is dead here (the next pair, if any, has another i and rewrites it): stage dQ_i through it
                attn_store_tile<HD>(qsm[wave], dq[i], dqkv + ((size_t)b * S + i * 32) * rs + h * HD, rs, S - i * 32, lane);
            }
        }
        {      // the K copy is dead until the next j rewrites it
            op16_t* gblk = dqkv + ((size_t)b * S + j * 32) * rs + h * HD;
            attn_store_tile<HD>(ksm[wave], dk, gblk + D, rs, S - j * 32, lane);
            attn_store_tile<HD>(ksm[wave], dv, gblk + 2 * D, rs, S - j * 32, lane);
        }
    }
}

template <int HD, int NBLK>
static void attn_bwd_fused_launch(const op16_t* qkv, const op16_t* dout, const op16_t* o, const float* lse, int B, int S, int H, bool causal,
                                  op16_t* dqkv, hipStream_t st, Drop drop, float scale) {
    constexpr int OCC = CC_ATTN_FUSED_OCC;
    const dim3 grid((B * H + 3) / 4), blk(256);
#define CC_L(C, DR) attn_launch<k_attn_bwd_fused<HD, C, DR, NBLK, (C && HD == 64 ? OCC : 1)>>(grid, blk, 0, st, qkv, dout, o, lse, B, S, H, scale, dqkv, drop)
    if (drop.thresh || causal) ATTN_LADDER(CC_L)
    else {
        if constexpr (HD == 96 && NBLK == 1) {
            static const bool short_on = []() { const char* e = cc_lab_env("CC_ATTN_BWD_SHORT"); return !e || atoi(e) != 0; }();     // lab A/B switch
            if (S <= 24 && short_on) {
                attn_launch<k_attn_bwd_fused<HD, false, false, NBLK, 2, 24>>(grid, blk, 0, st, qkv, dout, o, lse, B, S, H, scale, dqkv, drop);
                return;
            }
        }
        CC_L(false, false);
    }
#undef CC_L
}

template <int HD>
static int attn_bwd_mfma_launch(const op16_t* qkv, const op16_t* dout, const op16_t* o, const float* lse, float* delta, int B, int S, int H,
                                bool causal, op16_t* dqkv, hipStream_t st, Drop drop) {
    const int items = B * H * ((S + 31) / 32);
    const float scale = 1.0f / sqrtf((float)HD);
    if (drop.thresh && !causal) return CC_ERR_SHAPE;
    static const int fused = []() { const char* e = cc_lab_env("CC_ATTN_BWD_FUSED"); return e ? atoi(e) : 1; }();   // A/B switch (0 = two-kernel path)
    if (fused && S <= 32) {
        attn_bwd_fused_launch<HD, 1>(qkv, dout, o, lse, B, S, H, causal, dqkv, st, drop, scale);
        return hipGetLastError() == hipSuccess ? CC_OK : CC_ERR_LAUNCH;
    }
    if constexpr (HD < 128) {      // two blocks at head dim 128 do not fit the register file (spills)
        if (fused && S <= 64) {
            attn_bwd_fused_launch<HD, 2>(qkv, dout, o, lse, B, S, H, causal, dqkv, st, drop, scale);
            return hipGetLastError() == hipSuccess ? CC_OK : CC_ERR_LAUNCH;
        }
    }
    // dQ first: it also produces delta, which the dK/dV kernel reads
#define CC_L(C, DR)                                                                                                                         \
    attn_launch<k_attn_bwd_dq<HD, C, DR>>(dim3((items + 3) / 4), dim3(256), 0, st, qkv, dout, o, lse, delta, B, S, H, scale, dqkv, drop); \
    attn_launch<k_attn_bwd_dkv<HD, C, DR>>(dim3((items + 3) / 4), dim3(256), 0, st, qkv, dout, lse, delta, B, S, H, scale, dqkv, drop)
    ATTN_LADDER(CC_L)
#undef CC_L
    return hipGetLastError() == hipSuccess ? CC_OK : CC_ERR_LAUNCH;
}

#endif   // CC_OP != 2

static size_t attn_fwd_lds(int S, int hd) { return ((size_t)3 * S * (hd + 4) + (size_t)S * (S + 1)) * 4; }
static size_t attn_bwd_lds(int S, int hd) {
    if (S < 32) return ((size_t)4 * S * (hd + 4) + (size_t)2 * S * (S + 1)) * 4;      // k_attn_bwd_small
    const size_t S4 = (S + 3) & ~3;
    return ((size_t)4 * S4 * (hd + 4) + (size_t)2 * S4 * (S4 + 4)) * 4;
}

// Attention probabilities of an un-masked self-attention layer, recomputed from the stored qkv rows: what the reference's
// MultiHeadAttention.forward returns as its second value (attention.py:32-42, layout (b, n, m, h)).  One wave per (b, h, query);
// an inspection / visualisation output, not on the training path.
__global__ __launch_bounds__(256) void k_attn_probs(const act_t* __restrict__ qkv, int B, int S, int H, int hd, float scale,
                                                    float* __restrict__ out) {
    const int wave = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (wave >= B * H * S) return;
    const int n = wave % S, h = (wave / S) % H, b = wave / (S * H);
    const int D = H * hd;
    const act_t* q = qkv + ((size_t)b * S + n) * 3 * D + h * hd;
    float mx = -INFINITY;
    for (int m0 = 0; m0 < S; m0 += 64) {
        const int m = m0 + lane;
        float sc = -INFINITY;
        if (m < S) {
            const act_t* k = qkv + ((size_t)b * S + m) * 3 * D + D + h * hd;
            float acc = 0.f;
            for (int d = 0; d < hd; d++) acc += act2f(q[d]) * act2f(k[d]);
            sc = acc * scale;
            out[(((size_t)b * S + n) * S + m) * H + h] = sc;
        }
        mx = fmaxf(mx, wave_max(sc));
    }
    float sum = 0.f;
    for (int m = lane; m < S; m += 64) sum += __expf(out[(((size_t)b * S + n) * S + m) * H + h] - mx);
    sum = wave_sum(sum);
    for (int m = lane; m < S; m += 64) {
        float* o = out + (((size_t)b * S + n) * S + m) * H + h;
        *o = __expf(*o - mx) / sum;
    }
}
int attn_probs(const act_t* qkv, int B, int S, int H, int hd, float* out, hipStream_t st) {
    const int waves = B * H * S;
    if (waves <= 0) return CC_OK;
    hipLaunchKernelGGL(k_attn_probs, dim3((waves + 3) / 4), dim3(256), 0, st, qkv, B, S, H, hd, 1.0f / sqrtf((float)hd), out);
    return CC_OK;
}

#if CC_OP == 2
// ------------------------------------------------------------------------------------------------------------
// bf16x3 build, sequences whose S x S tile does not fit the LDS kernels (the windowed mapper: S = 180): plain fp32 attention with one
// wave per row, any S <= 2048, K / V / Q rows read through the caches.  Parity mode: simplicity over speed.
//   forward   (wave per query i): scores over the keys -> LDS row, softmax, O_i = P_i V, log-sum-exp
//   backward  dq  (wave per query i): P_i, dP_i = dO_i V^T, delta_i = dO_i . O_i (stored), dS_i -> LDS row, dQ_i = dS_i K
//             dkv (wave per key j):   P_:j, dS_:j over the queries -> LDS, dK_j = dS_:j^T Q, dV_j = P_:j^T dO
// ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float row_dot(const float* a, const float* b, int hd) {
    float s0 = 0.f, s1 = 0.f;
    for (int d = 0; d < hd; d += 8) {
        const float4 x0 = *reinterpret_cast<const float4*>(a + d), y0 = *reinterpret_cast<const float4*>(b + d);
        const float4 x1 = *reinterpret_cast<const float4*>(a + d + 4), y1 = *reinterpret_cast<const float4*>(b + d + 4);
        s0 += x0.x * y0.x + x0.y * y0.y + x0.z * y0.z + x0.w * y0.w;
        s1 += x1.x * y1.x + x1.y * y1.y + x1.z * y1.z + x1.w * y1.w;
    }
    return s0 + s1;
}
template <bool CAUSAL>
__global__ __launch_bounds__(256) void k_attn_fwd_rows(const float* __restrict__ qkv, int B, int S, int H, int hd, float scale, float* __restrict__ out,
                                                       float* __restrict__ lse) {
    extern __shared__ float rsm[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int item = blockIdx.x * 4 + wave;
    if (item >= B * H * S) return;
    const int i = item % S, h = (item / S) % H, b = item / (S * H);
    const int D = H * hd;
    const size_t rs = (size_t)3 * D;
    const float* base = qkv + (size_t)b * S * rs + h * hd;
    const float* q = base + (size_t)i * rs;
    float* p = rsm + wave * S;
    const int nk = CAUSAL ? i + 1 : S;
    float m = -INFINITY;
    for (int j = lane; j < nk; j += 64) {
        const float sc = row_dot(q, base + D + (size_t)j * rs, hd) * scale;
        p[j] = sc;
        m = fmaxf(m, sc);
    }
    m = wave_max(m);
    float sum = 0.f;
    for (int j = lane; j < nk; j += 64) {
        const float e = __expf(p[j] - m);
        p[j] = e;
        sum += e;
    }
    sum = wave_sum(sum);
    const float inv = 1.f / sum;
    for (int d = lane; d < hd; d += 64) {
        float o = 0.f;
        const float* v = base + 2 * D + d;
        for (int j = 0; j < nk; j++) o += p[j] * v[(size_t)j * rs];
        out[((size_t)b * S + i) * D + h * hd + d] = o * inv;
    }
    if (lane == 0 && lse) lse[((size_t)b * H + h) * S + i] = m + __logf(sum);
}
template <bool CAUSAL>
__global__ __launch_bounds__(256) void k_attn_bwd_rows_dq(const float* __restrict__ qkv, const float* __restrict__ dout, const float* __restrict__ o,
                                                          const float* __restrict__ lse, float* __restrict__ delta, int B, int S, int H, int hd,
                                                          float scale, float* __restrict__ dqkv) {
    extern __shared__ float rsm[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int item = blockIdx.x * 4 + wave;
    if (item >= B * H * S) return;
    const int i = item % S, h = (item / S) % H, b = item / (S * H);
    const int D = H * hd;
    const size_t rs = (size_t)3 * D;
    const float* base = qkv + (size_t)b * S * rs + h * hd;
    const float* q = base + (size_t)i * rs;
    const float* dor = dout + ((size_t)b * S + i) * D + h * hd;
    const float* orow = o + ((size_t)b * S + i) * D + h * hd;
    float* ds = rsm + wave * S;
    float dl = 0.f;
    for (int d = lane; d < hd; d += 64) dl += dor[d] * orow[d];
    dl = wave_sum(dl);
    const float l = lse[((size_t)b * H + h) * S + i];
    if (lane == 0) delta[((size_t)b * H + h) * S + i] = dl;
    const int nk = CAUSAL ? i + 1 : S;
    for (int j = lane; j < nk; j += 64) {
        const float pj = __expf(row_dot(q, base + D + (size_t)j * rs, hd) * scale - l);
        const float dp = row_dot(dor, base + 2 * D + (size_t)j * rs, hd);
        ds[j] = pj * (dp - dl) * scale;
    }
    for (int d = lane; d < hd; d += 64) {
        float acc = 0.f;
        const float* k = base + D + d;
        for (int j = 0; j < nk; j++) acc += ds[j] * k[(size_t)j * rs];
        dqkv[((size_t)b * S + i) * rs + h * hd + d] = acc;
    }
}
template <bool CAUSAL>
__global__ __launch_bounds__(256) void k_attn_bwd_rows_dkv(const float* __restrict__ qkv, const float* __restrict__ dout, const float* __restrict__ lse,
                                                           const float* __restrict__ delta, int B, int S, int H, int hd, float scale,
                                                           float* __restrict__ dqkv) {
    extern __shared__ float rsm[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int item = blockIdx.x * 4 + wave;
    if (item >= B * H * S) return;
    const int j = item % S, h = (item / S) % H, b = item / (S * H);
    const int D = H * hd;
    const size_t rs = (size_t)3 * D;
    const float* base = qkv + (size_t)b * S * rs + h * hd;
    const float* k = base + D + (size_t)j * rs;
    const float* v = base + 2 * D + (size_t)j * rs;
    const float* dbase = dout + (size_t)b * S * D + h * hd;
    const float* lrow = lse + ((size_t)b * H + h) * S;
    const float* drow = delta + ((size_t)b * H + h) * S;
    float* pp = rsm + wave * 2 * S;
    float* ds = pp + S;
    const int i0 = CAUSAL ? j : 0;
    for (int i = i0 + lane; i < S; i += 64) {
        const float pij = __expf(row_dot(base + (size_t)i * rs, k, hd) * scale - lrow[i]);
        const float dp = row_dot(dbase + (size_t)i * D, v, hd);
        pp[i] = pij;
        ds[i] = pij * (dp - drow[i]) * scale;
    }
    for (int d = lane; d < hd; d += 64) {
        float dk = 0.f, dv = 0.f;
        for (int i = i0; i < S; i++) {
            dk += ds[i] * base[(size_t)i * rs + d];
            dv += pp[i] * dbase[(size_t)i * D + d];
        }
        float* orow = dqkv + ((size_t)b * S + j) * rs + h * hd + d;
        orow[D] = dk;
        orow[2 * D] = dv;
    }
}
static int attn_fwd_rows(const float* qkv, int B, int S, int H, int hd, bool causal, float* out, float* lse, float scale, hipStream_t st) {
    if (S > 2048) return CC_ERR_SHAPE;
    const int items = B * H * S;
    const size_t sh = (size_t)4 * S * sizeof(float);
    if (causal) hipLaunchKernelGGL(k_attn_fwd_rows<true>, dim3((items + 3) / 4), dim3(256), sh, st, qkv, B, S, H, hd, scale, out, lse);
    else hipLaunchKernelGGL(k_attn_fwd_rows<false>, dim3((items + 3) / 4), dim3(256), sh, st, qkv, B, S, H, hd, scale, out, lse);
    return hipGetLastError() == hipSuccess ? CC_OK : CC_ERR_LAUNCH;
}
static int attn_bwd_rows(const float* qkv, const float* dout, const float* o, const float* lse, float* delta, int B, int S, int H, int hd,
                         bool causal, float* dqkv, float scale, hipStream_t st) {
    if (S > 2048) return CC_ERR_SHAPE;
    const int items = B * H * S;
    const dim3 gr((items + 3) / 4), bl(256);
    const size_t sh1 = (size_t)4 * S * sizeof(float), sh2 = 2 * sh1;
    if (causal) {
        hipLaunchKernelGGL(k_attn_bwd_rows_dq<true>, gr, bl, sh1, st, qkv, dout, o, lse, delta, B, S, H, hd, scale, dqkv);
        hipLaunchKernelGGL(k_attn_bwd_rows_dkv<true>, gr, bl, sh2, st, qkv, dout, lse, delta, B, S, H, hd, scale, dqkv);
    } else {
        hipLaunchKernelGGL(k_attn_bwd_rows_dq<false>, gr, bl, sh1, st, qkv, dout, o, lse, delta, B, S, H, hd, scale, dqkv);
        hipLaunchKernelGGL(k_attn_bwd_rows_dkv<false>, gr, bl, sh2, st, qkv, dout, lse, delta, B, S, H, hd, scale, dqkv);
    }
    return hipGetLastError() == hipSuccess ? CC_OK : CC_ERR_LAUNCH;
}

#ifdef CC_EXPERIMENTS      // lab build only (make lab): measured slower than the VALU kernels, see attn_f32mfma_ok
// ------------------------------------------------------------------------------------------------------------
// fp32 attention on the fp32 MATRIX pipe (round 4, an A/B option — see attn_f32mfma_ok for the measurement that keeps it off): the LDS-tile
// kernels above with their three / five products moved from VALU dot
// products to v_mfma_f32_32x32x2_f32 (gfx950's fp32 MFMA: 64 FLOP/clk/SIMD — 1/16 of the bf16 MFMA, twice the VALU FMA rate, and no
// LDS operand read per FMA).  Same arithmetic (fp32 products, fp32 accumulation), same interface, same dropout rule; sequences up to 96
// (32-row tiles: NT = ceil(S / 32) <= 3), head dims that are multiples of 32.  Fragments: a lane feeds A[row = lane % 32][k] and
// B[k][col = lane % 32] with k chosen by its half (lane / 32); a 16-B LDS read per operand serves FOUR MFMAs (lanes < 32 hold
// k = 8t .. 8t+3, lanes >= 32 hold 8t+4 .. 8t+7 — any pairing works as long as A and B use the same one).  Accumulator register r of a
// lane is element (row 8 (r / 4) + 4 (lane / 32) + r % 4, col lane % 32).  Rows / columns beyond S are zero-filled in LDS.
// ------------------------------------------------------------------------------------------------------------
typedef float v16f __attribute__((ext_vector_type(16)));
#define CC_MFMA_F32(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0)

__device__ __forceinline__ void load_head_rows_pad(float* dst, int hdp, const float* src, size_t ld, int S, int RP, int hd) {
    const int c4n = hd >> 2;
    for (int idx = threadIdx.x; idx < RP * c4n; idx += blockDim.x) {
        const int r = idx / c4n, c = idx % c4n;
        const float4 v = r < S ? *reinterpret_cast<const float4*>(src + (size_t)r * ld + c * 4) : make_float4(0, 0, 0, 0);
        *reinterpret_cast<float4*>(dst + r * hdp + c * 4) = v;
    }
}
// acc += X[rows r0 ..][d] . Y[rows c0 ..][d]^T over d < hd (both row-major with stride hdp): the scores / dP form
__device__ __forceinline__ void mm_rows_rows(v16f& acc, const float* X, int r0, const float* Y, int c0, int hdp, int hd, int lane) {
    const float* xa = X + (r0 + (lane & 31)) * hdp + 4 * (lane >> 5);
    const float* yb = Y + (c0 + (lane & 31)) * hdp + 4 * (lane >> 5);
    for (int d8 = 0; d8 < hd; d8 += 8) {
        const float4 a = *reinterpret_cast<const float4*>(xa + d8), b = *reinterpret_cast<const float4*>(yb + d8);
        acc = CC_MFMA_F32(a.x, b.x, acc);
        acc = CC_MFMA_F32(a.y, b.y, acc);
        acc = CC_MFMA_F32(a.z, b.z, acc);
        acc = CC_MFMA_F32(a.w, b.w, acc);
    }
}

template <bool CAUSAL, bool DROP>
__global__ __launch_bounds__(256) void k_attn_fwd_f32mfma(const float* __restrict__ qkv, int S, int H, int hd, float scale, float* __restrict__ out,
                                                          float* __restrict__ lse, Drop drop) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int D = H * hd, hdp = hd + 4, NT = (S + 31) >> 5, RP = NT * 32, Sp = RP + 4;
    float* Qs = sm;
    float* Ks = Qs + RP * hdp;
    float* Vs = Ks + RP * hdp;
    float* Ps = Vs + RP * hdp;
    const int b = blockIdx.x / H, h = blockIdx.x % H;
    const float* base = qkv + (size_t)b * S * 3 * D + h * hd;
    load_head_rows_pad(Qs, hdp, base, 3 * D, S, RP, hd);
    load_head_rows_pad(Ks, hdp, base + D, 3 * D, S, RP, hd);
    load_head_rows_pad(Vs, hdp, base + 2 * D, 3 * D, S, RP, hd);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 31, lh = lane >> 5;
    for (int t = wave; t < NT * NT; t += 4) {
        const int ti = t / NT, tj = t - ti * NT;
        v16f acc;
        acc_zero(acc);
        if (!(CAUSAL && tj > ti)) mm_rows_rows(acc, Qs, ti * 32, Ks, tj * 32, hdp, hd, lane);
        const int j = tj * 32 + lr;
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int i = ti * 32 + 8 * (r >> 2) + 4 * lh + (r & 3);
            Ps[i * Sp + j] = (j < S && !(CAUSAL && j > i)) ? acc[r] * scale : -INFINITY;
        }
    }
    __syncthreads();
    for (int i = wave; i < S; i += 4) {                    // softmax: one wave per row (padding columns hold -inf -> 0)
        float m = -INFINITY;
        for (int j = lane; j < RP; j += 64) m = fmaxf(m, Ps[i * Sp + j]);
        m = wave_max(m);
        float sum = 0.f;
        for (int j = lane; j < RP; j += 64) {
            const float e = __expf(Ps[i * Sp + j] - m);
            Ps[i * Sp + j] = e;
            sum += e;
        }
        sum = wave_sum(sum);
        const float inv = 1.f / sum;
        for (int j = lane; j < RP; j += 64) Ps[i * Sp + j] *= inv;
        if (lane == 0 && lse) lse[((size_t)b * H + h) * S + i] = m + __logf(sum);
    }
    for (int i = S + wave; i < RP; i += 4)                 // padding rows: zero probabilities (never stored, but keep them finite)
        for (int j = lane; j < RP; j += 64) Ps[i * Sp + j] = 0.f;
    __syncthreads();
    const int nd = hd >> 5;
    for (int t = wave; t < NT * nd; t += 4) {              // O = P V, tile (ti, td)
        const int ti = t / nd, td = t - ti * nd;
        v16f acc;
        acc_zero(acc);
        const int jmax = CAUSAL ? (ti + 1) * 32 : RP;
        const int i = ti * 32 + lr;
        const float* pa = Ps + i * Sp + 4 * lh;
        const float* vb = Vs + 4 * lh * hdp + td * 32 + lr;
        for (int j8 = 0; j8 < jmax; j8 += 8) {
            float4 a = *reinterpret_cast<const float4*>(pa + j8);
            if (DROP) {                                    // attention-probability dropout: P V only
                const unsigned e0 = attn_drop_idx(b, H, h, S, i, j8 + 4 * lh);
                a.x *= drop_mul(drop, e0); a.y *= drop_mul(drop, e0 + 1); a.z *= drop_mul(drop, e0 + 2); a.w *= drop_mul(drop, e0 + 3);
            }
            const float* v = vb + j8 * hdp;
            acc = CC_MFMA_F32(a.x, v[0], acc);
            acc = CC_MFMA_F32(a.y, v[hdp], acc);
            acc = CC_MFMA_F32(a.z, v[2 * hdp], acc);
            acc = CC_MFMA_F32(a.w, v[3 * hdp], acc);
        }
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int io = ti * 32 + 8 * (r >> 2) + 4 * lh + (r & 3);
            if (io < S) out[((size_t)b * S + io) * D + h * hd + td * 32 + lr] = acc[r];
        }
    }
}

template <bool CAUSAL, bool DROP>
__global__ __launch_bounds__(256) void k_attn_bwd_f32mfma(const float* __restrict__ qkv, const float* __restrict__ dout, const float* __restrict__ lse,
                                                          int S, int H, int hd, float scale, float* __restrict__ dqkv, Drop drop) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int D = H * hd, hdp = hd + 4, NT = (S + 31) >> 5, RP = NT * 32, Sp = RP + 4;
    float* Qs = sm;
    float* Ks = Qs + RP * hdp;
    float* Vs = Ks + RP * hdp;
    float* Os = Vs + RP * hdp;   // dO
    float* Ps = Os + RP * hdp;
    float* Ds = Ps + RP * Sp;    // dP, then dS
    float* Ls = Ds + RP * Sp;    // lse of the rows
    const int b = blockIdx.x / H, h = blockIdx.x % H;
    const float* base = qkv + (size_t)b * S * 3 * D + h * hd;
    load_head_rows_pad(Qs, hdp, base, 3 * D, S, RP, hd);
    load_head_rows_pad(Ks, hdp, base + D, 3 * D, S, RP, hd);
    load_head_rows_pad(Vs, hdp, base + 2 * D, 3 * D, S, RP, hd);
    load_head_rows_pad(Os, hdp, dout + (size_t)b * S * D + h * hd, D, S, RP, hd);
    for (int i = threadIdx.x; i < RP; i += 256) Ls[i] = i < S ? lse[((size_t)b * H + h) * S + i] : 0.f;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 31, lh = lane >> 5;
    for (int t = wave; t < NT * NT; t += 4) {              // P = exp(Q K^T scale - lse), dP = dO V^T, tile (ti, tj)
        const int ti = t / NT, tj = t - ti * NT;
        v16f sa, da;
        acc_zero(sa);
        acc_zero(da);
        if (!(CAUSAL && tj > ti)) {
            mm_rows_rows(sa, Qs, ti * 32, Ks, tj * 32, hdp, hd, lane);
            mm_rows_rows(da, Os, ti * 32, Vs, tj * 32, hdp, hd, lane);
        }
        const int j = tj * 32 + lr;
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int i = ti * 32 + 8 * (r >> 2) + 4 * lh + (r & 3);
            const bool live = attn_live<CAUSAL>(i, j, S);
            Ps[i * Sp + j] = live ? __expf(sa[r] * scale - Ls[i]) : 0.f;
            float dp = live ? da[r] : 0.f;
            if (DROP && live) dp *= drop_mul(drop, attn_drop_idx(b, H, h, S, i, j));
            Ds[i * Sp + j] = dp;
        }
    }
    __syncthreads();
    for (int i = wave; i < S; i += 4) {                    // delta_i = sum_j P dP;  dS = P (dP - delta) scale
        float dl = 0.f;
        for (int j = lane; j < RP; j += 64) dl += Ps[i * Sp + j] * Ds[i * Sp + j];
        dl = wave_sum(dl);
        for (int j = lane; j < RP; j += 64) Ds[i * Sp + j] = Ps[i * Sp + j] * (Ds[i * Sp + j] - dl) * scale;
    }
    __syncthreads();
    const int nd = hd >> 5, per = NT * nd;
    for (int t = wave; t < 3 * per; t += 4) {              // dQ = dS K | dK = dS^T Q | dV = (P mask)^T dO, tile (tr, td)
        const int which = t / per, u = t - which * per, tr = u / nd, td = u - tr * nd;
        v16f acc;
        acc_zero(acc);
        if (which == 0) {
            const int jmax = CAUSAL ? (tr + 1) * 32 : RP;
            const float* pa = Ds + (tr * 32 + lr) * Sp + 4 * lh;
            const float* kb = Ks + 4 * lh * hdp + td * 32 + lr;
            for (int j8 = 0; j8 < jmax; j8 += 8) {
                const float4 a = *reinterpret_cast<const float4*>(pa + j8);
                const float* k = kb + j8 * hdp;
                acc = CC_MFMA_F32(a.x, k[0], acc);
                acc = CC_MFMA_F32(a.y, k[hdp], acc);
                acc = CC_MFMA_F32(a.z, k[2 * hdp], acc);
                acc = CC_MFMA_F32(a.w, k[3 * hdp], acc);
            }
        } else {
            const int ilo = CAUSAL ? tr * 32 : 0;          // queries i >= key block
            const float* W = which == 1 ? Ds : Ps;
            const float* X = which == 1 ? Qs : Os;
            const int j = tr * 32 + lr;
            for (int i8 = ilo; i8 < RP; i8 += 8) {
                const int i0 = i8 + 4 * lh;
                float a0 = W[i0 * Sp + j], a1 = W[(i0 + 1) * Sp + j], a2 = W[(i0 + 2) * Sp + j], a3 = W[(i0 + 3) * Sp + j];
                if (DROP && which == 2) {
                    const unsigned e0 = attn_drop_idx(b, H, h, S, i0, j);
                    a0 *= drop_mul(drop, e0); a1 *= drop_mul(drop, e0 + S); a2 *= drop_mul(drop, e0 + 2 * S); a3 *= drop_mul(drop, e0 + 3 * S);
                }
                const float* x = X + i0 * hdp + td * 32 + lr;
                acc = CC_MFMA_F32(a0, x[0], acc);
                acc = CC_MFMA_F32(a1, x[hdp], acc);
                acc = CC_MFMA_F32(a2, x[2 * hdp], acc);
                acc = CC_MFMA_F32(a3, x[3 * hdp], acc);
            }
        }
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int ro = tr * 32 + 8 * (r >> 2) + 4 * lh + (r & 3);
            if (ro < S) dqkv[((size_t)b * S + ro) * 3 * D + which * D + h * hd + td * 32 + lr] = acc[r];
        }
    }
}
#endif   // CC_EXPERIMENTS
static size_t attn_f32mfma_lds(int S, int hd, bool bwd) {
    const size_t RP = (size_t)((S + 31) / 32) * 32, hdp = hd + 4, Sp = RP + 4;
    return ((bwd ? 4 : 3) * RP * hdp + (bwd ? 2 : 1) * RP * Sp + (bwd ? RP : 0)) * sizeof(float);
}
static bool attn_f32mfma_ok(int S, int hd, bool bwd) {
    // OFF by default: measured on MI355X (config-2 step, split-bf16 mode, two alternations) 40.4 ms with these kernels against 38.6 ms with the
    // VALU LDS-tile kernels — the fp32 MFMA is only 2x the VALU FMA rate, and 32-row tiles pad S = 50 to 64 (1.64x the products) and skip
    // causal work per tile (3 of 4 tiles) instead of per element (51 %).  CC_ATTN_F32MFMA=1 selects them (same results: tests pass either way).
#ifdef CC_EXPERIMENTS
    static const bool on = cc_lab_env("CC_ATTN_F32MFMA") != nullptr;
    return on && S <= 96 && (hd & 31) == 0 && attn_f32mfma_lds(S, hd, bwd) <= 160 * 1024;
#else
    (void)S; (void)hd; (void)bwd;
    return false;              // the product library does not carry these kernels
#endif
}
#endif   // CC_OP == 2

int attn_fwd(const act_t* qkv, int B, int S, int H, int hd, bool causal, Act outo, float* lse, hipStream_t st, Drop drop) {
    if ((hd & 7) || S <= 0) return CC_ERR_SHAPE;
    act_t* const out = outo.p;
    const int img = outo.img ? 1 : 0;       // the next GEMM reads `out` as an operand image (the owner asked attn_fwd_can_image)
    if (img && (outo.img != H * hd || !attn_fwd_can_image(S, hd))) return CC_ERR_STATE;
#if CC_OP != 2
    static const bool no_mfma = cc_lab_env("CC_ATTN_VALU") != nullptr;   // A/B switch for profiling
    if (!no_mfma || drop.thresh) {
        if (hd == 64) return attn_fwd_mfma_launch<64>(qkv, B, S, H, causal, out, lse, st, drop);
        if (hd == 96) return attn_fwd_mfma_launch<96>(qkv, B, S, H, causal, out, lse, st, drop);
        if (hd == 128) return attn_fwd_mfma_launch<128>(qkv, B, S, H, causal, out, lse, st, drop);
    }
#endif
    if (drop.thresh && (!kX3 || !causal)) return CC_ERR_SHAPE;          // dropout on the VALU kernels: the bf16x3 build's GPT-2 path only
    const float scale = 1.0f / sqrtf((float)hd);
#if CC_OP == 2
    if (attn_x3mfma_on() && (hd == 64 || hd == 96 || hd == 128)) {       // three bf16 MFMA terms per product
        if (hd == 64) return attn_fwd_mfma3_launch<64>(qkv, B, S, H, causal, out, lse, st, drop, img);
        if (hd == 96) return attn_fwd_mfma3_launch<96>(qkv, B, S, H, causal, out, lse, st, drop, img);
        return attn_fwd_mfma3_launch<128>(qkv, B, S, H, causal, out, lse, st, drop, img);
    }
#ifdef CC_EXPERIMENTS
    if (attn_f32mfma_ok(S, hd, false)) {                                 // fp32 products on the fp32 MFMA
        const size_t sh = attn_f32mfma_lds(S, hd, false);
#define CC_L(C, DR) attn_launch<k_attn_fwd_f32mfma<C, DR>>(dim3(B * H), dim3(256), sh, st, qkv, S, H, hd, scale, out, lse, drop)
        ATTN_LADDER(CC_L)
#undef CC_L
        return hipGetLastError() == hipSuccess ? CC_OK : CC_ERR_LAUNCH;
    }
#endif
#endif
    const size_t sh = attn_fwd_lds(S, hd);
    if (sh > 160 * 1024) {
#if CC_OP == 2
        if (drop.thresh) return CC_ERR_SHAPE;
        return attn_fwd_rows(qkv, B, S, H, hd, causal, out, lse, scale, st);
#else
        return CC_ERR_SHAPE;
#endif
    }
#define CC_L(C, DR) attn_launch<k_attn_fwd<C, DR>>(dim3(B * H), dim3(256), sh, st, qkv, S, H, hd, scale, out, lse, DR ? drop : Drop(), img)
    ATTN_LADDER(CC_L)
#undef CC_L
    return hipGetLastError() == hipSuccess ? CC_OK : CC_ERR_LAUNCH;
}

// Backward: recompute P from the saved lse; dP = dO V^T; delta_i = sum_j P_ij dP_ij (== dO_i . O_i);
// dS = P (dP - delta) * scale; dQ = dS K; dK = dS^T Q; dV = P^T dO.  Writes dqkv (bf16) in the qkv layout.
// With attention-probability dropout (DROP; mask M, keep scale 1/(1-p)): A_d = M A / (1-p) entered the forward's P V, so
// dV = A_d^T dO, dA = M dA_d / (1-p) with dA_d = dO V^T, delta = rowsum(A dA), dS = A (dA - delta) scale.
template <bool CAUSAL, bool DROP = false>
__global__ __launch_bounds__(256) void k_attn_bwd(const act_t* __restrict__ qkv, const act_t* __restrict__ dout,
                                                  const float* __restrict__ lse, int S, int H, int hd, float scale,
                                                  act_t* __restrict__ dqkv, Drop drop = Drop(), int img = 0) {
    // img (bf16x3 build): dqkv receives the [hi | hi | lo] operand image (rows of 3 * 3D 16-bit elements) of c_attn's input-gradient GEMM.
    // Round 4: 4 x 4 register blocks.  The first form (a thread = 4 queries x 1 key, then 1 row x 4 columns) read 5-6 B of LDS per FMA and
    // was bound by the LDS port (2.9 MB per block at S = 50, hd = 64); blocks of 4 queries x 4 keys and 4 rows x 4 columns read 2 B per
    // FMA.  Rows / columns beyond S are zero in LDS, so the inner loops carry no bounds or mask tests.
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int D = H * hd, hdp = hd + 4, S4 = (S + 3) & ~3, Sp = S4 + 4, NB = S4 >> 2;
    float* Qs = sm;
    float* Ks = Qs + S4 * hdp;
    float* Vs = Ks + S4 * hdp;
    float* Os = Vs + S4 * hdp;  // dO
    float* Ps = Os + S4 * hdp;
    float* Ds = Ps + S4 * Sp;   // dP then dS
    const int b = blockIdx.x / H, h = blockIdx.x % H;
    const act_t* base = qkv + (size_t)b * S * 3 * D + h * hd;
    load_head_rows(Qs, hdp, base, 3 * D, S, hd);
    load_head_rows(Ks, hdp, base + D, 3 * D, S, hd);
    load_head_rows(Vs, hdp, base + 2 * D, 3 * D, S, hd);
    load_head_rows(Os, hdp, dout + (size_t)b * S * D + h * hd, D, S, hd);
    for (int idx = threadIdx.x; idx < (S4 - S) * hdp; idx += 256) {          // zero rows S .. S4-1 of the four operand tiles
        const int o = S * hdp + idx;
        Qs[o] = 0.f; Ks[o] = 0.f; Vs[o] = 0.f; Os[o] = 0.f;
    }
    __syncthreads();
    const float* lrow = lse + ((size_t)b * H + h) * S;
    // ---- P = exp(Q K^T scale - lse), dP = dO V^T: thread = (4 queries, 4 keys)
    for (int idx = threadIdx.x; idx < NB * NB; idx += 256) {
        const int qb = idx / NB, kb = idx - qb * NB, i0 = qb * 4, j0 = kb * 4;
        float sa[4][4], da[4][4];
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int j = 0; j < 4; j++) { sa[i][j] = 0.f; da[i][j] = 0.f; }
        if (!(CAUSAL && kb > qb)) {
            for (int d = 0; d < hd; d += 4) {
                float4 q[4], o[4], k[4], v[4];
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    q[i] = *reinterpret_cast<const float4*>(Qs + (i0 + i) * hdp + d);
                    o[i] = *reinterpret_cast<const float4*>(Os + (i0 + i) * hdp + d);
                    k[i] = *reinterpret_cast<const float4*>(Ks + (j0 + i) * hdp + d);
                    v[i] = *reinterpret_cast<const float4*>(Vs + (j0 + i) * hdp + d);
                }
#pragma unroll
                for (int i = 0; i < 4; i++)
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        sa[i][j] += q[i].x * k[j].x + q[i].y * k[j].y + q[i].z * k[j].z + q[i].w * k[j].w;
                        da[i][j] += o[i].x * v[j].x + o[i].y * v[j].y + o[i].z * v[j].z + o[i].w * v[j].w;
                    }
            }
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int qi = i0 + i;
            const float l = qi < S ? lrow[qi] : 0.f;
            float pr[4], dp[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int kj = j0 + j;
                const bool live = qi < S && kj < S && !(CAUSAL && kj > qi);
                pr[j] = live ? __expf(sa[i][j] * scale - l) : 0.f;
                dp[j] = live ? (DROP ? da[i][j] * drop_mul(drop, attn_drop_idx(b, H, h, S, qi, kj)) : da[i][j]) : 0.f;
            }
            *reinterpret_cast<float4*>(Ps + qi * Sp + j0) = make_float4(pr[0], pr[1], pr[2], pr[3]);
            *reinterpret_cast<float4*>(Ds + qi * Sp + j0) = make_float4(dp[0], dp[1], dp[2], dp[3]);
        }
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i = wave; i < S; i += 4) {                    // delta_i = sum_j P dP;  dS = P (dP - delta) scale
        float dl = 0.f;
        for (int j = lane; j < S4; j += 64) dl += Ps[i * Sp + j] * Ds[i * Sp + j];
        dl = wave_sum(dl);
        for (int j = lane; j < S4; j += 64) Ds[i * Sp + j] = Ps[i * Sp + j] * (Ds[i * Sp + j] - dl) * scale;
    }
    __syncthreads();
    // ---- dQ = dS K, dK = dS^T Q, dV = (P mask)^T dO: thread = (4 rows, 4 columns) of all three (dQ's work grows with the row block,
    //      dK / dV's shrinks: balanced under the causal mask)
    const int d4n = hd >> 2;
    for (int idx = threadIdx.x; idx < NB * d4n; idx += 256) {
        const int rb = idx / d4n, d0 = (idx - rb * d4n) * 4, r0 = rb * 4;
        float4 dq[4], dk[4], dv[4];
#pragma unroll
        for (int i = 0; i < 4; i++) { dq[i] = make_float4(0, 0, 0, 0); dk[i] = dq[i]; dv[i] = dq[i]; }
        const int jhi = CAUSAL ? r0 + 4 : S4;              // dQ rows r0..r0+3: keys j <= r (dS is zero above the diagonal and beyond S)
        for (int j = 0; j < jhi; j += 4) {
            float4 w[4], k[4];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                w[i] = *reinterpret_cast<const float4*>(Ds + (r0 + i) * Sp + j);
                k[i] = *reinterpret_cast<const float4*>(Ks + (j + i) * hdp + d0);
            }
#pragma unroll
            for (int i = 0; i < 4; i++) {
                dq[i].x += w[i].x * k[0].x + w[i].y * k[1].x + w[i].z * k[2].x + w[i].w * k[3].x;
                dq[i].y += w[i].x * k[0].y + w[i].y * k[1].y + w[i].z * k[2].y + w[i].w * k[3].y;
                dq[i].z += w[i].x * k[0].z + w[i].y * k[1].z + w[i].z * k[2].z + w[i].w * k[3].z;
                dq[i].w += w[i].x * k[0].w + w[i].y * k[1].w + w[i].z * k[2].w + w[i].w * k[3].w;
            }
        }
        const int ilo = CAUSAL ? r0 : 0;                   // dK / dV rows (keys) r0..r0+3: queries i >= r
        for (int i = ilo; i < S4; i++) {
            const float4 w = *reinterpret_cast<const float4*>(Ds + i * Sp + r0);
            float4 pm = *reinterpret_cast<const float4*>(Ps + i * Sp + r0);
            if (DROP) {
                const unsigned e0 = attn_drop_idx(b, H, h, S, i, r0);
                pm.x *= drop_mul(drop, e0); pm.y *= drop_mul(drop, e0 + 1); pm.z *= drop_mul(drop, e0 + 2); pm.w *= drop_mul(drop, e0 + 3);
            }
            const float4 q = *reinterpret_cast<const float4*>(Qs + i * hdp + d0), o = *reinterpret_cast<const float4*>(Os + i * hdp + d0);
            dk[0].x += w.x * q.x; dk[0].y += w.x * q.y; dk[0].z += w.x * q.z; dk[0].w += w.x * q.w;
            dk[1].x += w.y * q.x; dk[1].y += w.y * q.y; dk[1].z += w.y * q.z; dk[1].w += w.y * q.w;
            dk[2].x += w.z * q.x; dk[2].y += w.z * q.y; dk[2].z += w.z * q.z; dk[2].w += w.z * q.w;
            dk[3].x += w.w * q.x; dk[3].y += w.w * q.y; dk[3].z += w.w * q.z; dk[3].w += w.w * q.w;
            dv[0].x += pm.x * o.x; dv[0].y += pm.x * o.y; dv[0].z += pm.x * o.z; dv[0].w += pm.x * o.w;
            dv[1].x += pm.y * o.x; dv[1].y += pm.y * o.y; dv[1].z += pm.y * o.z; dv[1].w += pm.y * o.w;
            dv[2].x += pm.z * o.x; dv[2].y += pm.z * o.y; dv[2].z += pm.z * o.z; dv[2].w += pm.z * o.w;
            dv[3].x += pm.w * o.x; dv[3].y += pm.w * o.y; dv[3].z += pm.w * o.z; dv[3].w += pm.w * o.w;
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int r = r0 + i;
            if (r >= S) break;
#if CC_OP == 2
            if (img) {
                op16_t* r3 = reinterpret_cast<op16_t*>(dqkv) + ((size_t)b * S + r) * 9 * D + h * hd + d0;
                const float4 gq[3] = {dq[i], dk[i], dv[i]};
#pragma unroll
                for (int t = 0; t < 3; t++) {
                    const unsigned h01 = pack2op(gq[t].x, gq[t].y), h23 = pack2op(gq[t].z, gq[t].w);
                    float a0, a1, a2, a3;
                    unpack2(h01, a0, a1);
                    unpack2(h23, a2, a3);
                    const uint2 hi = make_uint2(h01, h23), lo = make_uint2(pack2op(gq[t].x - a0, gq[t].y - a1), pack2op(gq[t].z - a2, gq[t].w - a3));
                    *reinterpret_cast<uint2*>(r3 + t * D) = hi;
                    *reinterpret_cast<uint2*>(r3 + 3 * D + t * D) = hi;
                    *reinterpret_cast<uint2*>(r3 + 6 * D + t * D) = lo;
                }
                continue;
            }
#endif
            act_t* o = dqkv + ((size_t)b * S + r) * 3 * D + h * hd + d0;
            act_st4(o, dq[i].x, dq[i].y, dq[i].z, dq[i].w);
            act_st4(o + D, dk[i].x, dk[i].y, dk[i].z, dk[i].w);
            act_st4(o + 2 * D, dv[i].x, dv[i].y, dv[i].z, dv[i].w);
        }
    }
}
// Short sequences (S < 32: the mapper's 20 rows): the first form — a thread = 4 queries x 1 key, then 1 row x 4 columns.  The 4 x 4 blocks
// above leave 25 of 256 threads busy there (measured 47 -> 55 us per mapper layer).
template <bool CAUSAL, bool DROP = false>
__global__ __launch_bounds__(256) void k_attn_bwd_small(const act_t* __restrict__ qkv, const act_t* __restrict__ dout,
                                                  const float* __restrict__ lse, int S, int H, int hd, float scale,
                                                  act_t* __restrict__ dqkv, Drop drop = Drop(), int img = 0) {
    // img (bf16x3 build): dqkv receives the [hi | hi | lo] operand image (rows of 3 * 3D 16-bit elements) of c_attn's input-gradient GEMM
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int D = H * hd, hdp = hd + 4, Sp = S + 1;
    float* Qs = sm;
    float* Ks = Qs + S * hdp;
    float* Vs = Ks + S * hdp;
    float* Os = Vs + S * hdp;  // dO
    float* Ps = Os + S * hdp;
    float* Ds = Ps + S * Sp;   // dP then dS
    const int b = blockIdx.x / H, h = blockIdx.x % H;
    const act_t* base = qkv + (size_t)b * S * 3 * D + h * hd;
    load_head_rows(Qs, hdp, base, 3 * D, S, hd);
    load_head_rows(Ks, hdp, base + D, 3 * D, S, hd);
    load_head_rows(Vs, hdp, base + 2 * D, 3 * D, S, hd);
    load_head_rows(Os, hdp, dout + (size_t)b * S * D + h * hd, D, S, hd);
    __syncthreads();
    const float* lrow = lse + ((size_t)b * H + h) * S;
    const int nib = (S + 3) >> 2;
    for (int idx = threadIdx.x; idx < nib * S; idx += 256) {
        const int ib = idx / S, j = idx % S, i0 = ib * 4;
        if (CAUSAL && j > i0 + 3) {
#pragma unroll
            for (int ii = 0; ii < 4; ii++)
                if (i0 + ii < S) { Ps[(i0 + ii) * Sp + j] = 0.f; Ds[(i0 + ii) * Sp + j] = 0.f; }
            continue;
        }
        float s[4] = {0, 0, 0, 0}, dp[4] = {0, 0, 0, 0};
        const float* kr = Ks + j * hdp;
        const float* vr = Vs + j * hdp;
        for (int d = 0; d < hd; d += 4) {
            const float4 k = *reinterpret_cast<const float4*>(kr + d), v = *reinterpret_cast<const float4*>(vr + d);
#pragma unroll
            for (int ii = 0; ii < 4; ii++) {
                const int i = min(i0 + ii, S - 1);
                const float4 q = *reinterpret_cast<const float4*>(Qs + i * hdp + d);
                const float4 o = *reinterpret_cast<const float4*>(Os + i * hdp + d);
                s[ii] += q.x * k.x + q.y * k.y + q.z * k.z + q.w * k.w;
                dp[ii] += o.x * v.x + o.y * v.y + o.z * v.z + o.w * v.w;
            }
        }
#pragma unroll
        for (int ii = 0; ii < 4; ii++) {
            const int i = i0 + ii;
            if (i < S) {
                const bool masked = CAUSAL && j > i;
                Ps[i * Sp + j] = masked ? 0.f : __expf(s[ii] * scale - lrow[i]);
                Ds[i * Sp + j] = masked ? 0.f : (DROP ? dp[ii] * drop_mul(drop, attn_drop_idx(b, H, h, S, i, j)) : dp[ii]);
            }
        }
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i = wave; i < S; i += 4) {
        float dl = 0.f;
        for (int j = lane; j < S; j += 64) dl += Ps[i * Sp + j] * Ds[i * Sp + j];
        dl = wave_sum(dl);
        for (int j = lane; j < S; j += 64) Ds[i * Sp + j] = Ps[i * Sp + j] * (Ds[i * Sp + j] - dl) * scale;
    }
    __syncthreads();
    const int d4n = hd >> 2;
    for (int idx = threadIdx.x; idx < S * d4n; idx += 256) {
        const int r = idx / d4n, d0 = (idx % d4n) * 4;
        float4 dq = make_float4(0, 0, 0, 0), dk = dq, dv = dq;
        const int jhi = CAUSAL ? r + 1 : S;   // dQ_r: keys j <= r
        for (int j = 0; j < jhi; j++) {
            const float w = Ds[r * Sp + j];
            const float4 k = *reinterpret_cast<const float4*>(Ks + j * hdp + d0);
            dq.x += w * k.x; dq.y += w * k.y; dq.z += w * k.z; dq.w += w * k.w;
        }
        const int ilo = CAUSAL ? r : 0;       // dK_r, dV_r: queries i >= r
        for (int i = ilo; i < S; i++) {
            const float w = Ds[i * Sp + r];
            float p = Ps[i * Sp + r];
            if (DROP) p *= drop_mul(drop, attn_drop_idx(b, H, h, S, i, r));
            const float4 q = *reinterpret_cast<const float4*>(Qs + i * hdp + d0);
            const float4 o = *reinterpret_cast<const float4*>(Os + i * hdp + d0);
            dk.x += w * q.x; dk.y += w * q.y; dk.z += w * q.z; dk.w += w * q.w;
            dv.x += p * o.x; dv.y += p * o.y; dv.z += p * o.z; dv.w += p * o.w;
        }
#if CC_OP == 2
        if (img) {
            op16_t* r3 = reinterpret_cast<op16_t*>(dqkv) + ((size_t)b * S + r) * 9 * D + h * hd + d0;
            const float4 gq[3] = {dq, dk, dv};
#pragma unroll
            for (int t = 0; t < 3; t++) {
                const unsigned h01 = pack2op(gq[t].x, gq[t].y), h23 = pack2op(gq[t].z, gq[t].w);
                float a0, a1, a2, a3;
                unpack2(h01, a0, a1);
                unpack2(h23, a2, a3);
                const uint2 hi = make_uint2(h01, h23), lo = make_uint2(pack2op(gq[t].x - a0, gq[t].y - a1), pack2op(gq[t].z - a2, gq[t].w - a3));
                *reinterpret_cast<uint2*>(r3 + t * D) = hi;
                *reinterpret_cast<uint2*>(r3 + 3 * D + t * D) = hi;
                *reinterpret_cast<uint2*>(r3 + 6 * D + t * D) = lo;
            }
            continue;
        }
#endif
        act_t* o = dqkv + ((size_t)b * S + r) * 3 * D + h * hd + d0;
        act_st4(o, dq.x, dq.y, dq.z, dq.w);
        act_st4(o + D, dk.x, dk.y, dk.z, dk.w);
        act_st4(o + 2 * D, dv.x, dv.y, dv.z, dv.w);
    }
}
// bf16x3: whether attn_fwd can write `out` as an operand image — the LDS-tile VALU kernels must serve BOTH directions for this shape
// (the backward of the other attention forms reads the fp32 output again)
bool attn_fwd_can_image(int S, int hd) {
#if CC_OP == 2
    const bool fwd_ok = (attn_x3mfma_on() && (hd == 64 || hd == 96 || hd == 128)) || (!attn_f32mfma_ok(S, hd, false) && attn_fwd_lds(S, hd) <= 160 * 1024);
    return (hd & 7) == 0 && S > 0 && fwd_ok && (attn_bwd_m3_ok(S, hd) || (!attn_f32mfma_ok(S, hd, true) && attn_bwd_lds(S, hd) <= 160 * 1024));
#else
    (void)S; (void)hd;
    return false;
#endif
}
// bf16x3: whether attn_bwd can write dqkv as an operand image for this shape (only the LDS-tile VALU kernel writes images)
bool attn_bwd_can_image(int S, int hd) {
#if CC_OP == 2
    return (hd & 7) == 0 && S > 0 && (attn_bwd_m3_ok(S, hd) || (!attn_f32mfma_ok(S, hd, true) && attn_bwd_lds(S, hd) <= 160 * 1024));
#else
    (void)S; (void)hd;
    return false;
#endif
}
int attn_bwd(const act_t* qkv, const act_t* dout, const act_t* o, const float* lse, float* delta, int B, int S, int H, int hd, bool causal,
             Act dqkvo, hipStream_t st, Drop drop) {
    if ((hd & 7) || S <= 0) return CC_ERR_SHAPE;
    act_t* const dqkv = dqkvo.p;
    const int img = dqkvo.img ? 1 : 0;
    if (img && (dqkvo.img != 3 * H * hd || !attn_bwd_can_image(S, hd))) return CC_ERR_STATE;
#if CC_OP != 2
    static const bool no_mfma = cc_lab_env("CC_ATTN_VALU") != nullptr;
    if ((!no_mfma || drop.thresh) && o && delta) {
        if (hd == 64) return attn_bwd_mfma_launch<64>(qkv, dout, o, lse, delta, B, S, H, causal, dqkv, st, drop);
        if (hd == 96) return attn_bwd_mfma_launch<96>(qkv, dout, o, lse, delta, B, S, H, causal, dqkv, st, drop);
        if (hd == 128) return attn_bwd_mfma_launch<128>(qkv, dout, o, lse, delta, B, S, H, causal, dqkv, st, drop);
    }
#endif
    if (drop.thresh && (!kX3 || !causal)) return CC_ERR_SHAPE;          // dropout on the VALU kernel: the bf16x3 build's GPT-2 path only
    const float scale = 1.0f / sqrtf((float)hd);
#if CC_OP == 2
    if (attn_bwd_m3_ok(S, hd)) {                                         // three bf16 MFMA terms per product
        if (hd == 64) return S <= 32 ? attn_bwd_m3_launch<64, 1>(qkv, dout, lse, B, S, H, causal, dqkv, st, drop, img)
                                     : attn_bwd_m3_launch<64, 2>(qkv, dout, lse, B, S, H, causal, dqkv, st, drop, img);
        return S <= 32 ? attn_bwd_m3_launch<96, 1>(qkv, dout, lse, B, S, H, causal, dqkv, st, drop, img)
                       : attn_bwd_m3_launch<96, 2>(qkv, dout, lse, B, S, H, causal, dqkv, st, drop, img);
    }
#ifdef CC_EXPERIMENTS
    if (attn_f32mfma_ok(S, hd, true)) {
        const size_t sh = attn_f32mfma_lds(S, hd, true);
#define CC_L(C, DR) attn_launch<k_attn_bwd_f32mfma<C, DR>>(dim3(B * H), dim3(256), sh, st, qkv, dout, lse, S, H, hd, scale, dqkv, drop)
        ATTN_LADDER(CC_L)
#undef CC_L
        return hipGetLastError() == hipSuccess ? CC_OK : CC_ERR_LAUNCH;
    }
#endif
#endif
    const size_t sh = attn_bwd_lds(S, hd);
    if (sh > 160 * 1024) {
#if CC_OP == 2
        if (drop.thresh || !o || !delta) return CC_ERR_SHAPE;
        return attn_bwd_rows(qkv, dout, o, lse, delta, B, S, H, hd, causal, dqkv, scale, st);
#else
        return CC_ERR_SHAPE;
#endif
    }
#define CC_RAISE(C, DR) (void)hipFuncSetAttribute((const void*)k_attn_bwd_small<C, DR>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh)
#define CC_L(C, DR) hipLaunchKernelGGL((k_attn_bwd_small<C, DR>), dim3(B * H), dim3(256), sh, st, qkv, dout, lse, S, H, hd, scale, dqkv, DR ? drop : Drop(), img)
#define CC_B(C, DR) attn_launch<k_attn_bwd<C, DR>>(dim3(B * H), dim3(256), sh, st, qkv, dout, lse, S, H, hd, scale, dqkv, DR ? drop : Drop(), img)
    if (S < 32) {
        if (sh > 64 * 1024) { CC_RAISE(true, true); CC_RAISE(true, false); CC_RAISE(false, false); }      // all three instantiations, whichever is launched
        ATTN_LADDER(CC_L)
    } else ATTN_LADDER(CC_B)
#undef CC_B
#undef CC_L
#undef CC_RAISE
    return hipGetLastError() == hipSuccess ? CC_OK : CC_ERR_LAUNCH;
}

}  // namespace CC_NS
