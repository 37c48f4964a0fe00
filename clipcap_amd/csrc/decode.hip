// KV-cached caption decode for gfx950: replaces the reference's full GPT-2 re-forward per generated token
// (clipcap/inference/base.py:81) with an O(ctx) step, plus the bookkeeping between two beam steps (k_beam_advance; the beam update
// itself is beam.hip).
// Decode is HBM-bound (every weight byte is read once per step); the GEMMs reuse gemm.hip.h, attention over the
// cache is one wave per (row, head, new position).
#include "../../include/clipcap_hip.h"
#ifdef CC_EXPERIMENTS
#include "../../include/clipcap_hip_lab.h"
#endif
#include "gemm_api.h"
#include "kernels.h"
#include "decode_pk.h"
#include "decode_xt.h"
#include "layout.h"

using namespace CC_NS;

#ifndef CC_DEC_SCU
#define CC_DEC_SCU 4   // K rows (score phase) / V rows (PV phase) a lane keeps in flight in k_decode_attn
#endif
#ifndef CC_DEC_PVU
#define CC_DEC_PVU 4
#endif

namespace {

// x[r,t,:] += wpe[pos0+t,:]
__global__ void k_add_wpe(const float* __restrict__ xin, const float* __restrict__ wpe, float* __restrict__ x, int R, int Tn, int D, int pos0) {
    const int d4n = D >> 2;
    const size_t total = (size_t)R * Tn * d4n;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % d4n), t = (int)((i / d4n) % Tn);
        const float4 a = reinterpret_cast<const float4*>(xin)[i];
        const float4 p = reinterpret_cast<const float4*>(wpe + (size_t)(pos0 + t) * D)[c];
        reinterpret_cast<float4*>(x)[i] = make_float4(a.x + p.x, a.y + p.y, a.z + p.z, a.w + p.w);
    }
}

// x[r,:] = xin[r,:] + wpe[pos,:] and xn = LayerNorm(x) (layer 0's ln_1) in one launch: the single-position decode step (one wave per row)
__global__ __launch_bounds__(256) void k_add_wpe_ln(const float* __restrict__ xin, const float* __restrict__ wpe, float* __restrict__ x,
                                                    const float* __restrict__ gamma, const float* __restrict__ beta, act_t* __restrict__ xn,
                                                    int R, int D, int pos) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= R) return;
    constexpr int MAXV = 8;                      // D <= 2048
    float4 v[MAXV];
    float s = 0.f;
#pragma unroll
    for (int it = 0; it < MAXV; it++) {
        const int c = lane * 4 + it * 256;
        if (c < D) {
            const float4 a = *reinterpret_cast<const float4*>(xin + (size_t)row * D + c);
            const float4 p = *reinterpret_cast<const float4*>(wpe + (size_t)pos * D + c);
            v[it] = make_float4(a.x + p.x, a.y + p.y, a.z + p.z, a.w + p.w);
            *reinterpret_cast<float4*>(x + (size_t)row * D + c) = v[it];
            s += v[it].x + v[it].y + v[it].z + v[it].w;
        }
    }
    const float mu = wave_sum(s) / D;
    float q = 0.f;
#pragma unroll
    for (int it = 0; it < MAXV; it++) {
        const int c = lane * 4 + it * 256;
        if (c < D) { const float a = v[it].x - mu, b = v[it].y - mu, c2 = v[it].z - mu, d = v[it].w - mu; q += a * a + b * b + c2 * c2 + d * d; }
    }
    const float rs = rsqrtf(wave_sum(q) / D + 1e-5f);
#pragma unroll
    for (int it = 0; it < MAXV; it++) {
        const int c = lane * 4 + it * 256;
        if (c < D) {
            const float4 g = *reinterpret_cast<const float4*>(gamma + c), b = *reinterpret_cast<const float4*>(beta + c);
            act_st4(xn + (size_t)row * D + c, (v[it].x - mu) * rs * g.x + b.x, (v[it].y - mu) * rs * g.y + b.y, (v[it].z - mu) * rs * g.z + b.z,
                    (v[it].w - mu) * rs * g.w + b.w);
        }
    }
}

// attention of the Tn new queries of every row against the cache (ctx = pos0 + Tn, causal): one wave per (r,h,t).
// scores: one key per lane (K row = hd contiguous bf16, 16-B loads).  PV: lane = (key group kg, 8-wide d chunk dc): every V load
// is a 16-B vector, the key loop is 64/(hd/8) times shorter than one-d-per-lane, partial sums meet in wave-private LDS.
// APPEND: the wave also writes its own (row, head, new position) K / V slice into the cache (instead of a separate append launch)
// and reads the keys / values of the NEW positions straight from qkv — other waves' cache writes are not ordered with its reads.
template <bool APPEND>
__global__ __launch_bounds__(256) void k_decode_attn(const act_t* __restrict__ qkv, act_t* __restrict__ kc,
                                                     act_t* __restrict__ vc, const int* __restrict__ row_map, act_t* __restrict__ out,
                                                     int R, int Tn, int H, int hd, int pos0, int ctx_max, float scale) {
    extern __shared__ float psm[];  // per wave: p[ctx_max] | srow[ctx_max] | red[8][hd]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int gid = blockIdx.x * 4 + wave;
    if (gid >= R * H * Tn) return;
    const int t = gid % Tn, h = (gid / Tn) % H, r = gid / (Tn * H);
    const int D = H * hd, nkeys = pos0 + t + 1;
    const int per_wave = 2 * ctx_max + 8 * hd;
    float* p = psm + wave * per_wave;
    int* srow = reinterpret_cast<int*>(p + ctx_max);
    float* red = p + 2 * ctx_max;
    const act_t* q = qkv + ((size_t)r * Tn + t) * 3 * D + h * hd;
    // position j of row r lives in cache row row_map[r*ctx_max + j] (beam ancestry table; identity when null)
    const act_t* kb = kc + h * hd;
    const act_t* vb = vc + h * hd;
    if (APPEND) {
        const int c8 = hd >> 3;                            // 16-B chunks per head slice
        if (lane < 2 * c8) {
            const int which = lane / c8, c = lane - which * c8;
            const act_raw8 v = act_ldraw8(q + (which + 1) * D + c * 8);
            act_t* dst = (which ? vc : kc) + ((size_t)r * ctx_max + pos0 + t) * D + h * hd + c * 8;
            act_straw8(dst, v);
        }
    }
    const act_t* knew = qkv + (size_t)r * Tn * 3 * D + D + h * hd;        // K of new position u: knew + u * 3D  (V: + D)
    for (int j = lane; j < nkeys; j += 64) srow[j] = row_map ? row_map[(size_t)r * ctx_max + j] : r;
    float m = -INFINITY;
    const int nchunk = hd >> 3;
    if ((nchunk & (nchunk - 1)) == 0 && nchunk <= 16) {
        // lane = (key group, 16-B chunk of the head slice): one load instruction covers 64 / nchunk whole K rows (full 128-B lines for
        // hd = 64) instead of 16 B of 64 different rows, SC_U of them in flight; the chunk dot products meet by xor-shuffles
        constexpr int SC_U = CC_DEC_SCU;
        const int kgs = 64 / nchunk, skg = lane / nchunk, sdc = lane - skg * nchunk;
        float qf[8];
        act_ld8(q + sdc * 8, qf);
        for (int j0 = 0; j0 < nkeys; j0 += kgs * SC_U) {
            act_raw8 kv[SC_U];
#pragma unroll
            for (int u = 0; u < SC_U; u++) {
                const int j = min(j0 + u * kgs + skg, nkeys - 1);
                const act_t* krow = (APPEND && j >= pos0) ? knew + (size_t)(j - pos0) * 3 * D : kb + ((size_t)srow[j] * ctx_max + j) * D;
                kv[u] = act_ldraw8(krow + sdc * 8);
            }
#pragma unroll
            for (int u = 0; u < SC_U; u++) {
                float b[8], sc = 0.f;
                act_unpack8(kv[u], b);
#pragma unroll
                for (int e = 0; e < 8; e++) sc += qf[e] * b[e];
                for (int o = 1; o < nchunk; o <<= 1) sc += __shfl_xor(sc, o);
                sc *= scale;
                const int j = j0 + u * kgs + skg;
                if (j < nkeys) {
                    if (sdc == 0) p[j] = sc;
                    m = fmaxf(m, sc);
                }
            }
        }
    } else {
        for (int j = lane; j < nkeys; j += 64) {
            float s = 0.f;
            const act_t* krow = (APPEND && j >= pos0) ? knew + (size_t)(j - pos0) * 3 * D : kb + ((size_t)srow[j] * ctx_max + j) * D;
            for (int d = 0; d < hd; d += 8) {
                float a[8], b[8];
                act_ld8(q + d, a);
                act_ld8(krow + d, b);
#pragma unroll
                for (int e = 0; e < 8; e++) s += a[e] * b[e];
            }
            s *= scale;
            p[j] = s;
            m = fmaxf(m, s);
        }
    }
    m = wave_max(m);
    float sum = 0.f;
    for (int j = lane; j < nkeys; j += 64) {
        const float e = __expf(p[j] - m);
        p[j] = e;
        sum += e;
    }
    sum = wave_sum(sum);
    const float inv = 1.f / sum;
    // wave-private LDS: same-wave writes above are visible to the reads below (in-order DS queue)
    const int kgroups = min(8, 64 / nchunk);
    const int kg = lane / nchunk, dc = lane - kg * nchunk;
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (kg < kgroups) {
        constexpr int PV_U = CC_DEC_PVU;                       // V rows in flight per lane
        for (int j0 = kg; j0 < nkeys; j0 += kgroups * PV_U) {
            act_raw8 vv[PV_U];
            float pj[PV_U];
#pragma unroll
            for (int u = 0; u < PV_U; u++) {
                const int j = min(j0 + u * kgroups, nkeys - 1);
                const act_t* vrow = (APPEND && j >= pos0) ? knew + D + (size_t)(j - pos0) * 3 * D : vb + ((size_t)srow[j] * ctx_max + j) * D;
                vv[u] = act_ldraw8(vrow + dc * 8);
                pj[u] = j0 + u * kgroups < nkeys ? p[j] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < PV_U; u++) {
                float v[8];
                act_unpack8(vv[u], v);
#pragma unroll
                for (int e = 0; e < 8; e++) acc[e] += pj[u] * v[e];
            }
        }
#pragma unroll
        for (int e = 0; e < 8; e++) red[kg * hd + dc * 8 + e] = acc[e];
    }
    for (int d = lane; d < hd; d += 64) {
        float o = 0.f;
        for (int g = 0; g < kgroups; g++) o += red[g * hd + d];
        out[((size_t)r * Tn + t) * D + h * hd + d] = f2act(o * inv);
    }
}

// Beam-group form of the single-position attention step (Tn == 1, head dim 64 = every GPT-2 size).  The G beams of a caption share
// their prefix rows and most of their ancestors (tools/decode_union_stats.py: 56 distinct rows against 217 read per group on the
// configs[4] decode), so
//   k_group_union   (once per position, one wave per group) builds the UNION of the (cache row, position) pairs the group's ancestry
//                   tables name: ent = {cache row * ctx_max + position, bit b set when beam b's table names that row}; the G new keys
//                   (one per beam) are the last G entries;
//   k_decode_attn_group (per layer, one 4-wave block per (group, head)) loads every distinct K / V row ONCE and scores it against all G
//                   queries; a beam's softmax runs over the entries whose bit it owns (the others hold -inf), i.e. exactly the keys
//                   k_decode_attn reads for it.  A wave owns 32 entries per pass (128 per block: one pass for the usual union): K as
//                   (key group, 16-B chunk) lanes like k_decode_attn, V one element per lane (a wave instruction = one 128-B row) with
//                   scalar entry loads, and ALL of a pass's K and V loads are in flight together — the chain is list -> rows -> done.
// Any row_map is handled exactly (rows that share nothing give G entries per position); sharing only decides how many rows are read.
// LDS per block: p[cap][8] | wmx[4][8] | wsum[8][8] | red2[8][G][64].
template <int G>
__global__ __launch_bounds__(64) void k_group_union(const int* __restrict__ row_map, int2* __restrict__ ent_g, int* __restrict__ cnt_g, int pos0,
                                                    int ctx_max, int cap, int append, unsigned* __restrict__ zero, int nzero) {
    const int lane = threadIdx.x, s = blockIdx.x, r0 = s * G;
    if (s == 0)                                            // the persistent layer launch that follows starts from cleared arrival counters
        for (int i = lane; i < nzero; i += 64) zero[i] = 0u;
    int2* ent = ent_g + (size_t)s * cap;
    int nU = 0;
    for (int j0 = 0; j0 < pos0; j0 += 64) {
        const int j = j0 + lane;
        const bool valid = j < pos0;
        int m[G];
#pragma unroll
        for (int b = 0; b < G; b++) m[b] = valid ? (row_map ? row_map[(size_t)(r0 + b) * ctx_max + j] : r0 + b) : -1 - b;
        unsigned lead = 0, mk[G];
#pragma unroll
        for (int b = 0; b < G; b++) {
            unsigned k = 0;
            bool l = valid;
#pragma unroll
            for (int b2 = 0; b2 < G; b2++)
                if (m[b2] == m[b]) { k |= 1u << b2; if (b2 < b) l = false; }
            mk[b] = k;
            if (l) lead |= 1u << b;
        }
        const int cnt = __popc(lead);
        int incl = cnt;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(incl, o); if (lane >= o) incl += t; }
        int idx = nU + incl - cnt;
#pragma unroll
        for (int b = 0; b < G; b++)
            if ((lead >> b) & 1) { ent[idx] = make_int2(m[b] * ctx_max + j, (int)mk[b]); idx++; }
        nU += __shfl(incl, 63);
    }
    // the new position: one private key per beam; append: still in qkv (the attention kernel is the one that stores it), marked -1 - b
    if (lane < G) ent[nU + lane] = make_int2(append ? -1 - lane : (r0 + lane) * ctx_max + pos0, 1 << lane);
    nU += G;
    // pad to whole passes of 128 with entries nobody owns (mask 0 -> score -inf -> weight 0) that name a readable row
    const int dummy = append ? -1 : r0 * ctx_max + pos0;
    for (int u = nU + lane; u < ((nU + 127) & ~127); u += 64) ent[u] = make_int2(dummy, 0);
    if (lane == 0) cnt_g[s] = nU;
}

// two consecutive stored elements as one load (k_decode_attn_group's V lanes: 32 lanes x 2 elements = one 64-wide head row)
#if CC_OP == 2
typedef float act_v2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void act_v2f(const act_v2& v, float& a, float& b) { a = v.x; b = v.y; }
#else
typedef unsigned act_v2;
__device__ __forceinline__ void act_v2f(const act_v2& v, float& a, float& b) { unpack2(v, a, b); }
#endif
typedef const __attribute__((address_space(1))) act_v2* g_v2p;

template <int G>
__global__ __launch_bounds__(256, kX3 ? 3 : 4) void k_decode_attn_group(const act_t* __restrict__ qkv, act_t* __restrict__ kc, act_t* __restrict__ vc,
                                                           const int2* __restrict__ ent_g, const int* __restrict__ cnt_g, act_t* __restrict__ out,
                                                           int H, int pos0, int ctx_max, float scale, int cap, int append) {
    constexpr int HD = 64, KPW = 32;                       // head dim; entries per wave and pass
    extern __shared__ __attribute__((aligned(16))) float gsm[];
    float* p = gsm;                                        // p[u * 8 + b], u < cap (a multiple of 128)
    float* wmx = p + (size_t)cap * 8;                      // [4][8]
    float* wsm = wmx + 32;                                 // [8][8]  (wave, half)
    float* red2 = wsm + 64;                                // [8][G][64]
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int s = blockIdx.x / H, h = blockIdx.x - s * H, r0 = s * G;
    const int D = H * HD;
    const int2* __restrict__ ent = ent_g + (size_t)s * cap;
    const act_t* kb = kc + h * HD;
    const act_t* vb = vc + h * HD;
    const act_t* qrow = qkv + (size_t)r0 * 3 * D + h * HD;          // row r0 + b: + b * 3D;  K: + D, V: + 2D
    const int skg = lane >> 3, sdc = lane & 7;
    // pass 0 always exists: its entries, then all of its K and V rows, are requested before anything is waited for
    int2 ek[4];
#pragma unroll
    for (int i = 0; i < 4; i++) ek[i] = ent[w * KPW + i * 8 + skg];
    int2 ev = ent[w * KPW + (lane & 31)];
    const int nU = cnt_g[s];
    if (append && tid < G * 16) {
        const int b = tid >> 4, wq = tid & 15, which = wq >> 3, c = wq & 7;
        const act_raw8 v = act_ldraw8(qrow + (size_t)b * 3 * D + (which + 1) * D + c * 8);
        act_straw8((which ? vc : kc) + ((size_t)(r0 + b) * ctx_max + pos0) * D + h * HD + c * 8, v);
    }
    float qf[G][8], mx[G];
#pragma unroll
    for (int b = 0; b < G; b++) { act_ld8(qrow + (size_t)b * 3 * D + sdc * 8, qf[b]); mx[b] = -INFINITY; }
    const int npass = (nU + 4 * KPW - 1) / (4 * KPW);
    // V lanes: (half = lane >> 5, element pair = lane & 31): one load instruction fetches the rows of two entries (2 x 128 B)
    const int hf = lane >> 5, dp = lane & 31;
#define CC_GRP_VLOAD()                                                                                                                        \
    {                                                                                                                                         \
        const act_t* vrow = ev.x < 0 ? qrow + (size_t)(-1 - ev.x) * 3 * D + 2 * D : vb + (size_t)ev.x * D;                                    \
        const unsigned long long va = reinterpret_cast<unsigned long long>(vrow);                                                             \
        const int valo = (int)(unsigned)va, vahi = (int)(unsigned)(va >> 32);                                                                 \
        _Pragma("unroll") for (int k = 0; k < KPW / 2; k++) {                                                                                 \
            const unsigned lo0 = __builtin_amdgcn_readlane(valo, 2 * k), hi0 = __builtin_amdgcn_readlane(vahi, 2 * k);                        \
            const unsigned lo1 = __builtin_amdgcn_readlane(valo, 2 * k + 1), hi1 = __builtin_amdgcn_readlane(vahi, 2 * k + 1);                \
            const unsigned long long a = ((unsigned long long)(hf ? hi1 : hi0) << 32) | (hf ? lo1 : lo0);                                     \
            vreg[k] = reinterpret_cast<g_v2p>(a)[dp];                                                                                         \
        }                                                                                                                                     \
    }
#define CC_GRP_PV()                                                                                                                           \
    _Pragma("unroll") for (int k = 0; k < KPW / 2; k++) {                                                                                     \
        float v0, v1;                                                                                                                         \
        act_v2f(vreg[k], v0, v1);                                                                                                             \
        const float* pu = p + (size_t)(ub + 2 * k + hf) * 8;                                                                                  \
        const float4 pa = *reinterpret_cast<const float4*>(pu), pb = *reinterpret_cast<const float4*>(pu + 4);                                \
        const float pj[8] = {pa.x, pa.y, pa.z, pa.w, pb.x, pb.y, pb.z, pb.w};                                                                 \
        _Pragma("unroll") for (int b = 0; b < G; b++) { acc[b][0] += pj[b] * v0; acc[b][1] += pj[b] * v1; lsum[b] += pj[b]; }                 \
    }
    act_v2 vreg[KPW / 2];                                  // pass 0's V rows
    for (int pass = 0; pass < npass; pass++) {
        const int ub = pass * 4 * KPW + w * KPW;           // wave-uniform
        if (pass > 0) {
#pragma unroll
            for (int i = 0; i < 4; i++) ek[i] = ent[ub + i * 8 + skg];
        }
        act_raw8 kv[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const act_t* krow = ek[i].x < 0 ? qrow + (size_t)(-1 - ek[i].x) * 3 * D + D : kb + (size_t)ek[i].x * D;
            kv[i] = act_ldraw8(krow + sdc * 8);
        }
        if (pass == 0) CC_GRP_VLOAD()
#pragma unroll
        for (int i = 0; i < 4; i++) {
            float kf[8], sc[8];
            act_unpack8(kv[i], kf);
#pragma unroll
            for (int b = 0; b < G; b++) {
                float a = 0.f;
#pragma unroll
                for (int e = 0; e < 8; e++) a += qf[b][e] * kf[e];
                sc[b] = a;
            }
#pragma unroll
            for (int b = 0; b < G; b++) sc[b] = sum8(sc[b]);
#pragma unroll
            for (int b = 0; b < 8; b++) {
                sc[b] = (b < G && ((ek[i].y >> b) & 1)) ? sc[b] * scale : -INFINITY;
                if (b < G) mx[b] = fmaxf(mx[b], sc[b]);
            }
            if (sdc == 0) {
                float* pu = p + (size_t)(ub + i * 8 + skg) * 8;
                *reinterpret_cast<float4*>(pu) = make_float4(sc[0], sc[1], sc[2], sc[3]);
                *reinterpret_cast<float4*>(pu + 4) = make_float4(sc[4], sc[5], sc[6], sc[7]);
            }
        }
    }
#pragma unroll
    for (int b = 0; b < G; b++) mx[b] = wave_max(mx[b]);
    if (lane == 0) {
#pragma unroll
        for (int b = 0; b < G; b++) wmx[w * 8 + b] = mx[b];
    }
    __syncthreads();
#pragma unroll
    for (int b = 0; b < G; b++) mx[b] = fmaxf(fmaxf(wmx[b], wmx[8 + b]), fmaxf(wmx[16 + b], wmx[24 + b]));     // finite: every beam owns its new key
    // ---- exp of the wave's own entries (only this wave reads them again), then P V with two output elements per lane and half
    float acc[G][2], lsum[G];
#pragma unroll
    for (int b = 0; b < G; b++) { acc[b][0] = acc[b][1] = 0.f; lsum[b] = 0.f; }
    for (int pass = 0; pass < npass; pass++) {
        const int ub = pass * 4 * KPW + w * KPW;
#pragma unroll
        for (int jj = 0; jj < KPW * 8 / 64; jj++) {
            const int idx = jj * 64 + lane, b = idx & 7;
            if (b < G) {
                float m = mx[0];
#pragma unroll
                for (int b2 = 1; b2 < G; b2++) m = b == b2 ? mx[b2] : m;
                p[(size_t)ub * 8 + idx] = __expf(p[(size_t)ub * 8 + idx] - m);
            }
        }
        if (pass > 0) {
            ev = ent[ub + (lane & 31)];
            CC_GRP_VLOAD()
        }
        CC_GRP_PV()
    }
#undef CC_GRP_VLOAD
#undef CC_GRP_PV
#pragma unroll
    for (int b = 0; b < G; b++) *reinterpret_cast<float2*>(red2 + ((w * 2 + hf) * G + b) * HD + 2 * dp) = make_float2(acc[b][0], acc[b][1]);
    if (dp == 0) {
#pragma unroll
        for (int b = 0; b < G; b++) wsm[(w * 2 + hf) * 8 + b] = lsum[b];
    }
    __syncthreads();
    for (int o = tid; o < G * HD; o += 256) {
        const int b = o >> 6, d = o & 63;
        float sum = 0.f, v = 0.f;
#pragma unroll
        for (int x = 0; x < 8; x++) { sum += wsm[x * 8 + b]; v += red2[(x * G + b) * HD + d]; }
        out[(size_t)(r0 + b) * D + h * HD + d] = f2act(v / sum);
    }
}

__global__ void k_kv_reorder(const act_t* __restrict__ src, act_t* __restrict__ dst, const int* __restrict__ map, int R_src, int R_dst,
                             int ctx, int ctx_max, int D, int NL2) {
    const int d8n = D * (int)sizeof(act_t) / 16;      // 16-B vectors per cache row
    const size_t per_row = (size_t)ctx * d8n;
    const size_t total = (size_t)NL2 * R_dst * per_row;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t e = i % per_row;
        const int r = (int)((i / per_row) % R_dst), l = (int)(i / (per_row * R_dst));
        const int sr = map[r];
        const uint4* s = reinterpret_cast<const uint4*>(src + ((size_t)l * R_src + sr) * ctx_max * D);
        uint4* d = reinterpret_cast<uint4*>(dst + ((size_t)l * R_dst + r) * ctx_max * D);
        d[e] = s[e];
    }
}

__global__ void k_last_rows(int* __restrict__ map, int R, int Tn) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < R) map[i] = i * Tn + Tn - 1;
}

__global__ void k_embed_tokens(const float* __restrict__ wte, const int* __restrict__ tok, float* __restrict__ out, int R, int D, int rows) {
    const int d4n = D >> 2;
    const size_t total = (size_t)R * d4n;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % d4n), r = (int)(i / d4n);
        const int id = min(max(tok[r], 0), rows - 1);       // never reads outside wte (callers validate ids; an out-of-range id must not fault the device)
        reinterpret_cast<float4*>(out)[i] = reinterpret_cast<const float4*>(wte + (size_t)id * D)[c];
    }
}

// Gradient of the gather: dwte[tok[r], :] += dout[r, :] (fp32 atomics; rows that share an id accumulate in arrival order: the
// non-deterministic form, kept for cc_embed_tokens_bwd; cc_embed_tokens_bwd_ws runs kernels.h scatter_rows).  Ids clamped like the forward's.
__global__ void k_embed_tokens_bwd(const float* __restrict__ dout, const int* __restrict__ tok, float* __restrict__ dwte, int R, int D, int rows) {
    const size_t total = (size_t)R * D;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int d = (int)(i % D), r = (int)(i / D);
        const int id = min(max(tok[r], 0), rows - 1);
        __hip_atomic_fetch_add(dwte + (size_t)id * D + d, dout[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// Bookkeeping between two beam steps in ONE launch (base.py:104-117: tokens = cat(tokens[src], next), embed(next), cache
// ancestry): row r continues group row g = (r / beam) * beam + src[r].  Replaces ~10 small framework launches per generated token.
__global__ __launch_bounds__(256) void k_beam_advance(int beam, int D, const float* __restrict__ wte, const int* __restrict__ next_tok,
                                                      const int* __restrict__ src, int pos, int ctx_max, const int* __restrict__ map_in,
                                                      int* __restrict__ map_out, int step, int tok_ld, const int* __restrict__ tok_in,
                                                      int* __restrict__ tok_out, float* __restrict__ x_out) {
    const int r = blockIdx.x, tid = threadIdx.x;
    const int g = src ? (r / beam) * beam + src[r] : r;
    int id = next_tok[r];
    if (map_out)
        for (int j = tid; j < ctx_max; j += 256) map_out[(size_t)r * ctx_max + j] = j < pos ? map_in[(size_t)g * ctx_max + j] : r;
    if (tok_out) {
        for (int j = tid; j < step; j += 256) tok_out[(size_t)r * tok_ld + j] = tok_in[(size_t)g * tok_ld + j];
        if (tid == 0) tok_out[(size_t)r * tok_ld + step] = id;
    }
    if (id < 0) id = 0;
    const float4* w = reinterpret_cast<const float4*>(wte + (size_t)id * D);
    for (int c = tid; c < (D >> 2); c += 256) reinterpret_cast<float4*>(x_out + (size_t)r * D)[c] = w[c];
}

// cc_decode_hidden_unit: out[r * ld_row + t * ld_pos + :] = ln_f(x[r * Tn + t]) / |ln_f(x[r * Tn + t])|_2 — k_ln_fwd's arithmetic (one wave per
// row, the row in registers, 16-B loads and stores), then one more wave reduction for the norm.  A zero vector stays zero.
template <int NV>   // float4 per lane: D <= 256 NV
__global__ __launch_bounds__(256) void k_ln_unit(const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                 float* __restrict__ out, int rows, int Tn, int D, size_t ld_row, size_t ld_pos) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;                                            // wave-uniform
    const float* xr = x + (size_t)row * D;
    float4 v[NV], g[NV], bt[NV];
#pragma unroll
    for (int it = 0; it < NV; it++) {
        const int c = lane * 4 + it * 256;
        v[it] = c < D ? *reinterpret_cast<const float4*>(xr + c) : make_float4(0, 0, 0, 0);
        g[it] = c < D ? *reinterpret_cast<const float4*>(gamma + c) : make_float4(0, 0, 0, 0);
        bt[it] = c < D ? *reinterpret_cast<const float4*>(beta + c) : make_float4(0, 0, 0, 0);
    }
    float s = 0.f;
#pragma unroll
    for (int it = 0; it < NV; it++) s += v[it].x + v[it].y + v[it].z + v[it].w;
    const float mu = wave_sum(s) / D;
    float q = 0.f;
#pragma unroll
    for (int it = 0; it < NV; it++) {
        if (lane * 4 + it * 256 < D) {
            const float a = v[it].x - mu, b = v[it].y - mu, c2 = v[it].z - mu, d = v[it].w - mu;
            q += a * a + b * b + c2 * c2 + d * d;
        }
    }
    const float rs = rsqrtf(wave_sum(q) / D + 1e-5f);
    float n2 = 0.f;
#pragma unroll
    for (int it = 0; it < NV; it++) {                                   // columns >= D: gamma = beta = 0 -> 0
        v[it] = make_float4((v[it].x - mu) * rs * g[it].x + bt[it].x, (v[it].y - mu) * rs * g[it].y + bt[it].y,
                            (v[it].z - mu) * rs * g[it].z + bt[it].z, (v[it].w - mu) * rs * g[it].w + bt[it].w);
        n2 += (v[it].x * v[it].x + v[it].y * v[it].y) + (v[it].z * v[it].z + v[it].w * v[it].w);
    }
    n2 = wave_sum(n2);
    const float inv = n2 > 0.f ? 1.0f / sqrtf(n2) : 0.f;
    float* o = out + (size_t)(row / Tn) * ld_row + (size_t)(row % Tn) * ld_pos;
#pragma unroll
    for (int it = 0; it < NV; it++) {
        const int c = lane * 4 + it * 256;
        if (c < D) *reinterpret_cast<float4*>(o + c) = make_float4(v[it].x * inv, v[it].y * inv, v[it].z * inv, v[it].w * inv);
    }
}

struct DecWS {
    float *x, *x1;
    act_t *xn, *qkv, *att, *hact, *hf;
    float *meanf, *rstdf;
    int* last;
    float* scratch;
    size_t scratch_bytes;
    unsigned long long* pk_prof;   // [256][21] profile of the persistent layer launch (CC_PK_PROF=1)
    unsigned* pk_ctr;      // persistent layer launch (decode_pk.hip): arrival counters + error word
    unsigned* xt_ctl;      // XCD-team engine (decode_xt.hip): control words (zeroed before every launch) + one sticky error word behind them
    unsigned long long* xt_prof;
    int2* grp_ent;         // beam-group attention: union list [R / group][group * (pos0 + 1)] + entry counts (k_group_union)
    int* grp_cnt;
    size_t grp_ents;
    char* x3;              // bf16x3 build: operand-image scratch (gemm_api.h)
    size_t x3_bytes;
    size_t bytes;
};
void dec_carve(const cc_gpt2_cfg* c, int R, int Tn, void* ws, DecWS& w) {
    Carver cv(ws);
    const size_t M = (size_t)R * Tn, D = c->D;
    w.x = cv.take<float>(M * D);
    w.x1 = cv.take<float>(M * D);
    w.xn = cv.take<act_t>(M * D);
    w.qkv = cv.take<act_t>(M * 3 * D);
    w.att = cv.take<act_t>(M * D);
    w.hact = cv.take<act_t>(M * 4 * D);
    w.hf = cv.take<act_t>((size_t)R * D);
    w.meanf = cv.take<float>(R);
    w.rstdf = cv.take<float>(R);
    w.last = cv.take<int>(R);
    w.scratch_bytes = (size_t)8 * M * 4 * D * sizeof(float);   // up to 8 K-slices of the widest (4D) output
    w.scratch = cv.take<float>(w.scratch_bytes / sizeof(float));
    w.pk_ctr = cv.take<unsigned>(PK_CTR_WORDS);
    w.pk_prof = cv.take<unsigned long long>((size_t)256 * 21);
    w.xt_ctl = cv.take<unsigned>(XT_CTL_WORDS + 16);
    w.xt_prof = cv.take<unsigned long long>((size_t)256 * XT_PROF_WORDS);
    w.grp_ents = Tn == 1 ? (size_t)R * c->NPOS + (size_t)R * 128 : 0;
    w.grp_ent = cv.take<int2>(w.grp_ents);
    w.grp_cnt = cv.take<int>(R);
    w.x3_bytes = kX3 ? x3_img(M, 4 * D) : 0;      // the deepest A image: mlp.c_proj, K = 4D
    w.x3 = kX3 ? cv.take<char>(w.x3_bytes) : nullptr;
    w.bytes = cv.bytes();
}

// the union list of one position's beam groups, for whichever attention form follows; the same launch clears `clear_words` control words
// of the persistent launch that consumes the list (none for the per-op path)
void launch_group_union(int group, int ngroups, hipStream_t st, const int* row_map, const DecWS& w, int pos0, int ctx_max, int cap, int append,
                        unsigned* clear_ptr, int clear_words) {
    switch (group) {
#define CC_GU(G_) case G_: hipLaunchKernelGGL((k_group_union<G_>), dim3(ngroups), dim3(64), 0, st, row_map, w.grp_ent, w.grp_cnt, pos0, ctx_max, cap, append, clear_ptr, clear_words); break;
        CC_GU(2) CC_GU(3) CC_GU(4) CC_GU(5) CC_GU(6) CC_GU(7) CC_GU(8)
#undef CC_GU
        default: break;
    }
}

// The attention step of one decode layer: which form runs (decode_attn_plan) and its launches (decode_attn_run).  decode_fwd_impl and the
// test hook cc_decode_attention both go through these two, so the hook launches what the product launches.
struct AttnPlan {
    int grp_cap;       // entries per group in the union list: whole passes of 128
    size_t grp_shm;    // k_decode_attn_group's LDS bytes
    bool grp_attn;     // beam-group form (k_group_union + k_decode_attn_group); false: k_decode_attn
    float scale;
};
// CC_ERR_SHAPE: the per-row kernel's LDS (p | srow | red per wave) does not fit — refused for every form, before anything is launched
int decode_attn_plan(int R, int Tn, int hd, int pos0, int ctx_max, int group, size_t grp_ents, AttnPlan& a) {
    if ((size_t)4 * (2 * ctx_max + 8 * hd) * sizeof(float) > 64 * 1024) return CC_ERR_SHAPE;
    a.scale = 1.0f / sqrtf((float)hd);
    // beam-group attention (k_decode_attn_group): single-position steps of `group` consecutive rows that share ancestry (a perf hint only)
    a.grp_cap = (group * (pos0 + 1) + 127) & ~127;          // entries per group, whole passes of 128
    a.grp_shm = ((size_t)a.grp_cap * 8 + 96 + (size_t)8 * group * 64) * sizeof(float);
    a.grp_attn = (cc_shared::g_decode_mode & 1) && Tn == 1 && group >= 2 && group <= 8 && hd == 64 && a.grp_shm <= 64 * 1024 &&
                 (size_t)(R / group) * a.grp_cap <= grp_ents;
    return CC_OK;
}
// append: the kernels store the new K / V slices and read them from qkv (else the caller's c_attn epilogue already has); build_union: this
// call also builds the groups' union list (once per position: the first layer that runs the group form)
int decode_attn_run(const AttnPlan& a, hipStream_t st, const DecWS& w, const act_t* qkv, act_t* kc, act_t* vc, const int* row_map, act_t* out, int R, int Tn,
                    int H, int hd, int pos0, int ctx_max, int group, bool append, bool build_union) {
    if (a.grp_attn) {
        const int ng = R / group, app = append ? 1 : 0;
        if (build_union) launch_group_union(group, ng, st, row_map, w, pos0, ctx_max, a.grp_cap, app, nullptr, 0);
#define CC_GRP(G_)                                                                                                                            \
    case G_:                                                                                                                                  \
        hipLaunchKernelGGL((k_decode_attn_group<G_>), dim3(ng * H), dim3(256), a.grp_shm, st, qkv, kc, vc, w.grp_ent, w.grp_cnt, out, H, pos0,    \
                           ctx_max, a.scale, a.grp_cap, app);                                                                                 \
        break;
        switch (group) { CC_GRP(2) CC_GRP(3) CC_GRP(4) CC_GRP(5) CC_GRP(6) CC_GRP(7) CC_GRP(8) default: return CC_ERR_ARG; }
#undef CC_GRP
    } else {
        const int nw = R * H * Tn;
        const size_t shm = (size_t)4 * (2 * ctx_max + 8 * hd) * sizeof(float);
        if (!append)
            hipLaunchKernelGGL(k_decode_attn<false>, dim3((nw + 3) / 4), dim3(256), shm, st, qkv, kc, vc, row_map, out, R, Tn, H, hd, pos0, ctx_max, a.scale);
        else
            hipLaunchKernelGGL(k_decode_attn<true>, dim3((nw + 3) / 4), dim3(256), shm, st, qkv, kc, vc, row_map, out, R, Tn, H, hd, pos0, ctx_max, a.scale);
    }
    return CC_OK;
}

}  // namespace

extern "C" {

int64_t CC_API(cc_decode_ws_bytes)(const cc_gpt2_cfg* cfg, int32_t R, int32_t Tnew) {
    if (!gpt2_dims_ok(cfg) || R <= 0 || Tnew <= 0) return CC_ERR_SHAPE;
    DecWS w;
    dec_carve(cfg, R, Tnew, nullptr, w);
    return (int64_t)w.bytes;
}

int64_t CC_API(cc_decode_part_floats)(const cc_gpt2_cfg* cfg, int32_t R) {
    if (!gpt2_dims_ok(cfg) || R <= 0) return CC_ERR_SHAPE;
    const int Ns = std::min(cfg->Vp, rup(cfg->V, 8));
    return (int64_t)2 * R * ((Ns + 63) / 64);
}

// the decode step behind every entry point; wimg / wteam: lab build only (include/clipcap_hip_lab.h: cc_decode_fwd_x), NULL in the product
static int decode_fwd_impl(const cc_gpt2_cfg* c, int32_t R, int32_t Tn, int32_t pos0, int32_t ctx_max, const float* w32, const uint16_t* w16, const uint16_t* wimg,
                           const uint16_t* wteam, const float* x, uint16_t* kv, const int32_t* row_map, int32_t group, void* ws, float* logits, int64_t ldl, float* lpart,
                           void* stream);
int CC_API(cc_decode_fwd_g)(const cc_gpt2_cfg* c, int32_t R, int32_t Tn, int32_t pos0, int32_t ctx_max, const float* w32, const uint16_t* w16,
                    const float* x, uint16_t* kv, const int32_t* row_map, int32_t group, void* ws, float* logits, int64_t ldl, float* lpart, void* stream) {
    return decode_fwd_impl(c, R, Tn, pos0, ctx_max, w32, w16, nullptr, nullptr, x, kv, row_map, group, ws, logits, ldl, lpart, stream);
}

int CC_API(cc_decode_fwd)(const cc_gpt2_cfg* c, int32_t R, int32_t Tn, int32_t pos0, int32_t ctx_max, const float* w32, const uint16_t* w16,
                  const float* x, uint16_t* kv, const int32_t* row_map, void* ws, float* logits, int64_t ldl, void* stream) {
    return CC_API(cc_decode_fwd_g)(c, R, Tn, pos0, ctx_max, w32, w16, x, kv, row_map, 1, ws, logits, ldl, nullptr, stream);
}

int CC_API(cc_decode_fwd_p)(const cc_gpt2_cfg* c, int32_t R, int32_t Tn, int32_t pos0, int32_t ctx_max, const float* w32, const uint16_t* w16,
                    const float* x, uint16_t* kv, const int32_t* row_map, void* ws, float* logits, int64_t ldl, float* lpart, void* stream) {
    return CC_API(cc_decode_fwd_g)(c, R, Tn, pos0, ctx_max, w32, w16, x, kv, row_map, 1, ws, logits, ldl, lpart, stream);
}

#ifdef CC_EXPERIMENTS      // ---- lab build only: the entry points of include/clipcap_hip_lab.h ----
// fragment-ordered images of the four GEMM weights of every block, at their arena offsets
int64_t CC_API(cc_decode_image_bytes)(const cc_gpt2_cfg* c) {
    if (!gpt2_dims_ok(c) || kX3 || (c->D % 64)) return 0;
    return 2 * Gpt2Off(c).total;
}

int CC_API(cc_decode_image)(const cc_gpt2_cfg* c, const uint16_t* w16, uint16_t* wimg, void* stream) {
    if (!gpt2_dims_ok(c) || !w16 || !wimg) return CC_ERR_ARG;
    if (kX3 || (c->D % 64)) return CC_ERR_SHAPE;
    const Gpt2Off o(c);
    const op16_t* w16t = reinterpret_cast<const op16_t*>(w16) + o.total;       // transposed Conv1D weights: [N][K], K contiguous
    op16_t* img = reinterpret_cast<op16_t*>(wimg);
    for (int l = 0; l < c->NL; l++) {
        const auto y = o.layer(l);
        CC_TRY(skinny_image(w16t + y.aw, img + y.aw, 3 * c->D, c->D, S_(stream)));
        CC_TRY(skinny_image(w16t + y.pw, img + y.pw, c->D, c->D, S_(stream)));
        CC_TRY(skinny_image(w16t + y.fw, img + y.fw, 4 * c->D, c->D, S_(stream)));
        CC_TRY(skinny_image(w16t + y.p2w, img + y.p2w, c->D, 4 * c->D, S_(stream)));
    }
    return CC_OK;
}

int64_t CC_API(cc_decode_xt_image_bytes)(const cc_gpt2_cfg* c) {
    if (!gpt2_dims_ok(c) || c->H * 64 != c->D) return 0;
    return xt_image_bytes(c->D, c->NL);
}

int CC_API(cc_decode_xt_image)(const cc_gpt2_cfg* c, const uint16_t* w16, uint16_t* wimg, void* stream) {
    if (!gpt2_dims_ok(c) || !w16 || !wimg) return CC_ERR_ARG;
    if (c->H * 64 != c->D || !xt_image_bytes(c->D, c->NL)) return CC_ERR_SHAPE;
    const Gpt2Off o(c);
    return xt_build_image(c->D, c->NL, o.layer0, o.layer_stride, o.total, w16, wimg, S_(stream));
}

int CC_API(cc_decode_fwd_x)(const cc_gpt2_cfg* c, int32_t R, int32_t Tn, int32_t pos0, int32_t ctx_max, const float* w32, const uint16_t* w16, const uint16_t* wimg,
                    const uint16_t* wteam, const float* x, uint16_t* kv, const int32_t* row_map, int32_t group, void* ws, float* logits, int64_t ldl, float* lpart,
                    void* stream) {
    return decode_fwd_impl(c, R, Tn, pos0, ctx_max, w32, w16, wimg, wteam, x, kv, row_map, group, ws, logits, ldl, lpart, stream);
}
#endif  // CC_EXPERIMENTS

static int decode_fwd_impl(const cc_gpt2_cfg* c, int32_t R, int32_t Tn, int32_t pos0, int32_t ctx_max, const float* w32, const uint16_t* w16, const uint16_t* wimg,
                           const uint16_t* wteam, const float* x, uint16_t* kv, const int32_t* row_map, int32_t group, void* ws, float* logits, int64_t ldl, float* lpart,
                           void* stream) {
    if (group < 1 || (R > 0 && R % group)) return CC_ERR_ARG;
    if (!gpt2_dims_ok(c) || R <= 0 || Tn <= 0 || pos0 < 0 || !w32 || !w16 || !x || !kv || !ws || !logits) return CC_ERR_ARG;
    const int Ns = std::min(c->Vp, rup(c->V, 8));
    if (pos0 + Tn > ctx_max || pos0 + Tn > c->NPOS || ldl < Ns || (ldl & 3) || ldl > 0x7fffffff) return CC_ERR_SHAPE;
    hipStream_t st = S_(stream);
    DecWS w;
    dec_carve(c, R, Tn, ws, w);
    AttnPlan ap;
    CC_TRY(decode_attn_plan(R, Tn, c->D / c->H, pos0, ctx_max, group, w.grp_ents, ap));
    Call cx{st, nullptr, w.x3, w.x3_bytes};
    const Gpt2Off o(c);
    const int D = c->D, M = R * Tn, H = c->H, hd = D / H;
    // single-position step: positional add + layer 0's ln_1 in one launch; the last layer's finishing pass applies ln_f (below)
    const bool one = Tn == 1 && D <= 2048 && (D & 3) == 0;
    if (one) {
        hipLaunchKernelGGL(k_add_wpe_ln, dim3((R + 3) / 4), dim3(256), 0, st, x, w32 + o.wpe, w.x, w32 + o.layer(0).l1w, w32 + o.layer(0).l1b, w.xn, R, D, pos0);
    } else {
        const size_t total = (size_t)M * (D >> 2);
        hipLaunchKernelGGL(k_add_wpe, dim3((int)std::min<size_t>((total + 255) / 256, 2048)), dim3(256), 0, st, x, w32 + o.wpe, w.x, R, Tn, D, pos0);
    }
    const size_t cache_layer = (size_t)2 * R * ctx_max * D;
    const uint16_t* w16t = W16(w16, o.total);   // transposed Conv1D weights (cc_gpt2_sync_weights): forward GEMMs are NT
    const int grp_cap = ap.grp_cap;
    const bool grp_attn = ap.grp_attn;
    bool xn_ready = one;
    bool hf_ready = false;
    int l_first = 0;
    if (one && group >= 2) cc_shared::g_decode_last_path = 0;
    if (grp_attn && one && !kX3 && wteam && (cc_shared::g_decode_mode & 4)) {
        // XCD-team engine (decode_xt.hip): every XCD runs the whole stack for its own captions; CC_ERR_SHAPE = not covered -> the paths below
        XtLaunch L{};
        L.w32 = w32; L.wimg = reinterpret_cast<const op16_t*>(wteam); L.D = D; L.H = H; L.NL = c->NL; L.M = M; L.group = group; L.pos0 = pos0; L.ctx_max = ctx_max;
        L.layer0 = o.layer0; L.layer_stride = o.layer_stride; L.x = w.x; L.x1 = w.x1; L.qkv = w.qkv; L.att = w.att; L.hact = w.hact; L.hf = w.hf;
        L.kv = reinterpret_cast<act_t*>(kv); L.cache_layer = cache_layer; L.ent = w.grp_ent; L.cnt = w.grp_cnt; L.cap = grp_cap;
        L.ctl = w.xt_ctl; L.sticky = w.xt_ctl + XT_CTL_WORDS;
        static const bool xt_prof = cc_lab_env("CC_XT_PROF") != nullptr;
        L.prof = xt_prof ? w.xt_prof : nullptr;
        // probe the geometry first (no launch): the union kernel below also clears the control words
        XtLaunch probe = L;
        probe.ctl = nullptr;
        if (xt_covers(probe)) {
            launch_group_union(group, R / group, st, row_map, w, pos0, ctx_max, grp_cap, 1, w.xt_ctl, XT_CTL_WORDS);
            const int rc = decode_layers_xt(L, st);
            if (rc != CC_OK) return rc;
            cc_shared::g_decode_last_path = 2;
            l_first = c->NL;
            hf_ready = true;
        }
    }
    if (l_first == 0 && grp_attn && one && !kX3 && (cc_shared::g_decode_mode & 2)) {
        // the whole layer stack as ONE persistent launch (decode_pk.hip); CC_ERR_SHAPE = geometry not covered -> the per-op launches below
        launch_group_union(group, R / group, st, row_map, w, pos0, ctx_max, grp_cap, 1, w.pk_ctr, PK_CTR_WORDS);
        PkLaunch L{};
        L.w32 = w32; L.w16t = reinterpret_cast<const op16_t*>(w16t); L.D = D; L.H = H; L.NL = c->NL; L.M = M; L.group = group; L.pos0 = pos0; L.ctx_max = ctx_max;
        L.layer0 = o.layer0; L.layer_stride = o.layer_stride; L.x = w.x; L.x1 = w.x1; L.xn = w.xn; L.qkv = w.qkv; L.att = w.att; L.hact = w.hact; L.hf = w.hf;
        L.slab = w.scratch; L.slab_bytes = w.scratch_bytes; L.kv = reinterpret_cast<act_t*>(kv); L.cache_layer = cache_layer;
        L.ent = w.grp_ent; L.cnt = w.grp_cnt; L.cap = grp_cap; L.ctr = w.pk_ctr;
        static const bool pk_prof = cc_lab_env("CC_PK_PROF") != nullptr;
        L.prof = pk_prof ? w.pk_prof : nullptr;
        const int rc = decode_layers_persistent(L, st);
        if (rc == CC_OK) {
            cc_shared::g_decode_last_path = 1;
            l_first = c->NL;
            hf_ready = true;
        } else if (rc != CC_ERR_SHAPE) {
            return rc;
        }
    }
    // fragment-ordered weight image (cc_decode_image): the K-over-the-waves GEMMs then load the weight operand global -> VGPR
    const op16_t* bimg = (!kX3 && wimg && (cc_shared::g_decode_mode & 8)) ? reinterpret_cast<const op16_t*>(wimg) : nullptr;
    for (int l = l_first; l < c->NL; l++) {
        const auto y = o.layer(l);
        act_t* kc = reinterpret_cast<act_t*>(kv) + (size_t)l * cache_layer;     // (bf16x3: the cache holds fp32, twice the bytes)
        act_t* vc = kc + (size_t)R * ctx_max * D;
        // xn = ln_1(x): produced by the previous layer's fused finish when possible
        if (!xn_ready) CC_TRY(ln_fwd(w.x, D, nullptr, w32 + y.l1w, w32 + y.l1b, w.xn, nullptr, nullptr, nullptr, M, D, st));
        // c_attn (+ fused KV append into the cache)
        const bool f_qkv = gemm_nt_skinny_can_fuse(M, 3 * D, D, w.scratch_bytes) &&
                           ((M + 127) / 128) * ((3 * D + 127) / 128) < skinny_single_min_tiles();
        SkinnyFuse fq;
        if (f_qkv) { fq.kcache = kc; fq.vcache = vc; fq.Tn = Tn; fq.pos0 = pos0; fq.ctx_max = ctx_max; }
        fq.bimg = bimg ? bimg + y.aw : nullptr;
        CC_TRY(gemm_nt_skinny(w.xn, D, W16(w16t, y.aw), D, M, 3 * D, D, w32 + y.ab, 0, nullptr, nullptr, w.qkv, 3 * D, w.scratch, w.scratch_bytes, cx, &fq));
        CC_TRY(decode_attn_run(ap, st, w, w.qkv, kc, vc, row_map, w.att, R, Tn, H, hd, pos0, ctx_max, group, !f_qkv, l == 0));
        // attn.c_proj + residual (+ fused ln_2)
        const bool f_d = gemm_nt_skinny_can_fuse(M, D, D, w.scratch_bytes) && gemm_nt_skinny_can_fuse(M, D, 4 * D, w.scratch_bytes);
        SkinnyFuse f2;
        if (f_d) { f2.ln_gamma = w32 + y.l2w; f2.ln_beta = w32 + y.l2b; f2.ln_out16 = w.xn; }
        f2.bimg = bimg ? bimg + y.pw : nullptr;
        CC_TRY(gemm_nt_skinny(w.att, D, W16(w16t, y.pw), D, M, D, D, w32 + y.pb, 0, w.x, w.x1, nullptr, D, w.scratch, w.scratch_bytes, cx, &f2));
        if (!f_d) CC_TRY(ln_fwd(w.x1, D, nullptr, w32 + y.l2w, w32 + y.l2b, w.xn, nullptr, nullptr, nullptr, M, D, st));
        SkinnyFuse f3;
        f3.bimg = bimg ? bimg + y.fw : nullptr;
        CC_TRY(gemm_nt_skinny(w.xn, D, W16(w16t, y.fw), D, M, 4 * D, D, w32 + y.fb, 2, nullptr, nullptr, w.hact, 4 * D, w.scratch, w.scratch_bytes, cx, &f3));
        // mlp.c_proj + residual (+ fused ln_1 of the next layer; after the LAST layer, ln_f: with one new position per row the finishing
        // pass normalises straight into hf)
        const bool last = l + 1 == c->NL;
        const bool f_next = f_d && (!last || one);
        SkinnyFuse f1;
        if (f_next) {
            f1.ln_gamma = w32 + (last ? o.lnf_w : o.layer(l + 1).l1w);
            f1.ln_beta = w32 + (last ? o.lnf_b : o.layer(l + 1).l1b);
            f1.ln_out16 = last ? w.hf : w.xn;
        }
        f1.bimg = bimg ? bimg + y.p2w : nullptr;
        CC_TRY(gemm_nt_skinny(w.hact, 4 * D, W16(w16t, y.p2w), 4 * D, M, D, 4 * D, w32 + y.p2b, 0, w.x1, w.x, nullptr, D, w.scratch, w.scratch_bytes, cx, &f1));
        xn_ready = f_next && !last;
        hf_ready = f_next && last;
    }
    if (!hf_ready) {
        hipLaunchKernelGGL(k_last_rows, dim3((R + 255) / 256), dim3(256), 0, st, w.last, R, Tn);
        CC_TRY(ln_fwd(w.x, D, w.last, w32 + o.lnf_w, w32 + o.lnf_b, w.hf, nullptr, w.meanf, w.rstdf, R, D, st));
    }
    if (lpart) {      // logits + per-(row, 64-column block) softmax partials for cc_beam_step_p
        const int npart = (Ns + 63) / 64;
        CC_TRY(gemm_logits_part(w.hf, D, W16(w16, o.wte), D, R, Ns, c->V, D, logits, (int)ldl, lpart, lpart + (size_t)R * npart, npart, cx));
    } else {
        CC_TRY(gemm_f32out(0, 0, w.hf, D, W16(w16, o.wte), D, R, Ns, D, logits, (int)ldl, nullptr, 0, 1.0f, 1, cx));
    }
    return hipGetLastError() == hipSuccess ? CC_OK : CC_ERR_LAUNCH;
}

#ifdef CC_EXPERIMENTS
int CC_API(cc_decode_ws_check)(const cc_gpt2_cfg* c, int32_t R, int32_t Tn, const void* ws, void* stream) {
    if (!gpt2_dims_ok(c) || R <= 0 || Tn <= 0 || !ws) return CC_ERR_ARG;
    DecWS w;
    dec_carve(c, R, Tn, const_cast<void*>(ws), w);
    unsigned e = 0;
    if (hipStreamSynchronize(S_(stream)) != hipSuccess) return CC_ERR_LAUNCH;
    if (hipMemcpy(&e, w.pk_ctr + 7 * PK_MAX_RT, sizeof(e), hipMemcpyDeviceToHost) != hipSuccess) return CC_ERR_LAUNCH;
    unsigned e2 = 0;
    if (hipMemcpy(&e2, w.xt_ctl + XT_CTL_WORDS, sizeof(e2), hipMemcpyDeviceToHost) != hipSuccess) return CC_ERR_LAUNCH;
    return (e | e2) ? CC_ERR_STATE : CC_OK;
}
#endif

// test hook: the attention step of one layer on caller buffers, through the product's own dispatch (decode_attn_plan / decode_attn_run)
int CC_API(cc_decode_attention)(const cc_gpt2_cfg* c, int32_t R, int32_t Tn, int32_t pos0, int32_t ctx_max, const uint16_t* qkv, uint16_t* kv_layer,
                        const int32_t* row_map, int32_t group, int32_t append, void* ws, uint16_t* out, int32_t* path, void* stream) {
    if (group < 1 || (R > 0 && R % group)) return CC_ERR_ARG;
    if (!gpt2_dims_ok(c) || R <= 0 || Tn <= 0 || pos0 < 0 || !qkv || !kv_layer || !ws || !out || (append != 0 && append != 1)) return CC_ERR_ARG;
    if (pos0 + Tn > ctx_max || pos0 + Tn > c->NPOS) return CC_ERR_SHAPE;
    DecWS w;
    dec_carve(c, R, Tn, ws, w);
    AttnPlan ap;
    const int D = c->D, H = c->H, hd = D / H;
    CC_TRY(decode_attn_plan(R, Tn, hd, pos0, ctx_max, group, w.grp_ents, ap));
    act_t* kc = reinterpret_cast<act_t*>(kv_layer);
    act_t* vc = kc + (size_t)R * ctx_max * D;
    CC_TRY(decode_attn_run(ap, S_(stream), w, reinterpret_cast<const act_t*>(qkv), kc, vc, row_map, reinterpret_cast<act_t*>(out), R, Tn, H, hd, pos0, ctx_max,
                           group, append != 0, true));
    if (path) *path = ap.grp_attn ? 1 : 0;
    return hipGetLastError() == hipSuccess ? CC_OK : CC_ERR_LAUNCH;
}

int CC_API(cc_decode_reorder)(const cc_gpt2_cfg* c, int32_t R_src, int32_t R_dst, int32_t ctx, int32_t ctx_max, const uint16_t* kv_src, uint16_t* kv_dst,
                      const int32_t* src, void* stream) {
    if (!gpt2_dims_ok(c) || R_src <= 0 || R_dst <= 0 || ctx < 0 || ctx > ctx_max || !kv_src || !kv_dst || !src || kv_src == kv_dst) return CC_ERR_ARG;
    if (ctx == 0) return CC_OK;
    const size_t total = (size_t)c->NL * 2 * R_dst * ctx * (c->D * sizeof(act_t) / 16);
    hipLaunchKernelGGL(k_kv_reorder, dim3((int)std::min<size_t>((total + 255) / 256, 4096)), dim3(256), 0, S_(stream),
                       reinterpret_cast<const act_t*>(kv_src), reinterpret_cast<act_t*>(kv_dst), src, R_src,
                       R_dst, ctx, ctx_max, c->D, c->NL * 2);
    return hipGetLastError() == hipSuccess ? CC_OK : CC_ERR_LAUNCH;
}

int CC_API(cc_embed_tokens)(const cc_gpt2_cfg* c, int32_t R, const float* w32, const int32_t* tokens, float* out, void* stream) {
    if (!gpt2_dims_ok(c) || R <= 0 || !w32 || !tokens || !out) return CC_ERR_ARG;
    const size_t total = (size_t)R * (c->D >> 2);
    hipLaunchKernelGGL(k_embed_tokens, dim3((int)std::min<size_t>((total + 255) / 256, 2048)), dim3(256), 0, S_(stream), w32, tokens, out, R, c->D, c->Vp);
    return hipGetLastError() == hipSuccess ? CC_OK : CC_ERR_LAUNCH;
}

int CC_API(cc_embed_tokens_bwd)(const cc_gpt2_cfg* c, int32_t R, const float* dout, const int32_t* tokens, float* dwte, void* stream) {
    if (!gpt2_dims_ok(c) || R <= 0 || !dout || !tokens || !dwte) return CC_ERR_ARG;
    const size_t total = (size_t)R * c->D;
    hipLaunchKernelGGL(k_embed_tokens_bwd, dim3((int)std::min<size_t>((total + 255) / 256, 4096)), dim3(256), 0, S_(stream), dout, tokens, dwte, R, c->D, c->Vp);
    return hipGetLastError() == hipSuccess ? CC_OK : CC_ERR_LAUNCH;
}

int CC_API(cc_embed_tokens_bwd_ws)(const cc_gpt2_cfg* c, int32_t R, const float* dout, const int32_t* tokens, float* dwte, void* ws, void* stream) {
    if (!gpt2_dims_ok(c) || R <= 0 || !dout || !tokens || !dwte) return CC_ERR_ARG;
    ScatterSrc e;
    e.ids32 = tokens; e.f32 = dout; e.rpb = 1; e.bstride = (size_t)c->D;
    return scatter_rows(e, R, c->D, c->Vp, dwte, ws, S_(stream));
}

int64_t CC_API(cc_embed_tokens_bwd_ws_bytes)(const cc_gpt2_cfg* c, int32_t R) {
    if (!gpt2_dims_ok(c) || R <= 0) return CC_ERR_ARG;
    return (int64_t)scatter_ws_bytes(R, c->D);
}

int CC_API(cc_beam_advance)(const cc_gpt2_cfg* c, int32_t R, int32_t beam, const float* w32, const int32_t* next_tokens, const int32_t* src_rows,
                    int32_t pos, int32_t ctx_max, const int32_t* row_map_in, int32_t* row_map_out, int32_t step, int32_t tok_ld,
                    const int32_t* tokens_in, int32_t* tokens_out, float* x_out, void* stream) {
    if (!gpt2_dims_ok(c) || R <= 0 || beam <= 0 || (R % beam) || !w32 || !next_tokens || !x_out || pos < 0 || pos > ctx_max) return CC_ERR_ARG;
    if ((row_map_out && (!row_map_in || row_map_in == row_map_out)) || (tokens_out && (step < 0 || step >= tok_ld || (step > 0 && !tokens_in) ||
                                                                                      tokens_in == tokens_out)))
        return CC_ERR_ARG;
    hipLaunchKernelGGL(k_beam_advance, dim3(R), dim3(256), 0, S_(stream), beam, c->D, w32, next_tokens, src_rows, pos, ctx_max, row_map_in, row_map_out,
                       step, tok_ld, tokens_in, tokens_out, x_out);
    return hipGetLastError() == hipSuccess ? CC_OK : CC_ERR_LAUNCH;
}

// The final hidden states of the last forward on this workspace, as unit vectors (contrastive search).  Every path of decode_fwd_impl's
// layer loop ends a layer with mlp.c_proj + residual stored to DecWS::x in fp32 for all R * Tn rows (gemm_nt_skinny's out32: the plain
// epilogue, k_splitk_finish and k_splitk_finish_row all store it before any fused LayerNorm), whether ln_f then runs fused (hf) or as
// ln_fwd over the last rows.  The lab library's persistent engines keep the stream elsewhere: refused.
int CC_API(cc_decode_hidden_unit)(const cc_gpt2_cfg* c, int32_t R, int32_t Tn, const float* w32, void* ws, float* out, int64_t ld_row, int64_t ld_pos,
                                  void* stream) {
    if (!gpt2_dims_ok(c) || R < 0 || Tn <= 0 || !w32 || !ws || !out || (reinterpret_cast<uintptr_t>(out) & 15)) return CC_ERR_ARG;
    const int D = c->D;
    if (ld_pos < D || ld_row < (int64_t)(Tn - 1) * ld_pos + D) return CC_ERR_ARG;
    if (D > 2048 || (D & 3) || (ld_row & 3) || (ld_pos & 3)) return CC_ERR_SHAPE;
    if (cc_shared::g_decode_mode & 6) return CC_ERR_STATE;
    if (R == 0) return CC_OK;
    DecWS w;
    dec_carve(c, R, Tn, ws, w);
    const Gpt2Off o(c);
    const int rows = R * Tn;
    const dim3 gr((rows + 3) / 4);
#define CC_LNU(NV) hipLaunchKernelGGL(k_ln_unit<NV>, gr, dim3(256), 0, S_(stream), w.x, w32 + o.lnf_w, w32 + o.lnf_b, out, rows, Tn, D, (size_t)ld_row, (size_t)ld_pos)
    if (D <= 256) CC_LNU(1); else if (D <= 512) CC_LNU(2); else if (D <= 768) CC_LNU(3); else if (D <= 1024) CC_LNU(4); else CC_LNU(8);
#undef CC_LNU
    return hipGetLastError() == hipSuccess ? CC_OK : CC_ERR_LAUNCH;
}

}  // extern "C"
