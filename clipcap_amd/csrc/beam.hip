// Device-side beam-search update of the caption decoders (reference: clipcap/inference/base.py:84-119): from one step's logits to the next
// tokens, source rows, scores, lengths and stop flags.  fp32 / integer work only, so this unit is built once (Makefile).
#include "beam.hip.h"

using namespace CC_NS;

namespace {

// ---- beam step (base.py:84-119) in three small kernels so that all CUs take part --------------------------------
//   k_beam_rowstats : one block per (sample, beam row): max and sum(exp) of logits/temperature
//   k_beam_partial  : grid (sample, chunk): top-`beam` of the length-normalised candidate scores inside one slice of the
//                     flattened beam*V candidate space (thread-local insertion lists + block-wide selection)
//   k_beam_final    : one block per sample merges the chunk winners, then gathers / updates scores, lengths, stopped flags
// Ties resolve to the lowest flat index b*V + v (cand_better, select.hip.h).
//
// Diverse beam search: beam groups with a Hamming penalty (Vijayakumar et al., 2016; not in the reference).  The `beam` rows of a sample
// are split into G beam groups of W consecutive rows; one step advances the groups one after the other, and a candidate of beam group g
// whose token v was picked c(v) times AT THIS STEP by the beam groups before it loses penalty * c(v) of its log-probability (before the
// length normalisation; a stopped beam's token-0 continuation is neither penalised nor counted).  Apart from that a beam group's update
// is the one above on its own W rows: the same two bodies (beam_partial_body, beam_final_body) with DIV = true.
//   k_beam_rowstats      : once for all rows
//   k_beam_group_partial : per beam group, grid (sample, chunk): top-W of a slice of the group's W * V candidates
//   k_beam_group_final   : per beam group, one block per sample: merges the chunk winners, commits the group's W slots and leaves its
//                          picks in the workspace for the groups after it
// The launches are stream-ordered: beam group g + 1 starts after beam group g has written its picks.  The picks of the earlier groups
// (at most beam - W ids) are loaded into LDS once per block, and a candidate is looked up in them only after the cheap key says it could
// be kept: the penalty only lowers a value, so the unpenalised key stays an upper bound.
constexpr int BEAM_MAX = 16;
constexpr int BEAM_CHUNKS = 16;
constexpr int PICK_NONE = -1;      // a slot whose source beam had stopped: its token 0 is padding, not a pick
// k_beam_rowstats, BeamRow, beam_key, beam_val, beam_commit and launch_rowstats: beam.hip.h (shared with lexbeam.hip)

__device__ __forceinline__ int picked_before(const int* picks, int n, int v) {
    int c = 0;
    for (int i = 0; i < n; i++) c += picks[i] == v ? 1 : 0;
    return c;
}

// The slice selection of k_beam_partial (DIV = false) and k_beam_group_partial (DIV = true), for blocks of 256 threads.
// TW = compile-time width (0: run-time width, dynamically indexed lists — the slow fallback for widths 6, 7 and > 8).  `beam`: rows per
// sample; row0 = first of the `width` rows selected from (0 and width = beam: the whole sample); picks: int [S][beam], entries [0, row0) of a
// sample are the earlier beam groups' picks of this step (DIV only: DIV = false has no pick list, no lookup and no penalty operand).
// Each candidate's exact value needs expf + divide + logf (the reference's softmax().log() arithmetic); almost all of the 250 k
// candidates lose against the thread's current worst kept value, so a cheap bound (x t - m - log(sum), equal up to ~1e-6) with a
// 1e-3 margin decides whether the exact value is evaluated at all.
template <int TW, bool DIV>
__device__ __forceinline__ void beam_partial_body(const float* __restrict__ logits, size_t ldl, int beam, int row0, int width_rt, int V, float inv_temp,
                                                  float penalty, int first, const float* __restrict__ rs, const float* __restrict__ scores,
                                                  const float* __restrict__ seq_len, const unsigned char* __restrict__ stopped,
                                                  const int* __restrict__ picks, float* __restrict__ pval, int* __restrict__ pidx) {
    __shared__ float red[8];
    __shared__ int redi[8];
    __shared__ float cval[TW > 0 ? 1 : 256 * BEAM_MAX];          // candidate arrays: run-time-width fallback only
    __shared__ int cidx[TW > 0 ? 1 : 256 * BEAM_MAX];
    __shared__ float sel_v[BEAM_MAX];
    __shared__ int sel_i[BEAM_MAX];
    __shared__ int s_pick[DIV ? BEAM_MAX : 1];                   // DIV only
    const int width = TW > 0 ? TW : width_rt;
    const int s = blockIdx.x, ch = blockIdx.y, tid = threadIdx.x;
    const int nrows = first ? 1 : width;
    const int total = nrows * V;
    const int per = (total + BEAM_CHUNKS - 1) / BEAM_CHUNKS;
    const int lo = ch * per, hi = min(total, lo + per);
    const int r0 = s * beam + (first ? 0 : row0);                 // the first step reads row 0 of the sample in every beam group
    const float* lg = logits + (size_t)r0 * ldl;
    const int npick = row0;                                       // row0 < beam <= BEAM_MAX
    if constexpr (DIV) {
        if (tid < npick) s_pick[tid] = picks[s * beam + tid];
        __syncthreads();
    }
    // a chunk (total / 16 candidates) spans at most two rows when V >= per; handled generally by walking row segments.
    // scan(f): f(idx, v, row record, raw logit) for every candidate of the chunk (b: row inside the selection, idx = b * V + v), SU logits
    // fetched per thread before any is looked at
    auto scan = [&](auto&& f) {
        for (int b = lo / V; b < nrows && b * V < hi; b++) {
            const int seg_lo = max(lo, b * V), seg_hi = min(hi, (b + 1) * V);
            BeamRow g;
            g.st = !first && stopped[r0 + b];
            g.m = rs[2 * (r0 + b)]; g.sum = rs[2 * (r0 + b) + 1];
            g.lsum = logf(g.sum);
            g.sc = first ? 0.f : scores[r0 + b];
            g.len = first ? 1.f : (seq_len[r0 + b] + (g.st ? 0.f : 1.f));
            const float* row = lg + (size_t)b * ldl - (size_t)b * V;      // row[idx] = lg[b * ldl + (idx - b V)]
            constexpr int SU = 8;
            for (int idx0 = seg_lo + tid; idx0 < seg_hi; idx0 += 256 * SU) {
                float xs[SU];
#pragma unroll
                for (int u = 0; u < SU; u++) xs[u] = g.st ? 0.f : row[min(idx0 + u * 256, seg_hi - 1)];
#pragma unroll
                for (int u = 0; u < SU; u++) {
                    const int idx = idx0 + u * 256;
                    if (idx < seg_hi) f(idx, idx - b * V, g, xs[u]);
                }
            }
        }
    };
    auto count = [&](const BeamRow& g, int v) {
        if constexpr (DIV) return (g.st || npick == 0) ? 0 : picked_before(s_pick, npick, v);
        else return 0;
    };
    bool done = false;
    if constexpr (TW > 0) {
        // Two passes instead of a sorted list per thread (with per-thread lists some lane of a wave inserts in almost every iteration,
        // so every wave ran the ~100-instruction exact-value + insertion path for all of its candidates):
        //   1. thread maxima of the cheap key; the TW-th largest thread maximum is a lower bound of the chunk's TW-th best value.  DIV: the
        //      maximum is of the PENALISED key (looked up only when the unpenalised key would raise the maximum), so the bound stays valid;
        //   2. only candidates within 1e-3 of that bound get the exact value and go to a small LDS list (a handful per block).  DIV: the
        //      filter is on the unpenalised key, an upper bound of the value;
        //   3. TW picks from the list (ties -> lowest flat index).
        constexpr int FCAP = 1024;
        __shared__ float fcv[FCAP];
        __shared__ int fci[FCAP];
        __shared__ int fcount;
        float tmax = -INFINITY;
        scan([&](int, int v, const BeamRow& g, float xraw) {
            float key = beam_key<false>(g, v, xraw, inv_temp, first, 0, 0.f);
            if constexpr (DIV) {
                if (key > tmax) {
                    const int c = count(g, v);
                    if (c) key = beam_key<true>(g, v, xraw, inv_temp, first, c, penalty);
                }
            }
            tmax = fmaxf(tmax, key);
        });
        if (tid == 0) fcount = 0;
        const float thr = kth_bound<TW>(tmax, red);
        scan([&](int idx, int v, const BeamRow& g, float xraw) {
            const float key = beam_key<false>(g, v, xraw, inv_temp, first, 0, 0.f);
            if (key > -INFINITY && key + 1e-3f >= thr) {
                const int pos = atomicAdd(&fcount, 1);
                if (pos < FCAP) { fcv[pos] = beam_val<DIV>(g, v, xraw, inv_temp, first, count(g, v), penalty); fci[pos] = idx; }
            }
        });
        __syncthreads();
        if (fcount <= FCAP) {
            pick_from_list<256>(fcv, fci, fcount, TW, red, redi, sel_v, sel_i);
            done = true;
        }
    }
    if (!done) {
        // sorted insertion list per thread: any width (TW = 0: run-time width), and the overflow path of the list above (e.g. all logits equal)
        // the exact value of a candidate whose cheap key says it could still beat the list's worst entry (a list with room also takes
        // candidates at -inf, banned tokens for instance: beam_final_body drops them)
        auto exact = [&](const BeamRow& g, int v, float xraw, float worst, float& val) {
            if (!g.st && beam_key<false>(g, v, xraw, inv_temp, first, 0, 0.f) + 1e-3f < worst) return false;
            val = beam_val<DIV>(g, v, xraw, inv_temp, first, count(g, v), penalty);
            return true;
        };
        if constexpr (TW > 0) {
            SortedList<TW> l;
            l.clear();
            scan([&](int idx, int v, const BeamRow& g, float xraw) {
                float val;
                if (exact(g, v, xraw, l.v[TW - 1], val)) l.enter(val, idx);
            });
            // every thread's list is sorted, so the block's next best is the best list HEAD; the owner pops its list
            for (int k = 0; k < TW; k++) {
                float bv = l.v[0];
                int bi = l.i[0];
                block_argmax<4>(k, bv, bi, red, redi);
                record_pick(k, bv, bi, sel_v, sel_i);
                l.retire(bi);
            }
            __syncthreads();
        } else {
            // run-time width: the list is indexed dynamically (two plain arrays, which the compiler keeps in indexed registers), then goes
            // to LDS for the picks
            float lv[BEAM_MAX];
            int li[BEAM_MAX];
#pragma unroll
            for (int k = 0; k < BEAM_MAX; k++) { lv[k] = -INFINITY; li[k] = SEL_NONE; }
            scan([&](int idx, int v, const BeamRow& g, float xraw) {
                float val;
                if (exact(g, v, xraw, lv[width - 1], val) && cand_better(val, idx, lv[width - 1], li[width - 1])) {
                    int k = width - 1;
                    while (k > 0 && cand_better(val, idx, lv[k - 1], li[k - 1])) { lv[k] = lv[k - 1]; li[k] = li[k - 1]; k--; }
                    lv[k] = val; li[k] = idx;
                }
            });
            for (int k = 0; k < width; k++) { cval[tid * width + k] = lv[k]; cidx[tid * width + k] = li[k]; }
            __syncthreads();
            pick_from_list<256>(cval, cidx, 256 * width, width, red, redi, sel_v, sel_i);
        }
    }
    if (tid < width) {
        pval[((size_t)s * BEAM_CHUNKS + ch) * width + tid] = sel_v[tid];
        pidx[((size_t)s * BEAM_CHUNKS + ch) * width + tid] = sel_i[tid];
    }
}

template <int TB>      // TB = compile-time beam width (0: run-time width beam_rt)
__global__ __launch_bounds__(256) void k_beam_partial(const float* __restrict__ logits, size_t ldl, int beam_rt, int V, float inv_temp, int first,
                                                      const float* __restrict__ rs, const float* __restrict__ scores,
                                                      const float* __restrict__ seq_len, const unsigned char* __restrict__ stopped,
                                                      float* __restrict__ pval, int* __restrict__ pidx) {
    beam_partial_body<TB, false>(logits, ldl, TB > 0 ? TB : beam_rt, 0, beam_rt, V, inv_temp, 0.f, first, rs, scores, seq_len, stopped, nullptr, pval,
                                 pidx);
}

template <int TW>      // TW = compile-time width of a beam group (0: run-time width width_rt)
__global__ __launch_bounds__(256) void k_beam_group_partial(const float* __restrict__ logits, size_t ldl, int beam, int row0, int width_rt, int V,
                                                            float inv_temp, float penalty, int first, const float* __restrict__ rs,
                                                            const float* __restrict__ scores, const float* __restrict__ seq_len,
                                                            const unsigned char* __restrict__ stopped, const int* __restrict__ picks,
                                                            float* __restrict__ pval, int* __restrict__ pidx) {
    beam_partial_body<TW, true>(logits, ldl, beam, row0, width_rt, V, inv_temp, penalty, first, rs, scores, seq_len, stopped, picks, pval, pidx);
}

// The merge of k_beam_final and k_beam_group_final, for blocks of 64 threads: the `width` best of the chunk winners, then the commit of slots
// row0 .. row0 + width - 1 of the sample.  src_row = the source row's index inside the SAMPLE (what cc_beam_advance expects; 0 on the
// first step, which reads row 0).  picks (null: none kept): picks[slot] = the token, or PICK_NONE when the source beam had stopped.
// Fewer finite candidates than slots (extreme token bans): the empty slots continue row row0 with token 0 at -inf.
__device__ __forceinline__ void beam_final_body(int beam, int row0, int width, int V, int first, int stop_token, const float* __restrict__ pval,
                                                const int* __restrict__ pidx, float* __restrict__ scores, float* __restrict__ seq_len,
                                                unsigned char* __restrict__ stopped, int* __restrict__ next_tok, int* __restrict__ src_row,
                                                int* __restrict__ picks) {
    __shared__ float red[2];
    __shared__ int redi[2];
    __shared__ float cval[BEAM_CHUNKS * BEAM_MAX];
    __shared__ int cidx[BEAM_CHUNKS * BEAM_MAX];
    __shared__ float sel_v[BEAM_MAX];
    __shared__ int sel_i[BEAM_MAX];
    const int s = blockIdx.x, tid = threadIdx.x;
    const int ncand = BEAM_CHUNKS * width;
    // A chunk winner at -inf (a banned token, a stopped beam's tokens other than 0) is no candidate.  The compare is not redundant: the
    // insertion lists of beam_partial_body (run-time width, list overflow) take -inf candidates with their real flat index while they have
    // room, the two-pass path drops them in pass 2, and this is what makes all three agree when a sample has fewer finite candidates than
    // slots.  Both loads come before the select, so the loop is two plain loads and a conditional move.
    for (int c = tid; c < ncand; c += 64) {
        const float val = pval[(size_t)s * ncand + c];
        const int idx = pidx[(size_t)s * ncand + c];
        cval[c] = val;
        cidx[c] = val > -INFINITY ? idx : SEL_NONE;
    }
    __syncthreads();
    pick_from_list<64>(cval, cidx, ncand, width, red, redi, sel_v, sel_i);
    // the source beams' state goes to registers before the barrier, the slots are written after it
    const int idx = (tid < width && sel_i[tid] != SEL_NONE) ? sel_i[tid] : 0;
    const int b = first ? 0 : row0 + idx / V, v = idx % V;
    int st = 0;
    float len = 1.f;
    if (tid < width && !first) {
        st = stopped[s * beam + b];
        len = seq_len[s * beam + b] + (st ? 0.f : 1.f);
    }
    __syncthreads();
    if (tid < width) {
        const int o = s * beam + row0 + tid;
        beam_commit(o, sel_v[tid], b, v, first, stop_token, len, st, scores, seq_len, stopped, next_tok, src_row);
        if (picks) picks[o] = st ? PICK_NONE : v;
    }
}

__global__ __launch_bounds__(64) void k_beam_final(int beam, int V, int first, int stop_token, const float* __restrict__ pval,
                                                   const int* __restrict__ pidx, float* __restrict__ scores, float* __restrict__ seq_len,
                                                   unsigned char* __restrict__ stopped, int* __restrict__ next_tok, int* __restrict__ src_row) {
    beam_final_body(beam, 0, beam, V, first, stop_token, pval, pidx, scores, seq_len, stopped, next_tok, src_row, nullptr);
}

__global__ __launch_bounds__(64) void k_beam_group_final(int beam, int row0, int width, int V, int first, int stop_token, const float* __restrict__ pval,
                                                         const int* __restrict__ pidx, float* __restrict__ scores, float* __restrict__ seq_len,
                                                         unsigned char* __restrict__ stopped, int* __restrict__ next_tok, int* __restrict__ src_row,
                                                         int* __restrict__ picks) {
    beam_final_body(beam, row0, width, V, first, stop_token, pval, pidx, scores, seq_len, stopped, next_tok, src_row, picks);
}

// ---- beam step in ONE kernel, fed by the lm_head epilogue's partials (gemm.hip.h EpiLogits) ----------------------------------
// One block per sample.  The row statistics (max, sum of exp) come from the per-(row, 64-column block) partials — no pass over the
// logits; every 64-column block is bounded by the key of its maximum, the TB-th largest bound is a lower bound of the sample's TB-th
// best candidate, and only the blocks whose bound reaches it (a handful) are read from the logits matrix at all.  Same arithmetic
// (softmax().log() as the reference writes it), same tie rule (lowest flat index) and same state update as the three-kernel path,
// which stays as the fallback for temperature != 1, run-time beam widths and candidate-list overflow (e.g. all logits equal).
// This is the product's kernel (all but the first steps of a decode batch), and its compiled code is held fixed: routed through the
// shared pieces (select.hip.h block_argmax + record_pick, pick_from_list, kth_bound; BeamRow / beam_key / beam_val, beam_commit), each tried alone, every
// instantiation compiles differently (profiles/r12_a_beam_refactor.md), so it keeps these five idioms written out.  A change to the tie
// rule, the stopped-beam rule or the length normalisation is made in the shared pieces AND here.
template <int TB, int PER>      // PER: (row, block) partials per thread = ceil(TB * ceil(V / 64) / 256) at most (checked by the host)
__global__ __launch_bounds__(256) void k_beam_fused(const float* __restrict__ logits, size_t ldl, int V, int npart, const float* __restrict__ pmax,
                                                    const float* __restrict__ psum, int first, int stop_token, float* __restrict__ scores,
                                                    float* __restrict__ seq_len, unsigned char* __restrict__ stopped, int* __restrict__ next_tok,
                                                    int* __restrict__ src_row) {
    constexpr int FCAP = 1024, SCAP = 512;
    __shared__ float red[8];
    __shared__ int redi[8];
    __shared__ float rowred[4][TB];
    __shared__ float s_m[TB], s_lsum[TB], s_sum[TB], s_sc[TB], s_len[TB];
    __shared__ int s_st[TB];
    __shared__ float fcv[FCAP];
    __shared__ int fci[FCAP];
    __shared__ int surv[SCAP];
    __shared__ int fcount, scount;
    __shared__ float sel_v[TB];
    __shared__ int sel_i[TB];
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int nrows = first ? 1 : TB;
    const int nblk = (V + 63) >> 6;
    // 1. every partial of the sample's rows is requested up front (entry i = tid + 256 e: row i / nblk, block i % nblk) — one round trip
    //    instead of two dependent ones per row — and the row statistics m = max_j pmax, sum = sum_j psum exp(pmax - m) come from registers
    const int total = nrows * nblk;
    float pm[PER], ps[PER];
#pragma unroll
    for (int e = 0; e < PER; e++) {
        const int i = tid + 256 * e;
        const int b = min(i, total - 1) / nblk, j = min(i, total - 1) - b * nblk;
        const size_t at = (size_t)(s * TB + b) * npart + j;
        const float a = pmax[at], c = psum[at];
        pm[e] = i < total ? a : -INFINITY;
        ps[e] = i < total ? c : 0.f;
    }
    float lm[TB];
#pragma unroll
    for (int b = 0; b < TB; b++) lm[b] = -INFINITY;
#pragma unroll
    for (int e = 0; e < PER; e++) {
        const int b = min(tid + 256 * e, total - 1) / nblk;
#pragma unroll
        for (int q = 0; q < TB; q++) lm[q] = (q == b) ? fmaxf(lm[q], pm[e]) : lm[q];
    }
#pragma unroll
    for (int b = 0; b < TB; b++) {
        const float m = wave_max(lm[b]);
        if (lane == 0) rowred[wv][b] = m;
    }
    __syncthreads();
    float ls[TB];
#pragma unroll
    for (int b = 0; b < TB; b++) {
        lm[b] = fmaxf(fmaxf(rowred[0][b], rowred[1][b]), fmaxf(rowred[2][b], rowred[3][b]));
        ls[b] = 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < PER; e++) {
        const int b = min(tid + 256 * e, total - 1) / nblk;
        float mb = -INFINITY;
#pragma unroll
        for (int q = 0; q < TB; q++) mb = (q == b) ? lm[q] : mb;
        const float t = pm[e] != -INFINITY ? ps[e] * expf(pm[e] - mb) : 0.f;
#pragma unroll
        for (int q = 0; q < TB; q++) ls[q] += (q == b) ? t : 0.f;
    }
#pragma unroll
    for (int b = 0; b < TB; b++) {
        const float t = wave_sum(ls[b]);
        if (lane == 0) rowred[wv][b] = t;
    }
    __syncthreads();
    if (tid < nrows) {
        const int b = tid;
        const float t = (rowred[0][b] + rowred[1][b]) + (rowred[2][b] + rowred[3][b]);
        const bool st = !first && stopped[s * TB + b];
        float mb = -INFINITY;
#pragma unroll
        for (int q = 0; q < TB; q++) mb = (q == b) ? lm[q] : mb;
        s_m[b] = mb; s_sum[b] = t; s_lsum[b] = logf(t); s_st[b] = st;
        s_sc[b] = first ? 0.f : scores[s * TB + b];
        s_len[b] = first ? 1.f : (seq_len[s * TB + b] + (st ? 0.f : 1.f));
    }
    if (tid == 0) { fcount = 0; scount = 0; }
    __syncthreads();
    // cheap image of a candidate's value (monotone in the logit), and the exact value (base.py:96-101)
    auto key_of = [&](int b, int v, float x) -> float {
        if (s_st[b]) return v == 0 ? (first ? 0.f : (s_sc[b] + 0.f) / s_len[b]) : -INFINITY;
        const float d = (x - s_m[b]) - s_lsum[b];
        return first ? d : (s_sc[b] + d) * (1.0f / s_len[b]);
    };
    auto val_of = [&](int b, int v, float x) -> float {
        if (s_st[b]) return v == 0 ? (first ? 0.f : (s_sc[b] + 0.f) / s_len[b]) : -INFINITY;
        const float lp = logf(expf(x - s_m[b]) / s_sum[b]);
        return first ? lp : (s_sc[b] + lp) / s_len[b];
    };
    // 2. bound of every (row, block): key of the block maximum (a stopped row: only token 0, i.e. block 0)
    float bk[PER];
    float tmax = -INFINITY;
#pragma unroll
    for (int e = 0; e < PER; e++) {
        const int i = tid + 256 * e;
        const int b = min(i, total - 1) / nblk, j = min(i, total - 1) - b * nblk;
        const float k = s_st[b] ? (j == 0 ? key_of(b, 0, 0.f) : -INFINITY) : key_of(b, 1, pm[e]);
        bk[e] = i < total ? k : -INFINITY;
        tmax = fmaxf(tmax, bk[e]);
    }
    float thr = -INFINITY;
    for (int k = 0; k < TB; k++) {
        float bv = wave_max(tmax);
        if (lane == 0) red[(k & 1) * 4 + wv] = bv;
        __syncthreads();
        thr = fmaxf(fmaxf(red[(k & 1) * 4], red[(k & 1) * 4 + 1]), fmaxf(red[(k & 1) * 4 + 2], red[(k & 1) * 4 + 3]));
        if (tmax == thr) tmax = -INFINITY;            // equal maxima leave together: the bound only gets lower (still valid)
    }
    // 3. surviving blocks -> LDS list
#pragma unroll
    for (int e = 0; e < PER; e++) {
        if (bk[e] > -INFINITY && bk[e] + 1e-3f >= thr) {
            const int pos = atomicAdd(&scount, 1);
            if (pos < SCAP) surv[pos] = tid + 256 * e;
        }
    }
    __syncthreads();
    const int ns = scount;
    bool ok = ns <= SCAP;
    if (ok) {       // 4. one wave per surviving block: its 64 logits, exact values of the candidates within 1e-3 of the bound
        for (int q = wv; q < ns; q += 4) {
            const int i = surv[q], b = i / nblk, j = i - b * nblk, v = j * 64 + lane;
            if (v < V) {
                const float x = s_st[b] ? 0.f : logits[(size_t)(s * TB + b) * ldl + v];
                const float key = key_of(b, v, x);
                if (key > -INFINITY && key + 1e-3f >= thr) {
                    const int pos = atomicAdd(&fcount, 1);
                    if (pos < FCAP) { fcv[pos] = val_of(b, v, x); fci[pos] = b * V + v; }
                }
            }
        }
        __syncthreads();
        ok = fcount <= FCAP;
    }
    if (!ok) {
        // block-uniform overflow path (degenerate inputs, e.g. all logits equal): TB rounds of a full scan, each picking the best candidate
        // that comes strictly after the previous pick in the (value descending, flat index ascending) order.  Slow and exact.
        float pv = INFINITY;
        int pi = -1;
        for (int k = 0; k < TB; k++) {
            float bv = -INFINITY;
            int bi = 0x7fffffff;
            for (int b = 0; b < nrows; b++)
                for (int v = tid; v < V; v += 256) {
                    const float x = s_st[b] ? 0.f : logits[(size_t)(s * TB + b) * ldl + v];
                    const float val = val_of(b, v, x);
                    const int idx = b * V + v;
                    if ((pi < 0 || cand_better(pv, pi, val, idx)) && cand_better(val, idx, bv, bi)) { bv = val; bi = idx; }
                }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float ov = __shfl_xor(bv, o, 64);
                const int oi = __shfl_xor(bi, o, 64);
                if (cand_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
            }
            if (lane == 0) { red[(k & 1) * 4 + wv] = bv; redi[(k & 1) * 4 + wv] = bi; }
            __syncthreads();
            bv = red[(k & 1) * 4]; bi = redi[(k & 1) * 4];
#pragma unroll
            for (int w = 1; w < 4; w++) {
                const float ov = red[(k & 1) * 4 + w];
                const int oi = redi[(k & 1) * 4 + w];
                if (cand_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
            }
            pv = bv; pi = bi;
            if (tid == 0) { sel_v[k] = bi != 0x7fffffff ? bv : -INFINITY; sel_i[k] = bi; }
        }
        __syncthreads();
    }
    const int n = ok ? fcount : 0;
    for (int k = 0; ok && k < TB; k++) {      // 5. TB rounds of block arg-max over the list (ties -> lowest flat index)
        float bv = -INFINITY;
        int bi = 0x7fffffff;
        for (int c = tid; c < n; c += 256)
            if (fci[c] != 0x7fffffff && cand_better(fcv[c], fci[c], bv, bi)) { bv = fcv[c]; bi = fci[c]; }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (cand_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
        }
        if (lane == 0) { red[(k & 1) * 4 + wv] = bv; redi[(k & 1) * 4 + wv] = bi; }
        __syncthreads();
        bv = red[(k & 1) * 4]; bi = redi[(k & 1) * 4];
#pragma unroll
        for (int w = 1; w < 4; w++) {
            const float ov = red[(k & 1) * 4 + w];
            const int oi = redi[(k & 1) * 4 + w];
            if (cand_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
        }
        for (int c = tid; c < n; c += 256)
            if (fci[c] == bi) fci[c] = 0x7fffffff;
        if (tid == 0) { sel_v[k] = bi != 0x7fffffff ? bv : -INFINITY; sel_i[k] = bi; }
        __syncthreads();
    }
    if (tid < TB) {      // 6. gather / update state (base.py:86-119), as k_beam_final
        const int idx = sel_i[tid];
        const int b = idx / V, v = idx % V;
        float nl, nsc;
        int hs;
        if (first) { nl = 1.f; nsc = sel_v[tid]; hs = 0; }
        else {
            nl = s_len[b];                          // = seq_len[b] + (stopped ? 0 : 1), read before any state was written
            nsc = sel_v[tid] * nl;                  // scores = scores_sum_average * seq_lengths (base.py:114)
            hs = s_st[b];
        }
        hs |= (v == stop_token) ? 1 : 0;
        next_tok[s * TB + tid] = v;
        src_row[s * TB + tid] = b;
        scores[s * TB + tid] = nsc;
        seq_len[s * TB + tid] = nl;
        stopped[s * TB + tid] = (unsigned char)hs;
    }
}

// ---- host side of the three-kernel path ----------------------------------------------------------------------------------------------
// Workspace: row statistics [S * beam][2] | chunk winners of ONE selection of `width` rows (values, then flat indices) | beam groups only:
// this step's picks [S * beam].  The plain update selects from all `beam` rows at once and keeps no picks (picks = null).
struct BeamWs {
    float *rs, *pval;
    int *pidx, *picks;
};
BeamWs beam_ws(void* ws, int S, int beam, int width, bool picks) {
    BeamWs w;
    w.rs = static_cast<float*>(ws);
    w.pval = w.rs + (size_t)S * beam * 2;
    w.pidx = reinterpret_cast<int*>(w.pval + (size_t)S * BEAM_CHUNKS * width);
    w.picks = picks ? w.pidx + (size_t)S * BEAM_CHUNKS * width : nullptr;
    return w;
}
int64_t beam_ws_bytes(int S, int beam, int width, bool picks) {
    return (int64_t)S * beam * 2 * sizeof(float) + (int64_t)S * BEAM_CHUNKS * width * (sizeof(float) + sizeof(int)) +
           (picks ? (int64_t)S * beam * sizeof(int) : 0) + 512;
}

// partial + final for rows [row0, row0 + width) of every sample.  w.picks null: the plain kernels (row0 = 0, width = beam); else a beam group.
void launch_select(hipStream_t st, int S, int beam, int row0, int width, int V, const float* logits, int64_t ldl, float inv_temp, float penalty, int first,
                   int stop_token, const BeamWs& w, float* scores, float* seq_lengths, uint8_t* has_stopped, int32_t* next_tokens, int32_t* src_rows) {
#define BEAM_PARTIAL(TW)                                                                                                                              \
    do {                                                                                                                                              \
        if (w.picks)                                                                                                                                  \
            hipLaunchKernelGGL(k_beam_group_partial<TW>, dim3(S, BEAM_CHUNKS), dim3(256), 0, st, logits, (size_t)ldl, beam, row0, width, V, inv_temp, \
                               penalty, first, w.rs, scores, seq_lengths, has_stopped, w.picks, w.pval, w.pidx);                                     \
        else                                                                                                                                          \
            hipLaunchKernelGGL(k_beam_partial<TW>, dim3(S, BEAM_CHUNKS), dim3(256), 0, st, logits, (size_t)ldl, beam, V, inv_temp, first, w.rs,      \
                               scores, seq_lengths, has_stopped, w.pval, w.pidx);                                                                    \
    } while (0)
    switch (width) {
        case 1: BEAM_PARTIAL(1); break;
        case 2: BEAM_PARTIAL(2); break;
        case 3: BEAM_PARTIAL(3); break;
        case 4: BEAM_PARTIAL(4); break;
        case 5: BEAM_PARTIAL(5); break;
        case 8: BEAM_PARTIAL(8); break;
        default: BEAM_PARTIAL(0); break;
    }
#undef BEAM_PARTIAL
    if (w.picks)
        hipLaunchKernelGGL(k_beam_group_final, dim3(S), dim3(64), 0, st, beam, row0, width, V, first, stop_token, w.pval, w.pidx, scores, seq_lengths,
                           has_stopped, next_tokens, src_rows, w.picks);
    else
        hipLaunchKernelGGL(k_beam_final, dim3(S), dim3(64), 0, st, beam, V, first, stop_token, w.pval, w.pidx, scores, seq_lengths, has_stopped,
                           next_tokens, src_rows);
}

}  // namespace

extern "C" {

int64_t CC_API(cc_beam_ws_bytes)(int32_t S, int32_t beam, int32_t V) {
    (void)V;
    if (S <= 0 || beam <= 0 || beam > BEAM_MAX) return CC_ERR_SHAPE;
    return beam_ws_bytes(S, beam, beam, false);
}

int CC_API(cc_beam_step_p)(int32_t S, int32_t beam, int32_t V, const float* logits, int64_t ldl, const float* lpart, int32_t npart, float temperature,
                   int32_t first, int32_t stop_token, float* scores, float* seq_lengths, uint8_t* has_stopped, int32_t* next_tokens,
                   int32_t* src_rows, void* ws, void* stream);

int CC_API(cc_beam_step)(int32_t S, int32_t beam, int32_t V, const float* logits, int64_t ldl, float temperature, int32_t first, int32_t stop_token,
                 float* scores, float* seq_lengths, uint8_t* has_stopped, int32_t* next_tokens, int32_t* src_rows, void* ws, void* stream) {
    return CC_API(cc_beam_step_p)(S, beam, V, logits, ldl, nullptr, 0, temperature, first, stop_token, scores, seq_lengths, has_stopped, next_tokens,
                                  src_rows, ws, stream);
}

int CC_API(cc_beam_step_p)(int32_t S, int32_t beam, int32_t V, const float* logits, int64_t ldl, const float* lpart, int32_t npart, float temperature,
                   int32_t first, int32_t stop_token, float* scores, float* seq_lengths, uint8_t* has_stopped, int32_t* next_tokens,
                   int32_t* src_rows, void* ws, void* stream) {
    if (S <= 0 || beam <= 0 || beam > BEAM_MAX || V <= 0 || !logits || ldl < V || !scores || !seq_lengths || !has_stopped || !next_tokens ||
        !src_rows || !ws || (lpart && npart * 64 < V))
        return CC_ERR_ARG;
    hipStream_t st = S_(stream);
    // partials from the lm_head epilogue (cc_decode_fwd_p), temperature 1: the whole update in one launch (k_beam_fused)
    constexpr int FUSED_VMAX = 51200;      // the fused kernel's per-thread register image of the partials is sized for vocabularies up to this
    if (lpart && (temperature <= 0.f || temperature == 1.0f) && (beam <= 5 || beam == 8) && V <= FUSED_VMAX) {
        const float* pmax = lpart;
        const float* psum = lpart + (size_t)S * beam * npart;
#define BEAM_FUSED(TB) hipLaunchKernelGGL((k_beam_fused<TB, (TB * (FUSED_VMAX / 64) + 255) / 256>), dim3(S), dim3(256), 0, st, logits, (size_t)ldl, V, npart, pmax, psum, first, stop_token, scores, seq_lengths, has_stopped, next_tokens, src_rows)
        switch (beam) {
            case 1: BEAM_FUSED(1); break;
            case 2: BEAM_FUSED(2); break;
            case 3: BEAM_FUSED(3); break;
            case 4: BEAM_FUSED(4); break;
            case 5: BEAM_FUSED(5); break;
            default: BEAM_FUSED(8); break;
        }
#undef BEAM_FUSED
        return hipGetLastError() == hipSuccess ? CC_OK : CC_ERR_LAUNCH;
    }
    const float inv_temp = 1.0f / (temperature > 0.f ? temperature : 1.0f);   // base.py:83
    const BeamWs w = beam_ws(ws, S, beam, beam, false);
    // step 0 reads only row 0 of every sample's block of `beam` rows, but computing all rows' statistics is harmless and uniform
    launch_rowstats(st, logits, ldl, S * beam, V, inv_temp, w.rs);
    launch_select(st, S, beam, 0, beam, V, logits, ldl, inv_temp, 0.f, first, stop_token, w, scores, seq_lengths, has_stopped, next_tokens, src_rows);
    return hipGetLastError() == hipSuccess ? CC_OK : CC_ERR_LAUNCH;
}

int64_t CC_API(cc_beam_group_ws_bytes)(int32_t S, int32_t beam, int32_t groups, int32_t V) {
    (void)V;
    if (S <= 0 || beam <= 0 || beam > BEAM_MAX || groups < 1 || beam % groups) return CC_ERR_SHAPE;
    return beam_ws_bytes(S, beam, beam / groups, true);
}

int CC_API(cc_beam_group_step)(int32_t S, int32_t beam, int32_t groups, int32_t V, const float* logits, int64_t ldl, float temperature,
                               float diversity_penalty, int32_t first, int32_t stop_token, float* scores, float* seq_lengths, uint8_t* has_stopped,
                               int32_t* next_tokens, int32_t* src_rows, void* ws, void* stream) {
    if (S < 0 || beam <= 0 || beam > BEAM_MAX || groups < 1 || beam % groups || V <= 0 || !logits || ldl < V || !scores || !seq_lengths ||
        !has_stopped || !next_tokens || !src_rows || !ws || !(diversity_penalty >= 0.f && diversity_penalty <= 3.402823466e38f))
        return CC_ERR_ARG;
    if (S == 0) return CC_OK;
    hipStream_t st = S_(stream);
    const int width = beam / groups;
    const float inv_temp = 1.0f / (temperature > 0.f ? temperature : 1.0f);   // base.py:83
    const BeamWs w = beam_ws(ws, S, beam, width, true);
    launch_rowstats(st, logits, ldl, S * beam, V, inv_temp, w.rs);
    for (int g = 0; g < groups; g++)
        launch_select(st, S, beam, g * width, width, V, logits, ldl, inv_temp, diversity_penalty, first, stop_token, w, scores, seq_lengths,
                      has_stopped, next_tokens, src_rows);
    return hipGetLastError() == hipSuccess ? CC_OK : CC_ERR_LAUNCH;
}

}  // extern "C"
