#include "gemm.hip.h"
#include "gemm_api.h"
namespace CC_NS {
int gemm_lmhead(ActIn A, int lda, const op16_t* B, int ldb, int M, int Vp, int V, int K, Act Co, int ldc, float* pmax,
                float* psum, int npart, const int* target, float* tgt_logit, Call& cx, const float* cref) {
    const hipStream_t st = cx.st;
    act_t* const C = Co.p;
    cc_shared::ProfScope _all(cc_shared::SITE_ALL_GEMMS, st, 2.0 * M * V * (double)K);
    if ((ldc & 63) || ldc < Vp || npart * 64 < Vp) return CC_ERR_SHAPE;
    const op16_t* A16;
    const int rca = nt_operand(cx, A, 0, 0, M, lda, ldb, K, A16);
    if (rca != CC_OK) return rca;
    if (cref) {      // exponential form: the caller takes the target logit from cref itself (tgt_logit unused)
        EpiLMHeadExp e{C, pmax, psum, cref, ldc, M, V, npart};
        e.img = Co.img;      // frozen-LM runs: E goes out as the input-gradient GEMM's operand image
        return launch_gemm(0, 0, A16, lda, B, ldb, M, Vp, K, 1, e, st);
    }
    EpiLMHead e{C, pmax, psum, target, tgt_logit, ldc, M, V, npart};
    return launch_gemm(0, 0, A16, lda, B, ldb, M, Vp, K, 1, e, st);
}
int gemm_lmhead_score(ActIn A, int lda, const op16_t* B, int ldb, int M, int Vp, int V, int K, float* pmax, float* psum, int npart,
                      const int* target, float* tgt_logit, Call& cx) {
    const hipStream_t st = cx.st;
    cc_shared::ProfScope _all(cc_shared::SITE_ALL_GEMMS, st, 2.0 * M * V * (double)K);
    if ((Vp & 63) || V > Vp || npart * 64 < Vp) return CC_ERR_SHAPE;
    const op16_t* A16;
    const int rca = nt_operand(cx, A, 0, 0, M, lda, ldb, K, A16);
    if (rca != CC_OK) return rca;
    EpiLMHeadScore e{pmax, psum, target, tgt_logit, M, Vp, V, npart};
    return launch_gemm(0, 0, A16, lda, B, ldb, M, Vp, K, 1, e, st);
}
int gemm_logits_part(ActIn A, int lda, const op16_t* B, int ldb, int M, int Ns, int V, int K, float* C, int ldc, float* pmax, float* psum,
                     int npart, Call& cx) {
    const hipStream_t st = cx.st;
    cc_shared::ProfScope _all(cc_shared::SITE_ALL_GEMMS, st, 2.0 * M * V * (double)K);
    if ((ldc & 3) || (Ns & 7) || npart * 64 < Ns) return CC_ERR_SHAPE;
    const op16_t* A16;
    const int rca = nt_operand(cx, A, 0, 0, M, lda, ldb, K, A16);
    if (rca != CC_OK) return rca;
    EpiLogits e{C, pmax, psum, ldc, M, Ns, V, npart};
    return launch_gemm(0, 0, A16, lda, B, ldb, M, Ns, K, 1, e, st);
}
}  // namespace CC_NS
