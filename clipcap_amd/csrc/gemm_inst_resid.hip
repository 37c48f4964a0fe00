#include "gemm.hip.h"
#include "gemm_api.h"
namespace CC_NS {
int gemm_resid(int al, int bl, ActIn A, int lda, const op16_t* B, int ldb, int M, int N, int K, float* out, const float* res,
               int ld, const float* bias, Call& cx, Drop drop) {
    const hipStream_t st = cx.st;
    cc_shared::ProfScope _all(cc_shared::SITE_ALL_GEMMS, st, 2.0 * M * N * (double)K);
    if ((ld & 7) || (N & 7)) return CC_ERR_SHAPE;
    const op16_t* A16;
    const int rca = nt_operand(cx, A, al, bl, M, lda, ldb, K, A16);
    if (rca != CC_OK) return rca;
    EpiResid e{out, res, bias, ld, M, N, drop};
    e.acc_init = cc_plan::pick_resid_init(drop.thresh != 0, cc_plan::gemm_knobs());
    return launch_gemm(al, bl, A16, lda, B, ldb, M, N, K, 1, e, st);
}
}  // namespace CC_NS
