#include "gemm.hip.h"
#include "gemm_api.h"
namespace CC_NS {
// the tile comes from the planner with the traits gemm_bf16out's functors have (no row strip, no aux, not K-sliced): the same shape gets the same form
int gemm_tanh(int al, int bl, ActIn A, int lda, const op16_t* B, int ldb, int M, int N, int K, Act Co, int ldc,
              const float* bias, act_t* pre, bool pre_nt, Call& cx) {
    const hipStream_t st = cx.st;
    cc_shared::ProfScope _all(cc_shared::SITE_ALL_GEMMS, st, 2.0 * M * N * (double)K);
    if ((ldc & 7) || (N & 7)) return CC_ERR_SHAPE;
    const op16_t* A16;
    const int rca = nt_operand(cx, A, al, bl, M, lda, ldb, K, A16);
    if (rca != CC_OK) return rca;
    EpiTanh e{Co.p, pre, bias, ldc, M, N};
    e.pre_nt = pre_nt;
    e.img = Co.img;
    return launch_gemm(al, bl, A16, lda, B, ldb, M, N, K, 1, e, st);
}
}  // namespace CC_NS
