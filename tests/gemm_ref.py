"""float64 reference of what the GEMM wrappers of clipcap_amd/csrc/gemm_api.h compute, and the error bounds the GPU tests hold them to
(tests/test_gpu_gemm_epilogues.py).  Plain torch, no GPU needed; tests/test_gemm_ref.py pins this module itself.

Everything is written from the definitions in clipcap_amd/csrc/common.hip.h (x3_pair8 / x3_store, gelu_new, the dropout mask), not from what the
kernels return:
  * split-bf16 operands: hi = bf16(x), lo = bf16(x - hi) (x - hi is exact in fp32); A image [hi | hi | lo], B image [hi | lo | hi];
  * gelu_new(x) = x s, s = 1 / (1 + exp(-2 k0 (x + k1 x^3))); gelu_new'(x) = s + x s (1 - s) 2 k0 (1 + 3 k1 x^2);
  * residual dropout: out = res + m * scale * (acc + bias), m the keep flag, scale = 1 / (1 - p) (as a float32, like make_drop).

Rounding model behind the bounds.  u32 = 2^-24, u_bf16 = 2^-8, u_fp16 = 2^-11 (unit roundoffs).  Products of two 16-bit operands are
exact in fp32, so before the epilogue the only error is the fp32 accumulation: every rounding on the way to one output is at most
u32 times a partial sum, and no partial sum exceeds S = sum |terms|.  One MFMA step (MFMA_DEPTH products added to the accumulator) is
modelled as ONE rounding; how many roundings the hardware really spends inside a step is not documented, so the step count is
multiplied by MFMA_ROUNDINGS, a measured allowance (see there).  acc_bound = (steps * MFMA_ROUNDINGS + extra) * u32 * S, with `extra`
the cross-wave / K-slice additions of the kernel that ran (chain_steps)."""
import functools
import math

import torch

U32 = 2.0 ** -24
U_BF16 = 2.0 ** -8
U_FP16 = 2.0 ** -11
FP16_SUBNORMAL_HALF = 2.0 ** -25      # half the spacing of fp16 subnormals: the absolute rounding error below 2^-14
K0, K1 = 0.7978845608028654, 0.044715

# ---- measured allowances (MI355X, against this module's float64; 4 x the worst value seen) --------------------
# Re-measure with `pytest tests/test_gpu_gemm_epilogues.py -m gpu -s -k test_measured_allowances`: it prints every raw figure below.
# One MFMA step against the exact sum of its products (single-step GEMMs: K = 32 on v_mfma_f32_16x16x32, zero accumulator, bf16 and
# fp16, five tile kernels, three shapes): worst |err| / (u32 * S) = 1.62.  A single correctly rounded sum would stay below 1: the
# instruction rounds (or truncates) more than once inside a step.  4 x 1.62 = 6.5 roundings allowed per step.
MFMA_ROUNDINGS = 6.5
# Device gelu_new / gelu_new' (v_exp_f32 + v_rcp_f32 in fp32, common.hip.h) against float64 on the same fp32 argument, measured in the
# split-bf16 build where argument and result cross the ABI as fp32 (|x| up to 34):
#   |gelu_dev(x) - gelu(x)| / (u32 * |x|)  worst seen 2.54  -> allowance 10.2
#   |gelu'_dev(x) - gelu'(x)| / u32        worst seen 33.07 (gelu_new_both and gelu_new_grad alike) -> allowance 132.3
# The derivative's 33 u32 (2e-6 absolute) is the cancellation in s (1 - s), evaluated as s - s * s, where s is within a few ulps of 1
# (|x| around 5) and the factor x * d(2u)/dx in front of it is about 35.
GELU_ULPS = 10.2
GELU_GRAD_ULPS = 132.3


# ---- split-bf16 operands ------------------------------------------------------------------------------------------------------------
def split(x):
    """fp32 tensor -> (hi, lo) as bfloat16 tensors, the library's split."""
    assert x.dtype == torch.float32
    hi = x.to(torch.bfloat16)
    lo = (x - hi.float()).to(torch.bfloat16)
    return hi, lo


def image(x, form):
    """fp32 [rows][K] -> bfloat16 [rows][3 K]: form 0 = [hi | hi | lo] (A side), form 1 = [hi | lo | hi] (B side)."""
    hi, lo = split(x)
    return torch.cat([hi, hi, lo] if form == 0 else [hi, lo, hi], dim=1).contiguous()


def unimage(img, form):
    """inverse of image(): (hi, lo, copy) with `copy` the second hi plane (must equal hi)."""
    K = img.shape[1] // 3
    a, b, c = img[:, :K], img[:, K:2 * K], img[:, 2 * K:]
    return (a, c, b) if form == 0 else (a, b, c)


def three_term(ahi, alo, bhi, blo):
    """float64 hi*hi + hi*lo + lo*hi of A [M][K] and B [N][K]: what the NT kernels sum over K' = 3K.  Returns (value, sum of |terms|)."""
    ah, al_, bh, bl_ = ahi.double(), alo.double(), bhi.double(), blo.double()
    v = ah @ bh.t() + ah @ bl_.t() + al_ @ bh.t()
    s = ah.abs() @ bh.abs().t() + ah.abs() @ bl_.abs().t() + al_.abs() @ bh.abs().t()
    return v, s


def split_product_bound(sabs):
    """|hh + hl + lh - a b| <= 3 u^2 sum |a||b|: a = hi + lo + e with |lo| <= u |a|, |e| <= u^2 |a|; the dropped lo*lo term is u^2, the two
    representation errors u^2 (1 + u) each."""
    return 3.0 * U_BF16 ** 2 * sabs


# ---- activations -------------------------------------------------------------------------------------------------------------------
def _sig(x):
    return 1.0 / (1.0 + torch.exp(-2.0 * K0 * (x + K1 * x ** 3)))


def gelu_new(x):
    x = x.double()
    return x * _sig(x)


def gelu_new_grad(x):
    x = x.double()
    s = _sig(x)
    return s + x * s * (1.0 - s) * 2.0 * K0 * (1.0 + 3.0 * K1 * x * x)


def relu(x):
    return torch.clamp_min(x.double(), 0.0)


@functools.lru_cache(maxsize=None)
def gelu_lipschitz():
    """(max |gelu_new'|, max |gelu_new''|) over the reals, from this module's float64 functions on a fine grid (both decay to 1 / 0 outside
    [-8, 8]); the second derivative by central differences of the first, rounded up by the grid's own resolution."""
    x = torch.linspace(-8.0, 8.0, 1_600_001, dtype=torch.float64)
    g1 = gelu_new_grad(x)
    h = (x[1] - x[0]).item()
    g2 = (g1[2:] - g1[:-2]) / (2 * h)
    return g1.abs().max().item() * (1 + 1e-6), g2.abs().max().item() * (1 + 1e-4)


def resid_drop(res, acc, bias, keep, p):
    """out = res + m * scale * (acc + bias) in float64; keep = uint8 / bool flags or None (dropout off)."""
    y = acc.double() + (bias.double() if bias is not None else 0.0)
    if keep is not None:
        scale = float(torch.tensor(1.0, dtype=torch.float32) / (torch.tensor(1.0, dtype=torch.float32) - torch.tensor(p, dtype=torch.float32)))
        y = y * keep.double() * scale
    return res.double() + y


# ---- accumulation chain ------------------------------------------------------------------------------------------------------------
# constants of clipcap_amd/csrc/gemm.hip.h: the tile kernels run v_mfma_f32_16x16x32 (32 products per step), the 64-row skinny kernels
# v_mfma_f32_32x32x16 (16 per step); skinny modes 3 / 4 split each 64-deep K tile over 4 waves and add the 4 partial tiles afterwards, the
# 8-wave 128 x 128 form splits it over 2 wave groups and adds once; K slices (ksplit) meet in fp32 atomics, one addition per slice.
MFMA_DEPTH_TILE = 32
MFMA_DEPTH_SKINNY = 16
G_BK = 64


def chain_steps(kp, skinny_mode=0, M=0, ksplit=1):
    """(MFMA steps, other fp32 additions) on the longest chain to one output of an NT launch over kp = K (16-bit builds) or 3 K (split-bf16)
    products.  The skinny kernels take a launch only when kp % 64 == 0 and M <= 1024 (launch_gemm)."""
    if skinny_mode > 0 and kp % G_BK == 0 and M <= 1024:
        if skinny_mode >= 3:      # K over 4 waves: a wave runs one 16-deep step per 64-deep tile, then 3 additions across the waves
            return kp // G_BK, 3 + ksplit
        return kp // MFMA_DEPTH_SKINNY, ksplit
    return -(-kp // MFMA_DEPTH_TILE), 1 + ksplit      # (+1: the wave-group exchange of the 8-wave form, when that is the kernel)


def acc_bound(sabs, kp, skinny_mode=0, M=0, ksplit=1, extra=0):
    steps, adds = chain_steps(kp, skinny_mode, M, ksplit)
    return (steps * MFMA_ROUNDINGS + adds + extra) * U32 * sabs


def u_out(dtype):
    return {torch.bfloat16: U_BF16, torch.float16: U_FP16, torch.float32: 0.0}[dtype]


def store_bound(ref, err_before, dtype):
    """bound after rounding a value with error `err_before` to the stored type: u |ref| + (1 + u) err (+ fp16 subnormal spacing)."""
    u = u_out(dtype)
    b = u * ref.abs() + (1.0 + u) * err_before
    if dtype == torch.float16:
        b = b + FP16_SUBNORMAL_HALF
    return b


def frobenius_threshold(correct, defects):
    """Where the relative-Frobenius check sits: the geometric mean of the float64 emulation of the correct three-term result's distance
    from the exact product and of the nearest emulated defect's."""
    d = min(defects)
    assert correct * 4 < d, (correct, d)      # the emulation itself must separate them, else the check says nothing
    return math.sqrt(correct * d)
