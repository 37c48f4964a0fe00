"""float64 reference of the MLP mapping network (include/clipcap_hip.h cc_mlp_*, clipcap_amd/csrc/mlp.hip) and of its tanh GEMM epilogue
(gemm.hip.h EpiTanh), written from the definitions, not from what the kernels return.  Plain torch, no GPU needed; tests/test_mlp_ref.py
pins this module itself.

    x16 = cast(emb)                    h = cast(tanh(u)),  u = x16 W1^T + b1        t = cast(1 - tanh(u)^2)
    out = h W2^T + b2                  (fp32, viewed [B][L][D])
    g16 = cast(dout)                   db2 = sum_b dout (fp32)                       dW2 = g16^T h
    dU  = cast((g16 W2) * t)           dW1 = dU^T x16                                db1 = column sums of dU

`cast` rounds to the operand type (bf16 / fp16); in the split-bf16 build activations stay fp32 and every GEMM operand is worth
hi + lo (tests/gemm_ref.py split / three_term).  The stage functions below take the DEVICE's own upstream values, so each stage is held
to its own bound: the accumulation bound of gemm_ref.acc_bound over the stage's products, one 2^-24 rounding per epilogue operation, the
store bound of the stage's type.  Lipschitz constants: tanh has 1; 1 - tanh^2 has max |2 tanh sech^2| = 4 / (3 sqrt 3), reached at
tanh^2 = 1 / 3."""
import math

import torch

from tests import gemm_ref as R

# ---- measured allowances (MI355X, against float64 on the same fp32 argument, split-bf16 build where argument and result cross the ABI
# as fp32; a grid over [-20, 20] plus the inputs of tests/test_gpu_gemm_tanh.py; 4 x the worst value seen) -------
# Re-measure with `pytest tests/test_gpu_gemm_tanh.py -m gpu -s -k test_measured_allowances`.
#   |tanh_dev(u) - tanh(u)| / u32              worst seen 2.079 (on the grid; the GEMM inputs 2.041)  -> allowance 4 x 2.08 = 8.32
#   |t_dev(u) - (1 - tanh(u)^2)| / u32         worst seen 3.994 (on the grid; the GEMM inputs 3.930)  -> allowance 4 x 4.00 = 16.0
#                                              (t = 1 - h h from the fp32 h: twice h's error, |h| <= 1, plus one rounding)
# A raw figure above 33 u32 (the worst the existing transcendental epilogue shows, gemm_ref.GELU_GRAD_ULPS' raw figure) would be a defect
# of tanh_f, not an allowance to record.
TANH_RAW = 2.08
TANH_GRAD_RAW = 4.00
TANH_ULPS = 4 * TANH_RAW
TANH_GRAD_ULPS = 4 * TANH_GRAD_RAW
RAW_LIMIT = 33.0

TANH_LIP = 1.0
TANH_GRAD_LIP = 4.0 / (3.0 * math.sqrt(3.0))

DTYPES = {0: torch.bfloat16, 1: torch.float16, 2: torch.float32}      # stored activation type per operand mode


def tanh(x):
    """(1 - e) / (1 + e), e = exp(-2 |x|), sign restored: float64, exactly +-1 from |x| ~ 19, no overflow anywhere."""
    x = x.double()
    e = torch.exp(-2.0 * x.abs())
    return torch.copysign((1.0 - e) / (1.0 + e), x)


def tanh_grad(x):
    """1 - tanh^2 = 4 e / (1 + e)^2: no cancellation near saturation."""
    e = torch.exp(-2.0 * x.double().abs())
    return 4.0 * e / (1.0 + e) ** 2


def cast(x, dt):
    """the stored value of an activation: rounded to the 16-bit type, or the fp32 value itself (split-bf16 build)"""
    return x.float().to(dt)


def nt(a, w32, dt):
    """A [M][K] (stored activations, dtype dt) times W [N][K]^T (fp32 master) as the kernels multiply them.
    Returns (float64 value, sum of |terms|, products per output)."""
    if dt == torch.float32:
        v, s = R.three_term(*R.split(a.float().contiguous()), *R.split(w32.float().contiguous()))
        return v, s, 3 * a.shape[1]
    a64, w64 = a.double(), w32.to(dt).double()
    return a64 @ w64.t(), a64.abs() @ w64.abs().t(), a.shape[1]


def tn(x, y, dt):
    """X [K][Mw]^T Y [K][Nw] (both stored activations): the weight-gradient product.  Same return as nt()."""
    if dt == torch.float32:
        xh, xl = R.split(x.float().contiguous())
        yh, yl = R.split(y.float().contiguous())
        v, s = R.three_term(xh.t(), xl.t(), yh.t(), yl.t())
        return v, s, 3 * x.shape[0]
    x64, y64 = x.double(), y.double()
    return x64.t() @ y64, x64.abs().t() @ y64.abs(), x.shape[0]


def wgrad_bound(s, kp, ref, before):
    """gemm_wgrad: the MFMA steps over kp products, one addition per K slice in a slab fold (a slice is at least 256 deep), then one
    rounding for the addition into dW (tests/test_gpu_gemm_epilogues.py test_x3_wgrad's chain)."""
    chain = (-(-kp // R.MFMA_DEPTH_TILE)) * R.MFMA_ROUNDINGS + -(-kp // 256)
    return chain * R.U32 * s + R.U32 * (ref.abs() + before.abs())


def prefix(p, emb, L, pre="", rb=False):
    """differentiable forward for the model tests, (B, L, D): torch autograd through the oracle's rounding points (oracle.clipcap_oracle._r;
    rb False = plain, True = bf16, "fp16")"""
    from oracle.clipcap_oracle import _r
    u = _r(emb, rb) @ _r(p[pre + "model.0.weight"], rb).t() + p[pre + "model.0.bias"]
    h = _r(torch.tanh(u), rb)
    out = h @ _r(p[pre + "model.2.weight"], rb).t() + p[pre + "model.2.bias"]
    return out.view(emb.shape[0], L, -1)
