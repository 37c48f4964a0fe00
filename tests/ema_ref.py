"""The weight average of the AdamW step, stated once in float64, and the bound one fp32 update is held to.

Semantics (clipcap_amd.engine._Arena.adamw_step(ema_decay=...), cc_adamw_step_ema):
    ema_0 = p_0                                          (the master when the average is enabled)
    ema_t = d_t * ema_{t-1} + (1 - d_t) * p_t            after every APPLIED optimizer step t, p_t = what that step wrote
    a step the loss scaler skips leaves ema untouched
    d_t = decay, or with warm-up min(decay, (1 + t) / (10 + t)), t = the host's 1-based count of optimizer steps
so after T steps at a constant d:  ema_T = d^T p_0 + (1 - d) sum_{t=1..T} d^(T-t) p_t.

The bound.  The kernel evaluates, in fp32 (unit roundoff u = 2^-24, round to nearest), with d an fp32 host scalar,
    w = fl(1 - d)                     w = (1 - d)(1 + a),          |a| <= u
    x = fl(d * e)                     x = d e (1 + b),             |b| <= u
    r = fl(x + fl(w * p))             r = (x + w p (1 + c))(1 + g), |c|, |g| <= u
or with the products contracted into FMAs one rounding fewer (fma(w, p, x) has no c; fma(d, e, fl(w p)) has no b), so the separate
form is the worse case.  With exact value y = d e + (1 - d) p and m = max(|e|, |p|), 0 <= d < 1:
    r - y = d e b + (1 - d) p (a + c + a c) + g (x + w p (1 + c))
    |r - y| <= u d m + (2u + u^2)(1 - d) m + u (1 + u)^2 (d m + (1 - d) m)
            <= u m (d + 2 (1 - d) + 1) + O(u^2) m  =  u m (3 - d) + O(u^2) m  <=  3 u m + 4 u^2 m  <  4 u m.
Hence EMA_ULPS = 4: three roundings on the worst path plus the rounding of 1 - d, with room for the second-order terms, FMA or not.
The statement assumes no intermediate underflows into the subnormal range (|d e|, |w p| >= 2^-126 or zero), which holds for every
input the tests use (magnitudes in [2^-60, 2^60] or exactly 0) and for any trained weight.  d = 0: w = 1, x = +-0, r = p exactly for
finite e — `ema == p` as numbers (the sign of a zero may differ).

The lerp form e + (1 - d)(p - e) is NOT what the kernel computes: p - e overflows for e = -p near the top of the range, and at d = 0
it returns e + fl(p - e), which is p only when the subtraction is exact.
"""
import torch

EMA_ULPS = 4
U = 2.0 ** -24


def warmup_decay(decay: float, t: int, warmup: bool = True) -> float:
    """d_t of optimizer step t (1-based host count)"""
    return min(decay, (1.0 + t) / (10.0 + t)) if warmup else decay


def ema_update64(ema: torch.Tensor, p: torch.Tensor, d: float) -> torch.Tensor:
    """one update in float64 with the decay the kernel receives: d rounded to fp32 (the exact 1 - d of THAT number is the reference;
    the kernel's rounding of 1 - d is part of the bound)"""
    d32 = float(torch.tensor(d, dtype=torch.float32))
    return d32 * ema.double() + (1.0 - d32) * p.double()


def ema_bound(ema: torch.Tensor, p: torch.Tensor) -> torch.Tensor:
    """per-element bound on |fp32 update - ema_update64|"""
    return EMA_ULPS * U * torch.maximum(ema.double().abs(), p.double().abs())


def ema_closed_form64(p0: torch.Tensor, ps, d: float) -> torch.Tensor:
    """d^T p_0 + (1 - d) sum_t d^(T-t) p_t in float64, ps = [p_1, ..., p_T]"""
    T = len(ps)
    out = (d ** T) * p0.double()
    for t, p in enumerate(ps, start=1):
        out = out + (1.0 - d) * (d ** (T - t)) * p.double()
    return out


def ema_convex_f32(ema: torch.Tensor, p: torch.Tensor, d: float) -> torch.Tensor:
    """the kernel's arithmetic restated in torch fp32: d * e + (1 - d) * p with 1 - d formed in fp32"""
    d32 = torch.tensor(d, dtype=torch.float32)
    w = torch.tensor(1.0, dtype=torch.float32) - d32
    return d32 * ema.float() + w * p.float()


def assert_ema_step(new_ema: torch.Tensor, old_ema: torch.Tensor, p: torch.Tensor, d: float, what: str = "") -> float:
    """new_ema (fp32, from the device) is one update of old_ema with p at decay d, within the bound; returns the worst error / bound"""
    ref = ema_update64(old_ema.cpu(), p.cpu(), d)
    err = (new_ema.cpu().double() - ref).abs()
    bound = ema_bound(old_ema.cpu(), p.cpu())
    ok = err <= bound
    assert bool(ok.all()), (what, int((~ok).sum()), float(err.max()), float(bound.max()))
    nz = bound > 0
    return float((err[nz] / bound[nz]).max()) if bool(nz.any()) else 0.0
