"""CPU tests of tests/ema_ref.py: the recurrence against its closed form, the warm-up schedule's first values, and the fp32 convex form
inside the stated bound on random and on adversarial inputs (which the lerp form misses)."""
import pytest
import torch

from tests import ema_ref as R


@pytest.mark.parametrize("d", [0.0, 0.5, 0.9, 0.9999])
def test_recurrence_equals_the_closed_form(d):
    g = torch.Generator().manual_seed(1)
    p0 = torch.randn(257, generator=g, dtype=torch.float64)
    ps = [p0 + 0.01 * (t + 1) * torch.randn(257, generator=g, dtype=torch.float64) for t in range(12)]
    ema = p0.clone()
    for p in ps:
        ema = d * ema + (1.0 - d) * p
    ref = R.ema_closed_form64(p0, ps, d)
    assert float((ema - ref).abs().max()) <= 1e-13 * float(ref.abs().max())
    # ema_update64 is that recurrence at the fp32-rounded decay
    d32 = float(torch.tensor(d, dtype=torch.float32))
    assert torch.equal(R.ema_update64(p0, ps[0], d), d32 * p0 + (1.0 - d32) * ps[0])


def test_warmup_schedule_first_values():
    got = [R.warmup_decay(0.999, t) for t in range(1, 6)]
    assert got == [2 / 11, 3 / 12, 4 / 13, 5 / 14, 6 / 15]
    assert R.warmup_decay(0.5, 7) == 8 / 17 and R.warmup_decay(0.5, 8) == 0.5 and R.warmup_decay(0.5, 1000) == 0.5     # 9/18 = decay
    assert R.warmup_decay(0.999, 8981) < 0.999 and R.warmup_decay(0.999, 8991) == 0.999                                  # (1+t)/(10+t) = 0.999 at t = 8990
    assert R.warmup_decay(0.9, 1, warmup=False) == 0.9
    # the engine's schedule is this one
    from clipcap_amd.engine import ema_decay_at
    for t in (1, 2, 9, 50, 10 ** 6):
        for w in (False, True):
            assert ema_decay_at(0.999, t, w) == R.warmup_decay(0.999, t, w)


def _cases():
    g = torch.Generator().manual_seed(2)
    e = torch.randn(4096, generator=g)
    p = torch.randn(4096, generator=g)
    big, small = torch.full((64,), 2.0 ** 60), torch.full((64,), 2.0 ** -60)
    x = torch.randn(64, generator=g)
    return {"random": (e, p), "e=-p": (-p, p), "e=-p, 2^60": (-big * x, big * x), "2^60 vs 2^-60": (big * x, small), "2^-60 vs 2^60": (small * x, big),
            "both 2^-60": (small * x, -small * x.flip(0)), "zeros": (torch.zeros(64), x), "p zero": (x, torch.zeros(64))}


@pytest.mark.parametrize("d", [0.0, 0.5, 0.9, 0.999, 0.9999])
def test_fp32_convex_form_stays_inside_the_bound(d):
    for name, (e, p) in _cases().items():
        got = R.ema_convex_f32(e, p, d)
        err = (got.double() - R.ema_update64(e, p, d)).abs()
        assert bool((err <= R.ema_bound(e, p)).all()), (name, d, float(err.max()))
        if d == 0.0:
            assert torch.equal(got, p), name                        # ema == p as numbers


def test_the_lerp_form_is_not_the_statement():
    """why the kernel must use the convex form: at d = 0 the lerp form returns e + fl(p - e), which is p only when the subtraction is exact"""
    e, p = torch.full((8,), 2.0 ** 60), torch.full((8,), 2.0 ** -60)
    lerp = e + (1.0 - 0.0) * (p - e)
    assert not torch.equal(lerp, p)
    assert torch.equal(R.ema_convex_f32(e, p, 0.0), p)
    top = torch.full((8,), 3.0e38)
    assert not bool(torch.isfinite(-top + 0.5 * (top - (-top))).all())          # p - e overflows for e = -p near the top of the range
    assert bool(torch.isfinite(R.ema_convex_f32(-top, top, 0.5)).all())


def test_assert_ema_step_catches_an_update_that_is_off():
    e, p = _cases()["random"]
    good = R.ema_convex_f32(e, p, 0.9)
    assert R.assert_ema_step(good, e, p, 0.9) <= 1.0
    bad = good.clone()
    bad[7] = bad[7] * (1 + 2.0 ** -20) + 2.0 ** -20
    with pytest.raises(AssertionError):
        R.assert_ema_step(bad, e, p, 0.9)
    with pytest.raises(AssertionError):
        R.assert_ema_step(R.ema_convex_f32(e, p, 0.91), e, p, 0.9)               # a different decay
