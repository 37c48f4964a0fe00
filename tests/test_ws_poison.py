"""tests/ws_poison.py on the CPU: the framing arithmetic and alignment, the guards, the two fill patterns as the kernels' types read
them, and the injection bookkeeping (the engine must still hold the injected buffer afterwards)."""
import pytest
import torch

from tests.ws_poison import ALIGN, FILL_NAN, FILL_ZERO, GUARD, GUARD_BYTE, Framed, Injection, inject, injected_workspaces


@pytest.mark.parametrize("nbytes", [1, 255, 256, 4096, 100_003])
@pytest.mark.parametrize("fill", [FILL_ZERO, FILL_NAN])
def test_frame_layout_and_alignment(nbytes, fill):
    f = Framed(nbytes, fill, "cpu")
    assert f.buf.dtype == torch.uint8 and f.buf.numel() == nbytes + 2 * GUARD
    assert f.body.numel() == nbytes and f.lo.numel() == GUARD and f.hi.numel() == GUARD
    assert f.body.data_ptr() % ALIGN == 0
    assert f.lo.data_ptr() == f.buf.data_ptr() and f.body.data_ptr() == f.buf.data_ptr() + GUARD
    assert f.hi.data_ptr() == f.body.data_ptr() + nbytes
    assert bool((f.lo == GUARD_BYTE).all()) and bool((f.hi == GUARD_BYTE).all()) and bool((f.body == fill).all())
    f.check_guards()
    assert not f.touched()


def test_only_the_two_patterns_are_accepted():
    for bad in (0x7F, 0xA5, 0x01):
        with pytest.raises(AssertionError):
            Framed(16, bad, "cpu")


@pytest.mark.parametrize("fill", [FILL_ZERO, FILL_NAN])
def test_guards_detect_a_one_byte_overrun_at_either_end(fill):
    for off in (-1, 0):                       # the byte before the body, the byte after it
        f = Framed(1000, fill, "cpu")
        f.buf[GUARD + (off if off < 0 else f.nbytes)] = fill
        with pytest.raises(AssertionError, match="guard"):
            f.check_guards()
        assert not f.touched()                # the body itself is as filled
    f = Framed(1000, fill, "cpu")
    f.buf[0] = 0
    with pytest.raises(AssertionError):
        f.check_guards()
    f = Framed(1000, fill, "cpu")
    f.buf[-1] = 0
    with pytest.raises(AssertionError):
        f.check_guards()


@pytest.mark.parametrize("fill", [FILL_ZERO, FILL_NAN])
def test_touched_sees_one_changed_body_byte_and_refill_clears_it(fill):
    f = Framed(513, fill, "cpu")
    for i in (0, 512):
        f.body[i] = 0x3C
        assert f.touched()
        f.check_guards()
        f.refill()
        assert not f.touched()
    f.refill(FILL_NAN if fill == FILL_ZERO else FILL_ZERO)
    assert not f.touched() and f.fill != fill and bool((f.body == f.fill).all())


def test_the_nan_fill_is_nan_in_every_float_type_and_minus_one_as_int32():
    f = Framed(64, FILL_NAN, "cpu")
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        v = f.view(dt)
        assert v.numel() == 64 // v.element_size() and bool(torch.isnan(v).all()), dt
    assert bool((f.view(torch.int32) == -1).all())
    z = Framed(64, FILL_ZERO, "cpu")
    for dt in (torch.float32, torch.bfloat16, torch.float16, torch.int32):
        assert bool((z.view(dt) == 0).all())
    assert Framed(10, FILL_NAN, "cpu").view(torch.float32).numel() == 2      # whole elements only


class _Holder:
    pass


def test_injection_into_dicts_and_attributes_and_its_verification():
    d, h = {}, _Holder()
    with injected_workspaces([("dict", d, (3, 1), 300, torch.uint8), ("attr", h, "scratch", 64, torch.float32)], FILL_NAN, device="cpu") as inj:
        assert d[(3, 1)].data_ptr() == inj["dict"].body.data_ptr() and d[(3, 1)].numel() == 300
        assert h.scratch.dtype == torch.float32 and h.scratch.numel() == 16 and h.scratch.data_ptr() == inj["attr"].body.data_ptr()
        d[(3, 1)][5] = 1                      # what a call does
        h.scratch[2] = 1.0
    # an untouched buffer fails the verification (the call ran on something else) ...
    with pytest.raises(AssertionError, match="no byte"):
        with injected_workspaces([("dict", d, 0, 32, torch.uint8)], FILL_ZERO, device="cpu"):
            pass
    # ... and so do a buffer the engine replaced and a guard it overwrote
    with pytest.raises(AssertionError, match="replaced"):
        with injected_workspaces([("dict", d, 1, 32, torch.uint8)], FILL_ZERO, device="cpu"):
            d[1] = torch.ones(64, dtype=torch.uint8)
    with pytest.raises(AssertionError, match="guard"):
        with injected_workspaces([("attr", h, "ws", 32, torch.uint8)], FILL_ZERO, device="cpu") as inj:
            h.ws[0] = 7
            inj["attr"].buf[GUARD + 32] = 0
    inj = Injection()
    inject(h, "other", Framed(8, FILL_ZERO, "cpu"), injection=inj, name="o")
    inj.verify(touched=False)
    h.other = None
    with pytest.raises(AssertionError, match="replaced"):
        inj.verify(touched=False)
