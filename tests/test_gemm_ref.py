"""CPU tests of tests/gemm_ref.py, the float64 reference the GEMM-epilogue GPU tests compare against: a reference that is itself wrong
would make those tests assert the wrong thing."""
import pytest
import torch

from tests import gemm_ref as R


def test_gelu_new_is_torch_tanh_gelu():
    x = torch.linspace(-12, 12, 48001, dtype=torch.float64)
    ref = torch.nn.functional.gelu(x, approximate="tanh")
    assert (R.gelu_new(x) - ref).abs().max().item() <= 1e-14


def test_gelu_new_grad_is_autograd():
    x = torch.linspace(-12, 12, 48001, dtype=torch.float64, requires_grad=True)
    torch.nn.functional.gelu(x, approximate="tanh").sum().backward()
    assert (R.gelu_new_grad(x.detach()) - x.grad).abs().max().item() <= 1e-13


def test_gelu_lipschitz_constants():
    l1, l2 = R.gelu_lipschitz()
    x = torch.linspace(-8, 8, 200001, dtype=torch.float64, requires_grad=True)
    g = torch.autograd.grad(torch.nn.functional.gelu(x, approximate="tanh").sum(), x, create_graph=True)[0]
    g2 = torch.autograd.grad(g.sum(), x)[0]
    assert g.abs().max().item() <= l1 <= 1.2
    assert g2.abs().max().item() <= l2 <= 1.3


def test_relu_and_resid_drop():
    a = torch.tensor([[-1.0, 0.0, -0.0, 2.0]])
    assert R.relu(a).tolist() == [[0.0, 0.0, 0.0, 2.0]]
    res = torch.tensor([[1.0, 2.0, 3.0, 4.0]])
    bias = torch.tensor([0.5, 0.5, 0.5, 0.5])
    keep = torch.tensor([[1, 0, 1, 0]], dtype=torch.uint8)
    out = R.resid_drop(res, a, bias, keep, 0.5)
    assert out.tolist() == [[1.0 + 2 * -0.5, 2.0, 3.0 + 2 * 0.5, 4.0]]          # the residual is never scaled, dropped elements keep it
    assert R.resid_drop(res, a, None, None, 0.0).tolist() == [[0.0, 2.0, 3.0, 6.0]]


@pytest.mark.parametrize("form", [0, 1])
def test_image_layout_round_trips(form):
    torch.manual_seed(form)
    x = torch.randn(37, 24) * 5 + 0.3
    img = R.image(x, form)
    assert img.shape == (37, 72) and img.dtype == torch.bfloat16
    hi, lo, copy = R.unimage(img, form)
    assert torch.equal(hi, copy)
    h, l = R.split(x)
    assert torch.equal(hi, h) and torch.equal(lo, l)
    # the lo plane sits where the OTHER operand's image has a hi plane, so that the element-wise product over 3K is hh + hl + lh
    other = R.image(x, 1 - form)
    K = 24
    planes = lambda t: [t[:, i * K:(i + 1) * K] for i in range(3)]
    kinds = [("hi" if torch.equal(p, h) else "lo", "hi" if torch.equal(q, h) else "lo") for p, q in zip(planes(img), planes(other))]
    assert sorted(kinds) == [("hi", "hi"), ("hi", "lo"), ("lo", "hi")]
    # x - hi - lo: at most u^2 |x|
    rec = hi.double() + lo.double()
    assert ((x.double() - rec).abs() <= R.U_BF16 ** 2 * x.double().abs()).all()


@pytest.mark.parametrize("scale", [1.0, 37.0])
@pytest.mark.parametrize("K", [8, 40, 128, 768, 4096])
def test_three_term_product_within_bound(K, scale):
    torch.manual_seed(K)
    a = (torch.randn(64, K) * scale + 0.3).float()
    b = (torch.randn(48, K) * 0.5 + 0.1).float()
    ahi, alo = R.split(a)
    bhi, blo = R.split(b)
    v, s3 = R.three_term(ahi, alo, bhi, blo)
    exact = a.double() @ b.double().t()
    sabs = a.double().abs() @ b.double().abs().t()
    ratio = ((v - exact).abs() / R.split_product_bound(sabs)).max().item()
    assert ratio <= 1.0, ratio
    assert (s3 <= sabs * (1 + 3 * R.U_BF16)).all()
    # a dropped lo term is far outside: the Frobenius threshold separates it at every K
    d1 = ahi.double() @ bhi.double().t() + ahi.double() @ blo.double().t()
    d2 = ahi.double() @ bhi.double().t() + alo.double() @ bhi.double().t()
    n = exact.norm().item()
    thr = R.frobenius_threshold((v - exact).norm().item() / n, [(d1 - exact).norm().item() / n, (d2 - exact).norm().item() / n])
    assert (v - exact).norm().item() / n < thr < min((d1 - exact).norm().item(), (d2 - exact).norm().item()) / n


def test_chain_steps_follow_the_kernel_constants():
    assert R.chain_steps(768) == (24, 2)
    assert R.chain_steps(40) == (2, 2)                       # ragged K: the last step is partly zero padding
    assert R.chain_steps(768, skinny_mode=1, M=300) == (48, 1)
    assert R.chain_steps(768, skinny_mode=3, M=300) == (12, 4)
    assert R.chain_steps(768, skinny_mode=3, M=2000) == (24, 2)   # too tall for the skinny kernels: the tile kernel ran
    assert R.chain_steps(96, skinny_mode=2, M=300) == (3, 2)      # K % 64 != 0: likewise
    assert R.chain_steps(1024, ksplit=4) == (32, 5)
    s = torch.ones(2, 2, dtype=torch.float64)
    assert torch.allclose(R.acc_bound(s, 768), (24 * R.MFMA_ROUNDINGS + 2) * R.U32 * s)


def test_store_bound():
    ref = torch.tensor([1.0, -4.0], dtype=torch.float64)
    e = torch.tensor([1e-6, 0.0], dtype=torch.float64)
    b = R.store_bound(ref, e, torch.bfloat16)
    assert torch.allclose(b, torch.tensor([2.0 ** -8 + (1 + 2.0 ** -8) * 1e-6, 4 * 2.0 ** -8], dtype=torch.float64))
    assert torch.equal(R.store_bound(ref, e, torch.float32), e)
    assert (R.store_bound(ref, e, torch.float16) >= 2.0 ** -25).all()
