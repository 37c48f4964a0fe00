"""CPU test of tests/mlp_ref.py itself: the closed forms against torch.tanh in float64, the Lipschitz constant of 1 - tanh^2 against a fine
grid, the stage products against plain float64 matmuls, and the measured allowances' bookkeeping."""
import math

import torch

from tests import gemm_ref as R
from tests import mlp_ref as MR


def test_closed_forms_against_torch_float64():
    x = torch.cat([torch.linspace(-45.0, 45.0, 200001, dtype=torch.float64), torch.tensor([0.0, -0.0, 1e-300, -1e-300, 700.0, -700.0], dtype=torch.float64)])
    ref = torch.tanh(x)
    assert (MR.tanh(x) - ref).abs().max().item() <= 2.0 ** -52
    assert (MR.tanh_grad(x) - (1.0 - ref * ref)).abs().max().item() <= 2.0 ** -51
    big = x.abs() >= 20.0
    assert (MR.tanh(x)[big] == torch.sign(x)[big]).all() and (MR.tanh_grad(x)[big] < 1e-16).all()
    z = MR.tanh(torch.tensor([0.0, -0.0], dtype=torch.float64))
    assert z[0] == 0 and not torch.signbit(z[0]) and z[1] == 0 and torch.signbit(z[1])
    assert torch.isnan(MR.tanh(torch.tensor([float("nan")]))).all() and torch.isnan(MR.tanh_grad(torch.tensor([float("nan")]))).all()
    assert torch.isfinite(MR.tanh(torch.tensor([1e308, -1e308], dtype=torch.float64))).all()


def test_lipschitz_constants_against_a_fine_grid():
    """|d/dx tanh| = sech^2 <= 1; |d/dx (1 - tanh^2)| = |2 tanh sech^2| peaks at tanh^2 = 1 / 3 with 4 / (3 sqrt 3)"""
    x = torch.linspace(-6.0, 6.0, 2_400_001, dtype=torch.float64)
    h = (x[1] - x[0]).item()
    d1 = MR.tanh_grad(x)
    d2 = (d1[2:] - d1[:-2]) / (2 * h)
    assert d1.max().item() <= MR.TANH_LIP and d1.max().item() >= 1.0 - 1e-9
    peak = d2.abs().max().item()
    assert abs(peak - MR.TANH_GRAD_LIP) <= 1e-9 and MR.TANH_GRAD_LIP == 4.0 / (3.0 * math.sqrt(3.0))
    at = x[1:-1][d2.abs().argmax()].abs().item()
    assert abs(math.tanh(at) ** 2 - 1.0 / 3.0) <= 1e-5


def test_stage_products_against_plain_float64():
    g = torch.Generator().manual_seed(3)
    a, w = torch.randn(5, 24, generator=g), torch.randn(16, 24, generator=g)
    for dt in (torch.bfloat16, torch.float16):
        v, s, kp = MR.nt(a.to(dt), w, dt)
        assert kp == 24 and torch.equal(v, a.to(dt).double() @ w.to(dt).double().t()) and (s >= v.abs() - 1e-12).all()
    v, s, kp = MR.nt(a, w, torch.float32)
    exact = a.double() @ w.double().t()
    assert kp == 72 and ((v - exact).abs() <= R.split_product_bound(a.double().abs() @ w.double().abs().t())).all()
    x, y = torch.randn(7, 8, generator=g), torch.randn(7, 16, generator=g)
    v, s, kp = MR.tn(x, y, torch.float32)
    assert kp == 21 and v.shape == (8, 16) and ((v - x.double().t() @ y.double()).abs() <= R.split_product_bound(x.double().abs().t() @ y.double().abs())).all()
    v, s, kp = MR.tn(x.bfloat16(), y.bfloat16(), torch.bfloat16)
    assert kp == 7 and torch.equal(v, x.bfloat16().double().t() @ y.bfloat16().double())
    assert torch.equal(MR.cast(a, torch.float32), a) and MR.cast(a, torch.bfloat16).dtype == torch.bfloat16


def test_prefix_is_the_plain_mlp_and_rounds_where_told():
    g = torch.Generator().manual_seed(4)
    E, D, L, B = 16, 8, 2, 3
    p = {"m.model.0.weight": torch.randn(L * D // 2, E, generator=g), "m.model.0.bias": torch.randn(L * D // 2, generator=g),
         "m.model.2.weight": torch.randn(L * D, L * D // 2, generator=g), "m.model.2.bias": torch.randn(L * D, generator=g)}
    emb = torch.randn(B, E, generator=g)
    seq = torch.nn.Sequential(torch.nn.Linear(E, L * D // 2), torch.nn.Tanh(), torch.nn.Linear(L * D // 2, L * D))
    seq.load_state_dict({k[len("m.model."):]: v for k, v in p.items()})
    out = MR.prefix(p, emb, L, pre="m.")
    assert out.shape == (B, L, D) and torch.allclose(out.reshape(B, -1), seq(emb), atol=1e-6)
    rb = MR.prefix(p, emb, L, pre="m.", rb=True)
    assert 0 < (rb - out).abs().max().item() < 0.2


def test_allowances_are_four_times_the_raw_figures_and_below_the_defect_line():
    assert MR.TANH_ULPS == 4 * MR.TANH_RAW and MR.TANH_GRAD_ULPS == 4 * MR.TANH_GRAD_RAW
    assert 0 < MR.TANH_RAW <= MR.RAW_LIMIT and 0 < MR.TANH_GRAD_RAW <= MR.RAW_LIMIT
    assert MR.RAW_LIMIT == 33.0 and abs(R.GELU_GRAD_ULPS / 4 - 33.07) < 0.01      # the defect line is the existing epilogue's raw figure
