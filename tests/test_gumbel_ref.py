"""CPU pins of stochastic beam search's float64 statement (tests/gumbel_ref.py) and of the host-buildable Philox header
(clipcap_amd/csrc/philox.h through tests/philox_check.cpp): the generator's known answers, beam 1 as the arg-max of the perturbed logits,
the invariants of the conditioned values, the sampling-without-replacement statistics on a small tree, and sbs_importance_weights against
a float64 evaluation of its formula."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests.gumbel_ref import gumbel_from_bits, gumbel_step_ref, noise, noise_bits, philox4x32_10

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def test_philox_known_answers():
    for ctr, key, want in KAT:
        assert tuple(int(w) for w in philox4x32_10(ctr, key)) == want
    got = philox4x32_10([k[0] for k in KAT], [k[1] for k in KAT])                      # and vectorised
    assert got.tolist() == [list(k[2]) for k in KAT]


def test_noise_words_are_keyed_on_token_row_step_and_seed():
    seed = 0x299f31d0a4093822
    bits = noise_bits(seed, 3, 2, 11)
    assert bits.shape == (11,) and bits.dtype == np.uint32
    for v in range(11):
        assert int(bits[v]) == int(philox4x32_10((v >> 2, 2, 3, 0), (0xa4093822, 0x299f31d0))[v & 3])
    assert not np.array_equal(bits, noise_bits(seed, 4, 2, 11)) and not np.array_equal(bits, noise_bits(seed, 3, 1, 11))
    assert not np.array_equal(bits, noise_bits(seed + 1, 3, 2, 11))
    n = gumbel_from_bits(np.array([0, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1], dtype=np.uint32))
    assert np.all(np.isfinite(n)) and -3.14 < n[0] < -3.12 and 22.8 < n[3] < 22.9 and n[1] < n[2]
    assert abs(n[0] + math.log(-math.log(0.5 / 2 ** 32))) < 1e-14 and abs(n[3] + math.log(-math.log1p(-0.5 / 2 ** 32))) < 1e-12


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_philox_header_alone(tmp_path, sanitize):
    """philox.h with a host compiler and no HIP include path, plainly and with -fsanitize=address,undefined, run directly."""
    assert CXX, "no host C++ compiler"
    exe = str(tmp_path / "philox_check")
    flags = ["-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-g", "-I", os.path.join(ROOT, "clipcap_amd", "csrc")]
    static = ["-static-libasan", "-static-libubsan"] if "g++" in os.path.basename(CXX) and "clang" not in os.path.basename(CXX) else ["-static-libsan"]
    flags += ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static] if sanitize else []
    subprocess.run([CXX, *flags, os.path.join(ROOT, "tests", "philox_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0 and out.stdout.strip().splitlines()[-1].startswith("ok:")


def _decode(logits_of, *, beam, steps, seed, row0=0, T=1.0, stop=10 ** 6):
    """``steps`` updates of one sample; logits_of(step, tokens-so-far (beam, step) or None) -> (beam, V).  -> the steps' GumbelStep."""
    out, toks, st = [], None, (None, None, None, None)
    for i in range(steps):
        r = gumbel_step_ref(logits_of(i, toks), *st, beam=beam, seed=seed, step=i, row0=row0, temperature=T, first=i == 0, stop_token=stop)
        toks = r.tokens.view(-1, 1) if toks is None else torch.cat((toks[r.src], r.tokens.view(-1, 1)), 1)
        st = (r.phi, r.gam, r.lengths, r.stopped)
        out.append((r, toks))
    return out


def test_beam_one_is_the_argmax_of_the_perturbed_logits():
    g = torch.Generator().manual_seed(5)
    V, T, row0, seed = 257, 0.8, 12, 991
    rows = [torch.randn(1, V, generator=g) * 3 for _ in range(6)]
    phi = 0.0
    for i, (r, _) in enumerate(_decode(lambda i, t: rows[i], beam=1, steps=6, seed=seed, row0=row0, T=T)):
        x = rows[i][0].double() / T
        v = int(torch.argmax(x + noise(seed, i, row0, V)))
        phi += float(torch.log_softmax(x, -1)[v])
        assert r.tokens.tolist() == [v] and r.src.tolist() == [0]
        assert float(r.gam[0]) == 0.0 and abs(float(r.phi[0]) - phi) < 1e-12 and float(r.lengths[0]) == i + 1


@pytest.mark.parametrize("beam", [2, 5, 7])
def test_invariants_of_the_conditioned_values(beam):
    """Slot 0 keeps Gamma == 0.0 exactly, the slots' Gamma are descending, every Gamma_c <= its parent's, a stopped parent passes phi and
    Gamma through, and no two slots share (source row, token)."""
    g = torch.Generator().manual_seed(beam)
    V, stop = 61, 17
    rows = [torch.randn(beam, V, generator=g) * 2 for _ in range(7)]
    for r in rows[2:]:
        r[::2, stop] += 6.0
    prev = None
    for i, (r, _) in enumerate(_decode(lambda i, t: rows[i], beam=beam, steps=7, seed=1234 + beam, T=0.9, stop=stop)):
        assert float(r.gam[0]) == 0.0
        assert all(float(a) >= float(b) for a, b in zip(r.gam, r.gam[1:]))
        assert len({(int(b), int(v)) for b, v in zip(r.src, r.tokens)}) == beam
        if prev is not None:
            for k in range(beam):
                b = int(r.src[k])
                assert float(r.gam[k]) <= float(prev.gam[b])
                if bool(prev.stopped[b]):
                    assert float(r.gam[k]) == float(prev.gam[b]) and float(r.phi[k]) == float(prev.phi[b]) and int(r.tokens[k]) == 0
                    assert float(r.lengths[k]) == float(prev.lengths[b]) and bool(r.stopped[k])
        prev = r
    assert bool(prev.stopped.any())


def test_fewer_candidates_than_slots_leave_empty_slots_that_stay_empty():
    V, beam = 9, 4
    lg = torch.full((beam, V), float("-inf"))
    lg[0, 3], lg[0, 6] = 1.0, 0.5
    r = gumbel_step_ref(lg, None, None, None, None, beam=beam, seed=3, step=0, row0=0, first=True, stop_token=8)
    assert sorted(r.tokens[:2].tolist()) == [3, 6] and r.tokens[2:].tolist() == [0, 0] and r.src.tolist() == [0] * 4
    assert torch.isinf(r.phi[2:]).all() and torch.isinf(r.gam[2:]).all() and r.stopped.tolist() == [False, False, True, True]
    assert r.lengths.tolist() == [1.0] * 4
    lg2 = torch.full((beam, V), float("-inf"))
    lg2[1, 2] = 0.0
    r2 = gumbel_step_ref(lg2, r.phi, r.gam, r.lengths, r.stopped, beam=beam, seed=3, step=1, row0=0, stop_token=8)
    assert r2.tokens.tolist() == [2, 0, 0, 0] and r2.src.tolist() == [1, 0, 0, 0] and r2.stopped.tolist() == [False, True, True, True]
    assert r2.lengths.tolist() == [2.0, 1.0, 1.0, 1.0] and torch.isinf(r2.gam[1:]).all() and float(r2.gam[0]) == float(r.gam[1])


def test_sampling_without_replacement_statistics():
    """A two-step tree with V = 3 and beam 2 over 20 000 seeds: the first slot's sequence is a sample from p(seq), and the ordered pair of
    the two slots has probability p_a p_b / (1 - p_a) — sampling without replacement in sampling order.  Every frequency within 4 binomial
    standard deviations.  The noise of all seeds comes from one vectorised Philox call with the seeds as keys, the statement's own mapping."""
    N, V, beam = 20000, 3, 2
    l1 = torch.tensor([0.3, -0.4, 0.9])
    l2 = torch.tensor([[0.1, 1.2, -0.7], [-1.0, 0.2, 0.4], [0.8, 0.8, -0.3]])             # second-step logits after first token a
    p1, p2 = torch.softmax(l1.double(), 0), torch.softmax(l2.double(), 1)
    p = {(a, b): float(p1[a] * p2[a, b]) for a in range(V) for b in range(V)}
    seeds = np.arange(N, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(12345)
    keys = np.stack((seeds & np.uint64(0xFFFFFFFF), seeds >> np.uint64(32)), -1)
    nz = {}
    for step, row in ((0, 0), (1, 0), (1, 1)):                                          # tokens 0..2 share counter word group 0
        bits = philox4x32_10(np.array([0, row, step, 0], dtype=np.uint64), keys)[:, :V]
        nz[step, row] = torch.from_numpy(gumbel_from_bits(bits))
    first, pairs = {}, {}
    for i in range(N):
        r0 = gumbel_step_ref(l1.expand(beam, -1), None, None, None, None, beam=beam, seed=0, step=0, row0=0, first=True, stop_token=99,
                             noise_rows=nz[0, 0][i].expand(beam, -1))
        r1 = gumbel_step_ref(l2[r0.tokens], r0.phi, r0.gam, r0.lengths, r0.stopped, beam=beam, seed=0, step=1, row0=0, stop_token=99,
                             noise_rows=torch.stack((nz[1, 0][i], nz[1, 1][i])))
        seqs = [(int(r0.tokens[int(r1.src[k])]), int(r1.tokens[k])) for k in range(beam)]
        assert seqs[0] != seqs[1] and float(r1.gam[0]) == 0.0
        first[seqs[0]] = first.get(seqs[0], 0) + 1
        pairs[tuple(seqs)] = pairs.get(tuple(seqs), 0) + 1
    worst = [0.0, 0.0]
    for a, pa in p.items():
        dev = abs(first.get(a, 0) / N - pa)
        worst[0] = max(worst[0], dev)
        assert dev <= 4 * math.sqrt(pa * (1 - pa) / N), (a, dev)
        for b, pb in p.items():
            if a != b:
                q = pa * pb / (1 - pa)
                dev = abs(pairs.get((a, b), 0) / N - q)
                worst[1] = max(worst[1], dev)
                assert dev <= 4 * math.sqrt(q * (1 - q) / N), (a, b, dev)
    print(f"largest deviation: first slot {worst[0]:.4f}, ordered pairs {worst[1]:.4f}")


def test_importance_weights_against_float64():
    from clipcap_amd.inference.stochastic_beam import sbs_importance_weights
    g = torch.Generator().manual_seed(2)
    phi = -torch.rand(3, 5, generator=g) * 6
    gam = torch.sort(phi + torch.randn(3, 5, generator=g), dim=1, descending=True).values
    gam[1] = gam[1].flip(0)                                                             # the threshold's slot is found, not assumed last
    for normalise in (False, True):
        w = sbs_importance_weights(phi, gam, normalise)
        assert w.shape == (3, 4)
        for s in range(3):
            at = int(torch.argmin(gam[s]))
            kappa = float(gam[s, at])
            want = [math.exp(float(phi[s, k])) / -math.expm1(-math.exp(float(phi[s, k]) - kappa)) for k in range(5) if k != at]
            if normalise:
                want = [x / sum(want) for x in want]
            assert np.allclose(w[s].double().numpy(), want, rtol=2e-6, atol=0)
    w64 = sbs_importance_weights(phi.double(), gam.double())
    assert w64.dtype == torch.float64 and torch.allclose(w64.sum(1), torch.ones(3, dtype=torch.float64))
    for bad in (phi[:, :1], phi[0]):
        with pytest.raises(ValueError, match="k >= 2"):
            sbs_importance_weights(bad, bad)
    with pytest.raises(ValueError):
        sbs_importance_weights(phi, gam[:, :4])
