"""The float64 statement of contrastive search (tests/contrastive_ref.py) pinned on the CPU: penalty 0 and one candidate are greedy
decoding, the statement equals a brute-force torch search that recomputes the full cosine matrix at every step, and on the beam_tiny
golden model the penalty removes the repetition greedy decoding falls into."""
import pytest
import torch

from tests.contrastive_ref import contrastive_search_ref, contrastive_select_ref, contrastive_topk_ref
from tests.util import load_golden, sd_of


def _tiny():
    g = load_golden("beam_tiny")
    D, n_layer, n_head, V, npos = [int(v) for v in g["cfg"]]
    sd = {"language_model." + k: v for k, v in sd_of(g).items()}
    return g, sd, dict(n_head=n_head, n_layer=n_layer)


def _greedy(sd, embeds, dims, entry_length, stop_token):
    from oracle import clipcap_oracle as O
    wte = sd["language_model.transformer.wte.weight"]
    out = []
    for _ in range(entry_length):
        t = int(O.gpt2_logits(sd, embeds, dims["n_head"], dims["n_layer"], pre="language_model.")[0, -1].argmax())
        out.append(t)
        if t == stop_token:
            break
        embeds = torch.cat((embeds, wte[t].view(1, 1, -1)), dim=1)
    return out


def _brute_force(sd, embeds, dims, k, alpha, entry_length, stop_token):
    """Contrastive search written the way the method is usually stated: re-forward the candidate sequences, take the full cosine matrix
    between every candidate's last hidden state and every earlier position's hidden state OF THE SAME FORWARD, max over positions."""
    from oracle import clipcap_oracle as O
    import torch.nn.functional as F
    wte = sd["language_model.transformer.wte.weight"]
    out = []
    for _ in range(entry_length):
        hid, _ = O.gpt2_hidden(sd, embeds, dims["n_head"], dims["n_layer"], pre="language_model.transformer.")
        p = torch.softmax((hid[0, -1] @ wte.t()).double(), -1)
        top = sorted(range(p.numel()), key=lambda v: (-float(p[v]), v))[:k]
        rows = torch.cat((embeds.expand(k, -1, -1), wte[top].view(k, 1, -1)), dim=1)
        h2, _ = O.gpt2_hidden(sd, rows, dims["n_head"], dims["n_layer"], pre="language_model.transformer.")
        cos = F.cosine_similarity(h2[:, -1:].double(), h2[:, :-1].double(), dim=-1)            # (k, positions so far)
        score = (1 - alpha) * p[top] - alpha * cos.max(dim=1).values
        w = int(score.argmax())
        out.append(top[w])
        if top[w] == stop_token:
            break
        embeds = rows[w:w + 1]
    return out


@pytest.mark.parametrize("case", ["1", "3"])
def test_alpha_zero_and_one_candidate_are_greedy(case):
    g, sd, dims = _tiny()
    pref = torch.from_numpy(g[f"beam{case}.prefix"])
    want = _greedy(sd, pref, dims, 10, 50)
    a = contrastive_search_ref(sd, pref, top_k=3, penalty_alpha=0.0, entry_length=10, stop_token=50, **dims)
    b = contrastive_search_ref(sd, pref, top_k=1, penalty_alpha=0.5, entry_length=10, stop_token=50, **dims)
    assert a[0].tolist() == want and b[0].tolist() == want
    assert a[4] == len(want)                                            # slot 0 won every step


@pytest.mark.parametrize("case,k,alpha", [("1", 3, 0.5), ("3", 3, 0.5), ("1", 4, 0.6)])
def test_statement_equals_the_brute_force_search(case, k, alpha):
    """The causal model's hidden state at a position does not depend on later positions: the history the statement accumulates step by step
    holds the vectors the brute-force search recomputes from the whole sequence (fp32 forwards of different lengths: equal to rounding;
    the score margins, 1e-2, are far above that)."""
    g, sd, dims = _tiny()
    pref = torch.from_numpy(g[f"beam{case}.prefix"])
    r = contrastive_search_ref(sd, pref, top_k=k, penalty_alpha=alpha, entry_length=10, stop_token=50, **dims)
    assert r[2] >= 2e-3 and r[3] >= 2e-3, r[2:]
    assert r[0].tolist() == _brute_force(sd, pref, dims, k, alpha, 10, 50)


def test_the_penalty_removes_the_repetition_of_greedy_decoding():
    g, sd, dims = _tiny()
    pref = torch.from_numpy(g["beam1.prefix"])
    greedy = contrastive_search_ref(sd, pref, top_k=3, penalty_alpha=0.0, entry_length=10, stop_token=50, **dims)[0].tolist()
    assert greedy[:4] == [40, 40, 40, 40], greedy
    toks = contrastive_search_ref(sd, pref, top_k=3, penalty_alpha=0.5, entry_length=10, stop_token=50, **dims)[0].tolist()
    assert toks.count(40) <= 1 and toks != greedy, toks                 # (this random model then repeats another token: [29, 1, 1, 1, 50])


def test_topk_statement_hand_cases():
    ninf = float("-inf")
    t, p, m = contrastive_topk_ref(torch.tensor([1.0, 3.0, 3.0, ninf, 2.0]), 3)
    assert t.tolist() == [1, 2, 4] and abs(m - 1.0) < 1e-12
    z = torch.tensor([1.0, 3.0, 3.0, 2.0]).double().exp().sum()
    assert torch.allclose(p, torch.tensor([3.0, 3.0, 2.0]).double().exp() / z)
    t, p, m = contrastive_topk_ref(torch.tensor([ninf, 0.5, ninf, 0.25]), 4)
    assert t.tolist() == [1, 3, 0, 0] and p[2:].tolist() == [-1.0, -1.0] and m == float("inf")
    t, p, m = contrastive_topk_ref(torch.zeros(7), 2)
    assert t.tolist() == [0, 1] and m == 0.0 and torch.allclose(p, torch.full((2,), 1 / 7, dtype=torch.float64))


def test_select_statement_hand_cases():
    e = torch.eye(4)
    cand = torch.stack((e[0], e[1], (e[0] + e[1]) / 2 ** 0.5))
    hist = torch.stack((e[0], e[2], e[1]))
    prob = torch.tensor([0.5, 0.3, 0.2])
    tok = torch.tensor([7, 8, 9])
    r = contrastive_select_ref(cand, prob, tok, hist, 0, 2, 0.5, 8)                  # history rows 0, 1: candidate 0 repeats row 0
    assert r.sel == 1 and r.token == 8 and abs(r.score - 0.15) < 1e-7 and r.deg.tolist()[:2] == [1.0, 0.0]
    assert abs(r.margin - 0.4) < 1e-7 and abs(float(r.scores[2]) - (0.1 - 0.5 * 2 ** -0.5)) < 1e-7      # second: slot 0 at 0.25 - 0.5
    r = contrastive_select_ref(cand, prob, tok, hist, 2, 2, 0.5, 8)                  # empty range: no penalty
    assert r.sel == 0 and abs(r.score - 0.25) < 1e-7 and r.deg.tolist() == [0.0, 0.0, 0.0]
    r = contrastive_select_ref(cand, torch.tensor([-1.0, -1.0, 0.2]), tok, hist, 0, 3, 0.5, 8)
    assert r.sel == 2 and r.margin == float("inf")
    r = contrastive_select_ref(cand, torch.tensor([-1.0, -1.0, -1.0]), tok, hist, 0, 3, 0.5, 8)
    assert not r.valid and r.token == 8 and r.sel == 0 and r.score == 0.0
    r = contrastive_select_ref(cand[[0, 0]], torch.tensor([0.4, 0.4]), tok[:2], hist, 0, 3, 0.3, 8)   # a tie goes to the lowest slot
    assert r.sel == 0 and r.margin == 0.0
