"""CPU side of the BLEU / ROUGE-L metrics: cc_bleu_stats and cc_rouge_l are declared, bound and exported under ABI version 3; every
documented return code is decided without a device; the engine wrappers raise before launching; MetricReward, clipcap_amd.eval and its
command line run end to end with the launches replaced by the Python reference statement (tests/metrics_cases.py) and reproduce the
numbers recorded from the reference project's scorers.  The kernels are tested on the device in tests/test_gpu_metrics.py."""
import ctypes as C
import csv
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import bleu_rouge_ref as ref
from tests.metrics_cases import bleu_stats_stand_in, cider_score_stand_in, golden_cases, rouge_l_stand_in

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_COMMON = ["const int64_t* cand", "int32_t C", "int32_t cand_len", "int64_t cand_ld", "int32_t stop_token", "int32_t count_stop",
           "const int32_t* cand_group", "const int32_t* refs", "int32_t G", "int32_t Rmax", "int32_t Lr", "const int32_t* ref_count"]
ENTRY = {
    "cc_bleu_stats": _COMMON + ["int32_t* stats", "float* bleu", "void* stream"],
    "cc_rouge_l": _COMMON + ["float beta", "int32_t* lcs", "float* out", "void* stream"],
}


@pytest.fixture
def stand_ins(monkeypatch):
    from clipcap_amd import engine
    monkeypatch.setattr(engine, "bleu_stats", bleu_stats_stand_in)
    monkeypatch.setattr(engine, "rouge_l", rouge_l_stand_in)
    monkeypatch.setattr(engine, "cider_score", cider_score_stand_in)


@pytest.mark.parametrize("name", sorted(ENTRY))
def test_header_binding_and_library_carry_the_entry_point(name):
    from clipcap_amd import _lib
    raw = open(os.path.join(ROOT, "include", "clipcap_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr, flags=re.M)
    assert m, f"{name} is not declared in include/clipcap_hip.h"
    params = [p.strip() for p in " ".join(m.group(1).split()).split(",")]
    assert params == ENTRY[name]
    res, args = _lib.SIGNATURES[name]
    assert res is _lib._I and len(args) == len(params)
    for p, a in zip(params, args):
        want = _lib._P if "*" in p else _lib._L if p.startswith("int64_t") else _lib._F if p.startswith("float") else _lib._I
        assert a is want, (p, a)
    l = _lib.lib()
    assert hasattr(l, name) and l.cc_abi_version() == 3 and _lib.ABI_VERSION == 3
    added = raw[raw.index("ADDED since (still 3"):raw.index("#define CC_ABI_VERSION")]
    assert name in added                                                                   # the list of entry points added without a bump


def test_generated_abi_files_makefile_and_limits():
    assert subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_abi.py"), "--check"]).returncode == 0
    csrc = os.path.join(ROOT, "clipcap_amd", "csrc")
    for f in ("abi_dispatch.cpp", "exports.map", "exports_lab.map"):
        text = open(os.path.join(csrc, f)).read()
        assert all(name in text for name in ENTRY), f
    mk = open(os.path.join(csrc, "Makefile")).read()
    once = next(line for line in mk.splitlines() if line.startswith("SRCS_ONCE"))
    srcs = next(line for line in mk.splitlines() if line.startswith("SRCS "))
    assert "metrics.hip" in once and "metrics.hip" not in srcs                              # integer / fp64 work: built once
    assert "caption_lds.h" in next(line for line in mk.splitlines() if line.startswith("HDRS"))
    hdr = open(os.path.join(ROOT, "include", "clipcap_hip.h")).read()
    assert "Limits (CC_ERR_SHAPE): cand_len <= 256, Lr <= 256, Rmax * Lr <= 4096.\n" in hdr   # the limits are written down


def test_argument_errors_need_no_device():
    """Every return code is decided before anything touches the device: the pointers given here are never followed.  The cases are the
    header comment's, one by one."""
    from clipcap_amd import _lib
    p = [C.c_void_p(4096 * (i + 1)) for i in range(6)]
    nan, inf = float("nan"), float("inf")

    def bleu(cand=p[0], C_=6, cand_len=20, cand_ld=24, stop=50256, count_stop=0, group=p[1], refs=p[2], G=3, Rmax=5, Lr=30, ref_count=p[3],
             out=p[4], extra=p[5]):
        return _lib.lib().cc_bleu_stats(cand, C_, cand_len, cand_ld, stop, count_stop, group, refs, G, Rmax, Lr, ref_count, out, extra, None)

    def rouge(cand=p[0], C_=6, cand_len=20, cand_ld=24, stop=50256, count_stop=0, group=p[1], refs=p[2], G=3, Rmax=5, Lr=30, ref_count=p[3],
              out=p[4], extra=p[5], beta=1.2):
        return _lib.lib().cc_rouge_l(cand, C_, cand_len, cand_ld, stop, count_stop, group, refs, G, Rmax, Lr, ref_count, beta, extra, out, None)

    for call in (bleu, rouge):
        # nothing to score: 0, nothing launched, whatever the pointers and the limits
        assert call(C_=0) == 0 and call(C_=0, cand=None, refs=None, out=None, extra=None, group=None, ref_count=None) == 0
        assert call(C_=0, cand_len=300, cand_ld=300) == 0 and call(C_=0, Rmax=100, Lr=100) == 0
        # -1: bad arguments
        assert call(C_=-1) == -1 and call(cand_len=-1) == -1 and call(cand_ld=19) == -1
        assert call(G=0) == -1 and call(Rmax=0) == -1 and call(Lr=0) == -1
        assert call(group=None, C_=7) == -1 and call(group=None, C_=2) == -1               # no map: C must be a multiple of G
        for bad in (dict(cand=None), dict(refs=None), dict(out=None)):
            assert call(**bad) == -1, bad
        assert call(C_=0, cand_ld=3) == -1 and call(C_=0, G=0) == -1 and call(C_=0, group=None, G=-2) == -1   # a bad argument is one whatever C is
        # -2: beyond the limits
        assert call(cand_len=257, cand_ld=257) == -2 and call(Lr=257, Rmax=1) == -2
        assert call(Rmax=17, Lr=256) == -2 and call(Rmax=4097, Lr=1) == -2 and call(Rmax=65, Lr=64) == -2
        assert call(cand=None, cand_len=257, cand_ld=257) == -1                             # the arguments are judged before the limits
    assert rouge(beta=0.0) == -1 and rouge(beta=-1.2) == -1 and rouge(beta=nan) == -1 and rouge(beta=inf) == -1
    assert rouge(C_=0, beta=nan) == -1
    # no limit on the stop token or on the ids; the optional outputs may be NULL: with C > 0 these calls would launch, so they are made
    # on the device (tests/test_gpu_metrics.py).  Here: the limits themselves pass the checks that come before the launch
    assert bleu(C_=0, stop=1 << 30) == 0 and rouge(C_=0, stop=-1) == 0


def test_engine_wrappers_validate_before_they_touch_a_device():
    from clipcap_amd import engine
    cand, refs = torch.zeros(4, 10, dtype=torch.int64), torch.zeros(2, 3, 12, dtype=torch.int32)
    for fn, shapes in ((engine.bleu_stats, [(0, 10), (0, 4)]), (engine.rouge_l, [(0,), (0, 3)])):
        got = fn(cand[:0], refs)                                                            # nothing to score: no device is needed
        assert [tuple(t.shape) for t in got] == shapes
        score = lambda c=cand, r=refs, **kw: fn(c, r, **kw)  # noqa: E731
        for bad in (lambda: score(cand.int()), lambda: score(cand[0]), lambda: score(r=refs.long()), lambda: score(r=refs[0]),
                    lambda: score(r=refs[:, :, ::2]), lambda: score(torch.zeros(4, 257, dtype=torch.int64)),
                    lambda: score(r=torch.zeros(2, 1, 257, dtype=torch.int32)), lambda: score(r=torch.zeros(2, 17, 256, dtype=torch.int32)),
                    lambda: score(cand[:3]), lambda: score(cand_group=torch.zeros(4, dtype=torch.int64)),
                    lambda: score(cand_group=torch.zeros(3, dtype=torch.int32)), lambda: score(ref_count=torch.ones(3, dtype=torch.int32)),
                    lambda: score(cand.t()), lambda: score(r=torch.zeros(0, 3, 12, dtype=torch.int32))):
            with pytest.raises(ValueError):
                bad()
        with pytest.raises(RuntimeError, match="MI355X"):                                   # valid arguments: only then the device matters
            score()
        with pytest.raises(RuntimeError, match="MI355X"):
            score(stop_token=70000, cand_group=torch.zeros(4, dtype=torch.int32), ref_count=torch.ones(2, dtype=torch.int32))
    for beta in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="beta"):
            engine.rouge_l(cand, refs, beta=beta)


def test_bleu_corpus_sums_the_counts_and_applies_the_formula():
    from clipcap_amd import engine
    for case in golden_cases():
        stats = torch.tensor(case["counts"], dtype=torch.int32)
        got = engine.bleu_corpus(stats)
        assert all(abs(a - b) <= 1e-12 * abs(b) for a, b in zip(got, case["case_bleu"]))
        for row, want in zip(case["counts"], case["bleu"]):
            assert all(abs(a - b) <= 1e-12 * abs(b) for a, b in zip(engine.bleu_from_counts(row), want))
    big = torch.full((3, 10), 2 ** 30, dtype=torch.int32)                                   # the sums are taken in int64
    assert engine.bleu_corpus(big) == ref.bleu_from_counts([3 * 2 ** 30] * 10)
    for bad in (torch.zeros(3, 9, dtype=torch.int32), torch.zeros(3, 10, dtype=torch.int64), torch.zeros(10, dtype=torch.int32)):
        with pytest.raises(ValueError):
            engine.bleu_corpus(bad)


def test_metric_reward_weights_and_what_is_launched(monkeypatch):
    from clipcap_amd import engine
    from clipcap_amd.train import CiderReward, MetricReward
    calls = []

    def fake(name, value, cols=None):
        def launch(cand, refs, *a, **kw):
            calls.append((name, kw.get("stop_token"), kw.get("count_stop"), kw.get("ref_count"), kw.get("cand_group")))
            v = torch.full((cand.shape[0],), value, dtype=torch.float32)
            if name == "bleu":
                return torch.zeros(cand.shape[0], 10, dtype=torch.int32), torch.stack([v + n for n in range(4)], dim=1)
            return (v, torch.zeros(cand.shape[0], refs.shape[1], dtype=torch.int32)) if name == "rouge" else v
        return launch

    monkeypatch.setattr(engine, "cider_score", fake("cider", 2.0))
    monkeypatch.setattr(engine, "bleu_stats", fake("bleu", 10.0))
    monkeypatch.setattr(engine, "rouge_l", fake("rouge", 100.0))
    cider = CiderReward.from_corpus([[[4, 5, 6], [7]], [[1, 2, 3, 4]]], stop_token=8, device="cpu")
    cand, refs = torch.zeros(4, 5, dtype=torch.int64), torch.zeros(2, 2, 4, dtype=torch.int32)
    count = torch.tensor([2, 1], dtype=torch.int32)
    # the default weights: cider + 0.5 bleu4, ROUGE-L (weight 0) is not launched
    rw = MetricReward(cider=cider, stop_token=8)
    assert rw.weights == {"cider": 1.0, "bleu4": 0.5}
    assert rw.score(cand, refs, count).tolist() == [2.0 + 0.5 * 13.0] * 4
    assert [c[0] for c in calls] == ["cider", "bleu"] and calls[1][1:] == (8, False, count, None)
    # all three, two BLEU orders from ONE launch, in the order of METRICS whatever the dict's order
    del calls[:]
    rw = MetricReward({"rouge_l": 0.25, "bleu2": 2.0, "cider": 1.0, "bleu4": 1.0, "bleu1": 0.0}, cider=cider, stop_token=8)
    assert list(rw.weights) == ["cider", "bleu2", "bleu4", "rouge_l"]
    assert rw.score(cand, refs).tolist() == [2.0 + 2.0 * 11.0 + 13.0 + 25.0] * 4
    assert [c[0] for c in calls] == ["cider", "bleu", "rouge"]
    # without CIDEr no CiderReward is needed
    del calls[:]
    assert MetricReward({"bleu4": 1.0, "cider": 0.0}).score(cand, refs).tolist() == [13.0] * 4 and [c[0] for c in calls] == ["bleu"]
    assert calls[0][1] == 50256
    with pytest.raises(ValueError, match="CiderReward"):
        MetricReward()                                                                      # the default weights name cider
    with pytest.raises(ValueError, match="CiderReward"):
        MetricReward({"cider": 0.1, "bleu4": 1.0})
    with pytest.raises(ValueError, match="stop_token"):
        MetricReward(cider=cider)                                                           # built with stop_token 8, asked for 50256
    with pytest.raises(ValueError, match="unknown"):
        MetricReward({"meteor": 1.0})
    with pytest.raises(ValueError, match="nothing to score"):
        MetricReward({"cider": 0.0, "bleu4": 0.0})
    with pytest.raises(ValueError, match="finite"):
        MetricReward({"bleu4": float("nan")})


def test_metric_reward_for_batch_pads_and_groups_as_cider_reward_does(stand_ins):
    from clipcap_amd.train import CiderReward, MetricReward
    B, stop = 3, 8
    refs = torch.tensor([[[4, 5, 6, -1], [7, -1, -1, -1]], [[1, 2, 3, 4], [-1, -1, -1, -1]], [[9, 9, -1, 3], [2, 2, 2, -1]]], dtype=torch.int32)
    count = torch.tensor([2, 1, 2], dtype=torch.int32)
    sampled = torch.tensor([[5, 6, 8, 0, 0], [1, 8, 3, 3, 3], [2, 2, 2, 2, 8]])
    greedy = torch.tensor([[5, 8], [8, 1], [4, 4]])
    docs = [[[4, 5, 6], [7]], [[1, 2, 3, 4]], [[9, 9], [2, 2, 2]]]
    weights = {"cider": 1.0, "bleu4": 0.5, "bleu1": 0.25, "rouge_l": 2.0}
    for count_stop in (False, True):
        cider = CiderReward.from_corpus(docs, stop_token=stop, count_stop=count_stop, device="cpu")
        rw = MetricReward(weights, cider=cider, stop_token=stop, count_stop=count_stop)
        r_s, r_g = rw.for_batch(refs, count)(sampled, greedy)
        c_s, c_g = cider.for_batch(refs, count)(sampled, greedy)
        tail = [stop] if count_stop else []
        for ids, got, cid in ((sampled, r_s, c_s), (greedy, r_g, c_g)):
            for b in range(B):
                words = [int(t) for t in ids[b].tolist()]
                words = words[:words.index(stop) + (1 if count_stop else 0)] if stop in words else words
                rows = [r + tail for r in docs[b]]
                bleu = ref.bleu_from_counts(ref.bleu_counts(words, rows))
                want = np.float32(cid[b]) * np.float32(1.0)
                want = want + np.float32(bleu[0]) * np.float32(0.25)
                want = want + np.float32(bleu[3]) * np.float32(0.5)
                want = want + np.float32(ref.rouge_l(words, rows)) * np.float32(2.0)
                assert float(got[b]) == float(want), (count_stop, b, words, rows)
        assert float(r_s.max()) > 0
    with pytest.raises(ValueError):
        rw.for_batch(refs)(sampled[:2], greedy)
    with pytest.raises(ValueError):
        rw.for_batch(refs.long())


def test_normalise_and_word_vocab():
    from clipcap_amd.eval import metrics as M
    assert M.normalise("A man, riding-a horse!  It's 2 p.m.\n") == ["a", "man", "riding", "a", "horse", "it", "s", "2", "p", "m"]
    assert M.normalise("") == [] and M.normalise(" ...  ") == []
    assert "PTB" in M.normalise.__doc__ and "NOT" in M.normalise.__doc__
    v = M.WordVocab.from_captions([["the", "cat", "sat"], ["the", "dog", "sat", "the"], ["a"]])
    assert v.words == ["the", "sat", "a", "cat", "dog"] and len(v) == 5                     # by descending frequency, ties by the word
    assert v.encode(["dog", "the"]) == [4, 0]
    v.require_cider()
    # 65535 distinct words are fine for CIDEr, one more is not; BLEU and ROUGE-L never ask
    many = [[f"w{i}"] * (2 if i < 10 else 1) for i in range(65536)]
    v = M.WordVocab.from_captions(many)
    assert len(v) == 65536 and sorted(v.words[:10]) == sorted(f"w{i}" for i in range(10)) and v.ids[v.words[-1]] == 65535
    with pytest.raises(ValueError, match="65535"):
        v.require_cider()
    M.WordVocab.from_captions(many[:65535]).require_cider()


def _as_strings(case):
    word = lambda t: f"w{t}"  # noqa: E731
    preds = [" ".join(word(t) for t in c) for c, _ in case["images"]]
    truths = [[" ".join(word(t) for t in r) for r in refs] for _, refs in case["images"]]
    return preds, truths


def test_evaluate_metrics_from_lists_reproduces_the_recorded_numbers(stand_ins):
    from clipcap_amd.eval.metrics import evaluate_metrics_from_lists
    for case in golden_cases():
        preds, truths = _as_strings(case)
        ids = [f"file{i}" for i in range(len(preds))]
        total, per = evaluate_metrics_from_lists(preds, truths, ids, device="cpu")
        assert list(total) == ["Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4", "ROUGE_L", "CIDEr"] and list(per) == ids
        for n in range(4):
            assert abs(total[f"Bleu_{n + 1}"] - case["case_bleu"][n]) <= 1e-12 * case["case_bleu"][n]
        assert abs(total["ROUGE_L"] - case["case_rouge"]) <= 2.0 ** -23 * case["case_rouge"]
        assert abs(total["CIDEr"] - case["case_cider"]) <= 2e-5 * case["case_cider"]
        for i, name in enumerate(ids):
            assert list(per[name]) == list(total)
            assert abs(per[name]["ROUGE_L"] - case["rouge"][i]) <= 2.0 ** -23 * case["rouge"][i]
            assert abs(per[name]["Bleu_4"] - case["bleu"][i][3]) <= 2.0 ** -23 * case["bleu"][i][3] + 2.0 ** -126
    # ragged reference counts were part of every case; a subset of the metrics; the first entry of a list prediction; default ids
    case = golden_cases()[0]
    preds, truths = _as_strings(case)
    total, per = evaluate_metrics_from_lists([[p, "ignored"] for p in preds], truths, metrics=("ROUGE_L",), device="cpu")
    assert list(total) == ["ROUGE_L"] and list(per) == list(range(len(preds)))
    with pytest.raises(ValueError):
        evaluate_metrics_from_lists(preds, truths[:-1], device="cpu")
    with pytest.raises(ValueError):
        evaluate_metrics_from_lists(preds, truths, metrics=("METEOR",), device="cpu")
    with pytest.raises(ValueError):
        evaluate_metrics_from_lists(preds, [[] for _ in truths], device="cpu")
    with pytest.raises(ValueError, match="256"):
        evaluate_metrics_from_lists(["a " * 257], [["a"]], device="cpu")


def _write_csvs(tmp_path, case, shuffle):
    preds, truths = _as_strings(case)
    names = [f"clip_{i:03d}.wav" for i in range(len(preds))]
    order = list(range(len(preds)))
    if shuffle:
        order = order[::-1]
    pfile, rfile = tmp_path / "predictions.csv", tmp_path / "references.csv"
    with open(pfile, "w", newline="") as f:
        w = csv.DictWriter(f, ["file_name", "caption_predicted"])
        w.writeheader()
        for i in order:
            w.writerow(dict(file_name=names[i], caption_predicted=preds[i]))
    with open(rfile, "w", newline="") as f:
        cols = [f"caption_reference_{k:02d}" for k in range(1, 6)]
        w = csv.DictWriter(f, ["file_name"] + cols)
        w.writeheader()
        for i in range(len(preds)):
            w.writerow(dict(file_name=names[i], **{c: (truths[i][k] if k < len(truths[i]) else "") for k, c in enumerate(cols)}))
    return pfile, rfile, names


def test_evaluate_metrics_reads_the_reference_csv_columns(stand_ins, tmp_path):
    from clipcap_amd.eval.metrics import evaluate_metrics
    case = golden_cases()[3]
    pfile, rfile, names = _write_csvs(tmp_path, case, shuffle=True)
    out = evaluate_metrics(str(pfile), rfile, device="cpu")
    assert sorted(out) == ["bleu_1", "bleu_2", "bleu_3", "bleu_4", "cider", "rouge_l"]
    for n in range(4):
        assert abs(out[f"bleu_{n + 1}"]["score"] - case["case_bleu"][n]) <= 1e-12 * case["case_bleu"][n]
    assert abs(out["rouge_l"]["score"] - case["case_rouge"]) <= 2.0 ** -23 * case["case_rouge"]
    assert list(out["rouge_l"]["scores"]) == names                                          # sorted by file name, as the reference sorts
    for i, name in enumerate(names):
        assert abs(out["rouge_l"]["scores"][name] - case["rouge"][i]) <= 2.0 ** -23 * case["rouge"][i]
    # rows given instead of files; fewer reference columns read
    rows_p, rows_r = list(csv.DictReader(open(pfile))), list(csv.DictReader(open(rfile)))
    again = evaluate_metrics(rows_p, rows_r, device="cpu")
    assert again == out
    one = evaluate_metrics(rows_p, rows_r, nb_reference_captions=1, metrics=("Bleu",), device="cpu")
    counts = [ref.bleu_counts(c, refs[:1]) for c, refs in case["images"]]
    assert sorted(one) == ["bleu_1", "bleu_2", "bleu_3", "bleu_4"] and one["bleu_4"]["score"] == ref.bleu_corpus(counts)[3]
    with pytest.raises(ValueError, match="no row"):
        evaluate_metrics(rows_p, rows_r[1:], device="cpu")


def test_command_line(stand_ins, tmp_path, capsys):
    from clipcap_amd.eval.base import run_eval
    case = golden_cases()[5]
    pfile, rfile, names = _write_csvs(tmp_path, case, shuffle=False)
    save = tmp_path / "out.json"
    assert run_eval(["--predictions", str(pfile), "--references", str(rfile), "--save-file", str(save), "--device", "cpu"]) == 0
    printed = capsys.readouterr().out
    saved = json.load(open(save))
    assert sorted(saved) == ["bleu_1", "bleu_2", "bleu_3", "bleu_4", "cider", "rouge_l"] and sorted(saved["cider"]["scores"]) == names
    assert abs(saved["bleu_4"]["score"] - case["case_bleu"][3]) <= 1e-12 * case["case_bleu"][3]
    assert f"{saved['rouge_l']['score']:.6f}" in printed and "bleu_4" in printed
    # the module form: argument parsing only (nothing is scored)
    out = subprocess.run([sys.executable, "-m", "clipcap_amd.eval", "--help"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "--nb-reference-captions" in out.stdout and "--save-file" in out.stdout


def test_eval_is_aliased_under_the_reference_name():
    code = ("import clipcap_amd; clipcap_amd.install_as_clipcap(); import clipcap.eval.metrics as m; import clipcap.eval as e; "
            "print(m.evaluate_metrics_from_lists.__module__, m.evaluate_metrics.__module__, e.evaluate_model.__module__)")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.split() == ["clipcap_amd.eval.metrics", "clipcap_amd.eval.metrics", "clipcap_amd.eval.base"]


def test_evaluate_model_word_and_token_levels(stand_ins):
    from types import SimpleNamespace

    from clipcap_amd.eval import evaluate_model
    case = golden_cases()[7]
    preds, truths = _as_strings(case)
    S = len(preds)
    embeds = torch.arange(S, dtype=torch.float32).reshape(S, 1, 1)
    seen = []

    def generate_fake(model, tokenizer, rows, **kw):
        seen.append((rows.shape[0], kw))
        return [preds[int(i)] for i in rows[:, 0, 0].tolist()]

    total, per = evaluate_model(None, None, embeds, truths, batch_size=3, decoder=generate_fake, beam_size=2)
    assert [n for n, _ in seen] == [3] * (S // 3) + ([S % 3] if S % 3 else []) and seen[0][1] == {"beam_size": 2}
    assert abs(total["Bleu_4"] - case["case_bleu"][3]) <= 1e-12 * case["case_bleu"][3] and list(per) == list(range(S))
    # token level: ids from the decoder's *_tokens form (best beam, cut at its length) against tokenizer.encode(reference)
    tokenizer = SimpleNamespace(eos_token="<eos>", encode=lambda s: [999] if s == "<eos>" else [int(w[1:]) for w in s.split()])

    def generate_fake_tokens(model, rows, **kw):
        idx = [int(i) for i in rows[:, 0, 0].tolist()]
        n = max(len(case["images"][i][0]) for i in idx) + 2
        toks = torch.full((len(idx), 2, n), 999, dtype=torch.int64)
        for k, i in enumerate(idx):
            c = case["images"][i][0]
            toks[k, 1, :len(c)] = torch.tensor(c)                                           # beam 1 is the best
            toks[k, 0, :] = 1
        scores = torch.tensor([[0.0, 1.0]] * len(idx))
        lengths = torch.tensor([[n, len(case["images"][i][0]) + 1] for i in idx])
        return toks, scores, lengths

    globals()["generate_fake_tokens"] = generate_fake_tokens
    generate_fake.__module__ = __name__
    total_t, _ = evaluate_model(None, tokenizer, embeds, truths, batch_size=4, level="token", decoder=generate_fake)
    for n in range(4):
        assert abs(total_t[f"Bleu_{n + 1}"] - case["case_bleu"][n]) <= 1e-12 * case["case_bleu"][n]
    assert abs(total_t["ROUGE_L"] - case["case_rouge"]) <= 2.0 ** -23 * case["case_rouge"]
    with pytest.raises(ValueError):
        evaluate_model(None, None, embeds, truths, level="sentence")
    with pytest.raises(ValueError):
        evaluate_model(None, None, embeds[:2], truths)
