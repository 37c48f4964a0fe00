"""CPU side of contrastive search: cc_decode_hidden_unit, cc_contrastive_topk and cc_contrastive_select are declared, bound and exported
under ABI version 3; their argument errors need no device; the decoders take their options as documented and validate them before
anything touches the device."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"cc_decode_hidden_unit": 9, "cc_contrastive_topk": 11, "cc_contrastive_select": 22}


def _declared(name):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "clipcap_hip.h")).read(), flags=re.S)
    m = re.search(r"^(int|int64_t)\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr, flags=re.M)
    assert m, f"{name} is not declared in include/clipcap_hip.h"
    return m.group(1), [p.strip() for p in " ".join(m.group(2).split()).split(",")]


@pytest.mark.parametrize("name", sorted(NAMES))
def test_header_binding_and_library_carry_the_entry_point(name):
    from clipcap_amd import _lib
    ret, params = _declared(name)
    assert ret == "int" and len(params) == NAMES[name]
    res, args = _lib.SIGNATURES[name]
    assert res is _lib._I and len(args) == len(params)
    for p, a in zip(params, args):
        want = _lib._GC if "cc_gpt2_cfg" in p else _lib._P if "*" in p else _lib._L if p.startswith("int64_t") else _lib._F if p.startswith("float") else _lib._I
        assert a is want, (p, a)
    l = _lib.lib()
    assert hasattr(l, name) and l.cc_abi_version() == 3 and _lib.ABI_VERSION == 3


def test_signatures_are_the_documented_ones():
    names = lambda n: [p.split()[-1].lstrip("*") for p in _declared(n)[1]]  # noqa: E731
    assert names("cc_decode_hidden_unit") == ["cfg", "R", "Tnew", "w32", "ws", "out", "ld_row", "ld_pos", "stream"]
    assert names("cc_contrastive_topk") == ["logits", "ldl", "S", "rows_per", "sel", "V", "k", "stopped", "cand_tok", "cand_prob", "stream"]
    assert names("cc_contrastive_select") == ["S", "k", "D", "cand_h", "cand_prob", "cand_tok", "hist", "hist_ld", "hist_lo", "hist_n", "alpha",
                                              "stop_token", "stopped", "lengths", "sel", "src_rows", "skip_rows", "captions", "cap_ld", "step",
                                              "sel_score", "stream"]


def test_generated_abi_files_are_current_and_name_them():
    assert subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_abi.py"), "--check"]).returncode == 0
    csrc = os.path.join(ROOT, "clipcap_amd", "csrc")
    for f in ("abi_dispatch.cpp", "exports.map", "exports_lab.map"):
        text = open(os.path.join(csrc, f)).read()
        for name in NAMES:
            assert name in text, (f, name)
    disp = open(os.path.join(csrc, "abi_dispatch.cpp")).read()
    # contrastive.hip is built once; the hidden states come from decode.hip, built per operand type and selected by the cfg
    for n in ("cc_contrastive_topk", "cc_contrastive_select"):
        assert n + "_bf16" in disp and n + "_f16" not in disp and n + "_x3" not in disp
    assert all("cc_decode_hidden_unit" + s in disp for s in ("_bf16", "_f16", "_x3"))
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^SRCS_ONCE\s*=.*\bcontrastive\.hip\b", mk, flags=re.M)


def _ptrs(n):
    return [C.c_void_p(4096 * (i + 1)) for i in range(n)]


def test_topk_argument_errors_need_no_device():
    from clipcap_amd import _lib
    f = _lib.lib().cc_contrastive_topk
    p = _ptrs(5)

    def call(logits=p[0], ldl=104, S=2, rows_per=1, sel=None, V=97, k=4, stopped=None, tok=p[3], prob=p[4]):
        return f(logits, ldl, S, rows_per, sel, V, k, stopped, tok, prob, None)

    for kw in (dict(logits=None), dict(tok=None), dict(prob=None)):
        assert call(**kw) == -1, kw
    assert call(k=0) == -1 and call(k=9) == -1 and call(k=-1) == -1
    assert call(ldl=96) == -1 and call(V=0, ldl=0) == -1 and call(rows_per=0) == -1 and call(S=-1) == -1
    assert call(V=2097153, ldl=2097153) == -2
    assert call(S=0) == 0 and call(S=0, k=8, sel=p[1], stopped=p[2], rows_per=8) == 0            # nothing is launched


def test_select_argument_errors_need_no_device():
    from clipcap_amd import _lib
    f = _lib.lib().cc_contrastive_select
    p = _ptrs(11)

    def call(S=2, k=4, D=32, cand_h=p[0], prob=p[1], tok=p[2], hist=p[3], hist_ld=12, hist_lo=0, hist_n=5, alpha=0.5, stop=5, stopped=p[4],
             lengths=p[5], sel=p[6], src=p[7], skip=p[8], captions=p[9], cap_ld=8, step=2, score=p[10]):
        return f(S, k, D, cand_h, prob, tok, hist, hist_ld, hist_lo, hist_n, alpha, stop, stopped, lengths, sel, src, skip, captions, cap_ld, step,
                 score, None)

    for kw in (dict(cand_h=None), dict(prob=None), dict(tok=None), dict(hist=None), dict(stopped=None), dict(lengths=None), dict(sel=None),
               dict(src=None), dict(skip=None), dict(captions=None)):
        assert call(**kw) == -1, kw
    assert call(k=0) == -1 and call(k=9) == -1
    assert call(D=30) == -2 and call(D=2052) == -2 and call(D=0) == -1
    assert call(hist_lo=-1) == -1 and call(hist_lo=6) == -1 and call(hist_n=12) == -1 and call(hist_n=13) == -1
    assert call(alpha=-0.1) == -1 and call(alpha=1.5) == -1 and call(alpha=float("nan")) == -1 and call(alpha=float("inf")) == -1
    assert call(step=-1) == -1 and call(step=8) == -1 and call(S=-1) == -1
    assert call(S=0) == 0 and call(S=0, score=None, k=8, D=2048, alpha=1.0, hist_lo=5) == 0      # nothing is launched


def test_hidden_unit_argument_errors_need_no_device():
    from clipcap_amd import _lib
    f = _lib.lib().cc_decode_hidden_unit
    p = _ptrs(3)
    for op in (0, 1, 2):
        cfg = _lib.Gpt2Cfg(32, 2, 2, 97, 128, 48, op)

        def call(cfg=cfg, R=2, Tn=4, w32=p[0], ws=p[1], out=p[2], ld_row=512, ld_pos=32):
            return f(C.byref(cfg) if cfg is not None else None, R, Tn, w32, ws, out, ld_row, ld_pos, None)

        for kw in (dict(cfg=None), dict(w32=None), dict(ws=None), dict(out=None), dict(out=C.c_void_p(4100))):
            assert call(**kw) == -1, kw
        assert call(R=-1) == -1 and call(Tn=0) == -1
        assert call(ld_pos=28) == -1 and call(ld_row=127) == -1 and call(ld_row=124) == -1       # rows would overlap
        assert call(ld_pos=34, ld_row=512) == -2 and call(ld_row=514) == -2                      # 16-byte stores
        assert call(cfg=_lib.Gpt2Cfg(4096, 32, 2, 97, 128, 48, op), ld_row=4 * 4096, ld_pos=4096) == -2
        assert call(R=0) == 0                                                                    # nothing is launched


def test_validate_contrastive_errors():
    from clipcap_amd.inference.utils import MAX_CONTRASTIVE_TOP_K, validate_contrastive
    assert MAX_CONTRASTIVE_TOP_K == 8
    for k, a in ((1, 0.0), (8, 1.0), (4, 0.6), (3, 0)):
        assert validate_contrastive(k, a) is None
    for k, a in ((0, 0.5), (9, 0.5), (-1, 0.5), (2.0, 0.5), ("4", 0.5), (True, 0.5), (None, 0.5),
                 (4, -0.1), (4, 1.01), (4, float("nan")), (4, float("inf")), (4, None), (4, "x")):
        with pytest.raises(ValueError):
            validate_contrastive(k, a)


def test_decoders_take_the_documented_options():
    from clipcap_amd import inference
    from clipcap_amd.inference import contrastive
    assert inference.generate_contrastive is contrastive.generate_contrastive
    assert inference.generate_contrastive_tokens is contrastive.generate_contrastive_tokens
    kwonly = [("include_prefix", True), ("no_repeat_ngram_size", 0), ("min_length", 0), ("suppress_tokens", None)]
    p = inspect.signature(contrastive.generate_contrastive_tokens).parameters
    assert list(p) == ["model", "embeds", "top_k", "penalty_alpha", "entry_length", "stop_token"] + [k for k, _ in kwonly]
    assert [p[k].default for k in ("top_k", "penalty_alpha", "entry_length", "stop_token")] == [4, 0.6, 67, 50256]
    q = inspect.signature(contrastive.generate_contrastive).parameters
    assert list(q) == ["model", "tokenizer", "embeds", "text_prefix_tokens", "top_k", "penalty_alpha", "entry_length"] + [k for k, _ in kwonly]
    assert [q[k].default for k in ("text_prefix_tokens", "top_k", "penalty_alpha", "entry_length")] == [None, 4, 0.6, 67]
    for sig in (p, q):
        for k, d in kwonly:
            assert sig[k].kind is inspect.Parameter.KEYWORD_ONLY and sig[k].default == d and type(sig[k].default) is type(d), k


def test_engine_wrappers_have_the_documented_signatures():
    from clipcap_amd import engine
    assert list(inspect.signature(engine.DecodeSession.hidden_unit).parameters) == ["self", "out", "ld_row", "ld_pos"]
    assert list(inspect.signature(engine.contrastive_buffers).parameters) == ["device", "S", "k", "D", "ctx_max", "entry_length"]
    assert list(inspect.signature(engine.contrastive_topk).parameters) == ["logits", "S", "rows_per", "sel", "k", "stopped", "cand_tok", "cand_prob"]
    assert list(inspect.signature(engine.contrastive_select).parameters) == ["bufs", "k", "hist_lo", "hist_n", "alpha", "stop_token", "step"]
    for fn in (engine.DecodeSession.hidden_unit, engine.contrastive_buffers, engine.contrastive_topk, engine.contrastive_select):
        assert fn.__doc__ and len(fn.__doc__) > 200
    b = engine.contrastive_buffers("cpu", 2, 3, 8, 10, 6)                    # plain tensors: allocates wherever it is told to
    assert b.hist.shape == (2, 10, 8) and b.cand_h.shape == (6, 8) and b.captions.shape == (2, 6) and b.scores.shape == (6, 2)
    assert b.stopped.dtype == torch.uint8 and b.lengths.dtype == torch.int32 and b.skip_rows.dtype == torch.uint8 and b.src_rows.numel() == 6


def test_decoders_validate_before_touching_the_device():
    """A bad option raises ValueError from the decoder itself (no GPU here: anything later would fail differently)."""
    from types import SimpleNamespace
    from clipcap_amd.inference import contrastive
    from clipcap_amd.model.gpt2 import GPT2LM
    lm = GPT2LM(n_embd=32, n_layer=1, n_head=2, vocab_size=97, n_positions=16)
    model = SimpleNamespace(language_model=lm)
    emb = torch.zeros(1, 2, 32)
    with pytest.raises(ValueError, match="top_k"):
        contrastive.generate_contrastive_tokens(model, emb, 9, 0.5, 4, 5)
    with pytest.raises(ValueError, match="top_k"):
        contrastive.generate_contrastive_tokens(model, emb, 0, 0.5, 4, 5)
    with pytest.raises(ValueError, match="penalty_alpha"):
        contrastive.generate_contrastive_tokens(model, emb, 4, 1.5, 4, 5)
    with pytest.raises(ValueError, match="no_repeat_ngram_size"):
        contrastive.generate_contrastive_tokens(model, emb, 4, 0.5, 4, 5, no_repeat_ngram_size=-1)
    with pytest.raises(ValueError, match="never stop"):
        contrastive.generate_contrastive_tokens(model, emb, 4, 0.5, 4, 5, suppress_tokens=[5])
    tok = SimpleNamespace(eos_token="<eos>", encode=lambda s: [5], decode=lambda ids: " ".join(str(int(i)) for i in ids))
    with pytest.raises(ValueError, match="penalty_alpha"):
        contrastive.generate_contrastive(model, tok, emb, top_k=4, penalty_alpha=float("nan"), entry_length=4)
    with pytest.raises(ValueError, match="top_k"):
        contrastive.generate_contrastive(model, tok, emb, top_k=2.5, entry_length=4)
