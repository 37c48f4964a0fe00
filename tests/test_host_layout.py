"""CPU tests of the host-only layout code (clipcap_amd/csrc/layout.h and the carve functions of api.hip / decode.hip): every size, offset and
refusal status that tests/golden/host_layout.json records (tools/record_host_layout.py, run on the commit before the layouts moved into one
header) is what the current build returns, and the GPT-2 arena has the closed form the decode kernels rely on.  No GPU: the size / offset
functions are host arithmetic and every refused call returns before the first HIP call."""
import ctypes as C
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "host_layout.json")


@pytest.fixture(scope="module")
def rec():
    spec = importlib.util.spec_from_file_location("record_host_layout", os.path.join(ROOT, "tools", "record_host_layout.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    libs = {}
    for which, name in (("product", "libclipcap_hip.so"), ("lab", "libclipcap_hip_lab.so")):
        path = os.path.join(ROOT, "clipcap_amd", name)
        assert os.path.exists(path), f"{name} has not been built"
        libs[which] = mod.load(path, which == "lab")
    return mod, libs


@pytest.mark.parametrize("op", [0, 1, 2])
def test_every_recorded_answer_is_returned(rec, op):
    mod, libs = rec
    rows = [r for r in json.load(open(GOLDEN)) if r["cfg"]["op_dtype"] == op]
    fns = {r["fn"] for r in rows}
    assert {"cc_mapper_param_count", "cc_mapper_param_offsets", "cc_mapper_ws_bytes", "cc_gpt2_param_count", "cc_gpt2_param_offsets",
            "cc_decode_ws_bytes", "cc_decode_part_floats", "cc_decode_image_bytes", "cc_decode_xt_image_bytes"} <= fns
    assert len(rows) >= 150 and sum(r["ret"] < 0 for r in rows) >= 40
    for r in rows:
        lib = libs[r["lib"]]
        if "offsets" in r:
            got = mod.offsets(lib, r["fn"], r["cfg"], len(r["offsets"]))
            assert got == (r["ret"], r["offsets"]), (r["fn"], r["cfg"])
        else:
            got = mod.call(lib, r["fn"], r["cfg"], r["args"])
            assert got == r["ret"], (r["fn"], r["cfg"], r["args"], got, r["ret"])


def test_decode_accepts_what_training_refuses(rec):
    """The decode entry points keep no per-layer tables and check positions per call: 97 layers and an empty position table pass their
    config check and are refused by the training side's."""
    mod, libs = rec
    for over in (dict(NL=97), dict(NPOS=0)):
        cfg = dict(mod.GPT2S["small"], op_dtype=0, **over)
        assert mod.call(libs["product"], "cc_gpt2_param_count", cfg, []) == -2
        assert mod.call(libs["product"], "cc_decode_ws_bytes", cfg, [5, 1]) > 0
        assert mod.call(libs["product"], "cc_decode_reorder", cfg, [1, 1, 0, 1, "PTR", "PTR2", "PTR", None]) == 0


@pytest.mark.parametrize("op", [0, 1, 2])
def test_gpt2_arena_closed_form(rec, op):
    """Uniform layers: layer(l + 1) - layer(l) = 12 D^2 + 13 D for every tensor, ln_f directly behind the last layer, total = ln_f + 2 D."""
    mod, libs = rec
    g = mod.GPT2S["small"]
    cfg = dict(g, op_dtype=op)
    D, NL = g["D"], g["NL"]
    rc, offs = mod.offsets(libs["product"], "cc_gpt2_param_offsets", cfg, 4 + 12 * NL)
    assert rc == 0
    wte, wpe, layers, (lnf_w, lnf_b) = offs[0], offs[1], [offs[2 + 12 * l:14 + 12 * l] for l in range(NL)], offs[-2:]
    stride = 12 * D * D + 13 * D
    assert wte == 0 and wpe == g["Vp"] * D and layers[0][0] == wpe + g["NPOS"] * D
    for l in range(NL - 1):
        assert [b - a for a, b in zip(layers[l], layers[l + 1])] == [stride] * 12, l
    sizes = [D, D, 3 * D * D, 3 * D, D * D, D, D, D, 4 * D * D, 4 * D, 4 * D * D, D]      # l1w l1b aw ab pw pb l2w l2b fw fb p2w p2b
    assert [b - a for a, b in zip(layers[0], layers[0][1:] + [layers[0][0] + stride])] == sizes
    assert lnf_w == layers[-1][0] + stride and lnf_b == lnf_w + D
    assert mod.call(libs["product"], "cc_gpt2_param_count", cfg, []) == lnf_b + D
    # the lab build's fragment-ordered decode image covers the arena: two bytes per element
    if op != 2:
        assert mod.call(libs["lab"], "cc_decode_image_bytes", cfg, []) == 2 * (lnf_b + D)
