"""CPU test of the GEMM host launchers (clipcap_amd/csrc/gemm_plan.h and the launchers that consume its plans): every launch that
tests/golden/gemm_launches.json.gz records (tools/record_gemm_launches.py, run on the commit before the dispatch rules moved into one header) is
what the current tree makes — kernel instantiation, grid, block, LDS bytes, every GemmShape field, the integer arguments and the return
status, in the three operand builds, product and lab, under every mode global and lab switch.

The recorder programs are host-only builds with no device image: they run on a machine without a GPU and are never started on one."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_launches.json.gz")

pytestmark = pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is visible: the launch recorder's programs have no device image and "
                                "are only run on machines without one")


@pytest.fixture(scope="module")
def recorded(tmp_path_factory):
    spec = importlib.util.spec_from_file_location("record_gemm_launches", os.path.join(ROOT, "tools", "record_gemm_launches.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    runs, stubs = mod.record(ROOT, str(tmp_path_factory.mktemp("gemm_launches")))
    golden = mod.unpack(mod.load(GOLDEN), [list(r["cases"]) for r in runs])
    return mod, runs, stubs, golden


def test_every_recorded_launch_is_reproduced(recorded):
    mod, runs, stubs, golden = recorded
    assert len(runs) == len(golden)
    n = 0
    for now, then in zip(runs, golden):
        key = {k: now[k] for k in ("op", "lab", "env", "modes")}
        assert key == {k: then[k] for k in key}
        assert len(now["cases"]) == then["n"], key
        for cid, rec in now["cases"].items():
            assert rec == then["cases"][cid], (key, cid, rec, then["cases"][cid])
            n += 1
    print(f"gemm launches: {n} cases in {len(runs)} runs reproduced field for field")


def test_the_table_covers_the_dispatch(recorded):
    """Every operand build, every mode global, every lab switch; the product shapes; at least a fifth refusals and fallbacks; and no kernel
    instantiation of the programs unlaunched beyond the ones profiles/r16_a_gemm_plan_refactor.md names as unreachable."""
    mod, runs, stubs, golden = recorded
    assert {(r["op"], r["lab"]) for r in golden} == {(op, lab) for op in (0, 1, 2) for lab in (False, True)}
    assert {r["modes"] for r in golden} >= {"", "tile=0", "tile=3", "tile=4", "tile=5", "tile=6", "tile=7", "s64=0", "s64=1", "s64=2", "x2=0"}
    for op in (0, 1, 2):
        assert {tuple(r["env"].items()) for r in golden if r["op"] == op and r["env"]} == {((k, v),) for k, v in mod.LAB_SWITCHES}
    assert {k for k, _ in mod.LAB_SWITCHES} == {"CC_GROUP_M", "CC_GEMM_STAGGER", "CC_GEMM_S160", "CC_GEMM_Q4", "CC_Q4_LAST", "CC_X3_FUSED", "CC_WGRAD_TAIL",
                                               "CC_WGRAD_TILE", "CC_WGRAD_KS", "CC_SKINNY_SINGLE", "CC_SKINNY_80", "CC_DEEPK", "CC_EPI_SPEC", "CC_EPI_PLAIN",
                                               "CC_PRE_NT", "CC_RESID_INIT"}
    ids = set(golden[0]["cases"])
    for must in ("bf16out:0,0,12800,3072,768,768,768,3072,1,3,1,0,0", "bf16out:0,0,12800,768,3072,3072,3072,768,0,0,0,0,0", "lmhead:10240,50304,50257,768,1",
                 "deepk:10240,768,50304,1,8", "skinny:320,3072,1024,0,0,16,2,256,0,0", "skinny:64,4096,1024,2,0,16,0,256,0,0", "lmhead:320,50264,50257,1024,3",
                 "bf16out:0,0,2560,2048,1024,1024,1024,2048,1,1,0,0,0", "wgrad:12800,2,1,4,0,0,0;3072,768;768,3072;768,768;768,2304"):
        assert must in ids, must
    missing, refused, total = mod.coverage(golden, stubs)
    assert 5 * refused >= total, (refused, total)
    # unreachable through the wrappers (profiles/r16_a_gemm_plan_refactor.md lists them by rule); anything else must be launched
    for (op, lab), names in missing.items():
        for name in names:
            assert unreachable(name, op, lab), (op, lab, name)


def unreachable(name, op, lab):
    lm = any(e in name for e in ("EpiLMHead", "EpiLogits"))
    if name.startswith("gemm_bf16_kernel<0, 1") or name.startswith("gemm_bf16_kernel<1, 1"):
        return lm or op == 2          # the lm_head wrappers fix both layouts; the split-bf16 build refuses K-strided operands
    if "EpiBF16T<3, 1>" in name and any(k in name for k in ("s64kw", "s80kw", "s64kwb")):
        return True                   # forms 3 / 4 / image are chosen by gemm_nt_skinny only, which never makes the act-3 functor
    if name == "gemm_nt_s64_kernel<EpiBF16T<2, 0>, 2, 3, 1>":
        return True                   # form 2 comes from the skinny mode of launch_gemm only, EpiBF16T<2, 0> from gemm_nt_skinny only
    if op == 2:
        if name.startswith("gemm_tt_"):
            return "group" in name or "tail" in name      # operand images are split per call: nothing is deferred
        if "s64kwb" in name:
            return True               # no weight image in the split-bf16 build
        # product program, the unfused forms of kernels that have a fused two-stage form.  128 x 128: taken where K' = 3 K misses the fused
        # chunk (never, for K % 64 == 0) or for K slices, which only the fp32 functor has.  256 x 192: K' % 32 == 0 implies K' % 96 == 0, and
        # more slices than chunks cannot be asked for (only gemm_nt_deepk names the tile, and it keeps 32 chunks per slice) — no functor.
        # The lab program reaches them all with CC_X3_FUSED=0.
        if not lab:
            return (name.startswith(("gemm_nt_glds_kernel", "gemm_nt_glds4x2_kernel")) and "EpiF32" not in name) or (
                name.startswith("gemm_nt_stag256_kernel") and name.endswith(", 3, false, 8, false>"))
    return False
