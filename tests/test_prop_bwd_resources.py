"""Register, LDS and instruction budgets of the proposal networks' backward kernel (prop_bwd.hip: k_prop_bwd<L, 16, position
gradient> for L = 1..8, 16 instantiations), read from the assembly and the metadata the compiler writes with it (no GPU needed).

The kernel runs three workgroups of four waves per CU (prop_mlp_bwd's grid: at most 3 x CUs workgroups):
  * no spilled scalar registers: its 16 (2L + 1) + 17 weights are read from LDS.  As uniform global reads they cost 302
    (L = 5) to 451 (L = 7) scalar registers parked in lanes of vector registers, a v_readlane_b32 per use and 158 scalar loads
    per launch (profiles/prop_bwd_diet.md);
  * <= 168 vector registers (three waves per SIMD), no vector spill, no scratch;
  * 3 x its static LDS (rounded to 512 B) inside a CU's 160 KiB;
  * 2 s_barrier in the whole kernel, both in the epilogue that combines the four waves (one in front of the reuse of s_dh, one
    behind its writes): the loop orders its two phases per wave (the tiles are wave-private);
  * 3 v_mfma_f32_16x16x4_f32 per step of phase 2, the step loop unrolled by 4: 12 in the kernel."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fruitnerf_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
LDS_PER_CU = 160 * 1024
FORMS = [(L, pos) for L in range(1, 9) for pos in (True, False)]
EPILOGUE_BARRIERS = 2
STEP_UNROLL = 4


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{(L, position gradient): {vgpr, agpr, sgpr_spill, vgpr_spill, scratch, lds, body}} of the k_prop_bwd kernels, compiled
    with the Makefile's flags (tests/test_isa_invariants.py and tests/test_scatter_emit_resources.py read theirs the same way)."""
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("hipcc not available")
    asm = tmp_path_factory.mktemp("prop_bwd") / "prop_bwd.s"
    cmd = [HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-munsafe-fp-atomics", "-ffp-contract=off",
           "-S", "--cuda-device-only", "-o", str(asm), os.path.join(CSRC, "prop_bwd.hip")]
    subprocess.run(cmd, check=True, capture_output=True, timeout=900)
    text = asm.read_text()
    lines = text.split("\n")
    meta = {}
    for blk in re.split(r"\n\s*- \.agpr_count:", text)[1:]:
        def num(key):
            return int(re.search(r"\.%s:\s*(\d+)" % key, blk).group(1))
        meta[re.search(r"\.name:\s*(\S+)", blk).group(1)] = dict(
            vgpr=num("vgpr_count"), agpr=int(re.match(r"\s*(\d+)", blk).group(1)), sgpr_spill=num("sgpr_spill_count"),
            vgpr_spill=num("vgpr_spill_count"), scratch=num("private_segment_fixed_size"), lds=num("group_segment_fixed_size"))
    names = [k for k in meta if "k_prop_bwd" in k]
    assert len(names) == len(FORMS), names
    out = {}
    for L, pos in FORMS:
        hit = [k for k in names if k.startswith(f"_ZN3fnr10k_prop_bwdILi{L}ELi16ELb{int(pos)}EEE")]
        assert len(hit) == 1, (L, pos, names)
        start = next(i for i, l in enumerate(lines) if l.startswith(hit[0] + ":"))
        end = next(i for i in range(start, len(lines)) if "s_endpgm" in lines[i])
        body = [l.strip() for l in lines[start:end + 1]]
        out[(L, pos)] = dict(meta[hit[0]], body=[l for l in body if l and not l.startswith((";", "."))])
        print(f"[prop bwd resources] L = {L}, position gradient {pos}: " + ", ".join(f"{k} {v}" for k, v in meta[hit[0]].items()) +
              f", {len(out[(L, pos)]['body'])} instructions")
    return out


@pytest.mark.parametrize("L,pos", FORMS)
def test_registers_lds_and_no_spill(kernels, L, pos):
    m = {k: v for k, v in kernels[(L, pos)].items() if k != "body"}
    assert m["sgpr_spill"] == 0 and m["vgpr_spill"] == 0 and m["scratch"] == 0, m
    assert m["vgpr"] <= 168, m
    assert 3 * ((m["lds"] + 511) // 512 * 512) <= LDS_PER_CU, m


@pytest.mark.parametrize("L,pos", FORMS)
def test_barriers_only_in_the_epilogue_and_three_mfma_per_step(kernels, L, pos):
    body = kernels[(L, pos)]["body"]
    barriers = [i for i, l in enumerate(body) if l.startswith("s_barrier")]
    mfma = [i for i, l in enumerate(body) if l.startswith("v_mfma_")]
    assert len(mfma) == 3 * STEP_UNROLL and all(body[i].startswith("v_mfma_f32_16x16x4_f32") for i in mfma), [body[i] for i in mfma]
    assert len(barriers) == EPILOGUE_BARRIERS and barriers[0] > mfma[-1], (barriers, mfma[-1])   # behind the loop's last MFMA
    assert not any(l.startswith("v_readlane_b32") for l in body[:mfma[-1]]), "a scalar value is fetched back from a vector lane inside the loop"
