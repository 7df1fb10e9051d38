"""Register, LDS and instruction budgets of the binned scatter's emit kernel (hash_scatter.hip: k_scatter_emit, both PAIRS forms),
read from the assembly and the metadata the compiler writes with it (no GPU needed).

The kernel is bound by vector issue and by its LDS atomics, at 3 workgroups of 8 waves per CU:
  * <= 80 registers (6 waves per SIMD), no spill, no scratch, 3 x its static LDS inside a CU's 160 KiB;
  * ONE LDS atomic per record (no-pair form: 8 per thread and level) or per pair of x-neighbours (pair form: 4): the count
    phase's returning atomic is the record's rank inside its bin, placement is s_off[bin] + rank — there is no second atomic
    (8 and 16 before);
  * no ds_bpermute_b32: the level maximum and the bin scan move lanes with DPP (12 shuffles before)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fruitnerf_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
LDS_PER_CU = 160 * 1024
FORMS = {"pairs": ("_ZN3fnr14k_scatter_emitINS_9RaySourceELb1EEE", 4), "no pairs": ("_ZN3fnr14k_scatter_emitINS_9RaySourceELb0EEE", 8)}


@pytest.fixture(scope="module")
def emit(tmp_path_factory):
    """{form: {vgpr, agpr, spill, scratch, lds, body}} of the k_scatter_emit kernels, compiled with the Makefile's flags
    (tests/test_isa_invariants.py and tests/test_per_ray_kernel_resources.py read their kernels the same way)."""
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("hipcc not available")
    asm = tmp_path_factory.mktemp("emit") / "hash_scatter.s"
    cmd = [HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-munsafe-fp-atomics", "-ffp-contract=off",
           "-S", "--cuda-device-only", "-o", str(asm), os.path.join(CSRC, "hash_scatter.hip")]
    subprocess.run(cmd, check=True, capture_output=True, timeout=900)
    text = asm.read_text()
    lines = text.split("\n")
    meta = {}
    for blk in re.split(r"\n\s*- \.agpr_count:", text)[1:]:
        def num(key):
            return int(re.search(r"\.%s:\s*(\d+)" % key, blk).group(1))
        meta[re.search(r"\.name:\s*(\S+)", blk).group(1)] = dict(
            vgpr=num("vgpr_count"), agpr=int(re.match(r"\s*(\d+)", blk).group(1)), spill=num("vgpr_spill_count"),
            scratch=num("private_segment_fixed_size"), lds=num("group_segment_fixed_size"))
    emit_kernels = [k for k in meta if "k_scatter_emit" in k]
    assert len(emit_kernels) == len(FORMS), emit_kernels
    out = {}
    for form, (prefix, _) in FORMS.items():
        hit = [k for k in emit_kernels if k.startswith(prefix)]
        assert len(hit) == 1, (form, emit_kernels)
        start = next(i for i, l in enumerate(lines) if l.startswith(hit[0] + ":"))
        end = next(i for i in range(start, len(lines)) if "s_endpgm" in lines[i])
        body = [l.strip() for l in lines[start:end + 1]]
        out[form] = dict(meta[hit[0]], body=[l for l in body if l and not l.startswith((";", "."))])
        print(f"[scatter emit resources] {form}: " + ", ".join(f"{k} {v}" for k, v in meta[hit[0]].items()) +
              f", {len(out[form]['body'])} instructions")
    return out


@pytest.mark.parametrize("form", list(FORMS))
def test_registers_lds_and_no_scratch(emit, form):
    m = emit[form]
    assert m["vgpr"] <= 80 and m["agpr"] == 0 and m["spill"] == 0 and m["scratch"] == 0, {k: v for k, v in m.items() if k != "body"}
    assert 3 * m["lds"] <= LDS_PER_CU, m["lds"]


@pytest.mark.parametrize("form", list(FORMS))
def test_one_lds_atomic_per_record_or_pair(emit, form):
    adds = [l for l in emit[form]["body"] if re.match(r"ds_add\w*_u32\b", l)]
    print(f"[scatter emit resources] {form}: {len(adds)} ds_add*_u32")
    assert 1 <= len(adds) <= FORMS[form][1], adds
    assert all(l.startswith("ds_add_rtn_u32") for l in adds), adds       # every one of them returns the rank


@pytest.mark.parametrize("form", list(FORMS))
def test_no_lds_shuffles(emit, form):
    shuffles = [l for l in emit[form]["body"] if l.startswith(("ds_bpermute_b32", "ds_permute_b32"))]
    assert not shuffles, shuffles
