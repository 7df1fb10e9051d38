"""Register and LDS budgets of the one-wave-per-ray loss, compositing and sampling kernels, read from the metadata the compiler writes
with the code (no GPU needed).

These kernels move a few MB; what they cost is set by how many generations of 4-wave workgroups a launch needs on the 256 CUs
and by how many dependent trips to memory a wave makes.  A 4096-ray batch is 1024 workgroups per role, so (512 registers per
SIMD lane, allocated in blocks of 8; 160 KiB of LDS per CU):
  * k_train_losses at two and four samples per lane (proposal levels up to 256 samples): <= 64 registers = 8 workgroups per CU —
    the two interlevel roles of a default step (2048 workgroups) are resident at once, and 8 x its dynamic LDS fits;
  * the weights / compositing backward family at one sample per lane (the final level's 48 samples): <= 128 registers = 4
    workgroups per CU, the whole launch resident;
  * k_weights_pdf at every width: <= 80 registers = 6 waves per SIMD, and its static LDS (CDF + staged bin edges per wave)
    leaves room for at least 4 workgroups per CU.
None of them may spill or use scratch.  (profiles/per_ray_kernels.md has the figures before and after.)"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fruitnerf_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
LDS_PER_CU = 160 * 1024


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{kernel symbol: {vgpr, agpr, spill, scratch, lds}} of every kernel of train.hip, composite_bwd.hip and sampler.hip, compiled
    with the Makefile's flags (tests/test_isa_invariants.py reads its kernels' metadata the same way)."""
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("hipcc not available")
    tmp = tmp_path_factory.mktemp("per_ray")
    out = {}
    for src in ("train.hip", "composite_bwd.hip", "sampler.hip"):
        asm = tmp / (src[:-4] + ".s")
        cmd = [HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-munsafe-fp-atomics", "-ffp-contract=off",
               "-S", "--cuda-device-only", "-o", str(asm), os.path.join(CSRC, src)]
        subprocess.run(cmd, check=True, capture_output=True, timeout=900)
        for blk in re.split(r"\n\s*- \.agpr_count:", asm.read_text())[1:]:
            def num(key):
                return int(re.search(r"\.%s:\s*(\d+)" % key, blk).group(1))
            name = re.search(r"\.name:\s*(\S+)", blk).group(1)
            assert name not in out, name
            out[name] = dict(vgpr=num("vgpr_count"), agpr=int(re.match(r"\s*(\d+)", blk).group(1)),
                             spill=num("vgpr_spill_count"), scratch=num("private_segment_fixed_size"),
                             lds=num("group_segment_fixed_size"))
    assert len(out) > 60, len(out)
    return out


def _one(kernels, mangled):
    hit = [k for k in kernels if k.startswith(mangled)]
    assert len(hit) == 1, (mangled, hit)
    print(f"[per-ray resources] {hit[0][:60]}: {kernels[hit[0]]}")
    return kernels[hit[0]]


def _clean(m):
    return m["spill"] == 0 and m["scratch"] == 0 and m["agpr"] == 0


@pytest.mark.parametrize("me,p_cap", [(2, 128), (4, 256)])
def test_train_losses_holds_eight_workgroups_per_cu(kernels, me, p_cap):
    m = _one(kernels, f"_ZN3fnr14k_train_lossesILi{me}EEE")
    assert _clean(m) and m["vgpr"] <= 64, m
    dynamic = 4 * (3 * p_cap + 4) * 4           # fnr_train_losses: lds_floats at the widest level the form serves
    assert 8 * (m["lds"] + dynamic) <= LDS_PER_CU, (m, dynamic)


def test_train_losses_eight_wide_form_does_not_spill(kernels):
    assert _clean(_one(kernels, "_ZN3fnr14k_train_lossesILi8EEE"))


def _compositing_backward_forms(me):
    """Mangled prefixes of the compositing / weights backward family at `me` samples per lane: k_weights_bwd (fnr_weights_bwd),
    k_composite_bwd<TARGETS, SEMGRAD, BG, SCALE> (the six standalone entry points) and k_composite_fwd_bwd<SEMGRAD, BG, SCALE>
    (the three fused ones; <0, 0, 0> is a default step's) — every combination of the switches."""
    b = "01"
    forms = [f"_ZN3fnr13k_weights_bwdILi{me}EEE"]
    forms += [f"_ZN3fnr15k_composite_bwdILb{t}ELb{sg}ELb{bg}ELb{sc}ELi{me}EEE" for t in b for sg in b for bg in b for sc in b]
    forms += [f"_ZN3fnr19k_composite_fwd_bwdILb{sg}ELb{bg}ELb{sc}ELi{me}EEE" for sg in b for bg in b for sc in b]
    return forms


@pytest.mark.parametrize("mangled", _compositing_backward_forms(1))
def test_compositing_backward_at_one_sample_per_lane_is_one_generation(kernels, mangled):
    m = _one(kernels, mangled)
    assert _clean(m) and m["vgpr"] <= 128 and m["lds"] == 0, m


@pytest.mark.parametrize("me", [2, 4, 8])
def test_wider_compositing_backward_forms_do_not_spill(kernels, me):
    for mangled in _compositing_backward_forms(me):
        assert _clean(_one(kernels, mangled)), mangled


@pytest.mark.parametrize("me", [1, 2, 4, 8])
def test_weights_pdf_stays_one_generation(kernels, me):
    m = _one(kernels, f"_ZN3fnr13k_weights_pdfILi{me}EEE")
    assert _clean(m) and m["vgpr"] <= 80, m
    assert m["lds"] == 2 * 4 * (64 * me + 1) * 4, m          # CDF + bin edges, per wave
    assert 4 * ((m["lds"] + 511) // 512 * 512) <= LDS_PER_CU, m
