"""The proposal networks' backward computes what it computed on the parent commit, bit for bit: every case of
tests/golden/make_prop_bwd_parent_golden.py (the generator, with the cases' inputs: the seeded helpers of
tests/test_gpu_proposal_kernels.py, imported) is run on the checked-out tree and the SHA-256 of the raw bytes of its arrays —
d_position and the gradients of w0, b0, w1, b1 and the table; parameters, both moments and the gradient arena for the calls
that take the optimiser's step — is compared with what the generator recorded on the parent commit
(tests/golden/prop_bwd_parent_digests.json: digests and the CU count they were recorded on; no arrays).

What changed under these digests is where k_prop_bwd keeps its weights (LDS, not spilled scalar registers) and how its two
phases are ordered (wave-private tiles, no workgroup barrier in the loop); what must not change is every expression per
sample, the order in which a wave's MFMA accumulators take its samples over all passes, the per-thread db1 sum, and the
(w0 + w1) + (w2 + w3) combination per workgroup.

Cases, the smallest shapes where the persistent loop can go wrong: L in {1, 2, 5, 7, 8} x position gradient on / off x
N in {1, 255, 256, 257, 1000, cap 256 - 56 (one pass per workgroup, the last one ragged)}, and for L = 5 also
N = 2 cap 256 + 300 (two and three passes per workgroup, the ragged tail in a late pass), cap = 3 x CUs;
fnr_prop_density_bwd_adam (L = 5 rays N = 1000, L = 7 points N = 257), fnr_prop_density_bwd_pair and _pair_split on an
L = 5 and an L = 7 level, each with and without the optimiser's step.  The cases whose N is made from cap are skipped on a
device with another CU count than the recorded one: their workgroups, and with them the weight sums, are others there."""
import json

import pytest

from tests.golden import make_prop_bwd_parent_golden as G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with open(G.FIXTURE) as f:
        return json.load(f)


def test_every_case_has_a_recorded_digest(golden):
    assert sorted(golden["cases"]) == sorted(G.CASES) and golden["cus"] > 0
    assert G.CAP_BOUND and G.CAP_BOUND < set(G.CASES)


@pytest.mark.parametrize("case", list(G.CASES))
def test_same_bits_as_the_parent_commit(dev, golden, case):
    if case in G.CAP_BOUND and G.cus() != golden["cus"]:
        pytest.skip(f"recorded on {golden['cus']} CUs, this device has {G.cus()}: other workgroups, other weight sums")
    got = G.compute(case, dev)
    want = golden["cases"][case]
    assert sorted(got) == sorted(want)
    differ = [name for name in want if got[name] != want[name]]
    for name in want:
        print(f"[prop bwd same bits] {case}: {name} {got[name][:12]} vs {want[name][:12]}")
    assert not differ, f"{case}: {differ} differ from the parent commit's"
