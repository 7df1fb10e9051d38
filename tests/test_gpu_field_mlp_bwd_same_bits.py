"""The field MLP's backward computes what it computed on the parent commit, bit for bit: every case of
tests/golden/make_field_mlp_bwd_parent_golden.py (the generator, with the cases' inputs: the seeded helpers of
tests/field_reference.py and tests/test_gpu_field_kernels.py, imported) is run on the checked-out tree and the SHA-256 of the
raw bytes of its arrays — d_feats, d_position where a Jacobian is given, the gradient arena with every weight, bias and
embedding gradient; parameters and both moments for the calls that take the optimiser's step — is compared with what the
generator recorded on the parent commit (tests/golden/field_mlp_bwd_parent_digests.json: digests and the CU count they were
recorded on; no arrays).

What changed under these digests is the host side: one argument block, one branch schedule for every shape x arithmetic x
semgrad x Jacobian x fused optimiser, the fp32 branch kernels in a file of their own.  What must not change is every launch,
its arguments and the order of the launches: the kernels are the parent's, instruction for instruction.

Cases: (`fruit_nerf` | `fruit_nerf_big`) x (fp32 | bf16x3 | bf16) x (R, S) in {(1, 16), (5, 16), (6, 24), just above 512 x CUs},
ten calls each: (plain | _rays | _adam with the Jacobian | _semgrad | _semgrad with the Jacobian and the optimiser's step) x
(the forward pass's saved workspace | a bare h).  Why these sizes, why S = 24 and why S < 16 is left to the float64 tests: the
generator's docstring.  The cases whose N is made from the CU count are skipped on a device with another CU count than the
recorded one: their workgroups, and with them the weight sums, are others there."""
import json

import pytest

from tests.golden import make_field_mlp_bwd_parent_golden as G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with open(G.FIXTURE) as f:
        return json.load(f)


def test_every_case_has_a_recorded_digest(golden):
    assert sorted(golden["cases"]) == sorted(G.CASES) and golden["cus"] > 0
    assert G.CAP_BOUND and G.CAP_BOUND < set(G.CASES)
    assert all(len(v) == 38 for v in golden["cases"].values())     # arrays per call form 2 + 3 + 6 + 2 + 6, x 2 workspaces


@pytest.mark.parametrize("case", list(G.CASES))
def test_same_bits_as_the_parent_commit(dev, golden, case):
    if case in G.CAP_BOUND and G.cus() != golden["cus"]:
        pytest.skip(f"recorded on {golden['cus']} CUs, this device has {G.cus()}: other workgroups, other weight sums")
    got = G.compute(case, dev)
    want = golden["cases"][case]
    assert sorted(got) == sorted(want)
    differ = [name for name in want if got[name] != want[name]]
    for name in want:
        print(f"[field mlp bwd same bits] {case}: {name} {got[name][:12]} vs {want[name][:12]}")
    assert not differ, f"{case}: {differ} differ from the parent commit's"
