"""The optimiser sweeps compute what they computed on the parent commit, bit for bit: every case of
tests/golden/make_optimizer_parent_golden.py (the generator, with the cases' inputs: _update_inputs of
tests/test_gpu_hash_scatter.py, seeded on the CPU) is run on the checked-out tree and the SHA-256 of the raw bytes of the
parameters, exp_avg, exp_avg_sq and the gradient after the call — and of the device step counters for
fnr_adam_step_spans_dev — is compared with what the generator recorded on the parent commit
(tests/golden/optimizer_parent_digests.json: digests, no arrays).

What changed under these digests: the four sweep kernels of the parent (k_adam, k_radam, k_adam_spans, k_adam_spans_dev in
train.hip) became one template in optim.hip whose element loop calls table_adam_update (adam.hpp), the rule that the fused
kernels apply; fnr_adam_step and fnr_radam_step became the one-span case; the step-dependent scalars come from one
function on the host and in the device prologue.  What must not change is every operation per element and its order, and
where the doubles are rounded to float.

Cases, the smallest shapes where a sweep can go wrong:
  * fnr_adam_step (steps 1, 1000) and fnr_radam_step (steps 1, 5, 6: with beta2 = 0.999 the last unrectified and the first
    rectified step, confirmed below with the formula on the host) at 1, 3, 255, 257 and 8192 x 256 + 5 float4s (the last: the
    first size at which the grid-stride loop takes a second trip), each x zero_grad {0, 1} x weight_decay {0, 1e-2} x
    grad_scale {1, 0.5};
  * fnr_adam_step_spans, both algorithms: 1 span; 8 spans with gaps, own steps and learning rates; a span of count 0 in the
    middle; 2 adjacent spans;
  * fnr_adam_step_spans_dev on the same span sets: found_inf absent / 0 / 1 x grad_scale absent / 1024 x zero_grad {0, 1},
    two consecutive calls each; a skipped step is also asserted outright (the generator's spans_dev_case)."""
import json

import pytest

from tests.golden import make_optimizer_parent_golden as G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with open(G.FIXTURE) as f:
        return json.load(f)["cases"]


def test_every_case_has_a_recorded_digest(golden):
    assert sorted(golden) == sorted(G.CASES)


def test_radam_cases_straddle_the_rectification_threshold():
    assert G.STEPS["radam"] == (1, 5, 6)
    assert not G.rectified(G.B2, 1) and not G.rectified(G.B2, 5) and G.rectified(G.B2, 6)


@pytest.mark.parametrize("case", list(G.CASES))
def test_same_bits_as_the_parent_commit(dev, golden, case):
    got = G.compute(case, dev)
    want = golden[case]
    assert sorted(got) == sorted(want)
    differ = [name for name in want if got[name] != want[name]]
    print(f"[optimizer same bits] {case}: {len(want) - len(differ)} of {len(want)} digests equal")
    assert not differ, f"{case}: {differ} differ from the parent commit's"
