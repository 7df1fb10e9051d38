"""What a training step launches, in which order and on which stream, is what the commit before the orchestration refactor
launched: tests/golden/step_schedule_parent.json holds, per configuration, every `fnr_*` entry point Python called on that
commit (name, order, and launch stream / second stream / other per stream argument); the same recording on this tree must
give the same lists, exactly.  Cases, recorder and generator: tests/golden/make_step_schedule_golden.py."""
import json

import pytest

from tests.golden import make_step_schedule_golden as G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def parent():
    with open(G.FIXTURE) as f:
        return json.load(f)


def test_fixture_holds_every_case(parent):
    assert sorted(parent) == sorted(G.CASES)


@pytest.mark.parametrize("case", list(G.CASES))
def test_step_schedule_is_the_parent_commit_s(dev, parent, case):
    got, want = G.expand(G.record(case, dev)), G.expand(parent[case])
    assert len(got) == len(want), f"{case}: {len(got)} recorded blocks, the parent commit has {len(want)}"
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            first = next((j for j, (a, b) in enumerate(zip(g, w)) if a != b), min(len(g), len(w)))
            pytest.fail(f"{case}, step {i}: {len(g)} calls against the parent's {len(w)}; first difference at call {first}: "
                        f"{g[first:first + 4]} against {w[first:first + 4]}")
    assert sum(len(s) for s in got) > 0
