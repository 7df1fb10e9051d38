"""tests/test_gpu_hash_scatter.py without a GPU: where its constants and the CPU column of its docstring come from.

The GPU file's tests take the float32 CPU evaluation of their own reference (index_add_ in float32, table_adam_update's
operations in float32) in place of the kernel when handed `FLOAT32` for a device.  Over the GPU file's own inputs that
evaluation stays within 1/4 of every bound — the factor 4 the kernel gets for its other order of summation — except the
accumulate test, whose worst rows are the final rounding of prefill + sum alone (outside the constant; round-to-nearest
attains it).  Run through the tests, the inputs' own conditions are checked here too: the share of samples next to a
lattice plane, the overflowing histogram, the placement of the runs.  And the bounds bite: three stand-ins of kernel bugs
in the float32 evaluation (two swapped corner weights, one dropped record, a fixed point 2^24 too coarse) leave them.
`pytest -s` prints the worst |err| / bound per quantity."""
import pytest

from tests import test_gpu_hash_scatter as hs

QUARTER = 0.25


def _worst(test, *args):
    hs.WORST.clear()
    test(hs.FLOAT32, *args)
    return dict(hs.WORST)


@pytest.mark.parametrize("kind", ["points", "rays"])
@pytest.mark.parametrize("name", hs.GRIDS)
def test_float32_table_gradient_is_within_a_quarter_of_the_bound(name, kind):
    assert 0.0 < _worst(hs.test_gradient_per_row_and_feature, name, kind)["table"] <= QUARTER


@pytest.mark.parametrize("name", ["small16", "rows8k"])
def test_float32_runs_dynamic_range_and_accumulate(name):
    assert 0.0 < _worst(hs.test_runs_of_samples_in_one_cell, name)["runs"] <= QUARTER
    assert 0.0 < _worst(hs.test_dynamic_range_inside_a_level, name)["dynamic range"] <= QUARTER
    assert 0.0 < _worst(hs.test_gradient_is_added_to_a_prefilled_table, name)["accumulate"] <= 1.0


def test_float32_overflow_input_and_the_random_input_that_follows_it():
    assert 0.0 < _worst(hs.test_overflowing_queues_per_row_and_the_workspace_after_them)["overflow"] <= QUARTER
    hs._random_case_that_fits(6)                                     # its own assertion: no bin above the capacity


@pytest.mark.parametrize("case", hs.ADAM_CASES)
def test_float32_update_is_within_a_quarter_of_the_bound(case):
    w = _worst(hs.test_optimiser_sweeps_per_entry, case)
    if case in hs.ADAM_CASES[:4]:
        hs.test_fused_sweep_per_entry(hs.FLOAT32, case)
        w = {k: max(v, hs.WORST[k]) for k, v in w.items()}
    assert set(w) == {"update.parameters", "update.exp_avg", "update.exp_avg_sq"}
    assert all(0.0 < v <= QUARTER for v in w.values()), w


@pytest.mark.parametrize("mutation,test,args", [
    ("swapped corner weights", "test_gradient_per_row_and_feature", ("edge2", "points")),
    ("dropped last record", "test_gradient_per_row_and_feature", ("tiny10", "rays")),
    ("fixed point 2^24 too coarse", "test_dynamic_range_inside_a_level", ("small16",))])
def test_a_wrong_float32_evaluation_leaves_the_bound(monkeypatch, mutation, test, args):
    monkeypatch.setattr(hs, "MUTATION", mutation)
    with pytest.raises(AssertionError):
        getattr(hs, test)(hs.FLOAT32, *args)
